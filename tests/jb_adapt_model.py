"""A plain-Python restatement of igdsp_jb_receive_adaptive (include/igdsp.h, "Jitter buffer, adaptive"), written from the header's
rules: jb_model.Channel with the pre-roll of every Start taken from the Start rule, the LATE bookkeeping and the late re-sync.  It
shares no code with the kernel or with igdsp_jb_adapt_next.

A cfg is the tuple (min_frames, max_frames, init_frames, jitter_mult, late_restart); adapt_record() gives the igdsp_jb_adapt layout
(capi.JB_ADAPT) for comparisons."""
import numpy as np

from tests import jb_model as jm

SET = 0x01
DEFAULT_CFG = (1, 12, 3, 4, 3)          # IGDSP_JB_ADAPT_MIN, _MAX, IGDSP_JB_DELAY, IGDSP_JB_ADAPT_MULT, IGDSP_JB_ADAPT_LATE_RESTART
ADAPT_FIELDS = ("delay", "flags", "need", "late_run", "grows", "shrinks")


def cfg_ok(cfg):
    lo, hi, init, mult, _ = cfg
    return lo <= init <= hi <= jm.DEPTH - 1 and mult <= 16


class AdaptChannel(jm.Channel):
    """One channel's igdsp_jb_state, ring and igdsp_jb_adapt (delay, aflags, need, late_run, grows, shrinks)."""

    def __init__(self, cfg=DEFAULT_CFG, n=160):
        super().__init__()
        assert cfg_ok(cfg)
        self.cfg, self.n = tuple(cfg), n
        self.delay = self.aflags = self.need = self.late_run = self.grows = self.shrinks = 0
        self.delay_trace = []                # igdsp_jb_adapt.delay after each tick's arrivals: d_delay_out

    def start_rule(self):
        """the Start rule: the new delay from the state's jitter J (after the packet's step 6), need and the cfg"""
        lo, hi, init, mult, _ = self.cfg
        was_set = bool(self.aflags & SET)
        cur = self.delay if was_set else init
        tj = min(hi, (mult * self.jitter + 16 * self.n - 1) // (16 * self.n))
        want = max(tj, self.need)
        new = want if want >= cur else cur - 1
        new = max(lo, min(hi, new))
        if was_set and new > self.delay:
            self.grows = min(self.grows + 1, 65535)
        if was_set and new < self.delay:
            self.shrinks = min(self.shrinks + 1, 65535)
        self.delay = new
        self.aflags |= SET
        self.need = 0
        self.late_run = 0
        return new

    def start(self, seq, frame, delay):
        """every Start of step 7: wait = the Start rule's delay, where igdsp_jb_receive writes delay_frames (`delay` is not used)"""
        super().start(seq, frame, self.start_rule())

    def packet(self, hdr, size, radio, arrival, delay, frame):
        head = self.head
        st, is_ka = super().packet(hdr, size, radio, arrival, delay, frame)
        if st == jm.P_LATE:                  # late += 1 was counted; nothing else of the state has changed
            hdr = bytes(np.asarray(hdr, np.uint8)[:12])
            seq = hdr[2] << 8 | hdr[3]
            d = (seq - head) % jm.RTP_SEQ_MOD
            d = d - jm.RTP_SEQ_MOD if d >= 1 << 15 else d
            assert d < 0
            hi, late_restart = self.cfg[1], self.cfg[4]
            self.need = max(self.need, min(self.delay + (-d), hi))
            self.late_run = min(self.late_run + 1, 255)
            if late_restart > 0 and self.late_run >= late_restart:      # the late re-sync: a Start at this packet
                self.start(seq, frame, None)                            # playout was running: restarts += 1, the ring discarded
                return jm.P_RESTART, False
        elif st in (jm.P_PLACED, jm.P_DUPLICATE, jm.P_RESTART):
            self.late_run = 0
        return st, is_ka

    def tick(self):
        self.delay_trace.append(self.delay)
        return super().tick()

    def adapt_record(self, dtype):
        r = np.zeros((), dtype)
        r["delay"], r["flags"], r["need"], r["late_run"], r["grows"], r["shrinks"] = (self.delay, self.aflags, self.need, self.late_run,
                                                                                       self.grows, self.shrinks)
        return r


def run(packets, sizes, radio, S, cfg=DEFAULT_CFG, n=160, arrival=None, chans=None, dep=None):
    """jb_model.run over AdaptChannels (made here with cfg and n unless given): returns its six results and delay_out [T][C] u8."""
    A, C_, _ = packets.shape
    T = A // S
    chans = chans if chans is not None else [AdaptChannel(cfg, n) for _ in range(C_)]
    out = jm.run(packets, sizes, radio, S, 0, n, arrival, chans, dep)
    delay_out = np.array([ch.delay_trace[-T:] for ch in chans], np.uint8).reshape(C_, T).T.copy()
    return out + (delay_out,)
