"""A plain-Python restatement of igdsp_jb_receive (include/igdsp.h, "Jitter buffer"), one channel at a time, written from RFC 3550's
Appendix A.1 (init_seq / update_seq), A.3 (receiver-report fields) and A.8 (interarrival jitter).  It shares no code with the kernel:
the per-packet depayload records come from the oracle's C depayload (oracle/oracle.py), the sequence and playout logic is below.

Everything is carried in plain ints; state_record() gives the igdsp_jb_state layout (capi.JB_STATE) for comparisons."""
import numpy as np

RTP_SEQ_MOD = 1 << 16
MAX_DROPOUT = 3000
MAX_MISORDER = 100
MIN_SEQUENTIAL = 2
DEPTH = 16
IDLE, PLAYED, LOST = 1, 2, 3
P_NONE, P_INVALID, P_KEEPALIVE, P_PLACED, P_LATE, P_DUPLICATE, P_RESTART = 0, 1, 2, 3, 4, 5, 6
HEARD, PLAYING, TRANSIT = 1, 2, 4
RUNT = 0x40
MISSING_INFO = (0, 0, 0, RUNT)       # ed137, payload_len, pt, flags
U32 = 0xFFFFFFFF

COUNTERS = ("played", "lost", "late", "duplicate", "invalid", "keepalives", "discarded", "restarts")


class Channel:
    """One channel's igdsp_jb_state and ring.  ring[slot] is None or (seq, frame), frame = (payload bytes [n], len, info tuple)."""

    def __init__(self):
        self.ssrc = self.cycles = self.base_seq = self.bad_seq = self.probation = self.received = 0
        self.transit = self.jitter = self.epoch = 0
        self.max_seq = self.head = self.wait = self.lost_run = self.flags = 0
        for k in COUNTERS:
            setattr(self, k, 0)
        self.ring = [None] * DEPTH

    # ---- RFC 3550 A.1
    def init_seq(self, seq):
        self.base_seq = seq
        self.max_seq = seq
        self.bad_seq = RTP_SEQ_MOD + 1          # so seq == bad_seq is false
        self.cycles = 0
        self.received = 0
        self.epoch = (self.epoch + 1) & U32     # received_prior = expected_prior = 0

    def update_seq(self, seq):
        """returns (valid, ran_init_seq)"""
        udelta = (seq - self.max_seq) % RTP_SEQ_MOD
        if self.probation:
            if seq == self.max_seq + 1:          # in C an int comparison: 65535 + 1 is 65536, never a u16 seq
                self.probation -= 1
                self.max_seq = seq
                if self.probation == 0:
                    self.init_seq(seq)
                    self.received += 1
                    return True, True
            else:
                self.probation = MIN_SEQUENTIAL - 1
                self.max_seq = seq
            return False, False
        ran_init = False
        if udelta < MAX_DROPOUT:
            if seq < self.max_seq:
                self.cycles = (self.cycles + RTP_SEQ_MOD) & U32
            self.max_seq = seq
        elif udelta <= RTP_SEQ_MOD - MAX_MISORDER:
            if seq == self.bad_seq:
                self.init_seq(seq)              # two sequential packets: the other side restarted
                ran_init = True
            else:
                self.bad_seq = (seq + 1) & (RTP_SEQ_MOD - 1)
                return False, False
        # else: duplicate or reordered packet
        self.received = (self.received + 1) & U32
        return True, ran_init

    # ---- playout
    def ring_count(self):
        return sum(e is not None for e in self.ring)

    def discard_ring(self):
        self.discarded += self.ring_count()
        self.ring = [None] * DEPTH

    def stop(self):
        self.discard_ring()
        self.flags &= ~PLAYING
        self.wait = 0
        self.lost_run = 0

    def start(self, seq, frame, delay):
        was_playing = bool(self.flags & PLAYING)
        self.discard_ring()
        if was_playing:
            self.restarts += 1
        self.flags |= PLAYING
        self.head = seq
        self.wait = delay
        self.lost_run = 0
        self.ring[seq % DEPTH] = (seq, frame)

    def packet(self, hdr, size, radio, arrival, delay, frame):
        """one arrival: hdr = the packet's first 12 bytes, size its size (> 0); returns (status, is_keepalive)"""
        hdr = bytes(np.asarray(hdr, np.uint8)[:12])
        if size < (20 if radio else 12):
            self.invalid += 1
            return P_INVALID, False
        if hdr[0] >> 6 != 2:
            self.invalid += 1
            return P_INVALID, False
        pt = hdr[1] & 0x7F
        if pt == 123:
            self.keepalives += 1
            return P_KEEPALIVE, True
        seq = hdr[2] << 8 | hdr[3]
        ts = int.from_bytes(hdr[4:8], "big")
        ssrc = int.from_bytes(hdr[8:12], "big")
        new = not (self.flags & HEARD)
        if not new and ssrc != self.ssrc:        # another source on the channel
            self.stop()
            self.restarts += 1
            new = True
        if new:                                  # A.1: state allocated for a source heard for the first time
            self.flags = (self.flags | HEARD) & ~TRANSIT
            self.ssrc = ssrc
            self.init_seq(seq)
            self.max_seq = (seq - 1) % RTP_SEQ_MOD
            self.probation = MIN_SEQUENTIAL
            self.transit = 0
            self.jitter = 0
        valid, ran_init = self.update_seq(seq)
        if not valid:
            self.invalid += 1
            return P_INVALID, False
        if arrival is not None:                  # A.8, integer form, mod 2^32
            transit = (arrival - ts) & U32
            if self.flags & TRANSIT:
                d = (transit - self.transit) & U32
                d = d - (1 << 32) if d >= 1 << 31 else d
                d = abs(d)
                self.jitter = (self.jitter + d - ((self.jitter + 8) >> 4)) & U32
            self.transit = transit
            self.flags |= TRANSIT
        playing = bool(self.flags & PLAYING)
        if not playing or ran_init:
            self.start(seq, frame, delay)
            return P_RESTART, False
        d = (seq - self.head) % RTP_SEQ_MOD
        d = d - RTP_SEQ_MOD if d >= 1 << 15 else d
        if d < 0:
            self.late += 1
            return P_LATE, False
        if d >= DEPTH:
            self.start(seq, frame, delay)
            return P_RESTART, False
        slot = (self.head + d) % DEPTH
        if self.ring[slot] is not None and self.ring[slot][0] == seq:
            self.duplicate += 1
            return P_DUPLICATE, False
        self.ring[slot] = (seq, frame)
        return P_PLACED, False

    def tick(self):
        """returns (flag, frame or None)"""
        if not (self.flags & PLAYING):
            return IDLE, None
        if self.wait > 0:
            self.wait -= 1
            return IDLE, None
        slot = self.head % DEPTH
        e = self.ring[slot]
        self.head = (self.head + 1) % RTP_SEQ_MOD
        if e is not None and e[0] == (self.head - 1) % RTP_SEQ_MOD:
            self.ring[slot] = None
            self.played += 1
            self.lost_run = 0
            return PLAYED, e[1]
        self.lost += 1
        self.lost_run += 1
        if self.lost_run >= DEPTH:
            self.stop()
        return LOST, None

    def state_record(self, dtype):
        r = np.zeros((), dtype)
        for k in ("ssrc", "cycles", "base_seq", "bad_seq", "probation", "received", "transit", "jitter", "epoch", "max_seq", "head", "wait",
                  "lost_run", "flags") + COUNTERS:
            r[k] = getattr(self, k)
        return r


def run(packets, sizes, radio, S, delay=3, n=160, arrival=None, chans=None, dep=None):
    """packets [T*S][C][stride] u8 in arrival order, sizes [T*S][C] (None: full slots), radio [C], arrival [T*S][C] u32 or None.
    dep = (payload, len, info) of oracle.depayload over the same arrays (every arrival's record as igdsp_depayload gives it).
    Returns (payload [T][C][n], len [T][C], info tuples [T][C] as (ed137, payload_len, pt, flags), tick flags [T][C], packet status
    [T*S][C], chans)."""
    A, C_, stride = packets.shape
    T = A // S
    if sizes is None:
        sizes = np.full((A, C_), stride, np.int64)
    chans = chans if chans is not None else [Channel() for _ in range(C_)]
    dpay, dlen, dinfo = dep
    out = np.zeros((T, C_, n), np.uint8)
    olen = np.zeros((T, C_), np.uint16)
    oinfo = np.zeros((T, C_, 4), np.int64)
    flags = np.zeros((T, C_), np.uint8)
    status = np.zeros((A, C_), np.uint8)
    for c in range(C_):
        ch = chans[c]
        for t in range(T):
            ka = None
            for k in range(S):
                a = t * S + k
                size = min(int(sizes[a, c]), stride)
                if size == 0:
                    continue
                frame = (dpay[a, c], int(dlen[a, c]), tuple(int(dinfo[a, c][f]) for f in ("ed137", "payload_len", "pt", "flags")))
                st, is_ka = ch.packet(packets[a, c, :12], size, bool(radio[c]), None if arrival is None else int(arrival[a, c]), delay, frame)
                status[a, c] = st
                if is_ka:
                    ka = frame
            flag, frame = ch.tick()
            flags[t, c] = flag
            if frame is not None:
                out[t, c], olen[t, c], oinfo[t, c] = frame[0], frame[1], frame[2]
            else:
                oinfo[t, c] = ka[2] if ka is not None else MISSING_INFO
    return out, olen, oinfo, flags, status, chans


def report(ch, prior):
    """RFC 3550 A.3 / 6.4.1 for one Channel; prior = dict(expected_prior, received_prior, epoch), advanced in place.  Returns a dict."""
    if not (ch.flags & HEARD):
        return dict(ssrc=0, ext_max_seq=0, cum_lost=0, jitter=0, fraction_lost=0, valid=0)
    extended_max = (ch.cycles + ch.max_seq) & U32
    expected = (extended_max - ch.base_seq + 1) & U32
    lost = max(-0x800000, min(0x7FFFFF, expected - ch.received))
    if prior["epoch"] != ch.epoch:
        prior["expected_prior"] = prior["received_prior"] = 0
    expected_interval = (expected - prior["expected_prior"]) & U32
    received_interval = (ch.received - prior["received_prior"]) & U32
    lost_interval = expected_interval - received_interval
    fraction = 0 if expected_interval == 0 or lost_interval <= 0 else min(255, (lost_interval << 8) // expected_interval)
    prior.update(expected_prior=expected, received_prior=ch.received, epoch=ch.epoch)
    return dict(ssrc=ch.ssrc, ext_max_seq=extended_max, cum_lost=lost, jitter=ch.jitter >> 4, fraction_lost=fraction, valid=1)


# ---- building arrival arrays for tests and benchmarks
def rtp_header(pt, seq, ts, ssrc, radio, word=0, marker=False):
    b = bytearray(20 if radio else 12)
    b[0] = 0x80 | (0x10 if radio else 0)
    b[1] = (0x80 if marker else 0) | (pt & 0x7F)
    b[2:4] = (seq & 0xFFFF).to_bytes(2, "big")
    b[4:8] = (ts & U32).to_bytes(4, "big")
    b[8:12] = (ssrc & U32).to_bytes(4, "big")
    if radio:
        b[12:16] = bytes([0x01, 0x67, 0x00, 0x01])
        b[16:20] = (word & U32).to_bytes(4, "big")
    return bytes(b)


def pack(arrivals, C_, T, S, stride=180):
    """arrivals: {(t, c): [packet bytes, ...]} (at most S per tick, in arrival order) -> (packets [T*S][C][stride], sizes [T*S][C])"""
    packets = np.zeros((T * S, C_, stride), np.uint8)
    sizes = np.zeros((T * S, C_), np.uint16)
    for (t, c), lst in arrivals.items():
        assert len(lst) <= S
        for k, p in enumerate(lst):
            a = t * S + k
            packets[a, c, :min(len(p), stride)] = np.frombuffer(p[:stride], np.uint8)
            sizes[a, c] = len(p)
    return packets, sizes
