"""-m "not gpu": hand cases of the jitter buffer's semantics (include/igdsp.h, "Jitter buffer") on tests/jb_model.py, each citing the
rule it checks, and the host-only helpers of the built library: igdsp_jb_report (RFC 3550 A.3 / 6.4.1), igdsp_jb_ring_bytes, and the
igdsp_jb_state / _prior / _rr layouts against their numpy mirrors in capi."""
import ctypes
import os
import re

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import jb_model as jm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSRC = 0x11223344


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


def pkt(seq, pt=8, ssrc=SSRC, ts=None, radio=True, word=0):
    return jm.rtp_header(pt, seq, seq * 160 if ts is None else ts, ssrc, radio, word) + bytes(160)


def feed(ch, ticks, delay=3, arrivals=None, radio=True):
    """ticks: list of lists of packets (bytes); returns (tick flags, statuses, played seqs or None per tick, keep-alive tick infos)"""
    flags, stats, played = [], [], []
    for t, lst in enumerate(ticks):
        st = []
        for k, p in enumerate(lst):
            seq = p[2] << 8 | p[3]
            frame = (None, 0, ("ka", t) if (p[1] & 0x7F) == 123 else seq)
            arr = None if arrivals is None else arrivals[t][k]
            s, _ = ch.packet(np.frombuffer(p[:12].ljust(12, b"\0"), np.uint8), len(p), radio, arr, delay, frame)
            st.append(s)
        f, fr = ch.tick()
        flags.append(f)
        stats.append(st)
        played.append(None if fr is None else fr[2])
    return flags, stats, played


def test_probation_drops_the_first_packet():
    # A.1: a new source starts with probation = MIN_SEQUENTIAL; update_seq returns 0 for the first packet -> counted invalid, not placed
    ch = jm.Channel()
    flags, stats, played = feed(ch, [[pkt(100)], [pkt(101)], [pkt(102)]], delay=0)
    assert stats == [[jm.P_INVALID], [jm.P_RESTART], [jm.P_PLACED]]
    assert flags == [jm.IDLE, jm.PLAYED, jm.PLAYED] and played == [None, 101, 102]
    assert (ch.invalid, ch.received, ch.base_seq, ch.probation) == (1, 2, 101, 0)


def test_probation_wrap_is_not_sequential():
    # A.1 compares seq == max_seq + 1 as ints: during probation 0 does not follow 65535
    ch = jm.Channel()
    _, stats, _ = feed(ch, [[pkt(65535)], [pkt(0)], [pkt(1)]], delay=0)
    assert stats == [[jm.P_INVALID], [jm.P_INVALID], [jm.P_RESTART]]


def test_seq_wrap_counts_a_cycle():
    # A.1: in order with permissible gap, seq < max_seq -> cycles += RTP_SEQ_MOD
    ch = jm.Channel()
    seqs = [65533, 65534, 65535, 0, 1]
    flags, stats, played = feed(ch, [[pkt(s)] for s in seqs], delay=0)
    assert ch.cycles == 1 << 16 and ch.max_seq == 1
    assert played == [None, 65534, 65535, 0, 1]
    rr = jm.report(ch, dict(expected_prior=0, received_prior=0, epoch=0))
    assert rr["ext_max_seq"] == (1 << 16) + 1 and rr["cum_lost"] == 0


def test_large_jump_rejected_once_then_resync():
    # A.1: a jump > MAX_DROPOUT is bad once (bad_seq = seq + 1); the next sequential packet re-syncs with init_seq -> playout restarts
    ch = jm.Channel()
    ticks = [[pkt(10)], [pkt(11)], [pkt(12)], [pkt(5000)], [pkt(5001)], [pkt(5002)]]
    flags, stats, played = feed(ch, ticks, delay=0)
    assert stats[3] == [jm.P_INVALID]
    assert stats[4] == [jm.P_RESTART] and stats[5] == [jm.P_PLACED]
    assert ch.base_seq == 5001 and ch.restarts == 1 and ch.received == 2
    assert played == [None, 11, 12, None, 5001, 5002] and flags[3] == jm.LOST


def test_reorder_within_the_ring_played_in_order():
    # placement: slot (head + d) % DEPTH; playout takes head, head + 1, ...
    ch = jm.Channel()
    ticks = [[pkt(0)], [pkt(1)], [pkt(3)], [pkt(2)], [pkt(4)], [], [], []]
    flags, stats, played = feed(ch, ticks, delay=2)
    assert stats[2] == [jm.P_PLACED] and stats[3] == [jm.P_PLACED]
    assert [p for p in played if p is not None] == [1, 2, 3, 4]
    assert flags[:4] == [jm.IDLE, jm.IDLE, jm.IDLE, jm.PLAYED]


def test_duplicate_kept_once():
    # placement: a slot that already holds this seq -> duplicate += 1, the first copy kept; A.1 still counts it as received
    ch = jm.Channel()
    ch.packet(np.frombuffer(pkt(1)[:12], np.uint8), 180, True, None, 3, (None, 0, "1"))
    ch.packet(np.frombuffer(pkt(2)[:12], np.uint8), 180, True, None, 3, (None, 0, "2"))   # start at 2 (after probation of 1)
    s3, _ = ch.packet(np.frombuffer(pkt(3)[:12], np.uint8), 180, True, None, 3, (None, 0, "3a"))
    s4, _ = ch.packet(np.frombuffer(pkt(3)[:12], np.uint8), 180, True, None, 3, (None, 0, "3b"))
    assert (s3, s4) == (jm.P_PLACED, jm.P_DUPLICATE) and ch.duplicate == 1 and ch.received == 3
    assert ch.ring[3][1][2] == "3a"


def test_late_packet_dropped():
    # placement: d = (int16)(seq - head) < 0 -> late += 1, dropped
    ch = jm.Channel()
    ticks = [[pkt(0)], [pkt(1)], [pkt(2)], [], [pkt(3)]]                    # 3 arrives after its tick went LOST
    flags, stats, played = feed(ch, ticks, delay=0)
    assert flags[3] == jm.LOST and stats[4] == [jm.P_LATE] and ch.late == 1 and ch.lost == 2   # ticks 3 and 4


def test_far_ahead_restarts_playout():
    # placement: d >= IGDSP_JB_DEPTH -> Start at this packet, restarts += 1, discarded += frames in the ring
    ch = jm.Channel()
    ticks = [[pkt(0)], [pkt(1), pkt(2)], [pkt(40)], [], [], []]
    flags, stats, played = feed(ch, ticks, delay=3)
    assert stats[2] == [jm.P_RESTART] and ch.restarts == 1 and ch.discarded == 2
    assert ch.head == 41 and played[5] == 40


def test_ssrc_change_resets_the_source():
    # new source: the source part resets, playout stops, the ring is discarded (discarded, restarts += 1); its first packet is on probation
    ch = jm.Channel()
    ticks = [[pkt(0)], [pkt(1)], [pkt(2)], [pkt(500, ssrc=7)], [pkt(501, ssrc=7)], [pkt(502, ssrc=7)]]
    flags, stats, played = feed(ch, ticks, delay=1)
    assert stats[3] == [jm.P_INVALID] and stats[4] == [jm.P_RESTART]
    assert ch.ssrc == 7 and ch.restarts == 1 and ch.discarded == 1 and ch.base_seq == 501
    assert flags == [jm.IDLE, jm.IDLE, jm.PLAYED, jm.IDLE, jm.IDLE, jm.PLAYED] and played[5] == 501


def test_stop_after_depth_lost_then_preroll():
    # per tick: lost_run reaching IGDSP_JB_DEPTH stops playout; the next accepted packet starts again with delay_frames of pre-roll
    ch = jm.Channel()
    ka = [jm.rtp_header(123, 0, 0, 0, True, 0x10000000)]
    ticks = [[pkt(0)], [pkt(1)]] + [ka] * 20 + [[pkt(40)]] + [[]] * 4
    flags, stats, played = feed(ch, ticks, delay=3)
    assert flags[:4] == [jm.IDLE] * 4 and played[4] == 1                   # seq 1 starts at tick 1, three ticks of pre-roll
    assert flags[5:21] == [jm.LOST] * 16 and flags[21] == jm.IDLE          # the 16th LOST tick stops playout
    assert stats[22] == [jm.P_RESTART] and flags[22:25] == [jm.IDLE] * 3 and played[25] == 40 and flags[26] == jm.LOST
    assert (ch.lost, ch.restarts, ch.discarded, ch.keepalives) == (17, 0, 0, 20)


def test_keepalive_info_on_idle_and_lost_ticks():
    # IDLE / LOST ticks carry the record of the tick's last keep-alive, else the missing-frame record (RUNT)
    C_, T, S = 1, 4, 2
    ka1 = jm.rtp_header(123, 0, 0, 0, True, 0x10000008)
    ka2 = jm.rtp_header(123, 0, 0, 0, True, 0x10000010)
    arrivals = {(0, 0): [ka1, ka2], (2, 0): [ka1]}
    packets, sizes = jm.pack(arrivals, C_, T, S)
    radio = np.ones(1, np.uint8)
    # depayload records as igdsp_depayload gives them for these headers
    dinfo = np.zeros((T * S, C_), capi.RTP_INFO)
    dinfo[0, 0] = (0x10000008, 0, 123, 0x1B)
    dinfo[1, 0] = (0x10000010, 0, 123, 0x1B)
    dinfo[4, 0] = (0x10000008, 0, 123, 0x1B)
    dinfo["flags"][sizes == 0] = jm.RUNT
    dep = (np.zeros((T * S, C_, 160), np.uint8), np.zeros((T * S, C_), np.uint16), dinfo)
    out, ln, info, flags, status, chans = jm.run(packets, sizes, radio, S, 3, 160, None, None, dep)
    assert list(flags[:, 0]) == [jm.IDLE] * 4 and chans[0].keepalives == 3
    assert tuple(info[0, 0]) == (0x10000010, 0, 123, 0x1B)                  # the LAST keep-alive of tick 0
    assert tuple(info[1, 0]) == jm.MISSING_INFO and tuple(info[2, 0]) == (0x10000008, 0, 123, 0x1B)
    assert list(status[:, 0]) == [jm.P_KEEPALIVE, jm.P_KEEPALIVE, 0, 0, jm.P_KEEPALIVE, 0, 0, 0]


def test_jitter_zero_for_constant_transit():
    # A.8: transit = arrival - ts; d = |transit - last transit| = 0 -> jitter stays 0
    ch = jm.Channel()
    ticks = [[pkt(s)] for s in range(10)]
    feed(ch, ticks, arrivals=[[1000 + 160 * s] for s in range(10)])
    assert ch.jitter == 0


def test_jitter_alternating_80():
    # A.8 integer form: arrivals alternately 80 early / late -> |d| = 160 from the second accepted packet on;
    # jitter += 160 - ((jitter + 8) >> 4), starting at the third packet (the first accepted one sets transit only)
    ch = jm.Channel()
    n = 12
    arr = [[160 * s + (80 if s % 2 else -80)] for s in range(n)]
    got = []
    for s in range(n):
        feed(ch, [[pkt(s)]], arrivals=[arr[s]])
        got.append(ch.jitter)
    want, j = [0, 0], 0
    for _ in range(n - 2):
        j += 160 - ((j + 8) >> 4)
        want.append(j)
    assert got == want
    assert want[2:6] == [160, 310, 451, 583]


def test_invalid_runt_and_version():
    # invalid: a runt (size < header) or V != 2 -> invalid += 1, otherwise ignored
    ch = jm.Channel()
    st1, _ = ch.packet(np.zeros(12, np.uint8), 15, True, None, 3, None)
    bad = bytearray(pkt(5)[:12])
    bad[0] = 0x40
    st2, _ = ch.packet(np.frombuffer(bytes(bad), np.uint8), 180, True, None, 3, None)
    assert (st1, st2) == (jm.P_INVALID, jm.P_INVALID) and ch.invalid == 2 and not (ch.flags & jm.HEARD)


# ---- the built library's host helpers
def test_ring_bytes(lib):
    assert capi.jb_ring_bytes(1, 160) == 16 * (4 + 16 + 160)
    assert capi.jb_ring_bytes(65536, 160) == 65536 * 16 * 180
    assert capi.jb_ring_bytes(3, 37) == 3 * 16 * (4 + 16 + 48)
    assert capi.jb_ring_bytes(2, 256) == 2 * 16 * (4 + 16 + 256)
    assert capi.jb_ring_bytes(4, 0) == 0 and capi.jb_ring_bytes(4, 257) == 0


def test_layouts_agree(lib):
    assert capi.JB_STATE.itemsize == 80 and capi.JB_PRIOR.itemsize == 16 and capi.JB_RR.itemsize == 20
    hdr = open(os.path.join(ROOT, "include", "igdsp.h")).read()
    body = re.search(r"typedef struct igdsp_jb_state \{(.*?)\} igdsp_jb_state;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [x.strip() for x in decl.split(None, 1)[1].split(",")]
    assert names == list(capi.JB_STATE.names)
    for name, val in (("IGDSP_JB_DEPTH", capi.JB_DEPTH), ("IGDSP_JB_DELAY", capi.JB_DELAY), ("IGDSP_JB_IDLE", capi.JB_IDLE),
                      ("IGDSP_JB_PLAYED", capi.JB_PLAYED), ("IGDSP_JB_LOST", capi.JB_LOST), ("IGDSP_JB_PKT_RESTART", capi.JB_PKT_RESTART),
                      ("IGDSP_JB_PKT_DUPLICATE", capi.JB_PKT_DUPLICATE), ("IGDSP_JB_PKT_LATE", capi.JB_PKT_LATE)):
        m = re.search(rf"#define\s+{name}\s+(\d+)", hdr)
        assert m and int(m.group(1)) == val, name
    assert (capi.JB_IDLE, capi.JB_PLAYED, capi.JB_LOST) == (jm.IDLE, jm.PLAYED, jm.LOST)
    assert (capi.JB_PKT_INVALID, capi.JB_PKT_KEEPALIVE, capi.JB_PKT_PLACED, capi.JB_PKT_LATE, capi.JB_PKT_DUPLICATE, capi.JB_PKT_RESTART) == (
        jm.P_INVALID, jm.P_KEEPALIVE, jm.P_PLACED, jm.P_LATE, jm.P_DUPLICATE, jm.P_RESTART)


def _report_both(ch, prior_np, prior_model):
    rr = capi.jb_report(ch.state_record(capi.JB_STATE), prior_np)
    want = jm.report(ch, prior_model)
    for k, v in want.items():
        assert int(rr[k]) == v, (k, int(rr[k]), v)
    assert int(prior_np["expected_prior"]) == prior_model["expected_prior"]
    return rr


def test_report_fraction_lost_and_prior(lib):
    # A.3: fraction over the interval since the last report, which then becomes the prior
    ch = jm.Channel()
    prior, pm = np.zeros((), capi.JB_PRIOR), dict(expected_prior=0, received_prior=0, epoch=0)
    rr = _report_both(ch, prior, pm)
    assert int(rr["valid"]) == 0 and int(rr["ext_max_seq"]) == 0       # nothing heard yet
    seqs = [0, 1, 2, 3, 5, 6, 9, 10]                                       # 4, 7, 8 lost
    feed(ch, [[pkt(s)] for s in seqs])
    rr = _report_both(ch, prior, pm)
    # after probation: base 1, max 10 -> expected 10, received 7, lost 3; the priors belong to the epoch of the probation's end
    assert (int(rr["ext_max_seq"]), int(rr["cum_lost"]), int(rr["fraction_lost"])) == (10, 3, (3 << 8) // 10)
    feed(ch, [[pkt(s)] for s in (11, 12, 14)])                             # 13 lost: 1 of 4
    rr = _report_both(ch, prior, pm)
    assert (int(rr["cum_lost"]), int(rr["fraction_lost"])) == (4, (1 << 8) // 4)
    rr = _report_both(ch, prior, pm)                                       # an empty interval
    assert int(rr["fraction_lost"]) == 0


def test_report_24bit_clamp(lib):
    # 6.4.1: cumulative lost is a signed 24-bit field: clamped to [-0x800000, 0x7FFFFF]
    st = np.zeros((), capi.JB_STATE)
    st["flags"], st["cycles"], st["max_seq"], st["base_seq"], st["received"], st["jitter"], st["ssrc"] = jm.HEARD, 1 << 28, 5, 0, 1, 33, 9
    prior = np.zeros((), capi.JB_PRIOR)
    rr = capi.jb_report(st, prior)
    assert int(rr["cum_lost"]) == 0x7FFFFF and int(rr["jitter"]) == 2 and int(rr["ssrc"]) == 9 and int(rr["ext_max_seq"]) == (1 << 28) + 5
    st["received"] = (1 << 28) + 6 + 0x900000                              # duplicates: lost below -2^23
    rr = capi.jb_report(st, np.zeros((), capi.JB_PRIOR))
    assert int(rr["cum_lost"]) == -0x800000 and int(rr["fraction_lost"]) == 0


def test_report_new_epoch_resets_priors(lib):
    # init_seq zeroes expected_prior / received_prior: a report after a re-sync counts from the new base
    ch = jm.Channel()
    prior, pm = np.zeros((), capi.JB_PRIOR), dict(expected_prior=0, received_prior=0, epoch=0)
    feed(ch, [[pkt(s)] for s in range(20)])
    _report_both(ch, prior, pm)
    feed(ch, [[pkt(s)] for s in (9000, 9001, 9002, 9004)])
    rr = _report_both(ch, prior, pm)
    assert int(prior["epoch"]) == ch.epoch and int(rr["ext_max_seq"]) == 9004 and int(rr["cum_lost"]) == 1


def test_report_rejects_null(lib):
    L = capi.load()
    st, pr, rr = np.zeros((), capi.JB_STATE), np.zeros((), capi.JB_PRIOR), np.zeros((), capi.JB_RR)
    vp = ctypes.c_void_p
    assert L.igdsp_jb_report(None, pr.ctypes.data_as(vp), rr.ctypes.data_as(vp)) == -22
    assert L.igdsp_jb_report(st.ctypes.data_as(vp), None, rr.ctypes.data_as(vp)) == -22
    assert L.igdsp_jb_report(st.ctypes.data_as(vp), pr.ctypes.data_as(vp), None) == -22
