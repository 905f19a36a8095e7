"""-m "not gpu": igdsp_link_watch's semantics without a device: the two restatements of tests/link_model.py against each other on seeded
random traffic, the host mirror's LinkWatch (libigdsp_host.so) against them, the reference scenario pinned by hand, the edge cases of
the header's steps, launch-split equivalence of the models, the host-only igdsp_link_work_bytes and the NULL-context paths."""
import ctypes

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import link_model as lm

EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


@pytest.fixture(scope="module")
def host(lib):
    H = ctypes.CDLL(igbuild.HOST_LIB)
    vp, i, u, ull = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_ulonglong
    pi = ctypes.POINTER(ctypes.c_int)
    for name, res, args in (("igdsp_host_link_new", vp, [i, i]), ("igdsp_host_link_free", None, [vp]),
                            ("igdsp_host_link_set_period", i, [vp, i, i]), ("igdsp_host_link_begin", i, [vp, ull, pi]),
                            ("igdsp_host_link_packet", i, [vp, i, i, u, i, ctypes.c_uint32]),
                            ("igdsp_host_link_end", i, [vp, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)]),
                            ("igdsp_host_link_leg", i, [vp, i, ctypes.POINTER(ull), pi, pi, ctypes.POINTER(u)])):
        getattr(H, name).restype = res
        getattr(H, name).argtypes = args
    return H


def same(a, b):
    sa, ka, ea, ta = a
    sb, kb, eb, tb = b
    np.testing.assert_array_equal(sa.view(np.uint8), sb.view(np.uint8))
    np.testing.assert_array_equal(ka, kb)
    np.testing.assert_array_equal(ea.view(np.uint8), eb.view(np.uint8))
    assert ta == tb


def packets(rows, C=1):
    """rows: per arrival slot (pt, payload_len, flags, word) or None for an empty slot -> info [A][1], sizes [A][1]"""
    info = np.zeros((len(rows), C), capi.RTP_INFO)
    sizes = np.zeros((len(rows), C), np.uint16)
    for a, r in enumerate(rows):
        if r is not None:
            info[a, 0] = (r[3], r[1], r[0], r[2])
            sizes[a, 0] = 180
    return info, sizes


def both(*args, **kw):
    a, b = lm.watch_scalar(*args, **kw), lm.watch_numpy(*args, **kw)
    same(a, b)
    return a


def test_struct_layouts_and_constants():
    import os
    import re

    assert capi.LINK_STATE.itemsize == 16 and capi.LINK_EVENT.itemsize == 16
    assert [capi.LINK_STATE.fields[n][1] for n in capi.LINK_STATE.names] == [0, 8, 12, 14, 15]
    assert [capi.LINK_EVENT.fields[n][1] for n in capi.LINK_EVENT.names] == [0, 4, 8, 12, 14, 15]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "igdsp.h")).read()
    for name, val in (("R2S_PERIOD_MS", capi.LINK_R2S_PERIOD_MS), ("MISS_TICKS", capi.LINK_MISS_TICKS), ("AUDIO_ON", capi.LINK_AUDIO_ON),
                      ("AUDIO_OFF", capi.LINK_AUDIO_OFF), ("MISSING", capi.LINK_MISSING), ("LATE", capi.LINK_LATE),
                      ("RECOVERED", capi.LINK_RECOVERED), ("CAME_UP", capi.LINK_CAME_UP), ("EVENT_DEFAULT", capi.LINK_EVENT_DEFAULT),
                      ("UP", capi.LINK_UP), ("AUDIO", capi.LINK_AUDIO), ("ALARMED", capi.LINK_ALARMED)):
        m = re.search(rf"#define\s+IGDSP_LINK_{name}\s+(0x[0-9a-fA-F]+|\d+)", hdr)
        assert m and int(m.group(1), 0) == val, name
    assert capi.LINK_EVENT_DEFAULT == 0x3F & ~capi.LINK_LATE


@pytest.mark.parametrize("seed", range(6))
def test_models_agree_on_random_traffic(seed):
    rng = np.random.default_rng(100 + seed)
    C, T, S = int(rng.integers(1, 40)), int(rng.integers(1, 90)), int(rng.choice([1, 2, 8]))
    tick_ms = int(rng.choice([20, 40]))
    t0 = int(rng.integers(0, 1 << 40))
    info, sizes = lm.traffic(rng, C, T, S, tick_ms, with_sizes=seed != 0)
    up = None if seed % 3 == 0 else (rng.random(C) < 0.8).astype(np.uint8)
    period = None if seed % 2 == 0 else rng.choice([0, 20, 40, 200, 65535], C).astype(np.uint16)
    state = np.zeros(C, capi.LINK_STATE) if seed < 3 else lm.garbage_state(rng, C, t0)
    miss = int(rng.choice([0, 1, 3, 6]))
    for mask in (0, 0x3F, capi.LINK_MISSING):
        st, kind, ev, total = both(info, sizes, up, period, T, S, t0, tick_ms, miss, mask, state)
        assert total == len(ev) == int(np.count_nonzero(kind & (mask or capi.LINK_EVENT_DEFAULT)))
        for cap in (0, 1, max(total - 1, 0), total, total + 7):
            _, _, ec, tc = both(info, sizes, up, period, T, S, t0, tick_ms, miss, mask, state, cap=cap)
            assert tc == total
            np.testing.assert_array_equal(ec.view(np.uint8), ev[:cap].view(np.uint8))
    # the list is tick-major, then ascending channel, and every field is the tick's
    key = ev["tick"].astype(np.int64) * C + ev["channel"]
    assert np.all(np.diff(key) > 0)
    np.testing.assert_array_equal(ev["kind"], kind[ev["tick"], ev["channel"]])
    assert np.all(ev["reserved"] == 0)


def test_traffic_generator_reaches_every_kind():
    rng = np.random.default_rng(7)
    C, T, S = 64, 80, 2
    info, sizes = lm.traffic(rng, C, T, S)
    period = rng.choice([20, 40, 200], C).astype(np.uint16)
    up = (rng.random(C) < 0.9).astype(np.uint8)
    _, kind, ev, _ = both(info, sizes, up, period, T, S, 1000, 20, 3, 0x3F, np.zeros(C, capi.LINK_STATE))
    seen = int(np.bitwise_or.reduce(kind.reshape(-1)))
    assert seen == 0x3F, hex(seen)
    assert np.all(kind[:, up == 0] == 0) and len(ev) > 0
    assert np.any((kind & 3) == 3)                                    # both edges inside one tick happen too


def test_models_are_launch_split_invariant():
    rng = np.random.default_rng(11)
    C, T, S, tick_ms, t0 = 17, 40, 2, 20, 5000
    info, sizes = lm.traffic(rng, C, T, S)
    period = rng.choice([20, 40, 200], C).astype(np.uint16)
    st0 = lm.garbage_state(rng, C, t0)
    whole = both(info, sizes, None, period, T, S, t0, tick_ms, 3, 0x3F, st0)
    st = st0.copy()
    kinds, evs = [], []
    for t in range(T):
        st, k, e, _ = lm.watch_numpy(info[t * S:(t + 1) * S], sizes[t * S:(t + 1) * S], None, period, 1, S, t0 + t * tick_ms, tick_ms, 3, 0x3F, st)
        e = e.copy()
        e["tick"] += t
        kinds.append(k)
        evs.append(e)
    same(whole, (st, np.concatenate(kinds), np.concatenate(evs), len(whole[2])))


def test_host_link_watch_agrees_with_the_models(host):
    for seed in range(4):
        rng = np.random.default_rng(300 + seed)
        C, T, S = int(rng.integers(1, 12)), int(rng.integers(10, 70)), int(rng.choice([1, 2, 8]))
        tick_ms, t0, miss = 20, int(rng.integers(0, 1 << 40)), int(rng.choice([0, 2, 6]))
        info, sizes = lm.traffic(rng, C, T, S)
        period = rng.choice([0, 20, 40, 200, 65535], C).astype(np.uint16)
        up = (rng.random(C) < 0.8).astype(np.uint8)
        st, kind, ev, _ = both(info, sizes, up, period, T, S, t0, tick_ms, miss, 0x3F, np.zeros(C, capi.LINK_STATE))
        v = host.igdsp_host_link_new(C, miss)
        assert v
        try:
            for c in range(C):
                assert host.igdsp_host_link_set_period(v, c, int(period[c])) == 0
            ups = (ctypes.c_int * C)(*[int(x) for x in up])
            kinds, words = (ctypes.c_uint8 * C)(), (ctypes.c_uint32 * C)()
            for t in range(T):
                assert host.igdsp_host_link_begin(v, t0 + t * tick_ms, ups) == 0
                for k in range(S):
                    a = t * S + k
                    for c in range(C):
                        if sizes[a, c]:
                            r = info[a, c]
                            edge = host.igdsp_host_link_packet(v, c, int(r["pt"]), int(r["payload_len"]), int(r["flags"]) & lm.RUNT, int(r["ed137"]))
                            assert edge in (0, lm.ON, lm.OFF)
                missing = host.igdsp_host_link_end(v, kinds, words)
                assert list(kinds) == kind[t].tolist(), (seed, t)
                assert missing == int(np.count_nonzero(kind[t] & lm.MISSING))
                for e in ev[ev["tick"] == t]:
                    assert words[int(e["channel"])] == int(e["word"])
            for c in range(C):
                last, cnt, fl, al = ctypes.c_ulonglong(), ctypes.c_int(), ctypes.c_int(), ctypes.c_uint()
                assert host.igdsp_host_link_leg(v, c, ctypes.byref(last), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(al)) == 0
                if up[c]:
                    assert (last.value, cnt.value, fl.value, al.value) == (int(st["last_ms"][c]), int(st["count"][c]), int(st["flags"][c]),
                                                                          int(st["alarms"][c])), (seed, c)
                else:
                    assert fl.value == 0 and cnt.value == 0
        finally:
            host.igdsp_host_link_free(v)


def test_reference_scenario_pinned_by_hand():
    """period 200, the reference's 40 ms timer and r2sCount == 5: one packet in tick 0, then silence.  diff = 40 t > 600 first at t = 16
    (640 ms): LATE from there on; the count is 5 when tick 21 checks it: MISSING there, once; the count keeps rising."""
    T = 60
    info, sizes = packets([(8, 160, 0, 0xABCD0000)] + [None] * (T - 1))
    st, kind, ev, total = both(info, sizes, None, None, T, 1, 1_000_000, 40, 6, 0x3F, np.zeros(1, capi.LINK_STATE))
    k = kind[:, 0]
    assert k[0] == lm.CAME_UP | lm.ON
    assert np.all(k[1:16] == 0)
    assert np.all(k[16:21] == lm.LATE) and k[21] == lm.LATE | lm.MISSING and np.all(k[22:] == lm.LATE)
    assert int(np.count_nonzero(k & lm.MISSING)) == 1
    assert int(st["count"][0]) == T - 16 and int(st["alarms"][0]) == 1 and int(st["flags"][0]) == lm.UP | lm.AUDIO | lm.ALARMED
    assert int(st["last_ms"][0]) == 1_000_000
    assert total == 1 + T - 16 and ev["tick"].tolist() == [0] + list(range(16, T))
    assert int(ev["word"][0]) == 0xABCD0000 and ev["count"].tolist() == [0] + list(range(1, T - 15))
    # the default mask leaves LATE out: the call coming up and the hang-up cue are the whole list
    _, _, ev, total = both(info, sizes, None, None, T, 1, 1_000_000, 40, 6, 0, np.zeros(1, capi.LINK_STATE))
    assert total == 2 and ev["tick"].tolist() == [0, 21] and ev["kind"].tolist() == [lm.CAME_UP | lm.ON, lm.LATE | lm.MISSING]
    assert ev["count"].tolist() == [0, 6]
    # a packet ends the outage: RECOVERED, the count and ALARMED are cleared, and the next outage fires again
    info, sizes = packets([(123, 0, 0, 1)] + [None] * 29 + [(123, 0, 0, 2)] + [None] * 29)
    st, kind, _, _ = both(info, sizes, None, None, T, 1, 0, 40, 6, 0, np.zeros(1, capi.LINK_STATE))
    assert kind[30, 0] == lm.RECOVERED and kind[21, 0] & lm.MISSING and kind[51, 0] & lm.MISSING and int(st["alarms"][0]) == 2
    # the default miss_ticks is 12 at one tick per 20 ms frame: late after 600 ms (tick 31), MISSING 11 ticks later
    info, sizes = packets([(123, 0, 0, 1)] + [None] * 59)
    _, kind, _, _ = both(info, sizes, None, None, T, 1, 0, 20, 0, 0, np.zeros(1, capi.LINK_STATE))
    assert np.flatnonzero(kind[:, 0] & lm.LATE)[0] == 31 and np.flatnonzero(kind[:, 0] & lm.MISSING).tolist() == [42]


def test_both_edges_inside_one_tick_and_packet_kinds():
    W1, W2, W3 = 0x11111111, 0x22222222, 0x33333333
    up1 = np.zeros(1, capi.LINK_STATE)
    # audio, then a keep-alive, in one tick of an idle leg: both edges, the word of the last one
    info, sizes = packets([(8, 160, 0, W1), (123, 0, 0, W2)])
    st, kind, ev, _ = both(info, sizes, None, None, 1, 2, 0, 20, 0, 0, up1)
    assert kind[0, 0] == lm.CAME_UP | lm.ON | lm.OFF and int(ev["word"][0]) == W2 and int(st["flags"][0]) == lm.UP
    # audio, keep-alive, audio: the leg ends in audio with the third word
    info, sizes = packets([(0, 160, 0, W1), (123, 0, 0, W2), (18, 2, 0, W3), None])
    st, kind, ev, _ = both(info, sizes, None, None, 1, 4, 0, 20, 0, 0, up1)
    assert kind[0, 0] == lm.CAME_UP | lm.ON | lm.OFF and int(ev["word"][0]) == W3 and int(st["flags"][0]) == lm.UP | lm.AUDIO
    # no edge: a second audio packet, a keep-alive on an idle leg; runts and payloads of 1024 or more only refresh the stamp
    talking = np.zeros(1, capi.LINK_STATE)
    talking["flags"], talking["last_ms"] = lm.UP | lm.AUDIO, 0
    for rows in ([(8, 160, 0, W1)], [(123, 0, lm.RUNT, W1)], [(123, 0, 0x40 | 0x01, W1)], [(8, 1024, 0, W1)], [(96, 65535, 0, W1)]):
        info, sizes = packets(rows)
        st, kind, ev, total = both(info, sizes, None, None, 1, 1, 10_000, 20, 0, 0x3F, talking)
        assert kind[0, 0] == 0 and total == 0 and int(st["last_ms"][0]) == 10_000 and int(st["flags"][0]) == lm.UP | lm.AUDIO, rows
    # ... while 1023 bytes of an unknown PT are audio, and an empty slot refreshes nothing
    idle = talking.copy()
    idle["flags"] = lm.UP
    info, sizes = packets([(96, 1023, 0, W1)])
    assert both(info, sizes, None, None, 1, 1, 100, 20, 0, 0, idle)[1][0, 0] == lm.ON
    info, sizes = packets([None])
    st, kind, _, _ = both(info, sizes, None, None, 1, 1, 10_000, 20, 0, 0x3F, talking)
    assert kind[0, 0] == lm.LATE and int(st["last_ms"][0]) == 0 and int(st["count"][0]) == 1


def test_last_ms_ahead_of_now_is_never_late():
    st0 = np.zeros(2, capi.LINK_STATE)
    st0["flags"], st0["last_ms"], st0["count"] = lm.UP, [5_000_000, (1 << 64) - 5], [3, 0]
    info, sizes = packets([None] * 4, C=2)
    st, kind, _, _ = both(info, sizes, None, None, 4, 1, 1000, 20, 0, 0x3F, st0)
    assert kind[:, 0].tolist() == [lm.RECOVERED, 0, 0, 0] and np.all(kind[:, 1] == lm.LATE)   # 2^64 - 5 is behind 1000 by 1005 ms
    assert st["count"].tolist() == [0, 4] and st["last_ms"].tolist() == [5_000_000, (1 << 64) - 5]


def test_t0_near_two_to_the_64():
    """now(t) wraps: a stamp taken just before the wrap is 40 ms old two ticks later, not 2^64 ms ahead"""
    t0 = (1 << 64) - 30
    T = 50
    info, sizes = packets([(123, 0, 0, 9)] + [None] * (T - 1))
    st, kind, _, _ = both(info, sizes, None, np.array([20], np.uint16), T, 1, t0, 20, 3, 0x3F, np.zeros(1, capi.LINK_STATE))
    assert int(st["last_ms"][0]) == t0
    assert np.flatnonzero(kind[:, 0] & lm.LATE)[0] == 4                # 80 ms > 60
    assert np.flatnonzero(kind[:, 0] & lm.MISSING).tolist() == [6] and int(st["count"][0]) == T - 4


def test_garbage_state_keeps_reserved_and_unknown_flag_bits():
    rng = np.random.default_rng(5)
    C, T = 64, 30
    st0 = lm.garbage_state(rng, C, 10_000)
    info, sizes = lm.traffic(rng, C, T, 1)
    up = (rng.random(C) < 0.7).astype(np.uint8)
    st, kind, _, _ = both(info, sizes, up, None, T, 1, 10_000, 20, 0, 0, st0)
    np.testing.assert_array_equal(st["reserved"], st0["reserved"])
    np.testing.assert_array_equal(st["flags"] & 0xF8, st0["flags"] & 0xF8)
    down = up == 0
    np.testing.assert_array_equal(st["flags"][down], st0["flags"][down] & ~np.uint8(lm.UP))
    for f in ("last_ms", "alarms", "count"):
        np.testing.assert_array_equal(st[f][down], st0[f][down])
    # a saturated count stays there
    sat = np.zeros(1, capi.LINK_STATE)
    sat["flags"], sat["count"] = lm.UP, 65535
    info, sizes = packets([None] * 3)
    st, kind, _, _ = both(info, sizes, None, None, 3, 1, 1 << 30, 20, 0, 0x3F, sat)
    assert int(st["count"][0]) == 65535 and np.all(kind[:, 0] == lm.LATE)
    # miss_ticks 65535 fires from count 65534 and only there
    sat["count"] = 65534
    st, kind, _, _ = both(info, sizes, None, None, 3, 1, 1 << 30, 20, 65535, 0x3F, sat)
    assert kind[:, 0].tolist() == [lm.LATE | lm.MISSING, lm.LATE, lm.LATE] and int(st["alarms"][0]) == 1


def test_link_work_bytes_is_host_only(lib):
    # 16 bytes of header, then a 32-bit count per (tick of a part, wave of 64 channels), in whole 16-byte units
    assert capi.link_work_bytes(65536, 128) == 16 + 128 * 1024 * 4
    assert capi.link_work_bytes(65536, 2) == 16 + 2 * 1024 * 4
    assert capi.link_work_bytes(65536, 300) == capi.link_work_bytes(65536, 128)      # parts of 128 ticks reuse it
    assert capi.link_work_bytes(1, 1) == 32 and capi.link_work_bytes(65, 1) == 32 and capi.link_work_bytes(257, 3) == 16 + 64
    assert capi.link_work_bytes(0, 5) == 16 and capi.link_work_bytes(5, 0) == 16
    assert capi.link_work_bytes(0xFFFFFFFF, 0xFFFFFFFF) == 16 + 128 * (1 << 26) * 4
    for c, t in ((1, 1), (63, 2), (4099, 129), (65536, 128)):
        assert capi.link_work_bytes(c, t) % 16 == 0


def test_null_context_and_host_handles(lib, host):
    assert lib.igdsp_link_watch(None, None, None, None, None, 1, 1, 1, 0, 20, 0, 0, None, None, None, 0, None, None, None) == EINVAL
    assert host.igdsp_host_link_begin(None, 0, None) == EINVAL
    assert host.igdsp_host_link_packet(None, 0, 0, 0, 0, 0) == EINVAL
    assert host.igdsp_host_link_end(None, None, None) == EINVAL
    assert host.igdsp_host_link_leg(None, 0, None, None, None, None) == EINVAL
    assert not host.igdsp_host_link_new(0, 0) and not host.igdsp_host_link_new(65537, 0) and not host.igdsp_host_link_new(4, 65536)
    v = host.igdsp_host_link_new(2, 6)
    try:
        assert host.igdsp_host_link_leg(v, 2, None, None, None, None) == EINVAL
        assert host.igdsp_host_link_packet(v, 2, 8, 160, 0, 0) == EINVAL
        assert host.igdsp_host_link_set_period(v, 0, 65536) == EINVAL
        assert host.igdsp_host_link_begin(v, 1000, None) == 0
        assert host.igdsp_host_link_packet(v, 1, 8, 160, 0, 7) == lm.ON
        assert host.igdsp_host_link_packet(v, 1, 8, 160, 0, 7) == 0
        assert host.igdsp_host_link_packet(v, 1, 123, 0, 0, 7) == lm.OFF
        kinds = (ctypes.c_uint8 * 2)()
        assert host.igdsp_host_link_end(v, kinds, None) == 0
        assert list(kinds) == [lm.CAME_UP, lm.CAME_UP | lm.ON | lm.OFF]
    finally:
        host.igdsp_host_link_free(v)
