"""-m "not gpu": the tone generator without a device.  The table's hash, igdsp_tone_plan_build and igdsp_tone_frame through ctypes against
tests/tone_model.py (the ring plan over 150 frames, a plan whose edges fall mid-frame, eight tones, plans that do not loop and end
mid-frame or on a frame edge, every cmd combination, n = 1 / 160 / 255 / 256, three clock rates, every EINVAL case), chaining, the
accuracy against float64, and the host mirror's RingTone cadence."""
import ctypes
import hashlib
import math
import os

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import tone_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
RING = [(440, 480, 2000, 1000)]
EDGES = [(440, 480, 30, 10)]                                              # 240 on / 80 off at 8 kHz: every edge falls inside a frame of 160
EIGHT = [(350, 440, 37, 5), (480, 620, 20, 0), (1000, 0, 13, 7), (1400, 0, 5, 1), (697, 1209, 50, 50, 32767), (3999, 1, 9, 3, 1),
         (2600, 0, 0, 11), (941, 1633, 2, 2, 20000)]


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


def test_table_hash_kat(lib):
    """the SHA-256 of the 1 024 int16-LE table values: of the model's table (math.sin) and of the list in the source"""
    want = "c0074ac685d02073a0c5bd8072657e3e2d4e3bd991288dd52ac6e02de941e729"
    assert hashlib.sha256(tm.TABLE.astype("<i2").tobytes()).hexdigest() == want
    text = open(os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc", "igdsp_tone_tab.h")).read()
    body = text[text.index("IGDSP_TONE_SIN_VALUES") + len("IGDSP_TONE_SIN_VALUES"):].replace("\\", " ")
    vals = np.array([int(v) for v in body.replace(",", " ").split()], "<i2")
    assert len(vals) == 1024 and hashlib.sha256(vals.tobytes()).hexdigest() == want
    assert vals[256] == 32767 and all(vals[i] == -vals[1024 - i] for i in range(1, 1024))
    x = 32767 * np.sin(2 * np.pi * np.arange(1024) / 1024) + 0.5
    off = np.abs(x - np.round(x))[np.arange(1024) % 256 != 0]             # (the four exact entries are no ties either: x.5 -> floor)
    assert off.min() > 1.2e-3


def check_plan(got, want):
    for k in ("n_tones", "options", "cycle", "clock_rate"):
        assert int(got[k]) == want[k], k
    for i, sg in enumerate(want["seg"]):
        for k in ("start", "on", "step1", "step2", "vol", "fade_in", "fade_out"):
            assert int(got["seg"][i][k]) == sg[k], (i, k)
        assert int(got["seg"][i]["reserved"]) == 0
    assert got["seg"][want["n_tones"]:].tobytes() == bytes(24 * (8 - want["n_tones"]))


@pytest.mark.parametrize("rate", [8000, 16000, 48000])
@pytest.mark.parametrize("tones", [RING, EDGES, EIGHT], ids=["ring", "edges", "eight"])
def test_plan_build_vs_model(lib, tones, rate):
    for options in (0, tm.LOOP, tm.NO_FADE, tm.LOOP | tm.NO_FADE):
        check_plan(capi.tone_plan_build(tones, rate, options), tm.plan_build(tones, rate, options))
    assert capi.TONE_DESC.itemsize == 12 and capi.TONE_SEG.itemsize == 24 and capi.TONE_PLAN.itemsize == 208 and capi.TONE_STATE.itemsize == 8
    assert (capi.TONE_MAX, capi.TONE_VOLUME) == (tm.TONE_MAX, tm.VOLUME) == (8, 12288)


def test_plan_build_einval(lib):
    ok = (440, 480, 100, 100, 0, 0)
    bad = [
        ([], 8000, 1), ([ok] * 9, 8000, 1),                               # count 1 .. 8
        ([ok], 7000, 1), ([ok], 49000, 1), ([ok], 8500, 1), ([ok], 0, 1), ([ok], 96000, 1),   # the clock rate
        ([(0, 480, 100, 100)], 8000, 1), ([(4000, 0, 100, 100)], 8000, 1), ([(440, 4000, 100, 100)], 8000, 1),   # 1 .. clock / 2 - 1
        ([(8000, 0, 100, 100)], 16000, 1),
        ([(440, 480, 100, 100, 32768)], 8000, 1),                         # volume
        ([(440, 480, 100, 100, 0, 1)], 8000, 1),                          # reserved
        ([(440, 480, 0, 0)], 8000, 1), ([(440, 0, 0, 0)] * 8, 8000, 0),   # cycle 0
        ([ok], 8000, 4), ([ok], 8000, 0x80000001),                        # unknown options
        ([ok, (440, 480, 100, 100, 40000)], 8000, 1),                     # a bad tone behind a good one
    ]
    for tones, rate, opt in bad:
        assert tm.plan_build(tones, rate, opt) is None, (tones, rate, opt)
        d = np.zeros(max(len(tones), 1), capi.TONE_DESC)
        for i, t in enumerate(tones):
            d[i] = tuple(t) + (0,) * (6 - len(t))
        out = np.full(208, 0xEE, np.uint8)
        assert lib.igdsp_tone_plan_build(d.ctypes.data, len(tones), rate, opt, out.ctypes.data) == EINVAL, (tones, rate, opt)
        assert np.all(out == 0xEE)                                        # nothing written
    d = np.zeros(1, capi.TONE_DESC)
    d[0] = ok
    out = np.zeros(208, np.uint8)
    assert lib.igdsp_tone_plan_build(None, 1, 8000, 1, out.ctypes.data) == EINVAL
    assert lib.igdsp_tone_plan_build(d.ctypes.data, 1, 8000, 1, None) == EINVAL
    # the edges of the ranges pass
    for tones, rate in (([(3999, 3999, 1, 0, 32767)], 8000), ([(1, 0, 0, 1)], 8000), ([(23999, 1, 65535, 65535)] * 8, 48000)):
        check_plan(capi.tone_plan_build(tones, rate, 0), tm.plan_build(tones, rate, 0))


def run_frames(plan_rec, pos, flags, n, cmds):
    """len(cmds) frames of one port through igdsp_tone_frame; cmds[i] applies to frame i"""
    st = np.zeros((), capi.TONE_STATE)
    st["pos"], st["flags"] = pos, flags
    rows, lens = [], []
    for c in cmds:
        row, ln = capi.tone_frame(plan_rec, st, n, c)
        rows.append(row)
        lens.append(ln)
    return np.array(rows), np.array(lens), int(st["pos"]), int(st["flags"])


def model_frames(plan, pos, flags, n, cmds):
    """the same through the model, a launch of one frame per cmd"""
    rows, lens = [], []
    pos, flags = np.array([pos]), np.array([flags])
    for c in cmds:
        pcm, ln, _, pos, flags = tm.generate([plan], None, [c], pos, flags, 1, n)
        rows.append(pcm[0, 0])
        lens.append(ln[0, 0])
    return np.array(rows), np.array(lens), int(pos[0]), int(flags[0])


def check_frames(plan, pos, flags, n, cmds):
    rec = tm.plan_record(plan, capi.TONE_PLAN)
    got, want = run_frames(rec, pos, flags, n, cmds), model_frames(plan, pos, flags, n, cmds)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert got[2:] == want[2:]
    return got


def test_ring_plan_150_frames(lib):
    """150 frames of 160 = 24 000 samples = exactly one cycle: 100 frames of tone (fades at both ends), 50 of zeros, back at 0"""
    plan = tm.plan_build(RING)
    rows, lens, pos, flags = check_frames(plan, 0, tm.PLAYING, 160, [0] * 150)
    assert np.all(lens == 160) and pos == 0 and flags == tm.PLAYING
    assert np.all(rows[100:] == 0) and np.abs(rows[:100]).max() > 11000 and rows[0, 0] == 0 and rows[99, 159] == 0
    assert np.all(np.abs(rows[:100].astype(int)).max(axis=1) > 100)
    # 50 more wrap into the second cycle: the same rows again
    rows2, _, pos2, _ = check_frames(plan, 16000 - 80, tm.PLAYING, 160, [0] * 60)
    assert pos2 == (16000 - 80 + 60 * 160) % 24000


@pytest.mark.parametrize("n", [1, 160, 255, 256])
@pytest.mark.parametrize("rate", [8000, 16000, 48000])
def test_frames_vs_model(lib, n, rate):
    frames = 40 if n > 1 else 700
    for tones, opt in ((EDGES, tm.LOOP), (EIGHT, tm.LOOP), (EIGHT, tm.LOOP | tm.NO_FADE), (EDGES, 0)):
        plan = tm.plan_build(tones, rate, opt)
        for pos in (0, plan["cycle"] // 3, plan["cycle"] - 1):
            check_frames(plan, pos, tm.PLAYING, n, [0] * frames)


def test_non_looping_end(lib):
    """a plan that does not loop: 25 ms + 5 ms = 240 samples ends mid-frame at n = 160, 40 ms = 320 samples on a frame edge"""
    mid = tm.plan_build([(440, 480, 25, 5)], 8000, 0)
    rows, lens, pos, flags = check_frames(mid, 0, tm.PLAYING, 160, [0] * 4)
    assert lens.tolist() == [160, 160, 0, 0] and pos == 240 and flags == 0 and np.all(rows[1, 80:] == 0) and np.any(rows[1, :40] != 0)
    edge = tm.plan_build([(440, 480, 35, 5)], 8000, 0)
    rows, lens, pos, flags = check_frames(edge, 0, tm.PLAYING, 160, [0] * 4)
    assert lens.tolist() == [160, 160, 0, 0] and pos == 320 and flags == 0
    # one frame before the end PLAYING is still set; REWIND plays it again
    assert check_frames(edge, 0, tm.PLAYING, 160, [0])[3] == tm.PLAYING
    rows, lens, pos, flags = check_frames(edge, 0, tm.PLAYING, 160, [0, 0, 0, tm.REWIND, 0, 0])
    assert lens.tolist() == [160, 160, 0, 160, 160, 0] and np.array_equal(rows[3], rows[0])


def test_every_cmd_combination(lib):
    plan = tm.plan_build(EDGES)
    for cmd in range(8):
        for flags in (0, tm.PLAYING, tm.PLAYING | 0x100):
            for pos in (0, 100, 319):
                check_frames(plan, pos, flags, 160, [cmd, 0, 0])
                check_frames(plan, pos, flags, 160, [0, cmd, cmd ^ 4])
    # the words of the rule, spelled out
    _, lens, pos, flags = check_frames(plan, 100, tm.PLAYING, 160, [tm.STOP])
    assert (lens.tolist(), pos, flags) == ([0], 100, 0)
    _, lens, pos, flags = check_frames(plan, 100, 0, 160, [tm.REWIND])
    assert (lens.tolist(), pos, flags) == ([160], 160, tm.PLAYING)
    _, lens, pos, flags = check_frames(plan, 100, tm.PLAYING, 160, [tm.REWIND | tm.STOP])
    assert (lens.tolist(), pos, flags) == ([0], 100, 0)
    _, lens, pos, flags = check_frames(plan, 100, tm.PLAYING, 160, [tm.HOLD])
    assert (lens.tolist(), pos, flags) == ([0], 100, tm.PLAYING)
    _, lens, pos, flags = check_frames(plan, 100, 0, 160, [tm.HOLD | tm.REWIND])
    assert (lens.tolist(), pos, flags) == ([0], 0, tm.PLAYING)


def test_chaining_any_split(lib):
    """F frames in one model launch, F single frames through the entry, and any split of the model in between: the same rows and state"""
    rng = np.random.default_rng(3)
    for tones, opt, n in ((EDGES, tm.LOOP, 160), (EIGHT, tm.LOOP, 255), ([(440, 480, 100, 25)], 0, 160)):
        plan = tm.plan_build(tones, 8000, opt)
        F = 12
        pos0 = int(rng.integers(0, plan["cycle"]))
        whole = tm.generate([plan], None, None, np.array([pos0]), np.array([tm.PLAYING]), F, n)
        got = run_frames(tm.plan_record(plan, capi.TONE_PLAN), pos0, tm.PLAYING, n, [0] * F)
        np.testing.assert_array_equal(got[0], whole[0][:, 0])
        np.testing.assert_array_equal(got[1], whole[1][:, 0])
        assert got[2:] == (int(whole[3][0]), int(whole[4][0]))
        for cut in (1, 5, 11):
            a = tm.generate([plan], None, None, np.array([pos0]), np.array([tm.PLAYING]), cut, n)
            b = tm.generate([plan], None, None, a[3], a[4], F - cut, n)
            np.testing.assert_array_equal(np.concatenate([a[0], b[0]]), whole[0])
            assert (b[3].tolist(), b[4].tolist()) == (whole[3].tolist(), whole[4].tolist())


def test_tone_frame_einval(lib):
    plan = capi.tone_plan_build(RING)
    st, out, ln = np.zeros((), capi.TONE_STATE), np.zeros(256, np.int16), np.zeros((), np.uint16)
    f = lib.igdsp_tone_frame
    assert f(plan.ctypes.data, st.ctypes.data, 0, 160, out.ctypes.data, ln.ctypes.data) == 0
    for args in ((None, st.ctypes.data, 0, 160, out.ctypes.data, ln.ctypes.data), (plan.ctypes.data, None, 0, 160, out.ctypes.data, ln.ctypes.data),
                 (plan.ctypes.data, st.ctypes.data, 0, 160, None, ln.ctypes.data), (plan.ctypes.data, st.ctypes.data, 0, 160, out.ctypes.data, None),
                 (plan.ctypes.data, st.ctypes.data, 0, 0, out.ctypes.data, ln.ctypes.data), (plan.ctypes.data, st.ctypes.data, 0, 257, out.ctypes.data, ln.ctypes.data)):
        assert f(*args) == EINVAL
    assert lib.igdsp_tone_generate(None, None, 1, None, None, None, 1, 1, 160, 0, None, None, None, None) == EINVAL   # a NULL context
    # a plan nobody built is read as it is: cycle 0 plays nothing, a position outside every segment is silence
    bad = np.zeros((), capi.TONE_PLAN)
    st["flags"] = tm.PLAYING
    row, n_out = capi.tone_frame(bad, st, 160)
    assert n_out == 0 and not row.any() and int(st["pos"]) == 0
    bad["cycle"], bad["options"], bad["n_tones"] = 1000, tm.LOOP, 99
    row, n_out = capi.tone_frame(bad, st, 160)
    assert n_out == 160 and not row.any() and int(st["pos"]) == 160


def test_accuracy_vs_float64(lib):
    """|osc - 32767 sin(2 pi ph / 2^32)| < 2 with the phase quantised as the rule quantises it (0.5 table rounding + 0.16 interpolation +
    1 floor); the output within 4 of vol sin / vol (sin + sin) / 2 (the vol / 32768 scale and one more floor); a step within
    clock_rate / 2^33 Hz of its frequency."""
    N = 400000
    k = np.arange(N, dtype=np.int64)
    worst_osc = worst_one = worst_two = 0.0
    for f1, f2, rate, vol in ((440, 480, 8000, 12288), (697, 1209, 8000, 32767), (3999, 1, 8000, 32767), (350, 440, 16000, 20000), (23999, 1000, 48000, 32767)):
        s1, s2 = tm.step_of(f1, rate), tm.step_of(f2, rate)
        for f, s in ((f1, s1), (f2, s2)):
            assert abs(s * rate / 2 ** 32 - f) <= rate / 2 ** 33
        ph1, ph2 = (k * s1) & 0xFFFFFFFF, (k * s2) & 0xFFFFFFFF
        o1, o2 = tm.osc(ph1), tm.osc(ph2)
        x1, x2 = np.sin(2 * np.pi * ph1 / 2.0 ** 32), np.sin(2 * np.pi * ph2 / 2.0 ** 32)
        worst_osc = max(worst_osc, np.abs(o1 - 32767 * x1).max(), np.abs(o2 - 32767 * x2).max())
        worst_one = max(worst_one, np.abs(((o1 * vol) >> 15) - vol * x1).max())
        worst_two = max(worst_two, np.abs((((o1 + o2) * vol) >> 16) - vol * (x1 + x2) / 2).max())
        # and the entry gives those very samples (no fade: the whole ON period is the oscillator rule)
        for freq2, want in ((0, (o1 * vol) >> 15), (f2, ((o1 + o2) * vol) >> 16)):
            plan = capi.tone_plan_build([(f1, freq2, 40, 0, vol)], rate, tm.LOOP | tm.NO_FADE)
            st = np.zeros((), capi.TONE_STATE)
            st["flags"] = tm.PLAYING
            got = np.concatenate([capi.tone_frame(plan, st, 256)[0] for _ in range(2)])
            np.testing.assert_array_equal(got[:320], want[:320])
    print(f"worst oscillator error {worst_osc:.3f}, single tone {worst_one:.3f}, dual tone {worst_two:.3f}")
    assert worst_osc < 2 and worst_one < 4 and worst_two < 4


@pytest.fixture(scope="module")
def host(lib):
    H = ctypes.CDLL(igbuild.HOST_LIB)
    vp, i, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    for name, res, args in (("igdsp_host_ring_new", vp, [u, u]), ("igdsp_host_ring_free", None, [vp]), ("igdsp_host_ring_play", i, [vp]),
                            ("igdsp_host_ring_stop", i, [vp]), ("igdsp_host_ring_connections", i, [vp, u, vp, vp]), ("igdsp_host_ring_cmd", i, [vp]),
                            ("igdsp_host_ring_frame", i, [vp, vp, vp]), ("igdsp_host_ring_get", i, [vp, vp, vp])):
        getattr(H, name).restype = res
        getattr(H, name).argtypes = args
    return H


def test_host_ring_tone_cadence(host):
    """RingTone: three descriptors filled, one played: 2 s on / 1 s off whatever tone[1] and tone[2] say; held until playRing, audible
    from the start of the tone after it, rewound by stopRing"""
    r = host.igdsp_host_ring_new(8000, 160)
    assert r
    try:
        plan, st = np.zeros((), capi.TONE_PLAN), np.zeros((), capi.TONE_STATE)
        assert host.igdsp_host_ring_get(r, plan.ctypes.data, st.ctypes.data) == 0
        check_plan(plan, tm.plan_build(RING, 8000, tm.LOOP))
        assert int(plan["cycle"]) == 24000 and int(plan["n_tones"]) == 1 and (int(st["pos"]), int(st["flags"])) == (0, tm.PLAYING)
        ch, port = np.full(1, 77, np.uint32), np.full(1, 77, np.uint32)
        row, ln = np.zeros(160, np.int16), np.zeros((), np.uint16)
        # not connected: no connection, the port is held
        assert host.igdsp_host_ring_connections(r, 5, ch.ctypes.data, port.ctypes.data) == 0 and ch[0] == 77
        assert host.igdsp_host_ring_frame(r, row.ctypes.data, ln.ctypes.data) == 0 and int(ln) == 0 and not row.any()
        assert host.igdsp_host_ring_play(r) == 0
        assert host.igdsp_host_ring_connections(r, 5, ch.ctypes.data, port.ctypes.data) == 1 and (ch[0], port[0]) == (5, 0)
        want = tm.cycle_wave(tm.plan_build(RING, 8000, tm.LOOP))
        on = []
        for f in range(310):                                               # two cycles and a bit
            assert host.igdsp_host_ring_frame(r, row.ctypes.data, ln.ctypes.data) == 0 and int(ln) == 160
            np.testing.assert_array_equal(row, want[(f * 160 + np.arange(160)) % 24000])
            on.append(bool(row.any()))
        assert on == ([True] * 100 + [False] * 50) * 2 + [True] * 10
        # stopRing: disconnected and rewound; the next playRing starts at the tone's first sample again
        assert host.igdsp_host_ring_stop(r) == 0
        assert host.igdsp_host_ring_connections(r, 5, ch.ctypes.data, port.ctypes.data) == 0
        assert host.igdsp_host_ring_cmd(r) == tm.REWIND | tm.HOLD and host.igdsp_host_ring_cmd(r) == tm.HOLD
        assert host.igdsp_host_ring_stop(r) == 0 and host.igdsp_host_ring_play(r) == 0
        assert host.igdsp_host_ring_frame(r, row.ctypes.data, ln.ctypes.data) == 0
        np.testing.assert_array_equal(row, want[:160])
        assert host.igdsp_host_ring_frame(r, None, ln.ctypes.data) == EINVAL
    finally:
        host.igdsp_host_ring_free(r)
    assert not host.igdsp_host_ring_new(8500, 160) and not host.igdsp_host_ring_new(8000, 0) and not host.igdsp_host_ring_new(8000, 257)
    assert host.igdsp_host_ring_play(None) == EINVAL and host.igdsp_host_ring_cmd(None) == EINVAL
