"""-m "not gpu": the rate converter without a device.  The tables (the header's through igdsp_rs_taps against the model's formula, the
pinned SHA-256, the phase sums, the 2^31 accumulator bound), igdsp_rs_frame through ctypes against tests/rs_model.py bit for bit (every
factor, both directions, n = 1 / 7 / 8 / 23 / 24 / 25 / 160 / 255 / 256, random, silent and full-scale inputs), chaining, the signal
properties (a constant reproduces itself, a sine against the delayed float64 ideal, the stop band, the pass band, a saturating
input), every EINVAL case, and the host mirror's Resampler."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import rs_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
SIZES = (1, 7, 8, 23, 24, 25, 160, 255, 256)
# the largest sum |q| of a phase (UP) / of the table (DOWN), as include/igdsp.h and the issue state them
ABS_SUMS = {2: (30150, 30152), 3: (34960, 29792), 4: (33694, 29740), 6: (34426, 29736)}


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


def frames(direction, R, x, n_in, state=None):
    """x [L] through igdsp_rs_frame in frames of n_in input samples; returns (the outputs concatenated, the state)"""
    st = np.zeros((), capi.RS_STATE) if state is None else state
    out = [capi.rs_frame(st, direction, R, x[i:i + n_in]) for i in range(0, len(x), n_in)]
    return np.concatenate(out), st


# ---- the tables
def test_model_tables_hash_and_spot_values():
    assert rm.table_digest() == rm.TABLE_SHA256
    u2, d2, u6, d6 = rm.up_table(2), rm.down_table(2), rm.up_table(6), rm.down_table(6)
    assert u2[0][:4].tolist() == [-3, 14, -38, 84] and u2[0][11:13].tolist() == [5399, 14141]
    assert d2[:3].tolist() == [-2, 5, 7] and d2[23:25].tolist() == [7074, 7070]
    assert u6[0][:4].tolist() == [-6, 20, -48, 96] and u6[0][11:13].tolist() == [2209, 15401] and d6[71:73].tolist() == [2565, 2567]


def test_header_tables_equal_model_and_hash(lib):
    d = hashlib.sha256()
    for R in rm.FACTORS:
        up, down = capi.rs_taps(capi.RS_UP, R), capi.rs_taps(capi.RS_DOWN, R)
        assert up.shape == (R, 24) and down.shape == (24 * R,)
        np.testing.assert_array_equal(up, rm.up_table(R))
        np.testing.assert_array_equal(down, rm.down_table(R))
        d.update(up.astype("<i2").tobytes())
        d.update(down.astype("<i2").tobytes())
    assert d.hexdigest() == rm.TABLE_SHA256


def test_generator_reproduces_the_committed_header():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rs_tables.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and rm.TABLE_SHA256 in r.stdout and "matches" in r.stdout, r.stdout + r.stderr


def test_phase_sums_and_accumulator_bound(lib):
    for R in rm.FACTORS:
        up, down = capi.rs_taps(capi.RS_UP, R).astype(np.int64), capi.rs_taps(capi.RS_DOWN, R).astype(np.int64)
        assert (up.sum(axis=1) == 16384).all() and down.sum() == 16384
        a_up, a_down = int(np.abs(up).sum(axis=1).max()), int(np.abs(down).sum())
        assert (a_up, a_down) == ABS_SUMS[R]
        for a in (a_up, a_down):
            assert a * 32768 + 8192 < 2 ** 31                              # |x| <= 32768: a 32-bit accumulator is exact
    assert max(ABS_SUMS[R][0] for R in rm.FACTORS) * 2 * 32768 + 16384 >= 2 ** 31   # the largest phase in Q15 would not fit
    worst = max(ABS_SUMS[R][0] for R in rm.FACTORS) * 32767 + 8192 >> 14
    assert 69000 < worst < 70000                                           # the clamp is real


# ---- igdsp_rs_frame against the model
@pytest.mark.parametrize("R", rm.FACTORS)
@pytest.mark.parametrize("direction", (rm.UP, rm.DOWN))
def test_frame_vs_model(lib, direction, R):
    rng = np.random.default_rng(100 * direction + R)
    for n in SIZES:
        n_in = n if direction == rm.UP else n * R
        F = 1 + 400 // n_in if n_in < 200 else 3                          # enough frames for the history to span several of them
        for kind in ("random", "silent", "full", "low"):
            x = {"random": rng.integers(-32768, 32768, F * n_in), "silent": np.zeros(F * n_in, np.int64),
                 "full": rng.choice([-32768, 32767], F * n_in), "low": np.full(F * n_in, -32768)}[kind].astype(np.int16)
            hist = rng.integers(-32768, 32768, 144).astype(np.int16) if kind != "silent" else np.zeros(144, np.int16)
            st = np.zeros((), capi.RS_STATE)
            st["hist"], st["flags"], st["frames"] = hist, 0x5A5A0000, 0xFFFFFFFF
            got, st = frames(direction, R, x, n_in, st)
            raw, new_hist = rm.convert(direction, R, x[None, :], hist[None, :])
            np.testing.assert_array_equal(got, rm.clamp(raw[0]), err_msg=f"{kind} n={n}")
            np.testing.assert_array_equal(st["hist"], new_hist[0])
            assert int(st["frames"]) == F - 1 and int(st["flags"]) == 0x5A5A0000   # frames wraps, flags is kept


@pytest.mark.parametrize("direction", (rm.UP, rm.DOWN))
def test_chaining_any_split(lib, direction):
    """the model: one stream in one piece, or cut anywhere on a frame edge, gives the same rows and state; the entry: frames of
    different sizes over the same stream give the same samples"""
    rng = np.random.default_rng(7)
    for R in rm.FACTORS:
        unit = 1 if direction == rm.UP else R
        x = rng.integers(-32768, 32768, (3, 600 * unit))
        hist = rng.integers(-32768, 32768, (3, 144))
        whole, wh = rm.convert(direction, R, x, hist)
        for cut in (1, 23, 24, 143, 144, 145, 599):
            a, ah = rm.convert(direction, R, x[:, :cut * unit], hist)
            b, bh = rm.convert(direction, R, x[:, cut * unit:], ah)
            np.testing.assert_array_equal(np.concatenate([a, b], axis=1), whole)
            np.testing.assert_array_equal(bh, wh)
        st0 = np.zeros((), capi.RS_STATE)
        st0["hist"] = hist[0]
        ref, ref_st = frames(direction, R, x[0].astype(np.int16), 600 * unit // 4, st0.copy())
        for n in (1, 8, 25, 100):
            got, st = frames(direction, R, x[0].astype(np.int16), n * unit, st0.copy())
            np.testing.assert_array_equal(got, ref)
            np.testing.assert_array_equal(st["hist"], ref_st["hist"])


# ---- signal properties (the bounds were measured on the model, not on the code under test)
def test_constant_reproduces_itself(lib):
    for R in rm.FACTORS:
        for direction, n_in in ((rm.UP, 160), (rm.DOWN, 160 * R)):
            for v in (-32768, -1, 1, 12345, 32767):
                got, _ = frames(direction, R, np.full(2 * n_in, v, np.int16), n_in)
                first = 24 * R if direction == rm.UP else 24                # the history has filled
                assert (got[first:] == v).all(), (R, direction, v)


def test_up_sine_against_delayed_ideal(lib):
    worst = 0.0
    for R in rm.FACTORS:
        N = 24 * R
        for freq in (300, 1000, 3000):
            x = np.round(20000 * np.sin(2 * np.pi * freq * np.arange(1600) / 8000)).astype(np.int16)
            got, _ = frames(rm.UP, R, x, 160)
            q = np.arange(len(got))
            ideal = 20000 * np.sin(2 * np.pi * freq * (q - (N - 1) / 2) / (8000 * R))
            dev = np.abs(got - ideal)[N:].max()                            # behind the start-up transient
            worst = max(worst, dev)
            assert dev <= 16, (R, freq, dev)
    print(f"largest deviation from the delayed float64 sine: {worst:.2f} (bound 16, measured on the model: 11.5)")


def test_down_stop_band_and_pass_band(lib):
    worst_stop, least_pass = 0, 1.0
    for R in rm.FACTORS:
        rate, N = 8000 * R, 24 * R
        t = np.arange(40 * 160 * R)
        for freq in (4600, rate // 2 - 500):
            x = np.round(20000 * np.sin(2 * np.pi * freq * t / rate)).astype(np.int16)
            got, _ = frames(rm.DOWN, R, x, 160 * R)
            peak = int(np.abs(got[24:].astype(int)).max())
            worst_stop = max(worst_stop, peak)
            assert peak <= 16, (R, freq, peak)
        x = np.round(20000 * np.sin(2 * np.pi * 3400 * t / rate)).astype(np.int16)
        got, _ = frames(rm.DOWN, R, x, 160 * R)
        keep = np.abs(got[24:].astype(int)).max() / 20000
        up, _ = frames(rm.UP, R, np.round(20000 * np.sin(2 * np.pi * 3400 * np.arange(6400) / 8000)).astype(np.int16), 160)
        keep = min(keep, np.abs(up[N:].astype(int)).max() / 20000)
        least_pass = min(least_pass, keep)
        assert keep > 0.9, (R, keep)
    print(f"largest stop-band peak {worst_stop} (bound 16, measured on the model: 8); least 3 400 Hz amplitude kept {least_pass:.3f} (bound 0.9, measured: 0.94)")


def test_saturating_input_clamps(lib):
    """the taps' signs times 32767 at a phase's window: the sum of |taps| x 32767 >> 14 is far outside int16, either way"""
    for R in rm.FACTORS:
        up, down = rm.up_table(R), rm.down_table(R)
        p = int(np.abs(up).sum(axis=1).argmax())
        for sign, want in ((1, 32767), (-1, -32768)):
            x = np.zeros(160, np.int64)
            x[100 - np.arange(24)] = sign * np.where(up[p] < 0, -32767, 32767)         # x[g - k] = sign(U[p][k]) 32767 at g = 100
            got, _ = frames(rm.UP, R, x.astype(np.int16), 160)
            raw, _ = rm.convert(rm.UP, R, x[None, :])
            assert got[100 * R + p] == want and abs(int(raw[0, 100 * R + p])) > 60000
            assert rm.records(raw)["flags"][0] & rm.FLAG_SATURATED
            x = np.zeros(160 * R, np.int64)
            x[100 * R + R - 1 - np.arange(24 * R)] = sign * np.where(down < 0, -32767, 32767)
            got, _ = frames(rm.DOWN, R, x.astype(np.int16), 160 * R)
            raw, _ = rm.convert(rm.DOWN, R, x[None, :])
            assert got[100] == want and rm.records(raw)["flags"][0] & rm.FLAG_SATURATED
    quiet, _ = rm.convert(rm.UP, 2, np.full((1, 160), 8), np.full((1, 144), 8))
    assert rm.records(quiet)["flags"][0] == rm.FLAG_SILENT


# ---- EINVAL
def test_einval(lib):
    st, x, out = np.zeros((), capi.RS_STATE), np.zeros(2048, np.int16), np.zeros(4096, np.int16)
    f, s, xi, o = lib.igdsp_rs_frame, st.ctypes.data, x.ctypes.data, out.ctypes.data
    assert f(s, 0, 2, xi, 160, o) == 0 and f(s, 1, 6, xi, 1536, o) == 0 and f(s, 0, 6, xi, 256, o) == 0 and f(s, 1, 3, xi, 3, o) == 0
    before = st.tobytes()
    for args in ((None, 0, 2, xi, 160, o), (s, 0, 2, None, 160, o), (s, 0, 2, xi, 160, None), (s, 2, 2, xi, 160, o), (s, 0, 1, xi, 160, o),
                 (s, 0, 5, xi, 160, o), (s, 0, 8, xi, 160, o), (s, 0, 0, xi, 160, o), (s, 0, 2, xi, 0, o), (s, 0, 2, xi, 257, o),
                 (s, 1, 2, xi, 0, o), (s, 1, 2, xi, 161, o), (s, 1, 3, xi, 160, o), (s, 1, 2, xi, 514, o), (s, 1, 6, xi, 1542, o)):
        assert f(*args) == EINVAL, args
    assert st.tobytes() == before                                          # nothing written
    p, n = ctypes.c_void_p(), ctypes.c_uint32(77)
    t = lib.igdsp_rs_taps
    assert t(0, 2, ctypes.byref(p), ctypes.byref(n)) == 0 and n.value == 48 and t(1, 6, ctypes.byref(p), ctypes.byref(n)) == 0 and n.value == 144
    for args in ((2, 2, ctypes.byref(p), ctypes.byref(n)), (0, 5, ctypes.byref(p), ctypes.byref(n)), (0, 0, ctypes.byref(p), ctypes.byref(n)),
                 (0, 2, None, ctypes.byref(n)), (0, 2, ctypes.byref(p), None)):
        assert t(*args) == EINVAL
    assert n.value == 144
    # a NULL context
    assert lib.igdsp_resample(None, 0, 2, 0, None, None, xi, None, s, 1, 1, 160, 0, 0, o, None, None) == EINVAL


# ---- the host mirror
def test_host_resampler(lib):
    H = ctypes.CDLL(igbuild.HOST_LIB)
    vp, i, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    for name, res, args in (("igdsp_host_rs_new", vp, [u, u]), ("igdsp_host_rs_free", None, [vp]), ("igdsp_host_rs_up", i, [vp, vp, vp]),
                            ("igdsp_host_rs_down", i, [vp, vp, vp])):
        getattr(H, name).restype = res
        getattr(H, name).argtypes = args
    rng = np.random.default_rng(3)
    for rate in (16000, 24000, 32000, 48000):
        R = rate // 8000
        r = H.igdsp_host_rs_new(rate, 160)
        assert r
        try:
            x = rng.integers(-20000, 20000, (4, 160)).astype(np.int16)
            wide, back = np.zeros((4, 160 * R), np.int16), np.zeros((4, 160), np.int16)
            for f in range(4):
                assert H.igdsp_host_rs_up(r, x[f].ctypes.data, wide[f].ctypes.data) == 0
                assert H.igdsp_host_rs_down(r, wide[f].ctypes.data, back[f].ctypes.data) == 0
            raw, _ = rm.convert(rm.UP, R, x.reshape(1, -1))
            np.testing.assert_array_equal(wide.reshape(-1), rm.clamp(raw[0]))
            raw2, _ = rm.convert(rm.DOWN, R, rm.clamp(raw))
            np.testing.assert_array_equal(back.reshape(-1), rm.clamp(raw2[0]))
            assert H.igdsp_host_rs_up(r, None, wide.ctypes.data) == EINVAL and H.igdsp_host_rs_down(r, wide.ctypes.data, None) == EINVAL
        finally:
            H.igdsp_host_rs_free(r)
    for bad in ((8000, 160), (12000, 160), (40000, 160), (16000, 0), (16000, 257), (44100, 160)):
        assert not H.igdsp_host_rs_new(*bad)
