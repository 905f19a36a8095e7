"""-m "not gpu": the delay buffer without a device.  igdsp_dbuf_step through ctypes against tests/dbuf_model.py bit for bit (rows, flags,
scalars, live samples) over the scenarios a sound port meets (steady, a producer 1 % fast and 1 % slow, bursts of three, random ops, a
garbage state), the inputs that stress the shrink (speech-like, all-zero and constant rows whose lags all tie, a full-scale square), every
frame size with the three maxima, chaining splits, the properties of the model itself, the state's layout, every EINVAL case, the
yardstick's binding and the host mirror's DelayBuf."""
import ctypes
import os
import re

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import dbuf_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
SIZES = (1, 24, 80, 160, 164, 256)


def maxima(n):
    return sorted({2 * n, 1024 // n * n, 1024})


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


def inputs(kind, T, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "speech":
        return dm.speech(rng, T, n, 95.0 + 7.0 * seed)
    if kind == "zero":
        return np.zeros((T, n), np.int16)
    if kind == "const":
        return np.full((T, n), -12345, np.int16)
    if kind == "square":
        return dm.square(T, n)
    raise KeyError(kind)


def scenario(kind, T, seed=0):
    rng = np.random.default_rng(100 + seed)
    if kind == "steady":
        return np.full(T, 3, np.uint8)
    if kind == "fast":
        return dm.clocked_ops(T, 1.01, 0.37)
    if kind == "slow":
        return dm.clocked_ops(T, 0.99, 0.37)
    if kind == "bursts":
        return np.tile(np.array([1, 1, 1, 2, 2, 2], np.uint8), T // 6 + 1)[:T]
    if kind == "random":
        return ((rng.random(T) < 0.95) * 1 + (rng.random(T) < 0.80) * 2).astype(np.uint8)
    if kind == "hungry":
        return ((rng.random(T) < 0.80) * 1 + (rng.random(T) < 0.95) * 2).astype(np.uint8)
    raise KeyError(kind)


def record_of(st):
    return np.zeros((), capi.DBUF_STATE) if st is None else st


def assert_same_state(rec, model):
    got = dm.from_record(rec)
    assert dm.scalars(got) == dm.scalars(model)
    np.testing.assert_array_equal(dm.live(got), dm.live(model))


def walk(ops, x, n, M, rec=None, model=None):
    """every step through igdsp_dbuf_step and through the model, compared step by step; returns (the record, the model state)"""
    rec = record_of(rec)
    model = dm.from_record(rec) if model is None else model
    for t, op in enumerate(ops):
        out, flag = capi.dbuf_step(rec, int(op), n, M, x[t] if op & 1 else None)
        want, wflag = dm.step(model, int(op), x[t], n, M)
        assert flag == wflag, (t, op)
        assert (out is None) == (want is None), (t, op)
        if out is not None:
            np.testing.assert_array_equal(out, want, err_msg=f"step {t} op {op}")
        assert int(rec["len"]) == model["len"], t
    assert_same_state(rec, model)
    return rec, model


@pytest.mark.parametrize("kind", ["steady", "fast", "slow", "bursts", "random", "hungry"])
@pytest.mark.parametrize("signal", ["speech", "zero", "const", "square"])
def test_step_equals_model(lib, kind, signal):
    T, n, M = 600, 160, 960            # a 1 % drift needs some 400 steps to fill the buffer past a frame plus the effective size
    _, model = walk(scenario(kind, T), inputs(signal, T, n), n, M)
    if kind in ("fast", "random"):
        assert model["shrinks"] > 0, "the scenario never reached the shrink"
    if kind in ("slow", "hungry"):
        assert model["underruns"] > 0
    if signal in ("zero", "const") and model["shrinks"]:
        assert model["shrunk"] == 40 * model["shrinks"], "every lag ties: the smallest wins"


@pytest.mark.parametrize("n", SIZES)
def test_every_frame_size_and_maximum(lib, n):
    for M in maxima(n):
        T = max(60, 2600 // n)
        for kind in ("fast", "random", "bursts"):
            walk(scenario(kind, T, seed=n), inputs("speech", T, n, seed=1), n, M)


def test_small_maximum_drops_and_never_shrinks(lib):
    """n = 24, M = 48: len never reaches the window, so every overflow is a drop"""
    T, n, M = 130, 24, 48
    _, model = walk(scenario("random", T), inputs("speech", T, n), n, M)
    assert model["shrinks"] == 0 and model["dropped"] > 0


def test_garbage_state_stays_in_bounds(lib):
    rng = np.random.default_rng(7)
    for i in range(12):
        rec = np.frombuffer(rng.integers(0, 256, capi.DBUF_STATE.itemsize, dtype=np.uint8).tobytes(), capi.DBUF_STATE).copy().reshape(())
        n, M = ((160, 960), (24, 48), (256, 1024), (1, 2))[i % 4]
        reserved0, reserved = int(rec["reserved0"]), rec["reserved"].copy()
        model = dm.from_record(rec)
        dm.read(model, M)
        assert model["len"] <= M and model["head"] < 1024 and 0 < model["eff"] <= M and model["last_op"] in (0, 1, 2) and model["since"] < 200
        rec, _ = walk(scenario("random", 40, seed=i), inputs("speech", 40, n, seed=i), n, M, rec=rec, model=dm.from_record(rec))
        assert int(rec["reserved0"]) == reserved0 and np.array_equal(rec["reserved"], reserved), "reserved fields stay as they are"


def test_op_zero_only_normalises(lib):
    rec = np.zeros((), capi.DBUF_STATE)
    rec["head"], rec["len"], rec["last_op"], rec["since"] = 5000, 2000, 9, 60000
    out, flag = capi.dbuf_step(rec, 0, 160, 960)
    assert out is None and flag == dm.IDLE
    assert (int(rec["head"]), int(rec["len"]), int(rec["eff"]), int(rec["last_op"]), int(rec["since"])) == ((5000 % 1024 + 1040) % 1024, 960, 480, 0, 199)


def test_chaining_splits(lib):
    """the same steps in one walk and in pieces with the record copied between them (a launch boundary reads the state again)"""
    T, n, M = 200, 160, 480
    ops, x = scenario("random", T, seed=3), inputs("speech", T, n, seed=3)
    whole, _ = walk(ops, x, n, M)
    for cuts in ((1,), (3, 127), (50, 51, 52, 199)):
        rec = np.zeros((), capi.DBUF_STATE)
        for a, b in zip((0,) + cuts, cuts + (T,)):
            rec, _ = walk(ops[a:b], x[a:b], n, M, rec=rec.copy())
        assert_same_state(rec, dm.from_record(whole))


# ---- properties of the model itself
def test_model_len_never_exceeds_the_maximum():
    for n, M in ((160, 320), (160, 960), (24, 48), (80, 1024)):
        st = dm.new_state()
        ops, x = scenario("random", 300, seed=n), inputs("speech", 300, n)
        for t in range(300):
            dm.step(st, int(ops[t]), x[t], n, M)
            assert st["len"] <= M


def test_model_shrink_drops_one_period_and_keeps_the_front():
    rng = np.random.default_rng(5)
    for f0, want in ((100.0, 80), (8000.0 / 65.0, 65), (70.0, 114)):      # periods whose multiples lie outside 40 .. 120
        st = dm.read(dm.new_state(), 1024)
        x = dm.speech(rng, 4, 160, f0)
        for t in range(4):
            dm.put(st, x[t], 160, 1024)
        st["shrinks"] = 0
        before, ln = dm.live(st), st["len"]
        p = dm.shrink(st)
        assert 40 <= p <= 120 and abs(p - want) <= 1, (f0, p)
        assert st["len"] == ln - p and st["shrinks"] == 1 and st["shrunk"] == p
        after = dm.live(st)
        np.testing.assert_array_equal(after[:ln - 2 * p], before[:ln - 2 * p])     # in front of the blended region: untouched
        # the blend starts near the older period and ends near the newer one
        assert abs(int(after[ln - 2 * p]) - int(before[ln - 2 * p])) <= abs(int(before[ln - p]) - int(before[ln - 2 * p])) // p + 1
        assert abs(int(after[-1]) - int(before[-1])) <= abs(int(before[-1]) - int(before[-1 - p])) // p + 1


def test_model_ties_take_the_smallest_lag_and_extremes_stay_in_range():
    assert dm.pitch(np.zeros(280, np.int64)) == 40 and dm.pitch(np.full(280, 777, np.int64)) == 40
    st = dm.read(dm.new_state(), 1024)
    x = dm.square(4, 160)
    for t in range(4):
        dm.put(st, x[t], 160, 1024)
    dm.shrink(st)
    assert dm.live(st).min() >= -32768 and dm.live(st).max() <= 32767


# ---- layout, arguments, binding
def test_state_layout():
    class St(ctypes.Structure):
        _fields_ = [("ring", ctypes.c_int16 * 1024)] + [(k, ctypes.c_uint16) for k in ("head", "len", "eff", "level", "max_level", "since", "last_op",
                                                                                       "reserved0")] + \
                   [(k, ctypes.c_uint32) for k in ("underruns", "shrinks", "shrunk", "dropped", "puts", "gets")] + [("reserved", ctypes.c_uint32 * 6)]

    assert ctypes.sizeof(St) == capi.DBUF_STATE.itemsize == 2112 and capi.DBUF_STATE.alignment == 4
    for name, _ in St._fields_:
        assert getattr(St, name).offset == capi.DBUF_STATE.fields[name][1], name
    hdr = open(os.path.join(ROOT, "include", "igdsp.h")).read()
    for name, val in (("IGDSP_DBUF_CAP", capi.DBUF_CAP), ("IGDSP_DBUF_WIN", capi.DBUF_WIN), ("IGDSP_DBUF_RECALC", capi.DBUF_RECALC),
                      ("IGDSP_DBUF_PUT", capi.DBUF_PUT), ("IGDSP_DBUF_GET", capi.DBUF_GET)):
        m = re.search(rf"#define\s+{name}\s+(\w+)", hdr)
        assert m and int(m.group(1), 0) == val, name
    assert (dm.CAP, dm.WIN, dm.RECALC, dm.PUT, dm.GET) == (capi.DBUF_CAP, capi.DBUF_WIN, capi.DBUF_RECALC, capi.DBUF_PUT, capi.DBUF_GET)
    assert (dm.IDLE, dm.PLAYED, dm.LOST) == (capi.JB_IDLE, capi.JB_PLAYED, capi.JB_LOST)


def test_step_einval(lib):
    st = np.zeros((), capi.DBUF_STATE)
    sp, x, out = st.ctypes.data_as(ctypes.c_void_p), np.zeros(256, np.int16), np.zeros(256, np.int16)
    xp, op_ = x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    f = lib.igdsp_dbuf_step
    assert f(sp, 3, xp, 160, 960, op_, None) == 0
    for args in ((None, 3, xp, 160, 960, op_, None), (sp, 4, xp, 160, 960, op_, None), (sp, 3, xp, 0, 960, op_, None),
                 (sp, 3, xp, 257, 1024, op_, None), (sp, 3, xp, 160, 319, op_, None), (sp, 3, xp, 160, 1025, op_, None),
                 (sp, 1, None, 160, 960, op_, None), (sp, 3, None, 160, 960, op_, None), (sp, 2, xp, 160, 960, None, None)):
        assert f(*args) == EINVAL, args
    assert f(sp, 1, xp, 160, 960, None, None) == 0 and f(sp, 2, None, 160, 960, op_, None) == 0 and f(sp, 0, None, 160, 320, None, None) == 0
    assert f(sp, 3, xp, 256, 512, op_, None) == 0 and f(sp, 3, xp, 1, 2, op_, None) == 0


def _param_types(text, name):
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = re.findall(rf"^\s*int\s+{name}\s*\(([^)]*)\)", text, flags=re.M)
    assert len(found) == 1, (name, len(found))
    types = []
    for p in found[0].split(","):
        m = re.fullmatch(r"\s*(.*?)\s*\b[A-Za-z_]\w*\s*", p, flags=re.S)
        types.append(re.sub(r"\s*\*\s*", " *", " ".join(m.group(1).split())))
    return types


def test_yardstick_binding_is_its_twins():
    """igdsp_internal_dbuf_move takes the arguments of igdsp_dbuf_run: its definition's parameter types equal the header's, its row of
    capi.INTERNAL_MORE is that list, capi.internal finds it, and it stays out of capi.INTERNAL"""
    hdr = _param_types(open(os.path.join(ROOT, "include", "igdsp.h")).read(), "igdsp_dbuf_run")
    src = _param_types(open(os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc", "igdsp_capi_dbuf.hip")).read(), "igdsp_internal_dbuf_move")
    assert src == hdr and len(hdr) == 14
    res, args = capi.INTERNAL_MORE["igdsp_internal_dbuf_move"]
    ctype = lambda t: ctypes.c_void_p if t.endswith("*") else {"uint32_t": ctypes.c_uint32}[t]
    assert res is ctypes.c_int and list(args) == [ctype(t) for t in hdr]
    assert "igdsp_internal_dbuf_move" not in capi.INTERNAL and capi.INTERNAL_MORE_TWIN["igdsp_internal_dbuf_move"] == "igdsp_dbuf_run"
    igbuild.build()
    assert capi.internal("dbuf_move").argtypes == list(args) and capi.internal("igdsp_internal_rs_copy") is not None
    with pytest.raises(KeyError):
        capi.internal("igdsp_internal_dbuf_copy")
    text = open(os.path.join(ROOT, "tools", "dbuf_bench.py")).read()
    assert 'capi.internal("igdsp_internal_dbuf_move")' in text and ".argtypes" not in text


# ---- the host mirror
def test_host_delaybuf(lib):
    H = ctypes.CDLL(igbuild.HOST_LIB)
    vp, i, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    for name, res, args in (("igdsp_host_dbuf_new", vp, [u, u]), ("igdsp_host_dbuf_free", None, [vp]), ("igdsp_host_dbuf_put", i, [vp, vp]),
                            ("igdsp_host_dbuf_get", i, [vp, vp]), ("igdsp_host_dbuf_fill", i, [vp]), ("igdsp_host_dbuf_state", i, [vp, vp])):
        getattr(H, name).restype = res
        getattr(H, name).argtypes = args
    T, n, M = 600, 160, 960
    ops, x = scenario("fast", T), inputs("speech", T, n)
    d = H.igdsp_host_dbuf_new(n, M)
    assert d
    try:
        model, out = dm.new_state(), np.zeros(n, np.int16)
        for t in range(T):
            if ops[t] & 1:
                assert H.igdsp_host_dbuf_put(d, x[t].ctypes.data) == 0
                dm.step(model, dm.PUT, x[t], n, M)
            if ops[t] & 2:
                want, flag = dm.step(model, dm.GET, None, n, M)
                assert H.igdsp_host_dbuf_get(d, out.ctypes.data) == flag
                np.testing.assert_array_equal(out, want)
            assert H.igdsp_host_dbuf_fill(d) == model["len"]
        assert model["shrinks"] > 0
        rec = np.zeros((), capi.DBUF_STATE)
        assert H.igdsp_host_dbuf_state(d, rec.ctypes.data) == 0
        assert_same_state(rec, model)
        assert H.igdsp_host_dbuf_put(d, None) == EINVAL and H.igdsp_host_dbuf_get(d, None) == EINVAL and H.igdsp_host_dbuf_fill(None) == EINVAL
    finally:
        H.igdsp_host_dbuf_free(d)
    for bad in ((0, 960), (257, 1024), (160, 319), (160, 1025)):
        assert not H.igdsp_host_dbuf_new(*bad)
