"""-m gpu: igdsp_dbuf_run (include/igdsp.h, "Delay buffer") against tests/dbuf_model.py through the C ABI: rows, flags, lengths, fills,
sumsq, peak, record flags, the state's scalars and its live samples bit for bit, rms at 1e-5 relative against float64.  Shapes around
the kernel's ownership units (a wave owns a channel, a block four; a part is 128 steps): steady, random ops that shrink, drop and
underrun at three maxima, the inputs whose lags all tie and the full-scale square beside speech, every frame size, one launch against
split launches, a garbage state, the footprint, the argument clauses and the compute-free yardstick."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import dbuf_model as dm  # noqa: E402
from tests import gpu_util as gu  # noqa: E402

GUARD = 256
EINVAL, ERANGE = -22, -34
SB = capi.DBUF_STATE.itemsize


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def run_dbuf(ctx, ops, x, n, M, state=None, optional=True, fill=0xEE, entry=None, raw=None, d_state=None):
    """One launch through the C ABI (entry: through that yardstick instead; fill: the byte the outputs and their guards hold before the
    launch; raw: a dict that takes the whole output buffers' bytes after it).  ops [T][C], x [T][C][n] int16, state [C] DBUF_STATE or
    None (reset), or d_state: a device tensor carried from an earlier launch.  Returns a dict of the outputs as laid out, the state
    records and the state tensor."""
    torch = gu.torch_cuda()
    T, C_ = ops.shape
    d_ops, d_in = gu.to_dev(np.asarray(ops, np.uint8)), gu.to_dev(np.asarray(x, "<i2"))
    if d_state is None:
        d_state = gu.to_dev(np.zeros(C_, capi.DBUF_STATE) if state is None else state)
    sizes = dict(out=T * C_ * n * 2, flags=T * C_, length=T * C_ * 2, fill=T * C_ * 2, stats=T * C_ * 16)
    bufs = {k: gu.dev_zeros(v + GUARD, fill) for k, v in sizes.items() if optional or k == "out"}
    fn = capi.internal(entry) if entry else None
    p = lambda k: bufs[k].data_ptr() if k in bufs else None
    if fn:
        rc = fn(ctx.h, d_ops.data_ptr(), d_in.data_ptr(), C_, T, n, M, d_state.data_ptr(), p("out"), p("flags"), p("length"), p("fill"), p("stats"), None)
        assert rc == 0, rc
    else:
        ctx.dbuf_run(d_ops, d_in, d_state, C_, T, n, M, bufs["out"], flags=bufs.get("flags"), length=bufs.get("length"), fill=bufs.get("fill"),
                     stats=bufs.get("stats"))
    torch.cuda.synchronize()
    host = {k: t.cpu().numpy() for k, t in bufs.items()}
    for k, b in host.items():
        assert np.all(b[sizes[k]:] == fill), f"bytes after d_{k} written"
    res = dict(out=host["out"][:sizes["out"]].view("<i2").reshape(T, C_, n), d_state=d_state,
               state=d_state.cpu().numpy().view(capi.DBUF_STATE).copy())
    if optional:
        res.update(flags=host["flags"][:sizes["flags"]].reshape(T, C_), length=host["length"][:sizes["length"]].view("<u2").reshape(T, C_),
                   fill=host["fill"][:sizes["fill"]].view("<u2").reshape(T, C_),
                   stats=host["stats"][:sizes["stats"]].view(capi.FRAME_STATS).reshape(T, C_))
    if raw is not None:
        raw.update(host)
        raw["state"] = d_state.cpu().numpy()
    return res


def model_run(ops, x, n, M, state=None):
    C_ = ops.shape[1]
    states = [dm.new_state() if state is None else dm.from_record(state[c]) for c in range(C_)]
    want = dm.run(states, ops, x, n, M)
    want["states"] = states
    return want


def assert_equal(got, want, n, fill_byte=0xEE):
    T, C_ = want["got"].shape
    live_rows = want["got"]
    np.testing.assert_array_equal(got["out"][live_rows], want["out"][live_rows])
    assert np.all(got["out"][~live_rows].view(np.uint8) == fill_byte), "a row of a step without a GET was written"
    if "flags" in got:
        np.testing.assert_array_equal(got["flags"], want["flags"])
        np.testing.assert_array_equal(got["length"], want["length"])
        np.testing.assert_array_equal(got["fill"], want["fill"])
        gu.assert_stats_equal(got["stats"], want["stats"], n=np.where(want["got"], n, 0))
    for c in range(C_):
        g = dm.from_record(got["state"][c])
        assert dm.scalars(g) == dm.scalars(want["states"][c]), c
        np.testing.assert_array_equal(dm.live(g), dm.live(want["states"][c]), err_msg=f"channel {c}")


def speech_rows(seed, T, C_, n):
    rng = np.random.default_rng(seed)
    return np.stack([dm.speech(rng, T, n, 72.0 + 113.0 * rng.random()) for _ in range(C_)], axis=1)


def random_ops(seed, T, C_, p_put, p_get):
    rng = np.random.default_rng(seed)
    return ((rng.random((T, C_)) < p_put) * 1 + (rng.random((T, C_)) < p_get) * 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def random_case(M, p_put=0.95, p_get=0.80):
    """test 2's launch and its model result, computed once and shared (nobody changes it)"""
    T, C_, n = 130, 67, 160
    ops, x = random_ops(11, T, C_, p_put, p_get), speech_rows(12, T, C_, n)
    return ops, x, n, model_run(ops, x, n, M)


# ---- 1. steady
def test_steady(ctx):
    T, C_, n, M = 9, 67, 160, 960
    ops, x = np.full((T, C_), 3, np.uint8), speech_rows(1, T, C_, n)
    want = model_run(ops, x, n, M)
    assert (want["flags"] == dm.PLAYED).all() and (want["fill"] == 0).all()
    np.testing.assert_array_equal(want["out"], x)                         # PUT then GET on an empty buffer: the row passes through
    assert_equal(run_dbuf(ctx, ops, x, n, M), want, n)
    # one PUT of delay ahead: the rows come out a step late
    ops2 = np.vstack([np.full((1, C_), 1, np.uint8), ops[:-1]])
    want2 = model_run(ops2, x, n, M)
    np.testing.assert_array_equal(want2["out"][1:], x[:-1])
    assert_equal(run_dbuf(ctx, ops2, x, n, M), want2, n)


# ---- 2. random ops
@pytest.mark.parametrize("M", (960, 480, 320))
def test_random_ops(ctx, M):
    ops, x, n, want = random_case(M)
    shrinks = np.array([s["shrinks"] for s in want["states"]])
    assert (shrinks > 0).sum() * 2 >= len(shrinks), "at least half the channels shrink"
    assert any(s["dropped"] for s in want["states"]) and any(s["underruns"] for s in want["states"])
    assert_equal(run_dbuf(ctx, ops, x, n, M), want, n)


def test_hungry_consumer(ctx):
    ops, x, n, want = random_case(960, 0.80, 0.95)
    assert all(s["underruns"] for s in want["states"]) and not any(s["shrinks"] for s in want["states"])
    assert_equal(run_dbuf(ctx, ops, x, n, 960), want, n)


# ---- 3. ties and extremes beside speech
def test_ties_and_extremes(ctx):
    T, C_, n, M = 60, 19, 160, 480
    x = speech_rows(3, T, C_, n)
    x[:, 0], x[:, 1], x[:, 2] = 0, -12345, dm.square(T, n)
    x[:, 17] = 32767
    ops = random_ops(31, T, C_, 1.0, 0.8)
    want = model_run(ops, x, n, M)
    for c in (0, 1, 17):
        assert want["states"][c]["shrinks"] > 0 and want["states"][c]["shrunk"] == 40 * want["states"][c]["shrinks"], "every lag ties: p = 40"
    assert want["states"][2]["shrinks"] > 0
    assert_equal(run_dbuf(ctx, ops, x, n, M), want, n)


# ---- 4. frame sizes
@pytest.mark.parametrize("n", (1, 24, 80, 164, 256))
def test_frame_sizes(ctx, n):
    T, C_ = 40, 33
    ops, x = random_ops(40 + n, T, C_, 0.95, 0.80), speech_rows(41, T, C_, n)
    for M in (2 * n, 1024):
        want = model_run(ops, x, n, M)
        if (n, M) == (24, 48):
            assert not any(s["shrinks"] for s in want["states"]) and all(s["dropped"] for s in want["states"]), "len never reaches 280"
        assert_equal(run_dbuf(ctx, ops, x, n, M), want, n)


def test_odd_frame_and_shifted_buffers(ctx):
    """the general form: an odd n; and the vector form after shrinks by odd periods (ring positions of either parity)"""
    T, C_, n, M = 70, 9, 255, 1020
    ops, x = random_ops(51, T, C_, 1.0, 0.7), speech_rows(52, T, C_, n)
    want = model_run(ops, x, n, M)
    assert any(s["shrinks"] for s in want["states"])
    assert_equal(run_dbuf(ctx, ops, x, n, M), want, n)
    _, _, _, w960 = random_case(960)
    assert any(s["shrunk"] % 2 for s in w960["states"]) and any(s["shrunk"] % 2 == 0 and s["shrinks"] for s in w960["states"])


# ---- 5. chaining
def test_chaining(ctx):
    ops, x, n, want = random_case(960)
    T = ops.shape[0]
    whole = run_dbuf(ctx, ops, x, n, 960)
    assert_equal(whole, want, n)
    for cuts in (tuple(range(1, T)), (3,)):
        parts, d_state = [], None
        for a, b in zip((0,) + cuts, cuts + (T,)):
            r = run_dbuf(ctx, ops[a:b], x[a:b], n, 960, d_state=d_state)
            d_state = r["d_state"]
            parts.append(r)
        got = {k: np.concatenate([p[k] for p in parts]) for k in ("out", "flags", "length", "fill", "stats")}
        got["state"] = parts[-1]["state"]
        assert_equal(got, want, n)
        for k in ("out", "flags", "length", "fill"):
            np.testing.assert_array_equal(got[k], whole[k])
        for f in ("sumsq", "rms", "peak", "flags"):
            np.testing.assert_array_equal(got["stats"][f], whole["stats"][f])


# ---- 6. garbage state
def test_garbage_state(ctx):
    T, C_, n, M = 20, 67, 160, 960
    rng = np.random.default_rng(6)
    state = np.frombuffer(rng.integers(0, 256, C_ * SB, dtype=np.uint8).tobytes(), capi.DBUF_STATE).copy()
    ops, x = random_ops(61, T, C_, 0.95, 0.8), speech_rows(62, T, C_, n)
    got = run_dbuf(ctx, ops, x, n, M, state=state)
    assert_equal(got, model_run(ops, x, n, M, state=state), n)
    assert np.array_equal(got["state"]["reserved0"], state["reserved0"]) and np.array_equal(got["state"]["reserved"], state["reserved"])


# ---- 7. footprint
def test_footprint(ctx):
    T, C_, n, M = 12, 21, 160, 480
    ops, x = random_ops(71, T, C_, 0.8, 0.7), speech_rows(72, T, C_, n)
    want = model_run(ops, x, n, M)

    def launch(fill, xin=x, optional=True):
        raw = {}
        run_dbuf(ctx, ops, xin, n, M, optional=optional, fill=fill, raw=raw)
        raw.pop("state")
        return raw

    mask = gu.written_mask(launch)
    out_mask = mask["out"][:T * C_ * n * 2].reshape(T, C_, n * 2)
    assert out_mask[want["got"]].all() and not out_mask[~want["got"]].any(), "exactly the rows of GET steps"
    for k, item in (("flags", 1), ("length", 2), ("fill", 2), ("stats", 16)):
        assert mask[k][:T * C_ * item].all() and not mask[k][T * C_ * item:].any(), k
    assert not mask["out"][T * C_ * n * 2:].any()
    # optional outputs left NULL: the rows are the same
    bare = run_dbuf(ctx, ops, x, n, M, optional=False)
    full = run_dbuf(ctx, ops, x, n, M)
    np.testing.assert_array_equal(bare["out"], full["out"])
    assert bare["state"].tobytes() == full["state"].tobytes()
    # rows of d_in whose step has no PUT are never read
    poisoned = x.copy()
    poisoned[(ops & 1) == 0] = -21555
    again = run_dbuf(ctx, ops, poisoned, n, M)
    for k in ("out", "flags", "length", "fill"):
        np.testing.assert_array_equal(again[k], full[k])
    assert again["stats"].tobytes() == full["stats"].tobytes() and again["state"].tobytes() == full["state"].tobytes()


# ---- 8. clauses
def test_argument_errors(ctx):
    L = capi.load()
    C_, T, n = 4, 2, 160
    d_state = gu.dev_zeros(C_ * SB + 64)
    d_ops, d_in = gu.dev_zeros(64), gu.dev_zeros(T * C_ * n * 2 + 64)
    d_out, d_fl, d_ln, d_fi, d_st = (gu.dev_zeros(k + 64, 0xEE) for k in (T * C_ * n * 2, T * C_, T * C_ * 2, T * C_ * 2, T * C_ * 16))
    ops, inp, stt, out, fl, ln, fi, st = (t.data_ptr() for t in (d_ops, d_in, d_state, d_out, d_fl, d_ln, d_fi, d_st))

    def call(ops_=ops, in_=inp, C=C_, T_=T, n_=n, M=960, state=stt, out_=out, fl_=fl, ln_=ln, fi_=fi, st_=st, h=ctx.h):
        return L.igdsp_dbuf_run(h, ops_, in_, C, T_, n_, M, state, out_, fl_, ln_, fi_, st_, None)

    assert call(h=None) == EINVAL
    for kw in (dict(n_=0), dict(n_=257, M=1024), dict(M=319), dict(M=1025)):                       # checked even with nothing to do
        assert call(**kw) == EINVAL and call(C=0, **kw) == EINVAL, kw
    assert call(C=0, ops_=None, in_=None, state=None, out_=None) == 0 and call(T_=0, out_=inp, fi_=fi + 1) == 0   # nothing to do comes next
    for kw in (dict(ops_=None), dict(in_=None), dict(state=None), dict(out_=None), dict(in_=inp + 1), dict(out_=out + 1), dict(ln_=ln + 1),
               dict(fi_=fi + 1), dict(state=stt + 2), dict(st_=st + 4), dict(out_=inp), dict(out_=inp + 2), dict(out_=stt + SB), dict(fl_=ops + 7),
               dict(st_=stt), dict(ln_=fi), dict(ln_=fi + 14), dict(fl_=out + 100)):
        assert call(**kw) == EINVAL, kw
    assert call(C=0x10000000, T_=16) == ERANGE and call(C=0x10000000, T_=16, n_=0) == EINVAL and call(C=0x10000000, T_=16, out_=out + 1) == ERANGE
    assert call(out_=inp + 2) == EINVAL and b"an output must not overlap an input or the state" in (L.igdsp_last_error(ctx.h) or b"")
    assert call(ln_=fi + 14) == EINVAL and b"two outputs must not overlap" in (L.igdsp_last_error(ctx.h) or b"")
    gu.torch_cuda().cuda.synchronize()
    for t in (d_out, d_fl, d_ln, d_fi, d_st):
        assert (t.cpu().numpy() == 0xEE).all()                                                   # nothing written
    assert not d_state.cpu().numpy().any()
    assert call() == 0 and call(fl_=None, ln_=None, fi_=None, st_=None) == 0 and call(n_=1, M=2) == 0 and call(n_=256, M=512, C=2, T_=1) == 0
    gu.torch_cuda().cuda.synchronize()


# ---- 9. yardstick
def test_yardstick_footprint_and_rules(ctx):
    """igdsp_internal_dbuf_move stores exactly the bytes igdsp_dbuf_run stores for an all-PUT|GET launch at a fill of n, and the rows it
    moves are that launch's rows; it rejects what its twin rejects"""
    T, C_, n, M = 3, 21, 160, 960
    ops, x = np.full((T, C_), 3, np.uint8), speech_rows(91, T + 1, C_, n)

    def start(fill):
        st = np.zeros(C_, capi.DBUF_STATE)
        st.view(np.uint8)[:] = fill                        # the ring outside the live samples and the reserved fields
        for k in dm.SCALARS + dm.COUNTERS:
            st[k] = 0
        st["head"], st["len"], st["eff"], st["last_op"], st["level"] = 100, n, 480, 1, 1
        for c in range(C_):
            st["ring"][c][(100 + np.arange(n)) % 1024] = x[T, c]
        return st

    def launch(entry):
        def go(fill):
            raw = {}
            res = run_dbuf(ctx, ops, x[:T], n, M, state=start(fill), fill=fill, entry=entry, raw=raw)
            go.res = res
            return raw
        return go

    real, yard = launch(None), launch("igdsp_internal_dbuf_move")
    gu.assert_same_footprint(gu.written_mask(yard), gu.written_mask(real))
    for k in ("out", "flags", "length", "fill"):
        np.testing.assert_array_equal(yard.res[k], real.res[k])
    np.testing.assert_array_equal(real.res["out"][0], x[T])                    # the delayed rows
    np.testing.assert_array_equal(real.res["out"][1:], x[:T - 1])
    assert (yard.res["stats"]["sumsq"] == 0).all() and (yard.res["stats"]["peak"] == 0).all()
    np.testing.assert_array_equal(yard.res["state"]["len"], real.res["state"]["len"])
    np.testing.assert_array_equal(yard.res["state"]["head"], real.res["state"]["head"])

    fn = capi.internal("dbuf_move")
    d_state, d_in, d_out = gu.dev_zeros(4 * SB, 0xEE), gu.dev_zeros(2 * 4 * 320 + 64), gu.dev_zeros(2 * 4 * 320 + 64, 0xEE)
    d_ops = gu.dev_zeros(64)
    stt, inp, out, op = (t.data_ptr() for t in (d_state, d_in, d_out, d_ops))

    def call(ops_=op, in_=inp, C=4, T_=2, n_=160, M_=960, state=stt, out_=out, h=ctx.h):
        return fn(h, ops_, in_, C, T_, n_, M_, state, out_, None, None, None, None, None)

    for kw in (dict(h=None), dict(n_=0), dict(M_=319), dict(ops_=None), dict(in_=None), dict(state=None), dict(out_=None), dict(out_=out + 1),
               dict(out_=inp), dict(state=stt + 2)):
        assert call(**kw) == EINVAL, kw
    assert call(C=0x10000000, T_=16) == ERANGE
    gu.torch_cuda().cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xEE).all() and (d_state.cpu().numpy() == 0xEE).all()
