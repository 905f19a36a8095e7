"""-m gpu: igdsp_plc_conceal (include/igdsp.h, "Packet loss concealment") bit for bit against tests/plc_model.py — out, len_out, the
records and the final state bytes: a fuzz over channel counts, frame sizes, tick counts and the three input forms with random loss,
bursts, IDLE spans, PLAYED ticks of len 0 and short len; split launches and runs that cross launches; a garbage state; guard bytes;
arguments; two streams at once; the chain igdsp_jb_receive -> igdsp_plc_conceal -> igdsp_conf_mix; and the full 65 536 x 128 shape,
lossless (identical to igdsp_decode_meter's PCM) and lossy (a sample of channels against the model)."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import conf_model as cm  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import plc_model as pm  # noqa: E402

GUARD = 256
SB = capi.PLC_STATE.itemsize


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def _guarded(nbytes, fill):
    return gu.dev_zeros(nbytes + GUARD, fill)


def _take(d, nbytes, fill, what):
    raw = d.cpu().numpy()
    assert np.all(raw[nbytes:] == fill), f"guard bytes after {what} written"
    return raw[:nbytes]


def ticks(rng, T, C_, n, loss=0.1):
    """tick flags [T][C] and len [T][C]: good spans, loss bursts of 1..30 ticks, IDLE spans, PLAYED with len 0, short len, odd flags"""
    fl = np.full((T, C_), pm.PLAYED, np.uint8)
    ln = np.full((T, C_), n, np.uint16)
    for c in range(C_):
        t = 0
        while t < T:
            r = rng.random()
            if r < loss:
                k = int(rng.integers(1, 31)) if rng.random() < 0.3 else int(rng.integers(1, 4))
                fl[t:t + k, c] = pm.LOST
            elif r < loss + 0.03:
                k = int(rng.integers(1, 8))
                fl[t:t + k, c] = pm.IDLE if rng.random() < 0.9 else int(rng.choice([0, 4, 200]))
            else:
                k = int(rng.integers(1, 12))
            t += k
    r = rng.random((T, C_))
    ln[(r < 0.03) & (fl == pm.PLAYED)] = 0
    short = (r > 0.97) & (fl == pm.PLAYED)
    ln[short] = rng.integers(1, n + 1, int(short.sum()))
    big = (r > 0.985) & (r <= 0.99)
    ln[big] = n + 7                                            # len past n: the whole row
    return fl, ln


def garbage_state(rng, C_):
    st = np.frombuffer(rng.integers(0, 256, C_ * SB, dtype=np.uint8).tobytes(), capi.PLC_STATE).copy()
    return st


class Inputs:
    def __init__(self, rng, T, C_, n, form):
        self.form = form
        self.codec = np.where(rng.random(C_) < 0.5, 8, 0).astype(np.uint8) if form == "mix" else np.full(C_, 8 if form == "alaw" else 0, np.uint8)
        if form == "pcm":
            self.pcm = rng.integers(-32768, 32768, (T, C_, n)).astype(np.int16)
            if T * C_ > 0:
                self.pcm.reshape(-1)[rng.integers(0, self.pcm.size, 8)] = -32768
            self.payload = None
        else:
            self.payload = rng.integers(0, 256, (T, C_, n), dtype=np.uint8)
            self.pcm = None

    def x(self, orc):
        return self.pcm.astype(np.int64) if self.pcm is not None else pm.decode(self.payload, self.codec, orc)

    def sl(self, a, b):
        s = Inputs.__new__(Inputs)
        s.form, s.codec = self.form, self.codec
        s.pcm = None if self.pcm is None else self.pcm[a:b]
        s.payload = None if self.payload is None else self.payload[a:b]
        return s


class Dev:
    """device state of C channels, carried across launches"""

    def __init__(self, C_, init=None):
        self.C = C_
        self.state = _guarded(C_ * SB, 0x77)
        self.state[:C_ * SB] = gu.to_dev(np.zeros(C_, capi.PLC_STATE) if init is None else init)

    def host(self):
        return _take(self.state, self.C * SB, 0x77, "d_state").view(capi.PLC_STATE)


def run_plc(ctx, dev, fl, ln, inp, n, stream=None, with_len=True, outs=True, entry=None, fill=None, raw=None):
    """one launch; entry: through that yardstick of capi.INTERNAL_TWIN instead; fill: the byte every output and its guard hold before
    the launch; raw: a dict that takes the whole output buffers' bytes after it"""
    torch = gu.torch_cuda()
    T, C_ = fl.shape
    fo, fl_, fs = (0xA5, 0x5A, 0x3C) if fill is None else (fill,) * 3
    d_out = _guarded(T * C_ * n * 2, fo)
    d_lo = _guarded(T * C_ * 2, fl_) if outs else None
    d_st = _guarded(T * C_ * 16, fs) if outs else None
    kw = dict(pcm=gu.to_dev(inp.pcm)) if inp.pcm is not None else dict(payload=gu.to_dev(inp.payload), codec=gu.to_dev(inp.codec))
    (ctx.via(entry) if entry else ctx).plc_conceal(gu.to_dev(fl), dev.state, d_out, C_, T, n,
                                                   length=gu.to_dev(np.asarray(ln, "<u2")) if with_len else None, len_out=d_lo, stats=d_st,
                                                   stream=stream, **kw)
    if stream is None:
        torch.cuda.synchronize()
    else:
        ctx.sync(stream)
    out = _take(d_out, T * C_ * n * 2, fo, "out").view("<i2").reshape(T, C_, n)
    lo = _take(d_lo, T * C_ * 2, fl_, "len_out").view("<u2").reshape(T, C_) if outs else None
    st = _take(d_st, T * C_ * 16, fs, "stats").view(capi.FRAME_STATS).reshape(T, C_) if outs else None
    if raw is not None:
        raw.update({k: t.cpu().numpy() for k, t in (("out", d_out), ("len_out", d_lo), ("stats", d_st)) if t is not None})
    return out, lo, st


def check(got, exp, n, dev=None):
    out, lo, st = got
    eo, elo, est, erec = exp
    if not np.array_equal(out, eo):
        bad = np.argwhere(out != eo)
        raise AssertionError(f"out differs at {bad[:5].tolist()} ({len(bad)} samples): got {out[tuple(bad[0])]} exp {eo[tuple(bad[0])]}")
    if lo is not None:
        assert np.array_equal(lo, elo)
        gu.assert_stats_equal(st, est)
    if dev is not None:
        assert dev.host().tobytes() == erec.tobytes(), "final state differs"


FUZZ = [(1, 160, 128, "ulaw"), (15, 24, 7, "alaw"), (16, 80, 128, "pcm"), (17, 164, 2, "mix"), (16, 1, 128, "ulaw"), (17, 256, 7, "pcm"),
        (1000, 160, 7, "mix"), (4099, 160, 2, "ulaw"), (1000, 256, 1, "pcm"), (15, 1, 2, "alaw"), (17, 80, 128, "mix"), (4099, 24, 1, "pcm"),
        (16, 164, 128, "alaw"), (1, 1, 1, "pcm"), (1000, 80, 2, "alaw")]


@pytest.mark.parametrize("C_,n,T,form", FUZZ, ids=[f"C{c}-n{n}-T{t}-{f}" for c, n, t, f in FUZZ])
def test_fuzz_vs_model(ctx, orc, C_, n, T, form):
    rng = np.random.default_rng(C_ * 7919 + n * 31 + T)
    fl, ln = ticks(rng, T, C_, n)
    inp = Inputs(rng, T, C_, n, form)
    init = None
    if C_ <= 1000:                                             # a state in the middle of things: runs, rings, cycles
        f0, l0 = ticks(rng, 40, C_, n, loss=0.3)
        init = pm.run(f0, rng.integers(-32768, 32768, (40, C_, n)), l0)[3]
    dev = Dev(C_, init)
    got = run_plc(ctx, dev, fl, ln, inp, n)
    exp = pm.run(fl, inp.x(orc), ln, init)
    check(got, exp, n, dev)
    if C_ >= 1000 and T >= 2:
        assert (exp[2]["flags"] & pm.FLAG_CONCEALED).any() and (exp[1] == 0).any()


def test_split_launches_identical(ctx, orc):
    """T launches of one tick (and uneven splits, runs crossing every boundary) == one launch of T ticks; 300 ticks cross the 128-tick
    parts of a single launch"""
    rng = np.random.default_rng(5)
    C_, T, n = 33, 300, 160
    fl, ln = ticks(rng, T, C_, n, loss=0.2)
    inp = Inputs(rng, T, C_, n, "mix")
    exp = pm.run(fl, inp.x(orc), ln)
    one = Dev(C_)
    check(run_plc(ctx, one, fl, ln, inp, n), exp, n, one)
    for cuts in ([1] * 40 + [260], [3, 129, 1, 7, 160]):
        dev = Dev(C_)
        t0, outs = 0, []
        for k in cuts:
            outs.append(run_plc(ctx, dev, fl[t0:t0 + k], ln[t0:t0 + k], inp.sl(t0, t0 + k), n))
            t0 += k
        assert t0 == T
        got = tuple(np.concatenate([o[i] for o in outs]) for i in range(3))
        check(got, exp, n, dev)


def test_garbage_state_stays_in_bounds(ctx, orc):
    rng = np.random.default_rng(9)
    C_, T, n = 64, 20, 160
    init = garbage_state(rng, C_)
    init["missing"][::2] = rng.integers(1, 65535, C_ // 2)
    fl, ln = ticks(rng, T, C_, n, loss=0.3)
    inp = Inputs(rng, T, C_, n, "pcm")
    dev = Dev(C_, init)
    got = run_plc(ctx, dev, fl, ln, inp, n)
    check(got, pm.run(fl, inp.x(orc), ln, init), n, dev)
    h = dev.host()
    assert np.all(h["head"] < pm.HIST) and np.all((h["pitch"] >= pm.PMIN) & (h["pitch"] <= pm.PMAX)) and np.all(h["pos"] < h["pitch"])
    assert h["reserved"].tobytes() == init["reserved"].tobytes()


def test_optional_outputs_and_no_len(ctx, orc):
    rng = np.random.default_rng(4)
    C_, T, n = 20, 9, 80
    fl, ln = ticks(rng, T, C_, n, loss=0.3)
    inp = Inputs(rng, T, C_, n, "ulaw")
    dev = Dev(C_)
    out, _, _ = run_plc(ctx, dev, fl, ln, inp, n, with_len=False, outs=False)
    exp = pm.run(fl, inp.x(orc), None)
    assert np.array_equal(out, exp[0]) and dev.host().tobytes() == exp[3].tobytes()


def test_arguments(ctx):
    torch = gu.torch_cuda()
    C_, T, n = 4, 2, 160
    fl, pl, cd = gu.dev_zeros(T * C_), gu.dev_zeros(T * C_ * n), gu.dev_zeros(C_)
    pcm, st, out = gu.dev_zeros(T * C_ * n * 2), gu.dev_zeros(C_ * SB), gu.dev_zeros(T * C_ * n * 2)
    L, h = capi.load(), ctx.h
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def call(fl_=fl, payload=pl, codec=cd, pcm_=None, C=C_, T_=T, n_=n, st_=st, out_=out, lo=None, stats=None):
        return L.igdsp_plc_conceal(h, p(fl_), p(payload), p(codec), p(pcm_), None, C, T_, n_, p(st_), p(out_), p(lo), p(stats), None)

    E = -22
    assert call() == 0
    assert call(fl_=None) == E and call(st_=None) == E and call(out_=None) == E
    assert call(pcm_=pcm) == E                                 # both inputs
    assert call(payload=None) == E                             # neither
    assert call(codec=None) == E                               # payload without codec
    assert call(n_=0) == E and call(n_=257) == E
    assert call(payload=None, codec=None, pcm_=pcm) == 0
    assert call(C=0, fl_=None) == 0 and call(T_=0, n_=0) == 0 # nothing to do
    assert L.igdsp_plc_conceal(None, p(fl), p(pl), p(cd), None, None, C_, T, n, p(st), p(out), None, None, None) == E
    torch.cuda.synchronize()


def test_two_streams(ctx, orc):
    torch = gu.torch_cuda()
    rng = np.random.default_rng(12)
    C_, T, n = 300, 16, 160
    jobs = []
    for k in range(2):
        fl, ln = ticks(rng, T, C_, n, loss=0.2)
        inp = Inputs(rng, T, C_, n, ("ulaw", "pcm")[k])
        jobs.append((fl, ln, inp, Dev(C_), torch.cuda.Stream()))
    res = [None, None]

    def work(k):
        fl, ln, inp, dev, s = jobs[k]
        res[k] = run_plc(ctx, dev, fl, ln, inp, n, stream=s.cuda_stream)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(2):
        fl, ln, inp, dev, _ = jobs[k]
        check(res[k], pm.run(fl, inp.x(orc), ln), n, dev)


def test_chain_jb_plc_conf(ctx, orc):
    """igdsp_jb_receive -> igdsp_plc_conceal(payload, len, tick flags) -> igdsp_conf_mix(d_pcm = out, d_len = len_out) against
    jb_model -> plc_model -> conf_model"""
    from tests import test_gpu_jb as tj

    torch = gu.torch_cuda()
    rng = np.random.default_rng(21)
    C_, T, S, n = 16, 60, 2, 160
    packets, sizes, radio, arrival = tj.simulate(rng, C_, T, S, radio=np.ones(C_, np.uint8))
    jd = tj.Dev(C_)
    pay, ln, _, fl, _ = tj.run_jb(ctx, jd, packets, sizes, radio, S, 3, arrival)
    epay, eln, _, efl, _, _ = tj.expect(orc, packets, sizes, radio, S, 3, arrival=arrival)
    assert np.array_equal(pay, epay) and np.array_equal(ln, eln) and np.array_equal(fl, efl)
    assert set(np.unique(efl)) >= {pm.PLAYED, pm.LOST}
    codec = np.full(C_, 8, np.uint8)
    inp = Inputs.__new__(Inputs)
    inp.form, inp.codec, inp.pcm, inp.payload = "alaw", codec, None, pay
    dev = Dev(C_)
    out, lo, st = run_plc(ctx, dev, fl, ln, inp, n)
    eo, elo, est, erec = pm.run(efl, pm.decode(epay, codec, orc), eln)
    check((out, lo, st), (eo, elo, est, erec), n, dev)
    gain = np.full(C_, 128, np.uint16)
    ptr, mem = np.array([0, 8, 16], np.uint32), np.arange(C_, dtype=np.uint32)
    d_mix = gu.dev_zeros(T * 2 * n * 2)
    s = torch.cuda.current_stream().cuda_stream
    ctx.conf_mix(gu.to_dev(gain), gu.to_dev(ptr), gu.to_dev(mem), C_, C_, 2, T, n, out=d_mix, pcm=gu.to_dev(out), length=gu.to_dev(lo),
                 stream=s)
    torch.cuda.synchronize()
    mix, _ = cm.mix(eo.astype(np.int64), gain, ptr, mem, C_, 2, elo)
    assert np.array_equal(d_mix.cpu().numpy().view("<i2").reshape(T, 2, n), mix)


def _full(ctx, fl, pl, codec, n, st_dev):
    torch = gu.torch_cuda()
    T, C_ = fl.shape[0], fl.shape[1]
    out = torch.empty(T * C_ * n, dtype=torch.int16, device="cuda")
    lo = torch.empty(T * C_, dtype=torch.int16, device="cuda")
    stats = torch.empty(T * C_ * 16, dtype=torch.uint8, device="cuda")
    ctx.plc_conceal(fl, st_dev, out, C_, T, n, payload=pl, codec=codec, len_out=lo, stats=stats, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out, lo, stats


def test_full_size_lossless_equals_decode_meter(ctx):
    """65 536 x 128 x 160, all PLAYED: out is igdsp_decode_meter's PCM bit for bit, len_out n, the ring the last 280 samples"""
    torch = gu.torch_cuda()
    C_, T, n = 65536, 128, 160
    g = torch.Generator(device="cuda").manual_seed(3)
    pl = torch.randint(0, 256, (T * C_ * n,), dtype=torch.uint8, device="cuda", generator=g)
    codec = (torch.arange(C_, device="cuda") % 3 == 0).to(torch.uint8) * 8
    fl = torch.full((T * C_,), pm.PLAYED, dtype=torch.uint8, device="cuda")
    st = torch.zeros(C_ * SB, dtype=torch.uint8, device="cuda")
    out, lo, stats = _full(ctx, fl.view(T, C_), pl, codec, n, st)
    ref = torch.empty(T * C_ * n, dtype=torch.int16, device="cuda")
    dst = torch.empty(T * C_ * 16, dtype=torch.uint8, device="cuda")
    ctx.decode_meter(pl, codec, C_, T, n, dst, pcm=ref, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert bool((lo == n).all())
    got = stats.view(torch.int64).view(T * C_, 2)[:, 0]
    exp = dst.view(torch.int64).view(T * C_, 2)[:, 0]
    assert torch.equal(got, exp)                                             # sumsq
    hs = st.view(torch.int16).view(C_, SB // 2)
    last = out.view(T, C_, n)[-2:].permute(1, 0, 2).reshape(C_, 2 * n)[:, -pm.HIST:]   # head = 128 * 160 % 280 = 40
    head = (T * n) % pm.HIST
    assert torch.equal(torch.roll(hs[:, :pm.HIST], -head, dims=1), last)
    del pl, out, ref, stats, dst
    torch.cuda.empty_cache()


def test_full_size_lossy_sample_vs_model(ctx, orc):
    """65 536 x 128 x 160 with loss and IDLE: 320 channels spread over the chip against the model (channels are independent)"""
    torch = gu.torch_cuda()
    C_, T, n = 65536, 128, 160
    rng = np.random.default_rng(77)
    g = torch.Generator(device="cuda").manual_seed(4)
    pl = torch.randint(0, 256, (T * C_ * n,), dtype=torch.uint8, device="cuda", generator=g)
    codec = (torch.arange(C_, device="cuda") % 2).to(torch.uint8) * 8
    r = torch.rand((T, C_), device="cuda", generator=g)
    fl = torch.where(r < 0.05, pm.LOST, torch.where(r < 0.06, pm.IDLE, pm.PLAYED)).to(torch.uint8)
    st = torch.zeros(C_ * SB, dtype=torch.uint8, device="cuda")
    out, lo, stats = _full(ctx, fl, pl, codec, n, st)
    pick = np.unique(np.concatenate([rng.choice(C_, 300, replace=False), [0, 15, 16, C_ - 1, C_ - 16, 4095, 4096]]))
    idx = torch.from_numpy(pick).cuda()
    p3 = pl.view(T, C_, n)[:, idx].cpu().numpy()
    fls = fl[:, idx].cpu().numpy()
    cd = codec[idx].cpu().numpy()
    eo, elo, est, erec = pm.run(fls, pm.decode(p3, cd, orc), None)
    assert np.array_equal(out.view(T, C_, n)[:, idx].cpu().numpy(), eo)
    assert np.array_equal(lo.view(T, C_)[:, idx].cpu().numpy().view("<u2"), elo)
    gu.assert_stats_equal(stats.view(T * C_, 16).view(T, C_, 16)[:, idx].cpu().numpy().reshape(-1).view(capi.FRAME_STATS).reshape(T, -1), est)
    assert st.view(C_, SB)[idx].cpu().numpy().tobytes() == erec.tobytes()
    assert (est["flags"] & pm.FLAG_CONCEALED).any()
    del pl, out, stats
    torch.cuda.empty_cache()


# ---- the compute-free yardstick (igdsp_internal_plc_copy, tools/plc_bench.py) against its promise in csrc/igdsp_capi.hip: "the same
# traversal with every tick taken as PLAIN: the input bits widened to the output, no decode, pitch search, synthesis or stats (the
# records carry only the length); the state's ring and scalars are written"

def _valid_state(rng, C_):
    st = garbage_state(rng, C_)
    st["head"], st["pitch"] = rng.integers(0, capi.PLC_HIST, C_), rng.integers(capi.PLC_PMIN, capi.PLC_PMAX + 1, C_)
    st["pos"], st["missing"] = st["pitch"] // 2, 0
    return st


@pytest.mark.parametrize("T", [3, 131])
@pytest.mark.parametrize("form", ["mix", "pcm"])
def test_yardstick_footprint_values_independence(ctx, form, T):
    """igdsp_internal_plc_copy, channel counts around the wave's, one part and two, every n of (160, 24, 13): on all-PLAIN tick flags
    it stores the bytes igdsp_plc_conceal stores in the rows, lengths and records; lossy flags and short lengths give the same bytes
    (every tick is taken as PLAIN); a row is the input code byte zero-extended or the input sample, a record that of n zeros, and the
    state's ring ends with the last 280 widened input samples behind the advanced head, the other scalars as they were"""
    from tests import record_model

    for n in (160, 24, 13):
        for C_ in (1, 15, 17, 65):
            rng = np.random.default_rng(700 + n + C_ + T)
            inp = Inputs(rng, T, C_, n, form)
            plain, full = np.full((T, C_), pm.PLAYED, np.uint8), np.full((T, C_), n, np.uint16)
            init = _valid_state(rng, C_)
            got = {}

            def launch(entry):
                def run(fill):
                    raw, dev = {}, Dev(C_, init)
                    got[entry, fill] = run_plc(ctx, dev, plain, full, inp, n, entry=entry, fill=fill, raw=raw), dev.host()
                    return raw
                return run

            yard, real = gu.written_mask(launch("plc_copy")), gu.written_mask(launch(None))
            assert all(real[k][:-GUARD].all() for k in real)
            gu.assert_same_footprint(yard, real)
            wide = inp.pcm if inp.pcm is not None else inp.payload.astype(np.int16)
            fl, ln = ticks(rng, T, C_, n, loss=0.3)
            dev = Dev(C_, init)
            lossy = run_plc(ctx, dev, fl, ln, inp, n, entry="plc_copy"), dev.host()
            exp_st = init.copy()
            x = wide.transpose(1, 0, 2).reshape(C_, T * n)
            for k in range(max(0, T * n - capi.PLC_HIST), T * n):
                exp_st["hist"][np.arange(C_), (init["head"].astype(np.int64) + k) % capi.PLC_HIST] = x[:, k]
            exp_st["head"] = (init["head"].astype(np.int64) + T * n) % capi.PLC_HIST
            for (out, lo, st), state in (got["plc_copy", gu.FILL_A], got["plc_copy", gu.FILL_B], lossy):
                np.testing.assert_array_equal(out, wide)
                assert (lo == n).all()
                gu.assert_stats_equal(st, record_model.records(np.zeros((T, C_, n), np.int64)))
                assert state.tobytes() == exp_st.tobytes(), [k for k in capi.PLC_STATE.names if not np.array_equal(state[k], exp_st[k])]
