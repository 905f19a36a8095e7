"""-m gpu: igdsp_ns_run (include/igdsp.h, "Noise suppression") through the C ABI against tests/ns_model.py, bit for bit: rows, records,
PCM records, state.  Shapes around the kernel's ownership units (16 lanes own a channel, a wave of four channels is a block): channels
1, 3, 4, 5, 16, 17, 63, 64, 65 and 130, frames 1, 2 and 5, every samples_per_frame, rows from mixed G.711 laws and from PCM, every launch
from fresh, garbage-under-tag and wrong-tag states side by side.  Bit for bit as well: one launch against the same frames in several, a
channel at another position and channel count; every d_ctl value side by side in one wave; every output set with guard bytes around
every buffer and the state; one channel of a wave clipping; a short noise scene whose records show the suppression; the chain
igdsp_filt_run -> igdsp_ns_run -> igdsp_agc_run -> igdsp_conf_mix on the device against the models chained; the argument clauses; the
yardstick against its written promise; one launch at full-chip size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import agc_model  # noqa: E402
from tests import conf_model  # noqa: E402
from tests import filt_model  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import ns_model as nm  # noqa: E402
from tests import tdet_model  # noqa: E402

GUARD = 256
EINVAL, ERANGE = -22, -34
SB = capi.NS_STATE.itemsize
NS = (80, 160, 240, 320)
CS = (1, 3, 4, 5, 16, 17, 63, 64, 65, 130)
STATE_GUARD = 0xA5
SIZES = dict(out=lambda F_, C_, n: F_ * C_ * n * 2, rec=lambda F_, C_, n: F_ * C_ * 16, stats=lambda F_, C_, n: F_ * C_ * 16)
ALL = ("out", "rec", "stats")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def mixed_laws(C_):
    return np.where(np.arange(C_) % 3 == 1, 8, 0).astype(np.uint8)


def mixed_states(C_, seed):
    """channel by channel: garbage under the tag, a wrong tag over garbage, fresh"""
    st = nm.garbage_state(C_, seed)
    st[1::3] = nm.garbage_state(C_, seed + 1, tagged=False)[1::3]
    st[2::3] = np.zeros((), nm.STATE)
    return st


def mixed_ctl(C_):
    ctl = (np.arange(C_) % 5).astype(np.uint8)                             # RUN FREEZE BYPASS RESET 4 (as RUN)
    ctl[ctl == 4] = 200
    return ctl


def state_dev(state):
    b = np.ascontiguousarray(state).view(np.uint8).reshape(-1)
    g = np.full(GUARD, STATE_GUARD, np.uint8)
    return gu.to_dev(np.concatenate([g, b, g]))                            # guard bytes in front of the state and behind it


def run_ns(ctx, x, codec=None, cfg=None, ctl=None, state=None, d_state=None, outputs=ALL, fill=0xEE, entry=None):
    """One launch through the C ABI (entry: through that yardstick instead).  x [F][C][n]: uint8 codes (with codec [C]) or int16 PCM;
    state [C] or None (all-zero), or d_state carried from an earlier launch.  Returns the outputs, the state records and the state
    tensor (with its guards); guard bytes in front of and behind every output buffer and the state are checked."""
    torch = gu.torch_cuda()
    F_, C_, n = x.shape
    g711 = x.dtype == np.uint8
    dev = lambda a, t: None if a is None else gu.to_dev(np.ascontiguousarray(a, t))
    d_x = gu.to_dev(x if g711 else np.asarray(x, "<i2"))
    d_codec, d_ctl = dev(codec if g711 else None, np.uint8), dev(ctl, np.uint8)
    c = np.ascontiguousarray(capi.ns_cfg_default() if cfg is None else np.frombuffer(np.asarray(cfg).tobytes(), capi.NS_CFG)[0], capi.NS_CFG)
    if d_state is None:
        d_state = state_dev(np.zeros(C_, nm.STATE) if state is None else state)
    sizes = {k: SIZES[k](F_, C_, n) for k in outputs}
    whole = {k: gu.dev_zeros(GUARD + v + GUARD, fill) for k, v in sizes.items()}      # guard bytes around every buffer
    bufs = {k: t[GUARD:] for k, t in whole.items()}                        # (GUARD keeps the allocation's alignment)
    p = lambda t: None if t is None else t.data_ptr()
    d_st = d_state[GUARD:]
    if entry:
        rc = capi.internal(entry)(ctx.h, p(d_x) if g711 else None, p(d_codec), None if g711 else p(d_x), p(d_ctl), c.ctypes.data, C_, F_, n, p(d_st),
                                  p(bufs.get("out")), p(bufs.get("rec")), p(bufs.get("stats")), None)
        assert rc == 0, rc
    else:
        ctx.ns_run(d_st, C_, F_, n, g711=d_x if g711 else None, codec=d_codec, pcm=None if g711 else d_x, ctl=d_ctl, cfg=c, out=bufs.get("out"),
                   rec=bufs.get("rec"), stats=bufs.get("stats"))
    torch.cuda.synchronize()
    host = {}
    for k, t in whole.items():
        b = t.cpu().numpy()
        assert np.all(b[:GUARD] == fill), f"bytes in front of d_{k} written"
        assert np.all(b[GUARD + sizes[k]:] == fill), f"bytes after d_{k} written"
        host[k] = b[GUARD:]
    sbytes = d_state.cpu().numpy()
    assert len(sbytes) == C_ * SB + 2 * GUARD and np.all(sbytes[:GUARD] == STATE_GUARD), "bytes in front of d_state written"
    assert np.all(sbytes[GUARD + C_ * SB:] == STATE_GUARD), "bytes after d_state written"
    res = dict(d_state=d_state, state=sbytes[GUARD:GUARD + C_ * SB].view(nm.STATE).copy())
    if "out" in host:
        res["out"] = host["out"][:sizes["out"]].view("<i2").reshape(F_, C_, n)
    if "rec" in host:
        res["rec"] = host["rec"][:sizes["rec"]].view(nm.REC).reshape(F_, C_)
    if "stats" in host:
        res["stats"] = host["stats"][:sizes["stats"]].view(capi.FRAME_STATS).reshape(F_, C_)
    return res


def pcm_of(x, codec):
    return tdet_model.decode(x, codec) if x.dtype == np.uint8 else np.asarray(x, np.int16)


def check(got, model):
    out, rec, stats, st = model
    if "out" in got:
        assert np.array_equal(got["out"], out), np.argwhere(got["out"] != out)[:6]
    if "rec" in got:
        assert got["rec"].tobytes() == rec.tobytes(), [(k, np.argwhere(got["rec"][k] != rec[k])[:4].tolist()) for k in rec.dtype.names
                                                        if not np.array_equal(got["rec"][k], rec[k])]
    if "stats" in got:
        gu.assert_stats_equal(got["stats"], stats)
    assert got["state"].tobytes() == st.tobytes(), [(k, np.argwhere(got["state"][k] != st[k])[:4].tolist()) for k in st.dtype.names
                                                    if not np.array_equal(got["state"][k], st[k])]


def scene(C_, F_, n, seed, form):
    """rows as codes of mixed laws or as PCM: full-range noise, every fifth channel quiet, every seventh silent"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, (F_, C_, n)).astype(np.int16)
    x[:, ::5] //= 256
    x[:, 6::7] = 0
    if form == "pcm":
        return x, None
    codec = mixed_laws(C_)
    return tdet_model.encode(x, codec), codec


def model(x, codec, **kw):
    return nm.run(pcm_of(x, codec), **kw)


# ---- 1. the shapes, rows from codes and from PCM, all three kinds of state, with and without d_ctl
@pytest.mark.parametrize("form", ("g711", "pcm"))
@pytest.mark.parametrize("n", NS)
def test_shapes(ctx, n, form):
    seen = 0
    for i, C_ in enumerate(CS):
        F_ = (1, 2, 5)[i % 3]
        x, codec = scene(C_, F_, n, 10 * n + C_, form)
        st = mixed_states(C_, n + C_)
        ctl = mixed_ctl(C_) if i % 2 else None
        m = model(x, codec, ctl=ctl, state=st)
        check(run_ns(ctx, x, codec, ctl=ctl, state=st), m)
        seen |= int(np.bitwise_or.reduce(m[1]["flags"].reshape(-1)))
    want = nm.BYPASSED | nm.WAS_RESET | nm.FROZEN | nm.LEARNING | nm.SUPPRESSING
    assert seen & want == want, hex(seen)


# ---- 2. the invariants: a split of the frames, position and count
def test_split_and_position(ctx):
    C_, F_, n = 131, 6, 160
    x, codec = scene(C_, F_, n, 5, "g711")
    st = mixed_states(C_, 4)
    ctl = mixed_ctl(C_)
    ctl[ctl == nm.RESET] = nm.RUN                                          # RESET holds for a launch: every launch of a split would reset
    whole = run_ns(ctx, x, codec, ctl=ctl, state=st)
    check(whole, model(x, codec, ctl=ctl, state=st))
    for cuts in ((1, 3, 6), tuple(range(1, 7))):
        d_state, a, parts = None, 0, []
        for b in cuts:
            parts.append(run_ns(ctx, x[a:b], codec, ctl=ctl, state=st if a == 0 else None, d_state=d_state))
            d_state, a = parts[-1]["d_state"], b
        for k in ALL:
            assert np.concatenate([q[k] for q in parts]).tobytes() == whole[k].tobytes(), (cuts, k)
        assert parts[-1]["state"].tobytes() == whole["state"].tobytes(), cuts
    # a channel's bytes at C = 131 and alone; channel 4's inputs and state in another wave and at the last index
    for c in (0, 77, 130):
        alone = run_ns(ctx, x[:, c:c + 1], codec[c:c + 1], ctl=ctl[c:c + 1], state=st[c:c + 1])
        for k in ALL:
            assert alone[k][:, 0].tobytes() == whole[k][:, c].tobytes(), (c, k)
        assert alone["state"].tobytes() == whole["state"][c:c + 1].tobytes()
    idx = np.arange(70)
    idx[33], idx[-1] = 4, 4
    big = run_ns(ctx, x[:, idx], codec[idx], ctl=ctl[idx], state=st[idx])
    for k in ALL:
        assert np.array_equal(big[k], whole[k][:, idx]), k
    assert big["state"].tobytes() == whole["state"][idx].tobytes()
    assert big["out"][:, 4].tobytes() == big["out"][:, 33].tobytes() == big["out"][:, -1].tobytes()
    # from G.711 or its decoded PCM
    dec = run_ns(ctx, pcm_of(x, codec), ctl=ctl, state=st)
    for k in ALL + ("state",):
        assert dec[k].tobytes() == whole[k].tobytes(), k


# ---- 3. control: every d_ctl value side by side in one wave over every kind of state
@pytest.mark.parametrize("form", ("g711", "pcm"))
def test_ctl_and_states(ctx, form):
    C_, F_, n = 23, 4, 240
    x, codec = scene(C_, F_, n, 31, form)
    for s in range(3):
        st = np.roll(mixed_states(C_, 20 + s), s)
        ctl = mixed_ctl(C_)                                                # four channels a wave: every wave holds four different values
        m = model(x, codec, ctl=ctl, state=st)
        got = run_ns(ctx, x, codec, ctl=ctl, state=st)
        check(got, m)
        byp, frz = ctl == nm.BYPASS, ctl == nm.FREEZE
        assert (m[1]["flags"][:, byp] == nm.BYPASSED).all() and (m[1]["flags"][:, frz] & nm.FROZEN).all()
        flat = pcm_of(x, codec).transpose(1, 0, 2).reshape(C_, -1)
        outs = got["out"].transpose(1, 0, 2).reshape(C_, -1)
        assert np.array_equal(outs[byp][:, 80:], flat[byp][:, :-80])       # the input through the delay, bit for bit
        keep = byp & (st["tag"] == nm.TAG)
        for k in ("S", "N", "Gt", "hops"):
            masked = st[k] & np.uint64(nm.LEVEL_MASK) if k in ("S", "N") else (np.minimum(st[k], nm.UNITY) if k == "Gt" else st[k])
            assert np.array_equal(got["state"][k][keep], masked[keep]), k
        held = frz & (st["tag"] == nm.TAG)
        assert np.array_equal(got["state"]["N"][held], (st["N"] & np.uint64(nm.LEVEL_MASK))[held]) and np.array_equal(got["state"]["hops"][held], st["hops"][held])
        fresh = ((st["tag"] != nm.TAG) | (ctl == nm.RESET)) & ~byp
        assert ((m[1]["flags"][0, fresh] & nm.WAS_RESET) != 0).all() and not (m[1]["flags"][0, ~fresh] & nm.WAS_RESET).any()
        assert not (m[1]["flags"][1:] & nm.WAS_RESET).any()


# ---- 4. every output set
@pytest.mark.parametrize("outputs", (ALL, ("out",), ("rec",), ("stats",), ("out", "rec"), ("out", "stats"), ("rec", "stats")))
def test_output_sets(ctx, outputs):
    C_, F_, n = 67, 3, 80
    x, codec = scene(C_, F_, n, 6, "pcm" if len(outputs) == 2 else "g711")
    st = mixed_states(C_, 3)
    check(run_ns(ctx, x, codec, state=st, outputs=outputs), model(x, codec, state=st))


# ---- 5. the rare branch: one channel of a wave clips
def test_rare_branch(ctx):
    C_, F_, n = 9, 4, 160
    rng = np.random.default_rng(8)
    x = rng.integers(-300, 300, (F_, C_, n)).astype(np.int16)
    x[1:3, 6] = np.where(rng.integers(0, 2, (2, n)) == 1, 32767, -32768)   # a full-scale square under unity gains overshoots by an LSB
    cfg = nm.cfg_of(floor_q15=32768)
    m = nm.run(x, cfg)
    check(run_ns(ctx, x, cfg=cfg), m)
    cl = m[1]["n_clipped"]
    assert cl[:, 6].sum() > 0 and cl.sum() == cl[:, 6].sum() and ((m[1]["flags"] & nm.CLIPPED) != 0).any(axis=0).sum() == 1


# ---- 6. a short scene: one second of noise at sigma = 300 on five channels; the device's records show the suppression
def test_scene_records(ctx):
    C_, n = 5, 160
    x = np.stack([nm.frames_of(nm.noise(300, 8000, 70 + c))[:, 0] for c in range(C_)], axis=1)
    m = nm.run(x)
    got = run_ns(ctx, x)
    check(got, m)
    rec = got["rec"]
    assert (rec["flags"][:8] & nm.LEARNING).all() and not (rec["flags"][8:] & nm.LEARNING).any()       # 16 hops
    assert (rec["flags"][25:] & nm.SUPPRESSING).all() and (rec["min_gain_q15"][25:] == 5827).all()
    down = 10 * np.log10(rec["in_energy"][25:-1].astype(np.float64).sum(axis=0) / rec["out_energy"][26:].astype(np.float64).sum(axis=0))
    assert ((down > 14.0) & (down < 15.0)).all(), down
    assert (np.abs(rec["noise_idx"][25:].astype(int) - rec["noise_idx"][-1].astype(int)) <= 1).all()


# ---- 7. the chain on the device: igdsp_filt_run (CTCSS_HP) -> igdsp_ns_run -> igdsp_agc_run -> igdsp_conf_mix, each stage taking the
# previous output unchanged, against the models chained
def test_chain_filt_ns_agc_conf(ctx):
    torch = gu.torch_cuda()
    C_, F_, n, P_ = 70, 12, 160, 5
    rng = np.random.default_rng(41)
    x = (rng.normal(0, 400, (F_, C_, n)) + 3000 * np.sin(2 * np.pi * 150 * np.arange(F_ * n).reshape(F_, 1, n) / 8000)).clip(-32768, 32767).astype(np.int16)
    plan = filt_model.plan_of_sections(filt_model.preset_sections(filt_model.CTCSS_HP, 8000), 8000)
    d_x, d_plan = gu.to_dev(x), gu.to_dev(np.atleast_1d(plan))
    d_fst, d_fout = gu.to_dev(np.zeros(C_, filt_model.STATE)), gu.dev_zeros(F_ * C_ * n * 2)
    ctx.filt_run(d_plan, 1, d_fst, C_, F_, n, pcm=d_x, max_sections=2, out=d_fout)
    d_nst, d_nout = gu.to_dev(np.zeros(C_, nm.STATE)), gu.dev_zeros(F_ * C_ * n * 2)
    ctx.ns_run(d_nst, C_, F_, n, pcm=d_fout, out=d_nout)
    d_ast, d_aout = gu.to_dev(np.zeros(C_, capi.AGC_STATE)), gu.dev_zeros(F_ * C_ * n * 2)
    ctx.agc_run(d_ast, C_, F_, n, pcm=d_nout, out=d_aout)
    ch, pt = np.arange(C_), np.arange(C_) % P_
    ptr, mem = capi.conf_build(ch, pt, C_, P_)
    gain = np.full(C_, 128, np.uint16)
    d_mix = gu.dev_zeros(F_ * P_ * n * 2)
    ctx.conf_mix(gu.to_dev(gain), gu.to_dev(ptr), gu.to_dev(mem), len(mem), C_, P_, F_, n, out=d_mix, pcm=d_aout)
    torch.cuda.synchronize()
    fout = filt_model.run(plan, x)[0]
    assert np.array_equal(gu.to_host(d_fout, "<i2", (F_, C_, n)), fout)
    nout = nm.run(fout)[0]
    assert np.array_equal(gu.to_host(d_nout, "<i2", (F_, C_, n)), nout)
    aout = agc_model.run(agc_model.cfg_default(), nout)[0]
    assert np.array_equal(gu.to_host(d_aout, "<i2", (F_, C_, n)), aout)
    eo, _ = conf_model.mix(aout.astype(np.int64), gain, ptr, mem, len(mem), P_)
    assert np.array_equal(gu.to_host(d_mix, "<i2", (F_, P_, n)), eo)


# ---- 8. the argument clauses through the C ABI
def test_argument_paths(ctx):
    L = capi.load()
    C_, F_, n = 4, 2, 160
    x, codec = scene(C_, F_, n, 1, "g711")
    d = dict(g=gu.to_dev(x), codec=gu.to_dev(codec), pcm=gu.to_dev(pcm_of(x, codec)), ctl=gu.to_dev(np.zeros(C_, np.uint8)), st=gu.dev_zeros(C_ * SB + 64),
             out=gu.dev_zeros(F_ * C_ * n * 2 + 64), rec=gu.dev_zeros(F_ * C_ * 16 + 64), stats=gu.dev_zeros(F_ * C_ * 16 + 64))
    p = {k: t.data_ptr() for k, t in d.items()}
    before = {k: d[k].cpu().numpy().copy() for k in ("st", "out", "rec", "stats")}
    good = np.ascontiguousarray(capi.ns_cfg_default())

    def call(h=ctx.h, g=None, codec=None, pcm=p["pcm"], ctl=p["ctl"], cfg=good, C=C_, F=F_, nn=n, st=p["st"], out=p["out"], rec=p["rec"], stats=p["stats"]):
        return L.igdsp_ns_run(h, g, codec, pcm, ctl, None if cfg is None else cfg.ctypes.data, C, F, nn, st, out, rec, stats, None)

    def cfg_with(**kw):
        c = good.copy()
        for k, v in kw.items():
            c[k] = v
        return c

    bad = [call(h=None)] + [call(nn=nn) for nn in (0, 8, 40, 81, 256, 400)] + [call(nn=8, C=0), call(cfg=None), call(cfg=None, F=0)]
    bad += [call(cfg=cfg_with(**{k: v})) for k, (lo, hi) in nm.RANGES.items() for v in (lo - 1, hi + 1)]
    bad += [call(g=p["g"], codec=p["codec"]), call(g=p["g"], pcm=None), call(pcm=None), call(st=None), call(out=None, rec=None, stats=None)]
    bad += [call(pcm=p["pcm"] + 8), call(g=p["g"] + 4, codec=p["codec"], pcm=None)]
    bad += [call(**{k: p[k] + 8}) for k in ("st", "out", "rec", "stats")]
    bad += [call(out=p["pcm"]), call(rec=p["stats"]), call(st=p["ctl"]), call(stats=p["out"])]
    assert bad == [EINVAL] * len(bad), bad
    assert b"overlap" in L.igdsp_last_error(ctx.h)
    assert call(C=1 << 20, F=1 << 12) == ERANGE
    gu.torch_cuda().cuda.synchronize()
    for k, b in before.items():                                            # every rejected call returned before any launch
        assert np.array_equal(d[k].cpu().numpy(), b), k
    assert call(C=0) == 0 and call(F=0) == 0 and call(C=0, st=None, out=None) == 0
    assert call() == 0 and call(ctl=None) == 0 and call(g=p["g"], codec=p["codec"], pcm=None) == 0 and call(out=None, stats=None) == 0
    assert call(g=p["g"] + 8, codec=p["codec"], pcm=None, F=1) == 0
    assert all(call(cfg=cfg_with(**{k: v})) == 0 for k, r in nm.RANGES.items() for v in r)
    gu.torch_cuda().cuda.synchronize()


# ---- 9. the yardstick: the same arguments, 0, and its written promise: the bytes of every channel at IGDSP_NS_BYPASS, d_ctl not read
@pytest.mark.parametrize("form", ("g711", "pcm"))
def test_yardstick_promise(ctx, form):
    C_, F_, n = 83, 3, 160
    x, codec = scene(C_, F_, n, 12, form)
    st = mixed_states(C_, 8)
    want = model(x, codec, ctl=np.full(C_, nm.BYPASS, np.uint8), state=st)
    assert (want[1]["flags"] == nm.BYPASSED).all() and (want[3]["tag"] == nm.TAG).all()
    got = run_ns(ctx, x, codec, ctl=np.full(C_, nm.RESET, np.uint8), state=st, entry="ns_move")
    check(got, want)
    for outputs in (("out",), ("rec",), ("out", "stats")):
        check(run_ns(ctx, x, codec, state=st, outputs=outputs, entry="ns_move"), want)

    # it touches exactly the stage's bytes: in every output buffer the entry's footprint, which is the whole buffer and no guard byte
    def masks(entry):
        def one(fill):
            g = run_ns(ctx, x, codec, state=st, fill=fill, entry=entry)
            return {k: g[k] for k in ALL}
        return gu.written_mask(one)
    ym, rm = masks("ns_move"), masks(None)
    gu.assert_same_footprint(ym, rm)
    assert all(ym[k].all() for k in ALL)


# ---- 10. the full chip: 65 536 channels x 2 frames in one launch, a sampled comparison
def test_full_chip(ctx):
    C_, F_, n = 65536, 2, 160
    rng = np.random.default_rng(21)
    codec = mixed_laws(C_)
    codes = rng.integers(0, 256, (F_, C_, n), dtype=np.uint8)
    st = mixed_states(C_, 5)
    ctl = mixed_ctl(C_)
    got = run_ns(ctx, codes, codec, ctl=ctl, state=st)
    sample = np.sort(rng.choice(C_, 256, replace=False))
    sample[0], sample[-1] = 0, C_ - 1
    m = model(codes[:, sample], codec[sample], ctl=ctl[sample], state=st[sample])
    check({k: (got[k][:, sample] if k in ALL else got[k][sample]) for k in ALL + ("state",)}, m)
    fl = got["rec"]["flags"]
    assert (fl[:, ctl == nm.BYPASS] == nm.BYPASSED).all() and (fl[:, ctl == nm.FREEZE] & nm.FROZEN).all()
    assert (fl[0] & nm.WAS_RESET).any() and not (fl[1] & nm.WAS_RESET).any() and (got["state"]["tag"] == nm.TAG).all()
