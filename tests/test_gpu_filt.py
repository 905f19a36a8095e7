"""-m gpu: igdsp_filt_run (include/igdsp.h, "Filter") through the C ABI against tests/filt_model.py, bit for bit: rows, records, PCM
records, state.  Shapes around the kernel's ownership units (a lane owns a channel, a wave of 64 lanes is a block and stores the
frame's rows as a tile of 16-byte pieces; a row's first 16 pieces are loaded ahead of the frame, the rest behind it): channels 1, 63,
64, 65, 130, 257, five frames, samples per frame 8, 24 (three pieces a row: no power of two), 160 and 256 (late pieces), rows from
mixed G.711 laws and from PCM, at one, two and four sections, every launch from fresh, garbage-under-tag and wrong-tag states side by
side.  Bit for bit as well: one launch against the same frames in several, a channel at another position and channel count.  Plans of
different section counts interleaved, an index past the plans, a bad plan, d_plan_of NULL, a plan above max_sections; every d_ctl value;
every output set with guard bytes around every buffer and the state; one channel of a wave clipping in one frame; the chain
igdsp_resample -> igdsp_filt_run -> igdsp_agc_run -> igdsp_conf_mix on the device; the argument clauses; the yardstick against its
written promise; one launch at full-chip size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import agc_model  # noqa: E402
from tests import conf_model  # noqa: E402
from tests import filt_model as fm  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import rs_model  # noqa: E402
from tests import tdet_model  # noqa: E402

GUARD = 256
EINVAL, ERANGE = -22, -34
SB = capi.FILT_STATE.itemsize
NS = (8, 24, 160, 256)
CS = (1, 63, 64, 65, 130, 257)
STATE_GUARD = 0xA5
SIZES = dict(out=lambda F_, C_, n: F_ * C_ * n * 2, rec=lambda F_, C_, n: F_ * C_ * 16, stats=lambda F_, C_, n: F_ * C_ * 16)
ALL = ("out", "rec", "stats")
EXTREMAL = (32767, 32767, 1, 0, 0)                                         # the magnitudes sum to 65 535; no feedback: a clip does not last


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def preset(p, rate=8000):
    return fm.plan_of_sections(fm.preset_sections(p, rate), rate)


def plans_of(sections):
    """four plans of 1, 2, 3 and 4 sections cut to at most `sections`, one of every preset among them"""
    v, c = fm.preset_sections(fm.VOICE_BAND, 8000), fm.preset_sections(fm.CTCSS_HP, 8000)
    d, e, q = fm.preset_sections(fm.DC_BLOCK, 8000), fm.preset_sections(fm.DEEMPH, 8000), fm.preset_sections(fm.PREEMPH, 8000)
    full = [d, c, e + q + d, c + v]
    return np.array([fm.plan_of_sections(s[:sections]) for s in full], fm.PLAN)


def mixed_laws(C_):
    return np.where(np.arange(C_) % 3 == 1, 8, 0).astype(np.uint8)


def mixed_states(C_, seed):
    """channel by channel: garbage under the tag, a wrong tag over garbage, fresh"""
    st = fm.garbage_state(C_, seed)
    st[1::3] = fm.garbage_state(C_, seed + 1, tagged=False)[1::3]
    st[2::3] = np.zeros((), fm.STATE)
    return st


def mixed_ctl(C_):
    ctl = (np.arange(C_) % 4).astype(np.uint8)                             # RUN BYPASS RESET 3 (as RUN)
    ctl[ctl == 3] = 200
    return ctl


def state_dev(state):
    b = np.ascontiguousarray(state).view(np.uint8).reshape(-1)
    g = np.full(GUARD, STATE_GUARD, np.uint8)
    return gu.to_dev(np.concatenate([g, b, g]))                            # guard bytes in front of the state and behind it


def run_filt(ctx, plans, x, codec=None, plan_of=None, ctl=None, state=None, d_state=None, max_sections=0, outputs=ALL, fill=0xEE, entry=None, n_plans=None):
    """One launch through the C ABI (entry: through that yardstick instead).  plans [n_plans] PLAN; x [F][C][n]: uint8 codes (with codec
    [C]) or int16 PCM; state [C] or None (all-zero), or d_state carried from an earlier launch.  Returns the outputs, the state records
    and the state tensor (with its guards); guard bytes in front of and behind every output buffer and the state are checked."""
    torch = gu.torch_cuda()
    F_, C_, n = x.shape
    g711 = x.dtype == np.uint8
    dev = lambda a, t: None if a is None else gu.to_dev(np.ascontiguousarray(a, t))
    d_x = gu.to_dev(x if g711 else np.asarray(x, "<i2"))
    d_codec, d_ctl, d_po = dev(codec if g711 else None, np.uint8), dev(ctl, np.uint8), dev(plan_of, "<u2")
    plans = np.atleast_1d(np.asarray(plans, fm.PLAN))
    d_plans = gu.to_dev(plans)
    n_plans = len(plans) if n_plans is None else n_plans
    if d_state is None:
        d_state = state_dev(np.zeros(C_, fm.STATE) if state is None else state)
    sizes = {k: SIZES[k](F_, C_, n) for k in outputs}
    whole = {k: gu.dev_zeros(GUARD + v + GUARD, fill) for k, v in sizes.items()}      # guard bytes around every buffer
    bufs = {k: t[GUARD:] for k, t in whole.items()}                        # (GUARD keeps the allocation's alignment)
    p = lambda t: None if t is None else t.data_ptr()
    d_st = d_state[GUARD:]
    if entry:
        rc = capi.internal(entry)(ctx.h, p(d_x) if g711 else None, p(d_codec), None if g711 else p(d_x), p(d_ctl), p(d_plans), n_plans, p(d_po), max_sections,
                                  C_, F_, n, p(d_st), p(bufs.get("out")), p(bufs.get("rec")), p(bufs.get("stats")), None)
        assert rc == 0, rc
    else:
        ctx.filt_run(d_plans, n_plans, d_st, C_, F_, n, g711=d_x if g711 else None, codec=d_codec, pcm=None if g711 else d_x, ctl=d_ctl, plan_of=d_po,
                     max_sections=max_sections, out=bufs.get("out"), rec=bufs.get("rec"), stats=bufs.get("stats"))
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
    res = dict(d_state=d_state, state=sbytes[GUARD:GUARD + C_ * SB].view(fm.STATE).copy())
    if "out" in host:
        res["out"] = host["out"][:sizes["out"]].view("<i2").reshape(F_, C_, n)
    if "rec" in host:
        res["rec"] = host["rec"][:sizes["rec"]].view(fm.REC).reshape(F_, C_)
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
    """rows as codes of mixed laws or as PCM: full-range noise, every fifth channel quiet"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, (F_, C_, n)).astype(np.int16)
    x[:, ::5] //= 256
    if form == "pcm":
        return x, None
    codec = mixed_laws(C_)
    return tdet_model.encode(x, codec), codec


def model(plans, x, codec, **kw):
    return fm.run(plans, pcm_of(x, codec), **kw)


# ---- 1. the shapes, rows from codes and from PCM, at one, two and four sections, all three kinds of state, with and without d_ctl
@pytest.mark.parametrize("form", ("g711", "pcm"))
@pytest.mark.parametrize("sections", (1, 2, 4))
@pytest.mark.parametrize("n", NS)
def test_shapes(ctx, n, sections, form):
    plans, F_, seen = plans_of(sections), 5, 0
    for i, C_ in enumerate(CS):
        x, codec = scene(C_, F_, n, 10 * n + C_, form)
        st = mixed_states(C_, n + C_)
        ctl = mixed_ctl(C_) if i % 2 else None
        po = (np.arange(C_) * 7 + i) % 4
        m = model(plans, x, codec, plan_of=po, ctl=ctl, state=st, max_sections=sections)
        check(run_filt(ctx, plans, x, codec, plan_of=po, ctl=ctl, state=st, max_sections=sections), m)
        seen |= int(np.bitwise_or.reduce(m[1]["flags"].reshape(-1)))
        assert (m[1]["n_sections"] == np.minimum(po + 1, sections)[None, :]).all()
    assert seen & (fm.BYPASSED | fm.WAS_RESET) == fm.BYPASSED | fm.WAS_RESET and not seen & (fm.NO_PLAN | fm.BAD_PLAN), hex(seen)


# ---- 2. the invariants: a split of the frames, position and count
def test_split_and_position(ctx):
    C_, F_, n = 257, 6, 160
    plans = plans_of(4)
    x, codec = scene(C_, F_, n, 5, "g711")
    st = mixed_states(C_, 4)
    po = np.arange(C_) % 4
    whole = run_filt(ctx, plans, x, codec, plan_of=po, state=st)
    check(whole, model(plans, x, codec, plan_of=po, state=st))
    for cuts in ((1, 3, 6), tuple(range(1, 7))):
        d_state, a, parts = None, 0, []
        for b in cuts:
            parts.append(run_filt(ctx, plans, x[a:b], codec, plan_of=po, state=st if a == 0 else None, d_state=d_state))
            d_state, a = parts[-1]["d_state"], b
        for k in ALL:
            assert np.concatenate([q[k] for q in parts]).tobytes() == whole[k].tobytes(), (cuts, k)
        assert parts[-1]["state"].tobytes() == whole["state"].tobytes(), cuts
    # a channel's bytes at C = 257 and alone; channel 4's inputs and state in the second wave and at the last index
    for c in (0, 77, 256):
        alone = run_filt(ctx, plans, x[:, c:c + 1], codec[c:c + 1], plan_of=po[c:c + 1], state=st[c:c + 1])
        for k in ALL:
            assert alone[k][:, 0].tobytes() == whole[k][:, c].tobytes(), (c, k)
        assert alone["state"].tobytes() == whole["state"][c:c + 1].tobytes()
    idx = np.arange(131)
    idx[77], idx[-1] = 4, 4
    big = run_filt(ctx, plans, x[:, idx], codec[idx], plan_of=po[idx], state=st[idx])
    for k in ALL:
        assert np.array_equal(big[k], whole[k][:, idx]), k
    assert big["state"].tobytes() == whole["state"][idx].tobytes()
    assert big["out"][:, 4].tobytes() == big["out"][:, 77].tobytes() == big["out"][:, -1].tobytes()


# ---- 3. plans: interleaved section counts, an index past the plans, a bad plan, a plan of any bytes, d_plan_of NULL, max_sections
def test_plans(ctx):
    C_, F_, n = 130, 5, 24
    x, codec = scene(C_, F_, n, 6, "pcm")
    st = mixed_states(C_, 3)
    good = fm.preset_sections(fm.CTCSS_HP, 8000)
    bad = (32767, -32768, 1, 0, 0)
    rng = np.random.default_rng(2)
    plans = np.concatenate([plans_of(4), np.array([fm.plan_of_sections([good[0], bad, good[1]]), fm.plan_of_sections(good, n_sections=0),
                                                   fm.plan_of_sections(good + good, n_sections=255),
                                                   np.frombuffer(rng.integers(0, 256, 48, dtype=np.uint8).tobytes(), fm.PLAN)[0]], fm.PLAN)])
    po = np.arange(C_) % 10                                                # 8 and 9: past the plans
    po[5] = 65535
    m = model(plans, x, codec, plan_of=po, state=st)
    got = run_filt(ctx, plans, x, codec, plan_of=po, state=st)
    check(got, m)
    fl = m[1]["flags"]
    assert (fl[:, po >= 8] == fm.NO_PLAN).all() and (fl[:, po == 5] == fm.NO_PLAN).all() and (fl[:, po == 4] & fm.BAD_PLAN).all()
    untouched = (po >= 8) | (po == 5)
    assert got["state"][untouched].tobytes() == st[untouched].tobytes() and np.array_equal(got["out"][:, untouched], x[:, untouched])
    assert (got["rec"]["plan"] == po[None, :]).all()
    # d_plan_of NULL: plan 0 for everyone; n_plans below the array's length cuts the indices off there
    check(run_filt(ctx, plans, x, codec, state=st), model(plans, x, codec, state=st))
    check(run_filt(ctx, plans, x, codec, plan_of=po, state=st, n_plans=3), model(plans[:3], x, codec, plan_of=po, state=st))
    # max_sections: plans with more sections are flagged and not run, whatever kernel the launch picks
    for ms in (1, 2, 3, 4):
        m = model(plans, x, codec, plan_of=po, state=st, max_sections=ms)
        check(run_filt(ctx, plans, x, codec, plan_of=po, state=st, max_sections=ms), m)
        over = np.minimum(plans["n_sections"], 4)[np.minimum(po, 7)] > ms
        assert ((m[1]["flags"][:, over & (po < 8)] & (fm.NO_PLAN | fm.BAD_PLAN)) == (fm.NO_PLAN | fm.BAD_PLAN)).all() and (over & (po < 8)).any() == (ms < 4)


# ---- 4. control: every d_ctl value over every kind of state; BYPASS and NO_PLAN leave the state's bytes as they were
@pytest.mark.parametrize("form", ("g711", "pcm"))
def test_ctl_and_states(ctx, form):
    C_, F_, n = 75, 4, 24
    x, codec = scene(C_, F_, n, 31, form)
    plans = plans_of(2)
    for s in range(3):
        st = np.roll(mixed_states(C_, 20 + s), s)
        ctl = (np.arange(C_) // 3 % 4).astype(np.uint8)                    # every ctl over every kind of state
        ctl[ctl == 3] = 77
        po = np.where(np.arange(C_) % 11 == 10, 9, np.arange(C_) % 4)
        m = model(plans, x, codec, plan_of=po, ctl=ctl, state=st, max_sections=2)
        got = run_filt(ctx, plans, x, codec, plan_of=po, ctl=ctl, state=st, max_sections=2)
        check(got, m)
        byp, nop = ctl == fm.BYPASS, po == 9
        assert got["state"][byp | nop].tobytes() == st[byp | nop].tobytes()      # the guard pattern of a garbage state stands
        assert (m[1]["flags"][:, byp] == fm.BYPASSED).all() and (m[1]["flags"][:, nop & ~byp] == fm.NO_PLAN).all()
        assert np.array_equal(got["out"][:, byp | nop], pcm_of(x, codec)[:, byp | nop])
        fresh = ((st["tag"] != fm.TAG) | (ctl == fm.RESET)) & ~byp & ~nop
        assert ((m[1]["flags"][0, fresh] & fm.WAS_RESET) != 0).all() and not (m[1]["flags"][0, ~fresh] & fm.WAS_RESET).any()


# ---- 5. every output set
@pytest.mark.parametrize("outputs", (ALL, ("out",), ("rec",), ("stats",), ("out", "rec"), ("out", "stats"), ("rec", "stats")))
def test_output_sets(ctx, outputs):
    C_, F_, n = 67, 3, 24
    x, codec = scene(C_, F_, n, 6, "pcm" if len(outputs) == 2 else "g711")
    st = mixed_states(C_, 3)
    plans, po = plans_of(4), np.arange(C_) % 4
    check(run_filt(ctx, plans, x, codec, plan_of=po, state=st, outputs=outputs), model(plans, x, codec, plan_of=po, state=st))


# ---- 6. the rare branch: one channel of a wave clips, in one frame only
def test_rare_branch(ctx):
    C_, F_, n = 130, 5, 160
    rng = np.random.default_rng(8)
    x = rng.integers(-300, 300, (F_, C_, n)).astype(np.int16)
    x[2, 70, 40:120] = 32767                                               # the extremal section under a full-scale run
    plans = np.array([fm.plan_of_sections([EXTREMAL])], fm.PLAN)
    m = fm.run(plans, x, max_sections=1)
    check(run_filt(ctx, plans, x, max_sections=1), m)
    cl = m[1]["n_clipped"]
    assert cl[2, 70] > 0 and cl.sum() == cl[2, 70] and (m[1]["flags"][2, 70] & fm.CLIPPED) and ((m[1]["flags"] & fm.CLIPPED) != 0).sum() == 1


# ---- 7. the chain on the device: igdsp_resample (up by 2) -> igdsp_filt_run (VOICE_BAND at 16 000, sub-frames) -> igdsp_agc_run ->
# igdsp_conf_mix, each hop taking the previous output unchanged, against the host chain
def test_chain_resample_filt_agc_conf(ctx):
    torch = gu.torch_cuda()
    C_, F_, n, P_, R = 70, 6, 160, 5, 2
    rng = np.random.default_rng(41)
    x = (rng.normal(0, 2500, (F_, C_, n)) + 3000 * np.sin(2 * np.pi * 150 * np.arange(F_ * n).reshape(F_, 1, n) / 8000)).clip(-32768, 32767).astype(np.int16)
    rows, _, _ = rs_model.launch(rs_model.UP, R, rs_model.SUBFRAMES, x)    # [F R][C][n]: sub-frames, the bridge's row order
    d_x = gu.to_dev(x)
    d_up, d_hist = gu.dev_zeros(F_ * R * C_ * n * 2), gu.to_dev(np.zeros(C_, capi.RS_STATE))
    ctx.resample(capi.RS_UP, R, d_hist, C_, F_, n, layout=capi.RS_SUBFRAMES, pcm=d_x, out=d_up)
    plan = preset(fm.VOICE_BAND, 16000)
    d_plan = gu.to_dev(np.atleast_1d(plan))
    d_fst, d_fout = gu.to_dev(np.zeros(C_, fm.STATE)), gu.dev_zeros(F_ * R * C_ * n * 2)
    ctx.filt_run(d_plan, 1, d_fst, C_, F_ * R, n, pcm=d_up, max_sections=2, out=d_fout)
    d_ast, d_aout = gu.to_dev(np.zeros(C_, capi.AGC_STATE)), gu.dev_zeros(F_ * R * C_ * n * 2)
    ctx.agc_run(d_ast, C_, F_ * R, n, pcm=d_fout, out=d_aout)
    ch, pt = np.arange(C_), np.arange(C_) % P_
    ptr, mem = capi.conf_build(ch, pt, C_, P_)
    gain = np.full(C_, 128, np.uint16)
    d_mix = gu.dev_zeros(F_ * R * P_ * n * 2)
    ctx.conf_mix(gu.to_dev(gain), gu.to_dev(ptr), gu.to_dev(mem), len(mem), C_, P_, F_ * R, n, out=d_mix, pcm=d_aout)
    torch.cuda.synchronize()
    assert np.array_equal(gu.to_host(d_up, "<i2", (F_ * R, C_, n)), rows)
    # the host chain: igdsp_filt_frame, then the level control's model, then the mix's
    fout = np.zeros_like(rows)
    for c in range(C_):
        s = np.zeros((), capi.FILT_STATE)
        for f in range(F_ * R):
            fout[f, c] = capi.filt_frame(np.frombuffer(plan.tobytes(), capi.FILT_PLAN)[0], s, rows[f, c])[0]
    assert np.array_equal(gu.to_host(d_fout, "<i2", (F_ * R, C_, n)), fout) and np.array_equal(fout, fm.run(plan, rows)[0])
    aout = agc_model.run(agc_model.cfg_default(), fout)[0]
    assert np.array_equal(gu.to_host(d_aout, "<i2", (F_ * R, C_, n)), aout)
    eo, _ = conf_model.mix(aout.astype(np.int64), gain, ptr, mem, len(mem), P_)
    assert np.array_equal(gu.to_host(d_mix, "<i2", (F_ * R, P_, n)), eo)
    lo = np.abs(np.fft.rfft(fout[2:, 0].reshape(-1).astype(np.float64)))   # the 150 Hz tone is down, the band stands
    hi = np.abs(np.fft.rfft(rows[2:, 0].reshape(-1).astype(np.float64)))
    k = round(150 * len(fout[2:, 0].reshape(-1)) / 16000)
    assert lo[k] < 0.35 * hi[k]


# ---- 8. the argument clauses through the C ABI
def test_argument_paths(ctx):
    L = capi.load()
    C_, F_, n = 4, 2, 160
    x, codec = scene(C_, F_, n, 1, "g711")
    d = dict(g=gu.to_dev(x), codec=gu.to_dev(codec), pcm=gu.to_dev(pcm_of(x, codec)), ctl=gu.to_dev(np.zeros(C_, np.uint8)), plans=gu.to_dev(plans_of(4)),
             po=gu.to_dev(np.zeros(C_, "<u2")), st=gu.dev_zeros(C_ * SB + 64), out=gu.dev_zeros(F_ * C_ * n * 2 + 64), rec=gu.dev_zeros(F_ * C_ * 16 + 64),
             stats=gu.dev_zeros(F_ * C_ * 16 + 64))
    p = {k: t.data_ptr() for k, t in d.items()}
    before = {k: d[k].cpu().numpy().copy() for k in ("st", "out", "rec", "stats")}

    def call(h=ctx.h, g=None, codec=None, pcm=p["pcm"], ctl=p["ctl"], plans=p["plans"], n_plans=4, po=p["po"], ms=0, C=C_, F=F_, nn=n, st=p["st"], out=p["out"],
             rec=p["rec"], stats=p["stats"]):
        return L.igdsp_filt_run(h, g, codec, pcm, ctl, plans, n_plans, po, ms, C, F, nn, st, out, rec, stats, None)

    bad = [call(h=None)] + [call(nn=nn) for nn in (0, 4, 20, 161, 264)] + [call(nn=4, C=0), call(ms=5), call(ms=5, F=0)]
    bad += [call(g=p["g"], codec=p["codec"]), call(g=p["g"], pcm=None), call(pcm=None), call(plans=None), call(n_plans=0), call(st=None),
            call(out=None, rec=None, stats=None)]
    bad += [call(pcm=p["pcm"] + 8), call(g=p["g"] + 4, codec=p["codec"], pcm=None), call(plans=p["plans"] + 2), call(po=p["po"] + 1)]
    bad += [call(**{k: p[k] + 8}) for k in ("st", "out", "rec", "stats")]
    bad += [call(out=p["pcm"]), call(rec=p["stats"]), call(st=p["plans"]), call(stats=p["po"])]
    assert bad == [EINVAL] * len(bad), bad
    assert b"overlap" in L.igdsp_last_error(ctx.h)
    assert call(C=1 << 20, F=1 << 12) == ERANGE
    gu.torch_cuda().cuda.synchronize()
    for k, b in before.items():                                            # every rejected call returned before any launch
        assert np.array_equal(d[k].cpu().numpy(), b), k
    assert call(C=0) == 0 and call(F=0) == 0 and call(C=0, st=None, out=None, plans=None, n_plans=0) == 0
    assert call() == 0 and call(ctl=None, po=None) == 0 and call(g=p["g"], codec=p["codec"], pcm=None) == 0 and call(out=None, stats=None) == 0
    assert call(g=p["g"] + 8, codec=p["codec"], pcm=None, F=1) == 0 and call(plans=p["plans"] + 4, n_plans=1) == 0 and call(po=p["po"] + 2, C=3) == 0
    gu.torch_cuda().cuda.synchronize()


# ---- 9. the yardstick: the same arguments, 0, and its written promise: the bytes of every channel at IGDSP_FILT_BYPASS, d_ctl not read,
# the state written back as it was read, with the tag
@pytest.mark.parametrize("form", ("g711", "pcm"))
def test_yardstick_promise(ctx, form):
    C_, F_, n = 83, 3, 160
    x, codec = scene(C_, F_, n, 12, form)
    st = mixed_states(C_, 8)
    plans, po = plans_of(4), np.arange(C_) % 5
    out, rec, stats, _ = model(plans, x, codec, plan_of=po, ctl=np.full(C_, fm.BYPASS, np.uint8), state=st)
    want = fm.yardstick_state(st)
    assert (rec["flags"] == fm.BYPASSED).all() and (want["tag"] == fm.TAG).all() and not want["reserved"].any()
    got = run_filt(ctx, plans, x, codec, plan_of=po, ctl=np.full(C_, fm.RESET, np.uint8), state=st, entry="filt_move")
    check(got, (out, rec, stats, want))
    for outputs in (("out",), ("rec",), ("out", "stats")):
        check(run_filt(ctx, plans, x, codec, plan_of=po, state=st, outputs=outputs, entry="filt_move", max_sections=2), (out, rec, stats, want))
    # it touches exactly the stage's bytes: in every output buffer the entry's footprint, which is the whole buffer and no guard byte
    def masks(entry):
        def one(fill):
            g = run_filt(ctx, plans, x, codec, plan_of=po, state=st, fill=fill, entry=entry)
            return {k: g[k] for k in ALL}
        return gu.written_mask(one)
    ym, rm = masks("filt_move"), masks(None)
    gu.assert_same_footprint(ym, rm)
    assert all(ym[k].all() for k in ALL)


# ---- 10. the full chip: 65 536 channels x 2 frames in one launch at two sections, a sampled comparison
def test_full_chip(ctx):
    C_, F_, n = 65536, 2, 160
    rng = np.random.default_rng(21)
    codec = mixed_laws(C_)
    codes = rng.integers(0, 256, (F_, C_, n), dtype=np.uint8)
    st = mixed_states(C_, 5)
    ctl = mixed_ctl(C_)
    plans = plans_of(2)
    po = rng.integers(0, 5, C_)
    got = run_filt(ctx, plans, codes, codec, plan_of=po, ctl=ctl, state=st, max_sections=2)
    sample = np.sort(rng.choice(C_, 512, replace=False))
    sample[0], sample[-1] = 0, C_ - 1
    m = model(plans, codes[:, sample], codec[sample], plan_of=po[sample], ctl=ctl[sample], state=st[sample], max_sections=2)
    check({k: (got[k][:, sample] if k in ALL else got[k][sample]) for k in ALL + ("state",)}, m)
    want_ns = np.where(po < 4, np.minimum(po + 1, 2), 0)
    assert (got["rec"]["n_sections"] == want_ns[None, :]).all() and (got["rec"]["plan"] == po[None, :]).all()
    fl = got["rec"]["flags"]
    assert (fl & fm.BYPASSED).any() and (fl & fm.NO_PLAN).any() and (fl[0] & fm.WAS_RESET).any() and not (fl[1] & fm.WAS_RESET).any()
