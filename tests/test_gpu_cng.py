"""-m gpu: igdsp_cng_run (include/igdsp.h, "Comfort noise") through the C ABI against tests/cng_model.py, bit for bit: rows, lengths,
records, PCM records, state.  Shapes around the kernel's ownership units (a lane owns a channel, a wave of 64 lanes is a block and
stores the frame's rows as a tile of 16-byte pieces): channels 1, 63, 64, 65, 130, 255, 256, 257, frames 1, 2, 9, samples per frame 16,
24 (three pieces a row: no power of two), 160 and 256, voice rows from mixed G.711 laws, from PCM and absent, every launch from fresh,
garbage-under-tag and wrong-tag states side by side.  Bit for bit as well: one launch against the same frames in several, a channel
at another position and channel count.  Every output set with guard bytes around every buffer and the state, the SID step under
every ballot pattern, waves without and with exactly one generating lane, every d_ctl value, d_seed, the chain igdsp_vad_run ->
igdsp_cng_run -> igdsp_conf_mix on the device, the argument clauses, the yardstick against its written promise, and one launch at
full-chip size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import cng_model as cm  # noqa: E402
from tests import conf_model  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import tdet_model  # noqa: E402
from tests import vad_model as vm  # noqa: E402

GUARD = 256
EINVAL, ERANGE = -22, -34
SB = capi.CNG_STATE.itemsize
NS = (16, 24, 160, 256)
CS = (1, 63, 64, 65, 130, 255, 256, 257)
STATE_GUARD = 0xA5
SIZES = dict(out=lambda F_, C_, n: F_ * C_ * n * 2, len=lambda F_, C_, n: F_ * C_ * 2, rec=lambda F_, C_, n: F_ * C_ * 16, stats=lambda F_, C_, n: F_ * C_ * 16)
ALL = ("out", "len", "rec", "stats")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def mixed_laws(C_):
    return np.where(np.arange(C_) % 3 == 1, 8, 0).astype(np.uint8)


def mixed_states(C_, seed):
    """channel by channel: garbage under the tag, a wrong tag over garbage, fresh"""
    st = cm.garbage_state(C_, seed)
    st[1::3] = cm.garbage_state(C_, seed + 1, tagged=False)[1::3]
    st[2::3] = np.zeros((), cm.STATE)
    return st


def mixed_ctl(C_):
    ctl = (np.arange(C_) % 5).astype(np.uint8)                             # RUN FREEZE BYPASS RESET 4 (as RUN)
    ctl[ctl == 4] = 200
    return ctl


def state_dev(state):
    b = np.ascontiguousarray(state).view(np.uint8).reshape(-1)
    g = np.full(GUARD, STATE_GUARD, np.uint8)
    return gu.to_dev(np.concatenate([g, b, g]))                            # guard bytes in front of the state and behind it


def run_cng(ctx, kind, sid, n, sid_len=None, voice=None, codec=None, ctl=None, seed=None, state=None, d_state=None, outputs=ALL, fill=0xEE, entry=None):
    """One launch through the C ABI (entry: through that yardstick instead).  kind [F][C], sid [F][C][16], sid_len [F][C] or None; voice
    [F][C][n]: uint8 codes (with codec [C]), int16 PCM or None; state [C] or None (all-zero), or d_state carried from an earlier launch.
    Returns the outputs, the state records and the state tensor (with its guards); guard bytes in front of and behind every output
    buffer and the state are checked."""
    torch = gu.torch_cuda()
    F_, C_ = np.asarray(kind).shape
    g711 = voice is not None and voice.dtype == np.uint8
    dev = lambda a, t: None if a is None else gu.to_dev(np.ascontiguousarray(a, t))
    d_kind, d_sid, d_len = dev(kind, np.uint8), dev(sid, np.uint8), dev(sid_len, np.uint8)
    d_v = None if voice is None else gu.to_dev(voice if g711 else np.asarray(voice, "<i2"))
    d_codec, d_ctl, d_seed = dev(codec if g711 else None, np.uint8), dev(ctl, np.uint8), dev(seed, "<u4")
    if d_state is None:
        d_state = state_dev(np.zeros(C_, capi.CNG_STATE) if state is None else state)
    sizes = {k: SIZES[k](F_, C_, n) for k in outputs}
    whole = {k: gu.dev_zeros(GUARD + v + GUARD, fill) for k, v in sizes.items()}      # guard bytes around every buffer
    bufs = {k: t[GUARD:] for k, t in whole.items()}                        # (GUARD keeps the allocation's alignment)
    p = lambda t: None if t is None else t.data_ptr()
    d_st = d_state[GUARD:]
    if entry:
        rc = capi.internal(entry)(ctx.h, p(d_kind), p(d_sid), p(d_len), p(d_v) if g711 else None, p(d_codec), None if g711 else p(d_v), p(d_ctl), p(d_seed),
                                  C_, F_, n, p(d_st), p(bufs.get("out")), p(bufs.get("len")), p(bufs.get("rec")), p(bufs.get("stats")), None)
        assert rc == 0, rc
    else:
        ctx.cng_run(d_kind, d_sid, d_st, bufs["out"], C_, F_, n, sid_len=d_len, g711=d_v if g711 else None, codec=d_codec, pcm=None if g711 else d_v,
                    ctl=d_ctl, seed=d_seed, len_out=bufs.get("len"), rec=bufs.get("rec"), stats=bufs.get("stats"))
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
    sbytes = sbytes[GUARD:]
    res = dict(d_state=d_state, state=sbytes[:C_ * SB].view(capi.CNG_STATE).copy())
    res["out"] = host["out"][:sizes["out"]].view("<i2").reshape(F_, C_, n)
    if "len" in host:
        res["len"] = host["len"][:sizes["len"]].view("<u2").reshape(F_, C_)
    if "rec" in host:
        res["rec"] = host["rec"][:sizes["rec"]].view(capi.CNG_REC).reshape(F_, C_)
    if "stats" in host:
        res["stats"] = host["stats"][:sizes["stats"]].view(capi.FRAME_STATS).reshape(F_, C_)
    return res


def pcm_of(voice, codec):
    if voice is None:
        return None
    return tdet_model.decode(voice, codec) if voice.dtype == np.uint8 else np.asarray(voice, np.int16)


def check(got, model):
    out, ln, rec, stats, st = model
    assert np.array_equal(got["out"], out), np.argwhere(got["out"] != out)[:6]
    if "len" in got:
        assert np.array_equal(got["len"], ln), np.argwhere(got["len"] != ln)[:6]
    if "rec" in got:
        assert got["rec"].tobytes() == rec.tobytes(), [(k, np.argwhere(got["rec"][k] != rec[k])[:4].tolist()) for k in rec.dtype.names
                                                        if not np.array_equal(got["rec"][k], rec[k])]
    if "stats" in got:
        gu.assert_stats_equal(got["stats"], stats)
    assert got["state"].tobytes() == st.tobytes(), [(k, np.argwhere(got["state"][k] != st[k])[:4].tolist()) for k in st.dtype.names
                                                    if not np.array_equal(got["state"][k], st[k])]


def scene(C_, F_, n, seed, form):
    """kinds that drive every branch, payloads of every length and order, voice rows as codes of mixed laws, as PCM or absent"""
    rng = np.random.default_rng(seed)
    kind = rng.choice(np.array([cm.NONE, cm.NONE, cm.SID, cm.VOICE, cm.VOICE, 9], np.uint8), (F_, C_))
    sid = np.clip(127 + rng.normal(0, 45, (F_, C_, 16)), 0, 255).astype(np.uint8)
    sid[:, :, 0] = rng.integers(0, 70, (F_, C_))
    sid_len = rng.integers(0, 17, (F_, C_)).astype(np.uint8)
    if form == "none":
        return kind, sid, sid_len, None, None
    x = rng.integers(-32768, 32768, (F_, C_, n)).astype(np.int16)
    x[:, ::5] //= 256
    if form == "pcm":
        return kind, sid, sid_len, x, None
    codec = mixed_laws(C_)
    return kind, sid, sid_len, tdet_model.encode(x, codec), codec


def model(kind, sid, n, sid_len, voice, codec, **kw):
    return cm.run(kind, sid, n, sid_len=sid_len, voice=pcm_of(voice, codec), **kw)


# ---- 1. the shapes, voice rows from codes, from PCM and absent, all three kinds of state, with and without d_ctl, d_seed and d_sid_len
@pytest.mark.parametrize("form", ("g711", "pcm", "none"))
@pytest.mark.parametrize("n", NS)
def test_shapes(ctx, n, form):
    seen = 0
    for i, C_ in enumerate(CS):
        F_ = (1, 2, 9)[i % 3]
        kind, sid, sid_len, v, codec = scene(C_, F_, n, 10 * n + C_, form)
        st = mixed_states(C_, n + C_)
        ctl = mixed_ctl(C_) if i % 2 else None
        seed = np.arange(C_, dtype=np.uint32) * 2654435761 if i % 3 else None
        sl = sid_len if i % 4 else None
        m = model(kind, sid, n, sl, v, codec, ctl=ctl, seed=seed, state=st)
        check(run_cng(ctx, kind, sid, n, sl, v, codec, ctl=ctl, seed=seed, state=st), m)
        seen |= int(np.bitwise_or.reduce(m[2]["flags"].reshape(-1)))
    assert seen & 0xEF == 0xEF, hex(seen)                                  # every flag but CLIPPED, which test_rare_branch drives


# ---- 2. the invariants: a split of the frames, position and count
def test_split_and_position(ctx):
    C_, F_, n = 70, 9, 160
    kind, sid, sid_len, v, codec = scene(C_, F_, n, 5, "g711")
    st = mixed_states(C_, 4)
    seed = np.arange(C_, dtype=np.uint32) + 99
    whole = run_cng(ctx, kind, sid, n, sid_len, v, codec, seed=seed, state=st)
    check(whole, model(kind, sid, n, sid_len, v, codec, seed=seed, state=st))
    for cuts in ((9,), tuple(range(1, 10)), (2, 3, 9)):
        d_state, a, parts = None, 0, []
        for b in cuts:
            parts.append(run_cng(ctx, kind[a:b], sid[a:b], n, sid_len[a:b], v[a:b], codec, seed=seed, state=st if a == 0 else None, d_state=d_state))
            d_state, a = parts[-1]["d_state"], b
        for k in ALL:
            assert np.concatenate([q[k] for q in parts]).tobytes() == whole[k].tobytes(), (cuts, k)
        assert parts[-1]["state"].tobytes() == whole["state"].tobytes(), cuts
    # channel 4's inputs and state at index 0, in the second wave and at the last index of a 131-channel launch
    idx = np.arange(131) % C_
    idx[0], idx[77], idx[-1] = 4, 4, 4
    big = run_cng(ctx, kind[:, idx], sid[:, idx], n, sid_len[:, idx], v[:, idx], codec[idx], seed=seed[idx], state=st[idx])
    for k in ALL:
        assert np.array_equal(big[k], whole[k][:, idx]), k
    assert big["state"].tobytes() == whole["state"][idx].tobytes()
    assert big["out"][:, 0].tobytes() == big["out"][:, 77].tobytes() == big["out"][:, -1].tobytes() == whole["out"][:, 4].tobytes()


# ---- 3. every output set
@pytest.mark.parametrize("outputs", (ALL, ("out",), ("out", "len"), ("out", "rec"), ("out", "stats"), ("out", "len", "rec"), ("out", "len", "stats"),
                                     ("out", "rec", "stats")))                 # d_out is required: all eight subsets of the other three
def test_output_sets(ctx, outputs):
    C_, F_, n = 67, 3, 24
    kind, sid, sid_len, v, codec = scene(C_, F_, n, 6, "pcm" if ("len" in outputs) != ("rec" in outputs) else "g711")
    st = mixed_states(C_, 3)
    check(run_cng(ctx, kind, sid, n, sid_len, v, codec, state=st, outputs=outputs), model(kind, sid, n, sid_len, v, codec, state=st))


# ---- 4. the rare branch: in wave 0 every channel takes its SID in another frame and at another order 0..10 (every ballot pattern of
# the SID step); wave 1 is voice throughout (no lane generates); in wave 2 exactly one lane generates; wave 3 takes level 0 (CLIPPED)
def test_rare_branch(ctx):
    C_, F_, n = 256, 11, 160
    rng = np.random.default_rng(8)
    kind = np.zeros((F_, C_), np.uint8)
    sid = np.clip(127 + rng.normal(0, 45, (F_, C_, 16)), 0, 255).astype(np.uint8)
    sid[:, :, 0] = 30 + np.arange(C_) % 40
    sid_len = np.zeros((F_, C_), np.uint8)
    c = np.arange(64)
    kind[c % F_, c] = cm.SID
    kind[(c + 5) % F_, c] = np.where(c % 3 == 0, cm.SID, cm.NONE)          # a second SID on every third channel
    sid_len[:, :64] = (c * 7) % 11 + 1                                     # order 0..10
    kind[:, 64:192] = cm.VOICE
    kind[:, 64 + 128 - 47] = cm.NONE
    kind[0, 64 + 128 - 47] = cm.SID
    sid_len[:, 64:] = 11
    kind[0, 192:] = cm.SID
    sid[0, 192:, 0] = 0
    x = rng.integers(-3000, 3000, (F_, C_, n)).astype(np.int16)
    m = cm.run(kind, sid, n, sid_len=sid_len, voice=x)
    check(run_cng(ctx, kind, sid, n, sid_len, x), m)
    fl = m[2]["flags"]
    assert ((fl[:, :64] & cm.F_SID) != 0).sum(axis=0).min() >= 1 and sorted(set(m[4]["order"][:64].tolist())) == list(range(11))
    assert (fl[:, 64:128] == cm.F_VOICE).all() and ((fl[:, 128:192] & cm.F_GENERATED) != 0).sum() == F_
    assert (fl[:, 192:] & cm.F_CLIPPED).any() and (fl[:, :64] & cm.F_NO_MODEL).any()


# ---- 5. control and state: every d_ctl value over every kind of state, the wrong tag with and without d_seed
@pytest.mark.parametrize("with_seed", (False, True))
def test_ctl_states_and_seed(ctx, with_seed):
    C_, F_, n = 75, 4, 24
    kind, sid, sid_len, v, codec = scene(C_, F_, n, 31, "pcm")
    kind[0, ::2] = cm.SID
    sid_len[0] = 11
    seed = (np.arange(C_, dtype=np.uint32) * 40503 + 1) if with_seed else None
    for s in range(3):
        st = np.roll(mixed_states(C_, 20 + s), s)
        ctl = (np.arange(C_) // 3 % 5).astype(np.uint8)                    # every ctl over every kind of state
        ctl[ctl == 4] = 77
        m = model(kind, sid, n, sid_len, v, codec, ctl=ctl, seed=seed, state=st)
        got = run_cng(ctx, kind, sid, n, sid_len, v, codec, ctl=ctl, seed=seed, state=st)
        check(got, m)
        byp = ctl == cm.BYPASS
        assert got["state"][byp].tobytes() == st[byp].tobytes() and (m[2]["flags"][:, byp] == cm.F_BYPASSED).all()
        fresh = ((st["tag"] != cm.TAG) | (ctl == cm.RESET)) & ~byp
        assert np.array_equal(got["state"]["seed"][fresh], (seed[fresh] if with_seed else np.zeros(fresh.sum(), np.uint32)))
        assert np.array_equal(got["state"]["seed"][~fresh & ~byp], st["seed"][~fresh & ~byp])


# ---- 6. the chain on the device: igdsp_vad_run with DTX -> igdsp_cng_run -> igdsp_conf_mix, against the three models chained
def test_chain_vad_cng_conf(ctx):
    torch = gu.torch_cuda()
    C_, F_, n, P_ = 70, 14, 160, 5
    x = vm.scene(F_, C_, n, 41, rms=100, burst=(4, 8)).astype(np.int16)
    codec = mixed_laws(C_)
    g711 = tdet_model.encode(x, codec)
    pcm = tdet_model.decode(g711, codec)
    kind, vrec, sid, _, _ = vm.run(None, pcm)
    assert (kind == vm.SID).any() and (kind == vm.NONE).any() and (kind == vm.VOICE).any()
    d_g, d_codec = gu.to_dev(g711), gu.to_dev(codec)
    d_kind, d_vrec, d_sid = gu.dev_zeros(F_ * C_), gu.dev_zeros(F_ * C_ * 16), gu.dev_zeros(F_ * C_ * 16)
    vst = gu.to_dev(np.zeros(C_, capi.VAD_STATE).view(np.uint8).reshape(-1))
    ctx.vad_run(vst, C_, F_, n, g711=d_g, codec=d_codec, kind=d_kind, rec=d_vrec, sid=d_sid)
    d_sid_len = d_vrec.view(F_ * C_, 16)[:, 14].contiguous()               # the records' sid_len
    seed = np.arange(C_, dtype=np.uint32) + 0x5000
    d_out, d_len = gu.dev_zeros(F_ * C_ * n * 2), gu.dev_zeros(F_ * C_ * 2)
    cst = gu.to_dev(np.zeros(C_, capi.CNG_STATE).view(np.uint8).reshape(-1))
    ctx.cng_run(d_kind, d_sid, cst, d_out, C_, F_, n, sid_len=d_sid_len, g711=d_g, codec=d_codec, seed=gu.to_dev(seed), len_out=d_len)
    ch, pt = np.arange(C_), np.arange(C_) % P_
    ptr, mem = capi.conf_build(ch, pt, C_, P_)
    gain = np.full(C_, 128, np.uint16)
    d_mix, d_ms = gu.dev_zeros(F_ * P_ * n * 2), gu.dev_zeros(F_ * P_ * 16)
    ctx.conf_mix(gu.to_dev(gain), gu.to_dev(ptr), gu.to_dev(mem), len(mem), C_, P_, F_, n, out=d_mix, stats=d_ms, pcm=d_out, length=d_len)
    torch.cuda.synchronize()
    assert np.array_equal(gu.to_host(d_kind, np.uint8, (F_, C_)), kind) and np.array_equal(gu.to_host(d_sid, np.uint8, (F_, C_, 16)), sid)
    out, ln, rec, _, _ = cm.run(kind, sid, n, sid_len=vrec["sid_len"], voice=pcm, seed=seed)
    assert np.array_equal(gu.to_host(d_out, "<i2", (F_, C_, n)), out) and np.array_equal(gu.to_host(d_len, "<u2", (F_, C_)), ln)
    gen = (rec["flags"] & cm.F_GENERATED) != 0
    assert gen.any() and np.array_equal(gen, (kind != vm.VOICE) & (np.cumsum(kind == vm.SID, axis=0) > 0))
    eo, es = conf_model.mix(out.astype(np.int64), gain, ptr, mem, len(mem), P_, ln)
    assert np.array_equal(gu.to_host(d_mix, "<i2", (F_, P_, n)), eo)
    got = gu.to_host(d_ms, capi.FRAME_STATS, (F_, P_))
    assert np.array_equal(got["sumsq"], es["sumsq"]) and np.array_equal(got["peak"], es["peak"]) and np.array_equal(got["flags"], es["flags"])


# ---- 7. the argument clauses through the C ABI
def test_argument_paths(ctx):
    L = capi.load()
    C_, F_, n = 4, 2, 160
    kind, sid, sid_len, v, codec = scene(C_, F_, n, 1, "g711")
    d = dict(kind=gu.to_dev(kind), sid=gu.to_dev(sid), sl=gu.to_dev(sid_len), g=gu.to_dev(v), codec=gu.to_dev(codec), pcm=gu.to_dev(pcm_of(v, codec)),
             ctl=gu.to_dev(np.zeros(C_, np.uint8)), seed=gu.to_dev(np.zeros(C_, "<u4")), st=gu.dev_zeros(C_ * SB + 64), out=gu.dev_zeros(F_ * C_ * n * 2 + 64),
             len=gu.dev_zeros(F_ * C_ * 2 + 64), rec=gu.dev_zeros(F_ * C_ * 16 + 64), stats=gu.dev_zeros(F_ * C_ * 16 + 64))
    p = {k: t.data_ptr() for k, t in d.items()}

    def call(h=ctx.h, kind=p["kind"], sid=p["sid"], sl=p["sl"], g=None, codec=None, pcm=p["pcm"], ctl=p["ctl"], seed=p["seed"], C=C_, F=F_, nn=n, st=p["st"],
             out=p["out"], ln=p["len"], rec=p["rec"], stats=p["stats"]):
        return L.igdsp_cng_run(h, kind, sid, sl, g, codec, pcm, ctl, seed, C, F, nn, st, out, ln, rec, stats, None)

    assert call() == 0 and call(sl=None, ctl=None, seed=None) == 0 and call(pcm=None) == 0 and call(g=p["g"], codec=p["codec"], pcm=None) == 0
    assert call(ln=None, rec=None, stats=None) == 0
    assert call(h=None) == EINVAL
    for nn in (0, 8, 20, 161, 264):
        assert call(nn=nn) == EINVAL and call(nn=nn, C=0) == EINVAL       # checked whether or not there is work
    assert call(C=0) == 0 and call(F=0) == 0 and call(C=0, st=None, out=None, kind=None, sid=None) == 0
    assert call(kind=None) == EINVAL and call(sid=None) == EINVAL and call(st=None) == EINVAL and call(out=None) == EINVAL
    assert call(g=p["g"], codec=p["codec"]) == EINVAL and call(g=p["g"], pcm=None) == EINVAL      # both inputs; codes without d_codec
    assert call(C=1 << 20, F=1 << 12) == ERANGE
    assert call(pcm=p["pcm"] + 8) == EINVAL and call(g=p["g"] + 4, codec=p["codec"], pcm=None) == EINVAL
    assert call(g=p["g"] + 8, codec=p["codec"], pcm=None, F=1) == 0
    for k in ("sid", "st", "out", "rec", "stats"):
        assert call(**{k: p[k] + 8}) == EINVAL, k
    assert call(out=p["pcm"]) == EINVAL and call(rec=p["stats"]) == EINVAL and call(st=p["seed"]) == EINVAL and call(ln=p["kind"]) == EINVAL
    assert b"overlap" in L.igdsp_last_error(ctx.h)
    gu.torch_cuda().cuda.synchronize()


# ---- 8. the yardstick: the same arguments, 0, and its written promise: the bytes of every channel at IGDSP_CNG_BYPASS, d_ctl not read,
# the state written back as it was read, clamped, with the tag
@pytest.mark.parametrize("form", ("g711", "pcm", "none"))
def test_yardstick_promise(ctx, form):
    C_, F_, n = 83, 3, 160
    kind, sid, sid_len, v, codec = scene(C_, F_, n, 12, form)
    st = mixed_states(C_, 8)
    seed = np.arange(C_, dtype=np.uint32) + 7
    out, ln, rec, stats, _ = model(kind, sid, n, sid_len, v, codec, ctl=np.full(C_, cm.BYPASS, np.uint8), seed=seed, state=st)
    want = cm.yardstick_state(st, seed)
    assert (rec["flags"] == cm.F_BYPASSED).all() and (want["tag"] == cm.TAG).all() and not want["reserved"].any()
    got = run_cng(ctx, kind, sid, n, sid_len, v, codec, ctl=np.full(C_, cm.RESET, np.uint8), seed=seed, state=st, entry="cng_move")
    check(got, (out, ln, rec, stats, want))
    for outputs in (("out",), ("out", "rec"), ("out", "len", "stats")):
        check(run_cng(ctx, kind, sid, n, sid_len, v, codec, seed=seed, state=st, outputs=outputs, entry="cng_move"), (out, ln, rec, stats, want))


# ---- 9. the full chip: 65 536 channels x 2 frames in one launch, a sampled comparison
def test_full_chip(ctx):
    C_, F_, n = 65536, 2, 160
    rng = np.random.default_rng(21)
    kind = rng.choice(np.array([cm.NONE, cm.SID, cm.SID, cm.VOICE], np.uint8), (F_, C_))
    sid = np.clip(127 + rng.normal(0, 45, (F_, C_, 16)), 0, 255).astype(np.uint8)
    sid[:, :, 0] = rng.integers(10, 70, (F_, C_))
    codec = mixed_laws(C_)
    codes = rng.integers(0, 256, (F_, C_, n), dtype=np.uint8)
    st = mixed_states(C_, 5)
    ctl = mixed_ctl(C_)
    seed = rng.integers(0, 1 << 32, C_, dtype=np.uint64).astype(np.uint32)
    got = run_cng(ctx, kind, sid, n, None, codes, codec, ctl=ctl, seed=seed, state=st)
    sample = np.sort(rng.choice(C_, 384, replace=False))
    sample[0], sample[-1] = 0, C_ - 1
    m = model(kind[:, sample], sid[:, sample], n, None, codes[:, sample], codec[sample], ctl=ctl[sample], seed=seed[sample], state=st[sample])
    check({k: (got[k][:, sample] if k in ALL else got[k][sample]) for k in ALL + ("state",)}, m)
    fl = got["rec"]["flags"]
    assert (fl & cm.F_SID).any() and (fl & cm.F_GENERATED).any() and (fl & cm.F_BYPASSED).any() and (fl & cm.F_VOICE).any()
    live = got["len"] == n
    assert np.array_equal(live, ((fl & (cm.F_GENERATED | cm.F_VOICE)) != 0) | ((fl == cm.F_BYPASSED) & (kind == cm.VOICE)))
    assert not got["out"][~live].any()
