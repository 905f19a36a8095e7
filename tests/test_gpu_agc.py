"""-m gpu: igdsp_agc_run (include/igdsp.h, "Level control") through the C ABI against tests/agc_model.py, bit for bit: output, records,
PCM records, state.  Shapes around the kernel's ownership units (32 lanes own a channel, a lane a block of 8 samples, a wave two
channels, a block of threads 8): channels 1, 2, 3, 5, 7, 8, 9, frames 1, 2, 3, samples per frame 8 (one block, two knots), 16, 24,
160 (20 of 32 lanes busy) and 256 (all 32), from mixed G.711 laws and from PCM, every launch from fresh, garbage-under-tag and
wrong-tag states side by side.  Bit for bit as well: one launch against the same frames in several, a channel at another position and
channel count, G.711 against its decoded PCM.  Every output set, every d_ctl value and d_ctl NULL, guard bytes behind every buffer
and behind the state, the argument clauses, the yardstick against its written promise, and one launch at full-chip size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import agc_model as am  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import tdet_model  # noqa: E402

GUARD = 256
EINVAL, ERANGE = -22, -34
SB = capi.AGC_STATE.itemsize
NS = (8, 16, 24, 160, 256)
SHAPES = ((1, 1), (2, 2), (3, 3), (5, 2), (7, 3), (8, 1), (9, 2))          # (C, F): a block of threads owns 8 channels
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
    st = am.garbage_state(C_, seed)
    st[1::3] = am.garbage_state(C_, seed + 1, tagged=False)[1::3]
    st[2::3] = np.zeros((), am.STATE)
    return st


def mixed_ctl(C_):
    ctl = (np.arange(C_) % 5).astype(np.uint8)                             # RUN FREEZE BYPASS RESET 4 (as RUN)
    ctl[ctl == 4] = 200
    return ctl


def state_dev(state):
    b = np.ascontiguousarray(state).view(np.uint8).reshape(-1)
    return gu.to_dev(np.concatenate([b, np.full(GUARD, STATE_GUARD, np.uint8)]))


def run_agc(ctx, x, cfg=None, codec=None, ctl=None, state=None, d_state=None, outputs=ALL, fill=0xEE, entry=None):
    """One launch through the C ABI (entry: through that yardstick instead).  x [F][C][n]: uint8 codes (with codec [C]) or int16 PCM;
    state [C] or None (all-zero), or d_state carried from an earlier launch.  Returns the outputs, the state records and the state
    tensor; guard bytes behind every buffer are checked."""
    torch = gu.torch_cuda()
    F_, C_, n = x.shape
    g711 = x.dtype == np.uint8
    d_x = gu.to_dev(x if g711 else np.asarray(x, "<i2"))
    d_codec = gu.to_dev(np.asarray(codec, np.uint8)) if g711 else None
    d_ctl = gu.to_dev(np.asarray(ctl, np.uint8)) if ctl is not None else None
    if d_state is None:
        d_state = state_dev(np.zeros(C_, capi.AGC_STATE) if state is None else state)
    sizes = {k: SIZES[k](F_, C_, n) for k in outputs}
    bufs = {k: gu.dev_zeros(v + GUARD, fill) for k, v in sizes.items()}
    p = lambda t: None if t is None else t.data_ptr()
    if entry:
        c = None if cfg is None else np.ascontiguousarray(cfg, capi.AGC_CFG)
        rc = capi.internal(entry)(ctx.h, p(d_x) if g711 else None, p(d_codec), None if g711 else p(d_x), p(d_ctl), None if c is None else c.ctypes.data,
                                  C_, F_, n, p(d_state), p(bufs.get("out")), p(bufs.get("rec")), p(bufs.get("stats")), None)
        assert rc == 0, rc
    else:
        ctx.agc_run(d_state, C_, F_, n, g711=d_x if g711 else None, codec=d_codec, pcm=None if g711 else d_x, ctl=d_ctl, cfg=cfg,
                    out=bufs.get("out"), rec=bufs.get("rec"), stats=bufs.get("stats"))
    torch.cuda.synchronize()
    host = {k: t.cpu().numpy() for k, t in bufs.items()}
    for k, b in host.items():
        assert np.all(b[sizes[k]:] == fill), f"bytes after d_{k} written"
    sbytes = d_state.cpu().numpy()
    assert len(sbytes) == C_ * SB + GUARD and np.all(sbytes[C_ * SB:] == STATE_GUARD), "bytes after d_state written"
    res = dict(d_state=d_state, state=sbytes[:C_ * SB].view(capi.AGC_STATE).copy())
    if "out" in host:
        res["out"] = host["out"][:sizes["out"]].view("<i2").reshape(F_, C_, n)
    if "rec" in host:
        res["rec"] = host["rec"][:sizes["rec"]].view(capi.AGC_REC).reshape(F_, C_)
    if "stats" in host:
        res["stats"] = host["stats"][:sizes["stats"]].view(capi.FRAME_STATS).reshape(F_, C_)
    return res


def pcm_of(x, codec):
    return tdet_model.decode(x, codec) if x.dtype == np.uint8 else np.asarray(x, np.int16)


def check(got, model):
    out, rec, stats, st = model[:4]
    if "out" in got:
        assert np.array_equal(got["out"], out), np.argwhere(got["out"] != out)[:6]
    if "rec" in got:
        assert got["rec"].tobytes() == rec.tobytes(), [(k, np.argwhere(got["rec"][k] != rec[k])[:4].tolist()) for k in rec.dtype.names
                                                        if not np.array_equal(got["rec"][k], rec[k])]
    if "stats" in got:
        gu.assert_stats_equal(got["stats"], stats)
    assert got["state"].tobytes() == st.tobytes(), [(k, np.argwhere(got["state"][k] != st[k])[:4].tolist()) for k in st.dtype.names
                                                    if not np.array_equal(got["state"][k], st[k])]


def scene(C_, F_, n, seed, law):
    """rows that drive every branch, as codes of mixed laws or as PCM"""
    x = am.mixed_scene(F_, C_, n, seed).astype(np.int16)
    if not law:
        return x, None
    codec = mixed_laws(C_)
    return tdet_model.encode(x, codec), codec


# ---- 1. the shapes, from codes and from PCM, all three kinds of state, with and without d_ctl
@pytest.mark.parametrize("law", ("g711", "pcm"))
@pytest.mark.parametrize("n", NS)
def test_shapes(ctx, n, law):
    seen = 0
    for i, (C_, F_) in enumerate(SHAPES):
        x, codec = scene(C_, F_, n, 10 * n + C_, law == "g711")
        st = mixed_states(C_, n + C_)
        ctl = mixed_ctl(C_) if i % 2 else None
        cfg = None if i % 3 == 0 else am.cfg_default(ceil=20000 + 1000 * i, lrel=1 + i, gmax=65535, att=i % 4)
        m = am.run(am.cfg_default() if cfg is None else cfg, pcm_of(x, codec), ctl=ctl, state=st)
        check(run_agc(ctx, x, cfg, codec, ctl=ctl, state=st), m)
        seen |= int(np.bitwise_or.reduce(m[1]["flags"].reshape(-1)))
    assert seen & am.LIMITED and seen & am.ACTIVE and seen & am.ATTACKED and seen & am.BYPASSED and seen & am.FROZEN, seen


# ---- 2. the invariants: a split of the frames, position and count, G.711 against its PCM
def test_split_position_and_form(ctx):
    C_, F_, n = 9, 3, 160
    cfg = am.cfg_default()
    x, codec = scene(C_, F_ + 3, n, 5, True)
    st = am.run(cfg, pcm_of(x[:3], codec))[3]                              # the state the scene's first frames leave
    x = x[3:]
    whole = run_agc(ctx, x, cfg, codec, state=st)
    check(whole, am.run(cfg, pcm_of(x, codec), state=st))
    for cuts in ((3,), (1, 3), (1, 2, 3)):
        d_state, a, parts = None, 0, []
        for b in cuts:
            parts.append(run_agc(ctx, x[a:b], cfg, codec, state=st if a == 0 else None, d_state=d_state))
            d_state, a = parts[-1]["d_state"], b
        for k in ALL:
            assert np.concatenate([q[k] for q in parts]).tobytes() == whole[k].tobytes(), (cuts, k)
        assert parts[-1]["state"].tobytes() == whole["state"].tobytes(), cuts
    pcm = run_agc(ctx, pcm_of(x, codec), cfg, state=st)                    # from the decoded PCM: the same bytes
    for k in ALL + ("state",):
        assert pcm[k].tobytes() == whole[k].tobytes(), k
    # channel 4's input and state at index 0 and at the last index of a 37-channel launch
    idx = np.arange(37) % C_
    idx[0], idx[-1] = 4, 4
    big = run_agc(ctx, x[:, idx], cfg, codec[idx], state=st[idx])
    for k in ALL:
        assert np.array_equal(big[k], whole[k][:, idx]), k
    assert big["state"].tobytes() == whole["state"][idx].tobytes()
    assert big["out"][:, 0].tobytes() == big["out"][:, -1].tobytes() == whole["out"][:, 4].tobytes()


# ---- 3. every output set
@pytest.mark.parametrize("outputs", (ALL, ("rec", "stats"), ("out",), ("rec",), ("stats",)))
def test_output_sets(ctx, outputs):
    C_, F_, n = 6, 3, 160
    x, codec = scene(C_, F_, n, 6, len(outputs) % 2 == 1)
    st = mixed_states(C_, 3)
    check(run_agc(ctx, x, None, codec, state=st, outputs=outputs), am.run(am.cfg_default(), pcm_of(x, codec), state=st))


# ---- 4. every control value and d_ctl NULL, on every kind of state
def test_ctl_and_states(ctx):
    C_, F_, n = 15, 3, 24
    cfg = am.cfg_default()
    x, _ = scene(C_, F_, n, 9, False)
    st = mixed_states(C_, 4)                                               # 15 channels: every (ctl, kind of state) pair
    ctl = mixed_ctl(C_)
    m = am.run(cfg, x, ctl=ctl, state=st)
    got = run_agc(ctx, x, cfg, ctl=ctl, state=st)
    check(got, m)
    byp = ctl == am.BYPASS
    assert got["state"][byp].tobytes() == st[byp].tobytes() and np.array_equal(got["out"][:, byp], x[:, byp])
    check(run_agc(ctx, x, cfg, state=st), am.run(cfg, x, state=st))        # d_ctl NULL


# ---- 5. the argument clauses through the C ABI
def test_argument_paths(ctx):
    L = capi.load()
    C_, F_, n = 4, 2, 160
    x, codec = scene(C_, F_, n, 1, True)
    d = dict(g=gu.to_dev(x), codec=gu.to_dev(codec), pcm=gu.to_dev(pcm_of(x, codec)), ctl=gu.to_dev(np.zeros(C_, np.uint8)), st=gu.dev_zeros(C_ * SB + 64),
             out=gu.dev_zeros(F_ * C_ * n * 2 + 64), rec=gu.dev_zeros(F_ * C_ * 16 + 64), stats=gu.dev_zeros(F_ * C_ * 16 + 64))
    p = {k: t.data_ptr() for k, t in d.items()}
    cfg = np.ascontiguousarray(am.cfg_default(), capi.AGC_CFG)

    def call(h=ctx.h, g=None, codec=None, pcm=p["pcm"], ctl=p["ctl"], c=cfg, C=C_, F=F_, nn=n, st=p["st"], out=p["out"], rec=p["rec"], stats=p["stats"]):
        return L.igdsp_agc_run(h, g, codec, pcm, ctl, None if c is None else c.ctypes.data, C, F, nn, st, out, rec, stats, None)

    assert call() == 0 and call(c=None) == 0 and call(ctl=None, out=None, rec=None) == 0 and call(g=p["g"], codec=p["codec"], pcm=None) == 0
    assert call(h=None) == EINVAL
    for nn in (0, 4, 12, 161, 264):
        assert call(nn=nn) == EINVAL and call(nn=nn, C=0) == EINVAL       # checked whether or not there is work
    for k, v in (("gate", 0), ("target", 30000), ("ceil", 40000), ("gmin", 5000), ("gmax", 100), ("att", 16), ("lrel", 0)):
        bad = cfg.copy()
        bad[k] = v
        assert call(c=bad) == EINVAL and call(c=bad, F=0) == EINVAL
    assert call(C=0) == 0 and call(F=0) == 0 and call(C=0, st=None, pcm=None) == 0
    assert call(g=p["g"], codec=p["codec"]) == EINVAL and call(pcm=None) == EINVAL and call(g=p["g"], pcm=None) == EINVAL      # both, neither, no codec
    assert call(st=None) == EINVAL and call(out=None, rec=None, stats=None) == EINVAL
    assert call(C=1 << 20, F=1 << 12) == ERANGE
    assert call(pcm=p["pcm"] + 8) == EINVAL and call(out=p["out"] + 8) == EINVAL and call(g=p["g"] + 4, codec=p["codec"], pcm=None) == EINVAL
    assert call(g=p["g"] + 8, codec=p["codec"], pcm=None, F=1) == 0
    assert call(stats=p["stats"] + 4) == EINVAL and call(rec=p["rec"] + 8) == EINVAL and call(st=p["st"] + 8) == EINVAL
    assert call(out=p["pcm"]) == EINVAL and call(rec=p["stats"]) == EINVAL and call(st=p["ctl"]) == EINVAL     # an output over an input / another output
    assert b"overlap" in L.igdsp_last_error(ctx.h)
    gu.torch_cuda().cuda.synchronize()


# ---- 6. the yardstick: the same arguments, 0, and its written promise: rows, records and PCM records of every channel at
# IGDSP_AGC_BYPASS, d_ctl not read, the state written as it was read with flags BYPASSED
@pytest.mark.parametrize("law", ("g711", "pcm"))
def test_yardstick_promise(ctx, law):
    C_, F_, n = 11, 3, 160
    cfg = am.cfg_default()
    x, codec = scene(C_, F_, n, 12, law == "g711")
    st = mixed_states(C_, 8)
    got = run_agc(ctx, x, cfg, codec, ctl=np.full(C_, am.RESET, np.uint8), state=st, entry="agc_move")
    out, rec, stats, _ = am.run(cfg, pcm_of(x, codec), ctl=np.full(C_, am.BYPASS, np.uint8), state=st)
    want = np.zeros(C_, am.STATE)
    keep = st["tag"] == am.TAG
    want["tag"], want["flags"] = am.TAG, am.BYPASSED
    want["env"], want["cap"] = np.where(keep, st["env"], 0), np.where(keep, st["cap"], am.CAP)
    want["gain"] = np.where(keep, np.clip(st["gain"], cfg["gmin"], cfg["gmax"]), am.UNITY)
    check(got, (out, rec, stats, want))
    assert np.array_equal(got["out"], pcm_of(x, codec))
    for outputs in (("rec", "stats"), ("out",)):
        check(run_agc(ctx, x, cfg, codec, state=st, outputs=outputs, entry="agc_move"), (out, rec, stats, want))


# ---- 7. the full chip: 65 536 channels x 2 frames of mixed laws in one launch
def test_full_chip(ctx):
    C_, F_, n = 65536, 2, 160
    rng = np.random.default_rng(21)
    codec = mixed_laws(C_)
    codes = rng.integers(0, 256, (F_, C_, n), dtype=np.uint8)              # every code of both laws: levels spread over 60 dB
    c4 = np.arange(C_) % 4
    alaw = (codec == 8)[None, :, None]
    codes = np.where((c4 == 1)[None, :, None], np.where(alaw, (codes & 0x8F) | 0x50, codes | 0x70), codes)      # segment 0: under the gate
    codes = np.where((c4 == 2)[None, :, None], codes | 0x40, codes).astype(np.uint8)                           # segments 0 .. 3: quiet rows
    pcm = pcm_of(codes, codec)
    st = mixed_states(C_, 5)
    ctl = mixed_ctl(C_)
    cfg = am.cfg_default()
    got = run_agc(ctx, codes, cfg, codec, ctl=ctl, state=st)
    parts = [am.run(cfg, pcm[:, a:a + 8192], ctl=ctl[a:a + 8192], state=st[a:a + 8192]) for a in range(0, C_, 8192)]
    out, rec, stats = (np.concatenate([q[i] for q in parts], axis=1) for i in range(3))
    state = np.concatenate([q[3] for q in parts])
    sample = np.sort(rng.choice(C_, 256, replace=False))
    sample[0], sample[-1] = 0, C_ - 1
    check({k: (got[k][:, sample] if k in ALL else got[k][sample]) for k in ALL + ("state",)}, (out[:, sample], rec[:, sample], stats[:, sample], state[sample]))
    w = (np.arange(n, dtype=np.int64) * 2654435761 % 65521)[None, None, :]
    assert np.array_equal((got["out"].astype(np.int64) * w).sum(axis=2), (out.astype(np.int64) * w).sum(axis=2))
    assert got["rec"].tobytes() == rec.tobytes() and got["state"].tobytes() == state.tobytes()
    gu.assert_stats_equal(got["stats"], stats)
    assert (rec["flags"] & am.LIMITED).mean() > 0.2 and (rec["flags"] & am.ATTACKED).any()
