"""-m gpu: igdsp_echo_cancel (include/igdsp.h, "Echo canceller") through the C ABI against tests/ec_model.py, bit for bit: output,
records, PCM records, state.  Shapes around the kernel's ownership units (16 lanes own a channel, a wave four, a block 16; a last block
shorter than 8 samples takes the masked path): (C, F, n) in (1, 1, 160), (3, 7, 24), (4, 5, 164), (5, 2, 160), (67, 3, 160), (5, 2, 256),
(3, 4, 2), at both tails, the near end from mixed laws and from PCM, d_far_of sharing rows with one index out of range.  Every launch
starts from the state the model reached over three earlier frames of the scene, so adaptation and a running hang are live at frame 0.
Bit for bit as well: one launch against the same frames in several, a channel at another position and channel count, G.711 against its
decoded PCM.  Every optional output absent in turn, every d_ctl value, guard bytes behind every buffer and behind the state, a garbage
state, the argument clauses, the yardstick against its written promise, and igdsp_conf_mix -> igdsp_echo_cancel on the device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import ec_model as em  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import tdet_model  # noqa: E402

GUARD = 256
EINVAL, ERANGE = -22, -34
SB = capi.EC_STATE.itemsize
SHAPES = ((1, 1, 160), (3, 7, 24), (4, 5, 164), (5, 2, 160), (67, 3, 160), (5, 2, 256), (3, 4, 2))
TAILS = (128, 256)
PRE = 3
STATE_GUARD = 0xA5
SIZES = dict(out=lambda F_, C_, n: F_ * C_ * n * 2, rec=lambda F_, C_, n: F_ * C_ * 16, stats=lambda F_, C_, n: F_ * C_ * 16)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def mixed_laws(C_):
    return np.where(np.arange(C_) % 3 == 1, 8, 0).astype(np.uint8)


def shared_rows(C_, P_):
    """channels share far rows two by two; with room for it one channel points past the rows"""
    fo = ((np.arange(C_) // 2) % P_).astype(np.uint32)
    if C_ >= 3:
        fo[1] = P_ + 5
    return fo


def state_dev(state):
    b = np.ascontiguousarray(state).view(np.uint8).reshape(-1)
    return gu.to_dev(np.concatenate([b, np.full(GUARD, STATE_GUARD, np.uint8)]))


def run_ec(ctx, near, far, cfg, codec=None, far_of=None, ctl=None, state=None, d_state=None, outputs=("out", "rec", "stats"), fill=0xEE, entry=None):
    """One launch through the C ABI (entry: through that yardstick instead).  near [F][C][n]: uint8 codes (with codec [C]) or int16 PCM;
    far [F][P][n] int16; state [C] or None (all-zero), or d_state carried from an earlier launch.  Returns the outputs, the state
    records and the state tensor; guard bytes behind every buffer are checked."""
    torch = gu.torch_cuda()
    F_, C_, n = near.shape
    P_ = far.shape[1]
    g711 = near.dtype == np.uint8
    d_x = gu.to_dev(near if g711 else np.asarray(near, "<i2"))
    d_codec = gu.to_dev(np.asarray(codec, np.uint8)) if g711 else None
    d_far = gu.to_dev(np.asarray(far, "<i2")) if P_ else None
    d_fo = gu.to_dev(np.asarray(far_of, "<u4")) if far_of is not None else None
    d_ctl = gu.to_dev(np.asarray(ctl, np.uint8)) if ctl is not None else None
    if d_state is None:
        d_state = state_dev(np.zeros(C_, capi.EC_STATE) if state is None else state)
    sizes = {k: SIZES[k](F_, C_, n) for k in outputs}
    bufs = {k: gu.dev_zeros(v + GUARD, fill) for k, v in sizes.items()}
    p = lambda t: None if t is None else t.data_ptr()
    if entry:
        c = np.ascontiguousarray(cfg, capi.EC_CFG)
        rc = capi.internal(entry)(ctx.h, p(d_x) if g711 else None, p(d_codec), None if g711 else p(d_x), p(d_far), P_, p(d_fo), p(d_ctl), c.ctypes.data,
                                  C_, F_, n, p(d_state), p(bufs.get("out")), p(bufs.get("rec")), p(bufs.get("stats")), None)
        assert rc == 0, rc
    else:
        ctx.echo_cancel(d_far, P_, d_state, C_, F_, n, g711=d_x if g711 else None, codec=d_codec, pcm=None if g711 else d_x, far_of=d_fo, ctl=d_ctl,
                        cfg=cfg, out=bufs.get("out"), rec=bufs.get("rec"), stats=bufs.get("stats"))
    torch.cuda.synchronize()
    host = {k: t.cpu().numpy() for k, t in bufs.items()}
    for k, b in host.items():
        assert np.all(b[sizes[k]:] == fill), f"bytes after d_{k} written"
    sbytes = d_state.cpu().numpy()
    assert len(sbytes) == C_ * SB + GUARD and np.all(sbytes[C_ * SB:] == STATE_GUARD), "bytes after d_state written"
    res = dict(d_state=d_state, state=sbytes[:C_ * SB].view(capi.EC_STATE).copy())
    if "out" in host:
        res["out"] = host["out"][:sizes["out"]].view("<i2").reshape(F_, C_, n)
    if "rec" in host:
        res["rec"] = host["rec"][:sizes["rec"]].view(capi.EC_REC).reshape(F_, C_)
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


def scene_with_state(C_, F_, n, seed, cfg, P_=None, far_of=None, law=False):
    """the scene's last F frames and the model's state after its first PRE; law: the near end as codes of mixed laws"""
    near, far = em.small_scene(C_, F_ + PRE, n, seed, P_)
    codec = None
    if law:
        codec = mixed_laws(C_)
        near = tdet_model.encode(near, codec)
    st = em.cancel(cfg, pcm_of(near[:PRE], codec), far[:PRE], far_of)[3]
    return near[PRE:], far[PRE:], codec, st


def scene_cfg(L, n=24):
    """a hang of one frame and three blocks: raised by the talker of the scene's frame 1, it still runs at frame 3, where the launches
    start, and runs out within that frame"""
    return em.cfg_default(L, hang=(n + 7) // 8 + 3, dmin=64)


# ---- 1. the shapes, both tails, from codes and from PCM, shared far rows
@pytest.mark.parametrize("law", ("g711", "pcm"))
@pytest.mark.parametrize("C_,F_,n", SHAPES)
def test_shapes(ctx, C_, F_, n, law):
    seen = np.zeros(3, np.int64)
    for L in TAILS:
        cfg = scene_cfg(L, n)
        P_ = max(1, (C_ + 1) // 2)
        fo = shared_rows(C_, P_)
        near, far, codec, st = scene_with_state(C_, F_, n, 10 + n + C_, cfg, P_, fo, law == "g711")
        assert np.any(st["hang"] > 0) or C_ < 3
        m = em.cancel(cfg, pcm_of(near, codec), far, fo, state=st)
        check(run_ec(ctx, near, far, cfg, codec, fo, state=st), m)
        seen += (int(m[1]["n_adapt"].sum()), int(m[1]["n_dt"].sum()), int((m[1]["flags"] & em.BYPASSED).astype(bool).sum()))
        # far rows by identity, no d_far_of, the defaults
        cfg = em.cfg_default(L)
        near, far, codec, st = scene_with_state(C_, F_, n, 20 + n + C_, cfg, None, None, law == "g711")
        m = em.cancel(cfg, pcm_of(near, codec), far, state=st)
        check(run_ec(ctx, near, far, cfg, codec, state=st), m)
        seen[0] += int(m[1]["n_adapt"].sum())
    assert seen[0] > 0 and (C_ < 3 or (seen[1] > 0 and seen[2] > 0)), seen


# ---- 2. the invariants: a split of the frames, position and count, G.711 against its PCM
@pytest.mark.parametrize("L", TAILS)
def test_split_position_and_form(ctx, L):
    C_, F_, n = 9, 6, 24
    cfg = scene_cfg(L)
    near, far, codec, st = scene_with_state(C_, F_, n, 5, cfg, law=True)
    whole = run_ec(ctx, near, far, cfg, codec, state=st)
    check(whole, em.cancel(cfg, pcm_of(near, codec), far, state=st))
    for cuts in ((1, 6), (2, 3, 6), (1, 2, 3, 4, 5, 6)):
        d_state, a, parts = None, 0, []
        for b in cuts:
            parts.append(run_ec(ctx, near[a:b], far[a:b], cfg, codec, state=st if a == 0 else None, d_state=d_state))
            d_state, a = parts[-1]["d_state"], b
        for k in ("out", "rec", "stats"):
            assert np.concatenate([q[k] for q in parts]).tobytes() == whole[k].tobytes(), (cuts, k)
        assert parts[-1]["state"].tobytes() == whole["state"].tobytes(), cuts
    # from the decoded PCM: the same bytes
    pcm = run_ec(ctx, pcm_of(near, codec), far, cfg, state=st)
    for k in ("out", "rec", "stats", "state"):
        assert pcm[k].tobytes() == whole[k].tobytes(), k
    # channels 3 .. 6 alone, and reversed among 70
    sub = run_ec(ctx, near[:, 3:7], far[:, 3:7], cfg, codec[3:7], state=st[3:7])
    for k in ("out", "rec", "stats"):
        assert np.array_equal(sub[k], whole[k][:, 3:7]), k
    assert sub["state"].tobytes() == whole["state"][3:7].tobytes()
    idx = np.arange(70) % C_
    idx[-C_:] = np.arange(C_)[::-1]
    big = run_ec(ctx, near[:, idx], far, cfg, codec[idx], far_of=idx.astype(np.uint32), state=st[idx])
    for k in ("out", "rec", "stats"):
        assert np.array_equal(big[k], whole[k][:, idx]), k
    assert big["state"].tobytes() == whole["state"][idx].tobytes()


# ---- 3. every optional output absent in turn
@pytest.mark.parametrize("outputs", (("rec", "stats"), ("out", "stats"), ("out", "rec"), ("rec",), ()))
def test_optional_outputs(ctx, outputs):
    C_, F_, n, L = 6, 3, 164, 128
    cfg = scene_cfg(L, n)
    near, far, codec, st = scene_with_state(C_, F_, n, 6, cfg)
    check(run_ec(ctx, near, far, cfg, state=st, outputs=outputs), em.cancel(cfg, near, far, state=st))


# ---- 4. every control value, a garbage state, full scale
@pytest.mark.parametrize("L", TAILS)
def test_ctl_and_garbage(ctx, L):
    C_, F_, n = 11, 3, 164
    cfg = em.cfg_default(L, hang=2, dmin=0)
    near, far = em.small_scene(C_, F_, n, 9, P_=10)                        # the last channel has no far row
    ctl = (np.arange(C_) % 5).astype(np.uint8)                             # RUN FREEZE BYPASS RESET 4 (as RUN)
    ctl[4] = 200
    st = em.garbage_state(C_, L, 3)
    m = em.cancel(cfg, near, far, ctl=ctl, state=st)
    assert m[1]["n_adapt"][:, 0].sum() > 0 and not m[1]["n_adapt"][:, 1].any() and np.all(m[1]["flags"][:, [2, 10]] == em.BYPASSED)
    check(run_ec(ctx, near, far, cfg, ctl=ctl, state=st), m)
    # a state of no tag and of the other tail's tag start as the reset state; full-scale rows against saturated weights, the largest step
    st = em.garbage_state(C_, L, 4, saturated=True)
    st["tag"][0], st["tag"][1] = 0, em.TAG | (384 - L)
    rng = np.random.default_rng(2)
    near = np.where(rng.integers(0, 2, near.shape) == 1, 32767, -32768).astype(np.int16)
    far = np.where(rng.integers(0, 2, far.shape) == 1, 32767, -32768).astype(np.int16)
    far[:, 3], st["w"][3] = -32768, -(1 << 31)
    cfg = em.cfg_default(L, hang=0, mu_shift=0, pmin=0)
    m = em.cancel(cfg, near, far, state=st)
    assert np.all(m[1]["flags"][0, 2:10] & em.W_SATURATED)
    check(run_ec(ctx, near, far, cfg, state=st), m)


# ---- 5. the argument clauses through the C ABI
def test_argument_paths(ctx):
    L = capi.load()
    C_, F_, n = 4, 2, 160
    near, far = em.small_scene(C_, F_, n, 1)
    d = dict(g=gu.to_dev(tdet_model.encode(near, mixed_laws(C_))), codec=gu.to_dev(mixed_laws(C_)), pcm=gu.to_dev(near), far=gu.to_dev(far),
             fo=gu.to_dev(np.arange(C_, dtype="<u4")), ctl=gu.to_dev(np.zeros(C_, np.uint8)), st=gu.dev_zeros(C_ * SB + 64), out=gu.dev_zeros(F_ * C_ * n * 2 + 64),
             rec=gu.dev_zeros(F_ * C_ * 16 + 64), stats=gu.dev_zeros(F_ * C_ * 16 + 64))
    p = {k: t.data_ptr() for k, t in d.items()}
    cfg = np.ascontiguousarray(em.cfg_default(128), capi.EC_CFG)

    def call(h=ctx.h, g=None, codec=None, pcm=p["pcm"], far_=p["far"], P_=C_, fo=p["fo"], ctl=p["ctl"], c=cfg, C=C_, F=F_, nn=n, st=p["st"], out=p["out"],
             rec=p["rec"], stats=p["stats"]):
        return L.igdsp_echo_cancel(h, g, codec, pcm, far_, P_, fo, ctl, None if c is None else c.ctypes.data, C, F, nn, st, out, rec, stats, None)

    assert call() == 0 and call(c=None) == 0 and call(fo=None, ctl=None, out=None, rec=None, stats=None) == 0
    assert call(g=p["g"], codec=p["codec"], pcm=None) == 0
    assert call(h=None) == EINVAL
    for nn in (0, 1, 161, 258):
        assert call(nn=nn) == EINVAL and call(nn=nn, C=0) == EINVAL       # checked whether or not there is work
    for k, v in (("tail", 64), ("tail", 192), ("mu_shift", 7)):
        bad = cfg.copy()
        bad[k] = v
        assert call(c=bad) == EINVAL and call(c=bad, F=0) == EINVAL
    assert call(C=0) == 0 and call(F=0) == 0 and call(C=0, st=None, pcm=None) == 0
    assert call(g=p["g"], codec=p["codec"]) == EINVAL and call(pcm=None) == EINVAL and call(g=p["g"], pcm=None) == EINVAL      # both, neither, no codec
    assert call(st=None) == EINVAL and call(far_=None) == EINVAL and call(far_=None, P_=0) == 0
    assert call(C=1 << 20, F=1 << 12) == ERANGE and call(P_=1 << 31, F=2) == ERANGE
    assert call(pcm=p["pcm"] + 2) == EINVAL and call(far_=p["far"] + 2) == EINVAL and call(fo=p["fo"] + 2) == EINVAL and call(out=p["out"] + 2) == EINVAL
    assert call(g=p["g"] + 1, codec=p["codec"], pcm=None) == EINVAL and call(g=p["g"] + 2, codec=p["codec"], pcm=None, F=1) == 0
    assert call(stats=p["stats"] + 4) == EINVAL and call(rec=p["rec"] + 8) == EINVAL and call(st=p["st"] + 8) == EINVAL
    assert call(out=p["pcm"]) == EINVAL and call(rec=p["stats"]) == EINVAL and call(st=p["far"]) == EINVAL     # an output over an input / another output
    assert b"overlap" in L.igdsp_last_error(ctx.h)
    gu.torch_cuda().cuda.synchronize()


# ---- 6. the yardstick against its written promise: the bytes of every channel at IGDSP_EC_BYPASS, d_ctl not read
@pytest.mark.parametrize("law", ("g711", "pcm"))
@pytest.mark.parametrize("L", TAILS)
def test_yardstick_promise(ctx, L, law):
    C_, F_, n = 7, 3, 164
    cfg = scene_cfg(L, n)
    P_ = 4
    fo = shared_rows(C_, P_)
    near, far, codec, st = scene_with_state(C_, F_, n, 12, cfg, P_, fo, law == "g711")
    st[1] = em.garbage_state(1, L, 8)[0]
    st["tag"][5] = 77                                                      # another tag: the RESET state
    ctl = np.full(C_, em.RESET, np.uint8)
    got = run_ec(ctx, near, far, cfg, codec, fo, ctl=ctl, state=st, entry="ec_move")
    check(got, em.cancel(cfg, pcm_of(near, codec), far, fo, ctl=np.full(C_, em.BYPASS, np.uint8), state=st))
    assert np.array_equal(got["out"], pcm_of(near, codec))                 # the output is the near row
    keep = [c for c in range(C_) if c != 5]
    assert np.array_equal(got["state"]["w"][keep, :L], st["w"][keep, :L]) and not got["state"]["w"][5].any()   # the weights unchanged
    assert np.array_equal(got["state"]["hang"][keep], st["hang"][keep])
    real = run_ec(ctx, near, far, cfg, codec, fo, state=st)
    hist = real["state"]["hist"].copy()
    hist[5] = got["state"]["hist"][5]                                      # (channel 5's reset history is checked against the model above)
    assert np.array_equal(got["state"]["hist"][keep], hist[keep])          # the history is the entry's


# ---- 7. igdsp_conf_mix -> igdsp_echo_cancel on the device: the receivers of a group share their transmitter's port row
def test_chain_conf_mix_then_echo_cancel(ctx):
    torch = gu.torch_cuda()
    from tests import conf_model as cm

    C_, P_, F_, n, L = 12, 4, 4, 160, 128
    rng = np.random.default_rng(4)
    src = np.clip(np.rint(rng.normal(0.0, 2500.0, (F_, C_, n))), -32768, 32767).astype(np.int16)
    gain = np.full(C_, 128, np.uint16)
    ptr, mem = capi.conf_build(np.arange(C_), np.arange(C_) % P_, C_, P_)
    d_mix = gu.dev_zeros(F_ * P_ * n * 2)
    ctx.conf_mix(gu.to_dev(gain), gu.to_dev(ptr), gu.to_dev(mem), len(mem), C_, P_, F_, n, out=d_mix, pcm=gu.to_dev(src))
    mix, _ = cm.mix(src.astype(np.int64), gain, ptr, mem, len(mem), P_)
    fo = (np.arange(C_) // 3).astype(np.uint32)
    near = np.clip(np.rint(0.4 * np.roll(mix[:, fo].astype(np.float64), 5, axis=2) + rng.normal(0.0, 10.0, (F_, C_, n))), -32768, 32767).astype(np.int16)
    cfg = em.cfg_default(L)
    d_state, d_out, d_rec = state_dev(np.zeros(C_, capi.EC_STATE)), gu.dev_zeros(F_ * C_ * n * 2), gu.dev_zeros(F_ * C_ * 16)
    ctx.echo_cancel(d_mix, P_, d_state, C_, F_, n, pcm=gu.to_dev(near), far_of=gu.to_dev(fo), cfg=cfg, out=d_out, rec=d_rec)
    torch.cuda.synchronize()
    out, rec, _, st = em.cancel(cfg, near, mix, fo)
    assert np.array_equal(gu.to_host(d_out, "<i2", (F_, C_, n)), out) and gu.to_host(d_rec, capi.EC_REC, (F_, C_)).tobytes() == rec.tobytes()
    assert d_state.cpu().numpy()[:C_ * SB].tobytes() == st.tobytes() and rec["n_adapt"].sum() > 0
