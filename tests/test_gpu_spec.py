"""-m gpu: igdsp_spectrum (include/igdsp.h, "Spectrum") through the C ABI against tests/spec_model.py by the model's comparison rule
(bound (a) 0.05 dB and bound (b) 32 x E32 on the bins within 60 dB of the frame's total for raw, the averaged array and peak_db; peak_bin;
the 3 dB rule outside the mask; flags, history, since and hops exactly).  Shapes around the kernel's ownership units (a wave owns a
channel, a block four): C in {1, 3, 4, 5, 64}, F in {1, 7, 13} (with n = 160 the history first wraps in frame 7), n in {1, 24, 160, 164,
256}, hop in {1, 2, 7} and a hop larger than F.  Bit for bit: one launch against the same frames in two and three launches, the same
channel at another position and channel count, G.711 against its decoded PCM.  Every optional output absent in turn, guard bytes behind
every buffer, a garbage state, the argument clauses through the ABI, the yardstick against its written promise.

Figures (MI355X, dB; d_raw holds a launch's last raw array, so that is the one compared): the largest deviation from the float64 model on
masked bins over all cases here was 5.8e-5 for raw (the ring tone; bound (b) there 6.8e-4), 1.8e-5 for the averaged array (+-1 LSB noise)
and 1.7e-5 for peak_db (n = 1); no figure reached 0.14 of its bound (b).  Silence reads -200.00002 where the float32 model's -200 is
exact: the device's log10f is a unit in the last place off at 1e-20f, which is what keeps E32's floor (spec_model.half_ulp32) honest."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import spec_model as sm  # noqa: E402

GUARD = 256
EINVAL, ERANGE = -22, -34
SB = capi.SPEC_STATE.itemsize
LINES = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def run_spec(ctx, x, cfg=None, codec=None, state=None, d_state=None, outputs=("rec", "avg", "raw"), fill=0xEE, entry=None, raw_bytes=None):
    """One launch through the C ABI (entry: through that yardstick instead; fill: the byte the outputs and their guards hold before the
    launch; raw_bytes: a dict that takes the whole buffers' bytes after it).  x [F][C][n]: uint8 codes (with codec [C]) or int16 PCM;
    state [C] SPEC_STATE or None (reset), or d_state: a device tensor carried from an earlier launch.  Returns a dict of the outputs
    named in `outputs`, the state records and the state tensor."""
    torch = gu.torch_cuda()
    F_, C_, n = x.shape
    g711 = x.dtype == np.uint8
    d_x = gu.to_dev(x if g711 else np.asarray(x, "<i2"))
    d_codec = gu.to_dev(np.asarray(codec, np.uint8)) if g711 else None
    if d_state is None:
        d_state = gu.to_dev(np.zeros(C_, capi.SPEC_STATE) if state is None else state)
    sizes = dict(rec=F_ * C_ * 8, avg=C_ * 2048, raw=C_ * 2048)
    bufs = {k: gu.dev_zeros(sizes[k] + GUARD, fill) for k in outputs}
    p = lambda k: bufs[k].data_ptr() if k in bufs else None
    c = capi._spec_cfg(cfg)
    if entry:
        rc = capi.internal(entry)(ctx.h, d_x.data_ptr() if g711 else None, d_codec.data_ptr() if g711 else None, None if g711 else d_x.data_ptr(), C_, F_, n,
                                  None if c is None else ctypes.cast(ctypes.pointer(c), ctypes.c_void_p), d_state.data_ptr(), p("rec"), p("avg"), p("raw"), None)
        assert rc == 0, rc
    else:
        ctx.spectrum(d_state, C_, F_, n, g711=d_x if g711 else None, codec=d_codec, pcm=None if g711 else d_x, cfg=c, rec=bufs.get("rec"),
                     avg=bufs.get("avg"), raw=bufs.get("raw"))
    torch.cuda.synchronize()
    host = {k: t.cpu().numpy() for k, t in bufs.items()}
    for k, b in host.items():
        assert np.all(b[sizes[k]:] == fill), f"bytes after d_{k} written"
    res = dict(d_state=d_state, state=d_state.cpu().numpy().view(capi.SPEC_STATE).copy())
    if "rec" in host:
        res["rec"] = host["rec"][:sizes["rec"]].view(capi.SPEC_REC).reshape(F_, C_)
    for k in ("avg", "raw"):
        if k in host:
            res[k] = host[k][:sizes[k]].view("<f4").reshape(C_, 512)
    if raw_bytes is not None:
        raw_bytes.update(host)
        raw_bytes["state"] = d_state.cpu().numpy()
    return res


def pcm_of(x, codec):
    return sm.decode(x, codec) if x.dtype == np.uint8 else np.asarray(x, np.int16)


def check_launch(x, got, hop=1, alpha=0.25, codec=None, what="", start=None):
    """every channel of a launch from a reset state against the model; returns the largest figures"""
    pcm = pcm_of(x, codec)
    F_, C_, n = pcm.shape
    worst = dict(raw=0.0, avg=0.0, peak=0.0)
    for c in range(C_):
        ref = sm.reference(pcm[:, c], hop, alpha)
        H = len(ref["r64"]["hop_frames"])
        raws = {H - 1: got["raw"][c]} if H and "raw" in got else {}
        rec = {k: got["rec"][k][:, c] for k in ("flags", "peak_bin", "peak_db")} if "rec" in got else None
        fig = sm.check(ref, raws, got["avg"][c] if "avg" in got else got["state"]["avg"][c], rec, f"{what} channel {c}")
        for k in worst:
            worst[k] = max(worst[k], fig[k])
        st = got["state"][c]
        np.testing.assert_array_equal(st["hist"], ref["r64"]["state"]["hist"], err_msg=f"{what} channel {c}")
        assert (int(st["since"]), int(st["hops"]), int(st["flags"])) == (F_ % hop, F_ // hop, capi.SPEC_LIVE), (what, c)
        if "avg" in got:
            assert got["avg"][c].tobytes() == st["avg"].tobytes(), "d_avg is the state's averaged array"
    print(f"spec gpu {what}: worst raw {worst['raw']:.3e} avg {worst['avg']:.3e} peak {worst['peak']:.3e}")
    return worst


def codes(seed, F_, C_, n):
    return np.random.default_rng(seed).integers(0, 256, (F_, C_, n), dtype=np.uint8)


def mixed_laws(C_):
    return np.where(np.arange(C_) % 3 == 1, 8, 0).astype(np.uint8)


# ---- 1. noise of both laws, mixed per channel, at the shapes the mask's share was checked for
@pytest.mark.parametrize("n,F_,hop", ((160, 13, 1), (164, 9, 2), (24, 50, 7), (256, 6, 1)))
def test_noise_codes(ctx, n, F_, hop):
    C_ = 5
    x, codec = codes(200 + n + F_, F_, C_, n), mixed_laws(C_)          # (seeds at which the mask keeps its share: it depends on the input alone)
    got = run_spec(ctx, x, (hop, 0.25), codec)
    check_launch(x, got, hop, codec=codec, what=f"noise n {n} hop {hop}")
    for c in range(C_):
        per_hop, all_hops = sm.mask_share(sm.reference(pcm_of(x, codec)[:, c], hop))
        assert per_hop >= 0.99 and all_hops >= 0.99, (c, per_hop, all_hops)


# ---- 2. the PCM inputs: +-1 LSB noise, silence, the full-scale sine, the single lines, the ring tone, the square
def test_pcm_inputs(ctx):
    F_, n = 13, 160
    chans = [sm.lsb_noise(21, F_, n), np.zeros((F_, n), np.int16), sm.sine(128, F_, n)]
    chans += [sm.sine(k, F_, n, 12000.0, 0.3) for k in LINES]
    chans += [sm.ring_tone(F_, n), sm.square16(F_, n)]
    x = np.stack(chans, axis=1)
    got = run_spec(ctx, x)
    check_launch(x, got, what="pcm inputs")
    last = got["rec"][-1]
    assert np.all(np.abs(got["raw"][1] + 200.0) <= 32 * sm.half_ulp32(np.float32(200.0))) and not got["rec"]["peak_bin"][:, 1].any(), "silence: -200 in every bin, the peak on bin 0"
    assert last["peak_bin"][2] == 128 and abs(float(last["peak_db"][2])) < 1e-3, "a full-scale sine on a bin centre reads 0 dBFS"
    assert last["peak_bin"][3:3 + len(LINES)].tolist() == list(LINES)
    assert int(last["peak_bin"][-2]) in (56, 57, 61, 62) and last["peak_bin"][-1] == 64
    assert sm.mask_share(sm.reference(x[:, 0]))[0] >= 0.99


# ---- 3. the shapes
@pytest.mark.parametrize("C_,F_,n,hop", ((1, 1, 1, 1), (3, 7, 24, 7), (4, 13, 164, 2), (5, 7, 160, 1), (64, 13, 160, 2), (5, 13, 256, 7), (3, 7, 1, 2),
                                         (5, 7, 160, 20), (4, 1, 256, 1)))
def test_shapes(ctx, C_, F_, n, hop):
    x, codec = codes(1000 * C_ + 10 * F_ + n, F_, C_, n), mixed_laws(C_)
    got = run_spec(ctx, x, (hop, 0.25), codec, fill=0xEE)
    check_launch(x, got, hop, codec=codec, what=f"shape C {C_} F {F_} n {n} hop {hop}")
    if hop > F_:                                                          # nothing but the history moves
        assert not got["rec"].view(np.uint8).any() and np.all(got["avg"] == np.float32(-70.0))
        assert np.all(got["raw"].view(np.uint8) == 0xEE), "d_raw is written only for channels that hopped"


def test_half_filled_history_and_other_alpha(ctx):
    x, codec = codes(31, 3, 4, 160), mixed_laws(4)
    check_launch(x, run_spec(ctx, x, None, codec), codec=codec, what="half-filled history, NULL cfg")
    check_launch(x, run_spec(ctx, x, (1, 1.0), codec), 1, 1.0, codec, "alpha 1")
    check_launch(x, run_spec(ctx, x, (2, 0.0625), codec), 2, 0.0625, codec, "alpha 1/16")


# ---- 4. bit for bit: splits, position, input form
def same_bits(a, b, keys=("rec", "avg", "raw")):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["state"].tobytes() == b["state"].tobytes(), "state"


@pytest.mark.parametrize("n,hop", ((160, 1), (164, 2), (24, 7), (1, 3), (255, 2)))
def test_split_launches_bitwise(ctx, n, hop):
    F_, C_ = 13, 5
    x = codes(40 + n, F_, C_, n) if n != 255 else np.random.default_rng(41).integers(-32768, 32768, (F_, C_, n)).astype(np.int16)
    codec = mixed_laws(C_)
    whole = run_spec(ctx, x, (hop, 0.25), codec)
    for cuts in ((6,), (1, 7), (3, 4)):
        parts, d_state = [], None
        for a, b in zip((0,) + cuts, cuts + (F_,)):
            r = run_spec(ctx, x[a:b], (hop, 0.25), codec, d_state=d_state)
            d_state = r["d_state"]
            parts.append((a, b, r))
        got = dict(rec=np.concatenate([r["rec"] for _, _, r in parts]), avg=parts[-1][2]["avg"], state=parts[-1][2]["state"])
        same_bits(got, whole, ("rec", "avg"))
        # d_raw: the last raw spectrum of the launch that last hopped
        hop_frames = np.flatnonzero(whole["rec"]["flags"][:, 0])
        for a, b, r in parts:
            if len(hop_frames) and a <= hop_frames[-1] < b:
                assert r["raw"].tobytes() == whole["raw"].tobytes()


def test_position_and_channel_count_bitwise(ctx):
    F_, n, hop = 13, 160, 2
    one = codes(51, F_, 1, n)
    alone = run_spec(ctx, one, (hop, 0.25), [8])
    for C_, at in ((3, 2), (5, 0), (5, 4), (64, 37), (64, 63)):
        x, codec = codes(52 + C_, F_, C_, n), mixed_laws(C_)
        x[:, at], codec[at] = one[:, 0], 8
        got = run_spec(ctx, x, (hop, 0.25), codec)
        assert got["rec"][:, at].tobytes() == alone["rec"][:, 0].tobytes() and got["avg"][at].tobytes() == alone["avg"][0].tobytes()
        assert got["raw"][at].tobytes() == alone["raw"][0].tobytes() and got["state"][at].tobytes() == alone["state"][0].tobytes(), (C_, at)


@pytest.mark.parametrize("n", (160, 255))
def test_g711_equals_its_decoded_pcm_bitwise(ctx, n):
    x, codec = codes(61, 7, 5, n), mixed_laws(5)
    same_bits(run_spec(ctx, x, (1, 0.25), codec), run_spec(ctx, sm.decode(x, codec), (1, 0.25)))


# ---- 5. optional outputs, footprint
def test_optional_outputs_absent_in_turn(ctx):
    x, codec = codes(71, 7, 5, 160), mixed_laws(5)
    full = run_spec(ctx, x, (2, 0.25), codec)
    for outs in (("avg", "raw"), ("rec", "raw"), ("rec", "avg"), ("rec",), ("avg",), ("raw",), ()):
        got = run_spec(ctx, x, (2, 0.25), codec, outputs=outs)
        same_bits(got, full, outs)


def test_footprint(ctx):
    F_, C_, n, hop = 7, 5, 160, 3
    x, codec = codes(81, F_, C_, n), mixed_laws(C_)

    def launch(fill):
        raw = {}
        run_spec(ctx, x, (hop, 0.25), codec, fill=fill, raw_bytes=raw)
        raw.pop("state")
        return raw

    mask = gu.written_mask(launch)
    assert mask["rec"][:F_ * C_ * 8].all() and not mask["rec"][F_ * C_ * 8:].any()
    for k in ("avg", "raw"):
        assert mask[k][:C_ * 2048].all() and not mask[k][C_ * 2048:].any(), k


# ---- 6. garbage state
def test_garbage_state(ctx):
    F_, C_, n, hop = 5, 5, 160, 4
    rng = np.random.default_rng(6)
    state = np.frombuffer(rng.integers(0, 256, C_ * SB, dtype=np.uint8).tobytes(), capi.SPEC_STATE).copy()
    state["avg"] = rng.uniform(-150, 0, (C_, 512)).astype(np.float32)
    x, codec = codes(91, F_, C_, n), mixed_laws(C_)
    got = run_spec(ctx, x, (hop, 0.25), codec, state=state)
    pcm = pcm_of(x, codec)
    for c in range(C_):
        live = bool(state["flags"][c] & capi.SPEC_LIVE)
        m64 = dict(hist=state["hist"][c].copy(), avg=state["avg"][c].astype(np.float64) if live else None, since=int(state["since"][c]), hops=0)
        m32 = dict(hist=state["hist"][c].copy(), avg=state["avg"][c].copy() if live else None, since=int(state["since"][c]), hops=0)
        ref = sm.reference(pcm[:, c], hop, 0.25, m64, m32)
        H = len(ref["r64"]["hop_frames"])
        assert H == 2 and got["rec"]["flags"][0, c] == capi.SPEC_HOP, "since >= hop_frames reads as hop_frames - 1: the first frame hops"
        sm.check(ref, {H - 1: got["raw"][c]}, got["avg"][c], {k: got["rec"][k][:, c] for k in ("flags", "peak_bin", "peak_db")}, f"garbage state channel {c}")
        st = got["state"][c]
        np.testing.assert_array_equal(st["hist"], ref["r64"]["state"]["hist"])
        assert st["flags"] == capi.SPEC_LIVE and st["reserved"] == state["reserved"][c] and st["hops"] == np.uint32(int(state["hops"][c]) + 2) and st["since"] == 0


# ---- 7. clauses
def test_argument_errors(ctx):
    L = capi.load()
    C_, F_, n = 4, 2, 160
    d_state = gu.dev_zeros(C_ * SB + 64)
    d_g, d_cd, d_pcm = gu.dev_zeros(F_ * C_ * n + 64), gu.dev_zeros(64), gu.dev_zeros(F_ * C_ * n * 2 + 64)
    d_rec, d_avg, d_raw = (gu.dev_zeros(k + 64, 0xEE) for k in (F_ * C_ * 8, C_ * 2048, C_ * 2048))
    g, cd, pc, stt, rec, avg, raw = (t.data_ptr() for t in (d_g, d_cd, d_pcm, d_state, d_rec, d_avg, d_raw))
    cfgs = []

    def cfg(h, a):
        cfgs.append(capi.SpecCfg(h, a))
        return ctypes.cast(ctypes.pointer(cfgs[-1]), ctypes.c_void_p)

    def call(g_=g, cd_=cd, pcm_=None, C=C_, F=F_, n_=n, cfg_=None, state=stt, rec_=rec, avg_=avg, raw_=raw, h=ctx.h):
        return L.igdsp_spectrum(h, g_, cd_, pcm_, C, F, n_, cfg_, state, rec_, avg_, raw_, None)

    assert call(h=None) == EINVAL
    for kw in (dict(n_=0), dict(n_=257), dict(cfg_=cfg(0, 0.25)), dict(cfg_=cfg(1, 0.0)), dict(cfg_=cfg(1, 1.5)), dict(cfg_=cfg(1, float("nan")))):
        assert call(**kw) == EINVAL and call(C=0, **kw) == EINVAL, kw                                # checked even with nothing to do
    assert call(C=0, g_=None, state=None) == 0 and call(F=0, pcm_=pc, avg_=raw) == 0                  # nothing to do comes next
    for kw in (dict(g_=None), dict(pcm_=pc), dict(cd_=None), dict(state=None), dict(g_=None, cd_=None, pcm_=pc + 1), dict(state=stt + 2),
               dict(avg_=avg + 2), dict(raw_=raw + 1), dict(rec_=rec + 4), dict(state=g), dict(rec_=g + 8), dict(avg_=cd), dict(rec_=stt + SB),
               dict(avg_=raw), dict(avg_=raw + 2044), dict(raw_=rec + 56), dict(g_=None, cd_=None, pcm_=pc, raw_=pc + 1000)):
        assert call(**kw) == EINVAL, kw
    assert call(C=0x10000000, F=16) == ERANGE and call(C=0x10000000, F=16, n_=0) == EINVAL and call(C=0x10000000, F=16, rec_=rec + 4) == ERANGE
    assert call(rec_=g + 8) == EINVAL and b"must not overlap an input" in (L.igdsp_last_error(ctx.h) or b"")
    assert call(avg_=raw + 2044) == EINVAL and b"must not overlap each other" in (L.igdsp_last_error(ctx.h) or b"")
    gu.torch_cuda().cuda.synchronize()
    for t in (d_rec, d_avg, d_raw):
        assert (t.cpu().numpy() == 0xEE).all()                                                       # nothing written
    assert not d_state.cpu().numpy().any()
    assert call() == 0 and call(rec_=None, avg_=None, raw_=None) == 0 and call(n_=1, cfg_=cfg(7, 1.0)) == 0 and call(g_=None, cd_=None, pcm_=pc, n_=256, C=2, F=1) == 0
    gu.torch_cuda().cuda.synchronize()


# ---- 8. yardstick
def test_yardstick_footprint_and_rules(ctx):
    """igdsp_internal_spec_move stores exactly the bytes igdsp_spectrum stores; the state's history, since and hops come out as by
    igdsp_spectrum, its averaged array and d_avg as read (-70 from a reset state); a hop's record carries IGDSP_SPEC_HOP, bin 0 and 0.0;
    it rejects what its twin rejects"""
    F_, C_, n, hop = 7, 5, 160, 3
    x, codec = codes(95, F_, C_, n), mixed_laws(C_)

    def launch(entry):
        def go(fill):
            raw = {}
            go.res = run_spec(ctx, x, (hop, 0.25), codec, fill=fill, entry=entry, raw_bytes=raw)
            return raw
        return go

    real, yard = launch(None), launch("igdsp_internal_spec_move")
    gu.assert_same_footprint(gu.written_mask(yard), gu.written_mask(real))
    for k in ("hist", "since", "hops", "flags"):
        np.testing.assert_array_equal(yard.res["state"][k], real.res["state"][k])
    np.testing.assert_array_equal(yard.res["rec"]["flags"], real.res["rec"]["flags"])
    assert not yard.res["rec"]["peak_bin"].any() and not yard.res["rec"]["peak_db"].view(np.uint32).any()
    assert np.all(yard.res["avg"] == np.float32(-70.0)) and np.all(yard.res["state"]["avg"] == np.float32(-70.0))

    fn = capi.internal("spec_move")
    d_state, d_g, d_cd, d_avg = gu.dev_zeros(4 * SB, 0xEE), gu.dev_zeros(2 * 4 * 160 + 64), gu.dev_zeros(64), gu.dev_zeros(4 * 2048 + 64, 0xEE)
    stt, g, cd, avg = (t.data_ptr() for t in (d_state, d_g, d_cd, d_avg))
    bad = capi.SpecCfg(0, 0.25)

    def call(g_=g, cd_=cd, C=4, F=2, n_=160, cfg_=None, state=stt, avg_=avg, h=ctx.h):
        return fn(h, g_, cd_, None, C, F, n_, cfg_, state, None, avg_, None, None)

    for kw in (dict(h=None), dict(n_=0), dict(cfg_=ctypes.cast(ctypes.pointer(bad), ctypes.c_void_p)), dict(g_=None), dict(cd_=None), dict(state=None),
               dict(state=stt + 2), dict(avg_=avg + 2), dict(avg_=g), dict(avg_=stt)):
        assert call(**kw) == EINVAL, kw
    assert call(C=0x10000000, F=16) == ERANGE
    gu.torch_cuda().cuda.synchronize()
    assert (d_avg.cpu().numpy() == 0xEE).all() and (d_state.cpu().numpy() == 0xEE).all()
