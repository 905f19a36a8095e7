"""Shared helpers for the -m gpu parity tests: torch is only plumbing here (device
memory + streams); every compute call goes through the C ABI (libigdsp.so)."""
import numpy as np

from igate4xsoftphonedsp_amd import capi


def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    return torch


def to_dev(a: np.ndarray):
    torch = torch_cuda()
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def dev_zeros(nbytes: int, fill: int = 0):
    torch = torch_cuda()
    return torch.full((max(int(nbytes), 1),), fill, dtype=torch.uint8, device="cuda")


def to_host(t, dtype, shape=None):
    a = t.cpu().numpy().view(dtype)
    return a.reshape(shape) if shape is not None else a


FILL_A, FILL_B = 0xEE, 0x11


def written_mask(run):
    """The bytes a deterministic launch stores.  run(fill) makes the launch with every output buffer (guard bytes and foreign rows
    included) pre-filled with `fill` and returns {name: the whole buffer's bytes after the launch}; it is called with 0xEE and with 0x11.
    Returns {name: after_A != 0xEE | after_B != 0x11}: no byte can equal both fills, so a byte is in the mask iff it was stored."""
    a, b = run(FILL_A), run(FILL_B)
    assert a.keys() == b.keys()
    mask = {}
    for k in a:
        ba, bb = np.ascontiguousarray(a[k]).view(np.uint8).reshape(-1), np.ascontiguousarray(b[k]).view(np.uint8).reshape(-1)
        assert ba.shape == bb.shape, k
        mask[k] = (ba != FILL_A) | (bb != FILL_B)
    return mask


def assert_same_footprint(yard, real, not_written=()):
    """masks of written_mask: the yardstick stores exactly the bytes the entry stores, but nothing at all in the buffers of not_written"""
    for k in yard:
        if k in not_written:
            assert not yard[k].any(), f"{k}: the yardstick wrote {int(yard[k].sum())} bytes, first at {int(np.flatnonzero(yard[k])[0])}"
        else:
            diff = np.flatnonzero(yard[k] != real[k])
            assert diff.size == 0, (f"{k}: {diff.size} bytes differ in the footprint, first at {int(diff[0])} "
                                    f"(yardstick {'wrote' if yard[k][diff[0]] else 'skipped'} it)")


def new_hold(C_):
    h = np.zeros((C_,), dtype=capi.CHAN_HOLD)
    h["level_min"] = 255
    return h


def run_decode_meter(ctx, payload, codec, length=None, want_pcm=False, want_agg=False, rank=0):
    """payload [F][C][n] u8 numpy -> (stats[F][C], pcm|None, agg|None) numpy, through the C ABI."""
    torch = torch_cuda()
    F_, C_, n = payload.shape
    d_pl, d_cd = to_dev(payload), to_dev(np.asarray(codec, dtype=np.uint8))
    d_len = to_dev(np.asarray(length, dtype="<u2")) if length is not None else None
    d_st = dev_zeros(F_ * C_ * 16, 0xEE)
    d_pcm = dev_zeros(F_ * C_ * n * 2, 0xEE) if want_pcm else None
    d_agg = dev_zeros(capi.AGGREGATE.itemsize) if want_agg else None
    s = torch.cuda.current_stream().cuda_stream
    if want_agg:
        ctx.agg_reset(d_agg, stream=s)
    ctx.decode_meter(d_pl, d_cd, C_, F_, n, d_st, pcm=d_pcm, length=d_len, agg=d_agg, rank=rank, stream=s)
    torch.cuda.synchronize()
    stats = to_host(d_st, capi.FRAME_STATS, (F_, C_)) if F_ * C_ else np.zeros((F_, C_), capi.FRAME_STATS)
    pcm = to_host(d_pcm, "<i2", (F_, C_, n)) if want_pcm and F_ * C_ else None
    agg = to_host(d_agg, capi.AGGREGATE)[0] if want_agg else None
    return stats, pcm, agg


def assert_stats_equal(got, exp, n=None, rtol=1e-5):
    """bit-exact on every integer field; fp32 rms within rtol of the float64 definition."""
    for f in ("sumsq", "peak", "byte_mean", "flags"):
        if not np.array_equal(got[f], exp[f]):
            bad = np.argwhere(got[f] != exp[f])
            raise AssertionError(f"{f} mismatch at {bad[:5].tolist()} got {got[f][tuple(bad[0])]} exp {exp[f][tuple(bad[0])]}")
    ref = exp["rms"].astype(np.float64)
    if n is not None:
        nn = np.broadcast_to(np.asarray(n, dtype=np.float64), exp["sumsq"].shape)
        ref = np.where(nn > 0, np.sqrt(exp["sumsq"].astype(np.float64) / np.maximum(nn, 1)), 0.0)
    err = np.abs(got["rms"].astype(np.float64) - ref)
    tol = rtol * np.abs(ref) + 1e-30     # north_star: fp32 RMS within 1e-5 relative
    assert np.all(err <= tol), f"rms rel err {np.max(err / np.maximum(np.abs(ref), 1e-30)):.3e} > {rtol}"
