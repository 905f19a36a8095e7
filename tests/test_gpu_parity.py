"""-m gpu parity tests: the HIP path (through the C ABI) against the CPU oracle on the
same seeded inputs, against the committed golden fixtures, and — at BASELINE.json's
full sizes — through size-independent properties.  Integer/byte results bit-exact;
fp32 RMS within 1e-5 relative of the float64 definition (north_star tolerance)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import gpu_util as gu  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=4096)
    yield c
    c.close()


def _edge_frames(n=160):
    ramp = (np.arange(n) & 0xFF).astype(np.uint8)
    return [np.full(n, 0xFF, np.uint8), np.full(n, 0xD5, np.uint8), np.full(n, 0x00, np.uint8),
            np.full(n, 0x80, np.uint8), np.full(n, 0x7F, np.uint8), np.full(n, 0x2A, np.uint8),
            np.full(n, 0xAA, np.uint8), ramp, ramp[::-1].copy()]


# ----------------------------------------------------------------------------- a1/a3/a5/a7
@pytest.mark.parametrize("variant", [1, 2, 3])
def test_all_codes_both_laws_bit_exact(ctx, orc, variant):
    """Every G.711 code, both laws, every lane/byte position: PCM and stats bit-exact."""
    ctx.set_variant(variant)
    C_, F_, n = 64, 5, 160
    rng = np.random.default_rng(7)
    payload = np.zeros((F_, C_, n), np.uint8)
    for f in range(F_):
        for c in range(C_):
            payload[f, c] = np.roll(np.arange(n * 2, dtype=np.uint32)[:n] * (1 + (c % 3)) + 37 * c + 11 * f, c) & 0xFF
    payload[0, :, :] = rng.permutation(np.tile(np.arange(256, dtype=np.uint8), C_ * n // 256 + 1)[: C_ * n]).reshape(C_, n)
    codec = np.where(np.arange(C_) % 3 == 1, 8, 0).astype(np.uint8)
    st, pcm, _ = gu.run_decode_meter(ctx, payload, codec, want_pcm=True)
    est, epcm = orc.decode_meter(payload, codec, want_pcm=True)
    assert np.array_equal(pcm, epcm)
    gu.assert_stats_equal(st, est, n=n)
    ctx.set_variant(0)


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_config2_4096ch_uniform_and_edges(ctx, orc, variant):
    """BASELINE config #2: 4 096 ch, F=16, D-uniform + D-edge, PCM store on, every int16 compared."""
    ctx.set_variant(variant)
    C_, F_, n = 4096, 16, 160
    payload = orc.gen_uniform(F_ * C_ * n).reshape(F_, C_, n).copy()
    edges = _edge_frames(n)
    for i, e in enumerate(edges):            # D-edge rows sprinkled over channels of both laws
        payload[i % F_, 100 + 2 * i] = e
        payload[(i + 3) % F_, 101 + 2 * i] = e
    codec = np.where(np.arange(C_) & 1, 8, 0).astype(np.uint8)
    st, pcm, agg = gu.run_decode_meter(ctx, payload, codec, want_pcm=True, want_agg=True, rank=3)
    est, epcm, eagg = orc.decode_meter(payload, codec, want_pcm=True, want_agg=True, rank=3)
    assert np.array_equal(pcm, epcm)
    gu.assert_stats_equal(st, est, n=n)
    for f in ("sumsq", "samples", "frames", "n_silent", "n_clipped", "byte_mean_sum"):
        assert int(agg[f]) == int(eagg[f]), f
    assert agg["peak_slot"].tolist() == eagg["peak_slot"].tolist()
    ctx.set_variant(0)


def test_chunk_path_tail_and_wraparound(ctx, orc):
    """n_frames not a multiple of 32 and C not a multiple of 32: tail clamping + channel wrap."""
    for C_, F_ in ((50, 3), (33, 7), (32, 1), (127, 9), (96, 2)):
        n = 160
        payload = orc.gen_uniform(F_ * C_ * n, seed=C_ * 1000 + F_).reshape(F_, C_, n)
        codec = np.where((np.arange(C_) * 7) % 5 < 2, 8, 0).astype(np.uint8)
        st, pcm, agg = gu.run_decode_meter(ctx, payload, codec, want_pcm=True, want_agg=True)
        est, epcm, eagg = orc.decode_meter(payload, codec, want_pcm=True, want_agg=True)
        assert np.array_equal(pcm, epcm), (C_, F_)
        gu.assert_stats_equal(st, est, n=n)
        assert int(agg["sumsq"]) == int(eagg["sumsq"]) and int(agg["frames"]) == C_ * F_


@pytest.mark.parametrize("n", [1, 3, 24, 159, 160, 164, 255, 256])
def test_ragged_lengths_and_odd_frame_sizes(ctx, orc, n):
    """Generic wave-per-frame path: any n in 1..256, per-frame valid length, empty slots."""
    C_, F_ = 37, 4
    rng = np.random.default_rng(n)
    payload = orc.gen_uniform(F_ * C_ * n, seed=n).reshape(F_, C_, n)
    codec = np.where(np.arange(C_) % 2, 8, 0).astype(np.uint8)
    length = rng.integers(0, n + 1, size=(F_, C_)).astype(np.uint16)
    length[0, 0] = 0
    length[0, 1] = n
    st, pcm, agg = gu.run_decode_meter(ctx, payload, codec, length=length, want_pcm=True, want_agg=True)
    est, epcm, eagg = orc.decode_meter(payload, codec, length=length, want_pcm=True, want_agg=True)
    assert np.array_equal(pcm, epcm)
    gu.assert_stats_equal(st, est, n=length)
    assert int(agg["samples"]) == int(length.sum()) == int(eagg["samples"])
    assert int(agg["frames"]) == int((length > 0).sum())
    # and without a length array
    st, pcm, _ = gu.run_decode_meter(ctx, payload, codec, want_pcm=True)
    est, epcm = orc.decode_meter(payload, codec, want_pcm=True)
    assert np.array_equal(pcm, epcm)
    gu.assert_stats_equal(st, est, n=n)


@pytest.mark.parametrize("n", [4, 16, 20, 24, 64, 72, 80, 88, 96, 100, 128, 136, 164, 168, 172, 192, 200, 240, 244, 256, 160])
@pytest.mark.parametrize("ragged", [False, True])
def test_other_frame_sizes_image_kernel(ctx, orc, n, ragged):
    """Frame sizes other than 160 (the reference's hook anticipates 164 and 24, roip_ed137.cpp:6561-6562) and ragged frames
    no longer fall to the wave-per-frame kernel.  Dense 16 .. 32-byte frames (16, 20, 24) go to k_meter_tiny (a lane per frame);
    dense frames of 16 Q + 4 T bytes with Q in {4, 5, 6, 8, 10, 12, 15}, T <= 2 (64, 72, 80, 88, 96, 100, 128, 136, 164, 168, 192,
    200, 240) keep the chunk pipeline at a frame stride (k_meter_strided, with the tail piece handed to the frame lane); every
    other n % 4 == 0 size (4, 172, 244, 256), ragged lengths and the < 64-frame tail go through k_meter_image (one frame per
    lane from an LDS image of 64 frames).  Whole items, a tail item, channel wrap inside an item, mixed laws, edge frames,
    the aggregate; every record against the oracle."""
    if n == 160 and not ragged:
        pytest.skip("dense 160-byte frames are the tuned kernel's (tested above)")
    C_, F_ = 150, 7                                  # 1050 frames = 16 items + a tail of 26
    payload = orc.gen_uniform(F_ * C_ * n, seed=n).reshape(F_, C_, n).copy()
    for k, fr in enumerate(_edge_frames(n)):
        payload[k % F_, (13 * k) % C_] = fr
    codec = np.where((np.arange(C_) * 7) % 5 < 2, 8, 0).astype(np.uint8)
    rng = np.random.default_rng(n)
    length = rng.integers(0, n + 1, size=(F_, C_)).astype(np.uint16) if ragged else None
    if ragged:
        length[0, :8] = [0, 1, 2, 3, n, max(n - 1, 0), min(49, n), min(48, n)]
    st, _, agg = gu.run_decode_meter(ctx, payload, codec, length=length, want_agg=True, rank=5)
    est, eagg = orc.decode_meter(payload, codec, length=length, want_agg=True, rank=5)
    gu.assert_stats_equal(st, est, n=length if ragged else n)
    for f in ("sumsq", "samples", "frames", "n_silent", "n_clipped", "byte_mean_sum"):
        assert int(agg[f]) == int(eagg[f]), f
    assert agg["peak_slot"].tolist() == eagg["peak_slot"].tolist()


@pytest.mark.parametrize("n", [160, 164])
def test_roundtrip_group_order_of_spread_outputs(ctx, orc, n):
    """When the re-encoded output sits half in one, half in another memory class (igdsp_io_alloc), the fused round-trip kernels
    give the waves of a block CONSECUTIVE channel groups in their first round and groups a grid apart in any remainder round.
    That order is forced here (IGDSP_RT_ORDER=1, read at launch) on a shape with a remainder round — 4 000 groups for 3 072
    waves — and on one with frame segments; codes, records and hold windows against the oracle."""
    import os
    torch = gu.torch_cuda()
    for C_, F_ in ((64 * 4000, 2), (64 * 37, 40)):
        payload = orc.gen_uniform(F_ * C_ * n, seed=C_ + n).reshape(F_, C_, n)
        codec = np.where(np.arange(C_) % 3 == 0, 8, 0).astype(np.uint8)
        hold0 = gu.new_hold(C_)
        eout, est, ehold = orc.roundtrip_peakhold(payload, codec, hold0.copy().view(orc.CHAN_HOLD))
        d_out, d_st, d_hold = gu.dev_zeros(F_ * C_ * n, 0xEE), gu.dev_zeros(F_ * C_ * 16, 0xEE), gu.to_dev(hold0)
        os.environ["IGDSP_RT_ORDER"] = "1"
        try:
            ctx.roundtrip_peakhold(gu.to_dev(payload), gu.to_dev(codec), C_, F_, n, d_out, d_st, d_hold)
            torch.cuda.synchronize()
        finally:
            del os.environ["IGDSP_RT_ORDER"]
        assert np.array_equal(gu.to_host(d_out, np.uint8, (F_, C_, n)), eout)
        gu.assert_stats_equal(gu.to_host(d_st, capi.FRAME_STATS, (F_, C_)), est, n=n)
        ghold = gu.to_host(d_hold, capi.CHAN_HOLD)
        for f in capi.CHAN_HOLD.names:
            assert np.array_equal(ghold[f], ehold[f]), f


@pytest.mark.parametrize("n", [164, 24, 240, 128])
def test_strided_peak_is_exact_for_every_code(ctx, orc, n):
    """The record-only k_meter_strided kernels look up (|x| / 4)^2 alone and recover the peak as the integer root of the largest
    square of a 16-sample piece (one v_sqrt_f32, isqrt_m2).  Every G.711 magnitude of both laws has to come back exactly:
    frame c of a launch holds code c in every byte (so its peak is |decode(c)|, in the pieces and in the tail dwords), plus
    frames with ONE loud sample at every position of a piece among quiet ones.  Records against the oracle."""
    C_, F_ = 256, 3
    payload = np.empty((F_, C_, n), dtype=np.uint8)
    payload[0] = np.arange(256, dtype=np.uint8)[:, None]                     # frame c: all bytes = c
    payload[1] = 0xFF                                                        # quiet frames with one loud sample each
    payload[2] = 0xD5
    for c in range(C_):
        payload[1, c, (c * 7) % n] = c
        payload[2, c, n - 1 - (c * 5) % n] = c
    for law in (0, 8):
        codec = np.full((C_,), law, dtype=np.uint8)
        st, _, _ = gu.run_decode_meter(ctx, payload, codec)
        est = orc.decode_meter(payload, codec)
        gu.assert_stats_equal(st, est, n=n)


@pytest.mark.parametrize("n", [160, 164, 80])
def test_dword_aligned_payload_keeps_the_chunk_pipeline(ctx, orc, n):
    """A payload buffer that is only dword aligned (base + 4) cannot take the 16-byte aligned loads of k_meter_chunk64 /
    k_meter_image; k_meter_strided's dword-aligned loads serve it (160-byte frames included) instead of the wave-per-frame
    kernel.  Records and aggregate against the oracle."""
    torch = gu.torch_cuda()
    C_, F_ = 200, 5
    payload = orc.gen_uniform(F_ * C_ * n, seed=n + 1).reshape(F_, C_, n)
    codec = np.where(np.arange(C_) % 3 == 1, 8, 0).astype(np.uint8)
    raw = gu.dev_zeros(F_ * C_ * n + 64, 0xEE)
    d_pl = raw[4:4 + F_ * C_ * n]
    d_pl.copy_(torch.from_numpy(payload.reshape(-1).copy()))
    assert d_pl.data_ptr() % 16 == 4
    d_st, d_agg = gu.dev_zeros(F_ * C_ * 16, 0xEE), gu.dev_zeros(capi.AGGREGATE.itemsize)
    ctx.decode_meter(d_pl, gu.to_dev(codec), C_, F_, n, d_st, agg=d_agg, rank=1)
    torch.cuda.synchronize()
    est, eagg = orc.decode_meter(payload, codec, want_agg=True, rank=1)
    gu.assert_stats_equal(gu.to_host(d_st, capi.FRAME_STATS, (F_, C_)), est, n=n)
    agg = gu.to_host(d_agg, capi.AGGREGATE)[0]
    for f in ("sumsq", "samples", "frames", "n_silent", "n_clipped", "byte_mean_sum"):
        assert int(agg[f]) == int(eagg[f]), f
    assert np.all(raw[:4].cpu().numpy() == 0xEE) and np.all(raw[4 + F_ * C_ * n:].cpu().numpy() == 0xEE)


@pytest.mark.parametrize("n", [24, 80, 164, 168, 240, 96])
def test_decode_with_pcm_at_other_frame_sizes(ctx, orc, n):
    """Config #2's check (every decoded int16 against the oracle) at the reference's other frame sizes: 24, 80, 164 / 168, 240 keep
    the chunk pipeline with PCM output (k_meter_strided<STORE>; tail samples stored by the frame lane), 96 falls to the
    wave-per-frame kernel.  Whole items plus a tail, mixed laws, edge frames, dword-aligned PCM buffer."""
    torch = gu.torch_cuda()
    C_, F_ = 170, 5                                   # 850 frames = 13 items + a tail of 18
    payload = orc.gen_uniform(F_ * C_ * n, seed=3 * n).reshape(F_, C_, n).copy()
    for k, fr in enumerate(_edge_frames(n)):
        payload[k % F_, (11 * k) % C_] = fr
    codec = np.where((np.arange(C_) * 5) % 7 < 3, 8, 0).astype(np.uint8)
    raw = gu.dev_zeros(F_ * C_ * n * 2 + 64, 0xEE)
    d_pcm = raw[4:4 + F_ * C_ * n * 2]
    d_st, d_agg = gu.dev_zeros(F_ * C_ * 16, 0xEE), gu.dev_zeros(capi.AGGREGATE.itemsize)
    ctx.decode_meter(gu.to_dev(payload), gu.to_dev(codec), C_, F_, n, d_st, pcm=d_pcm, agg=d_agg, rank=2)
    torch.cuda.synchronize()
    est, epcm, eagg = orc.decode_meter(payload, codec, want_pcm=True, want_agg=True, rank=2)
    assert np.array_equal(d_pcm.cpu().numpy().view("<i2").reshape(F_, C_, n), epcm)
    gu.assert_stats_equal(gu.to_host(d_st, capi.FRAME_STATS, (F_, C_)), est, n=n)
    agg = gu.to_host(d_agg, capi.AGGREGATE)[0]
    assert int(agg["sumsq"]) == int(eagg["sumsq"]) and int(agg["frames"]) == C_ * F_
    assert np.all(raw[:4].cpu().numpy() == 0xEE) and np.all(raw[4 + F_ * C_ * n * 2:].cpu().numpy() == 0xEE)


def test_config1_golden_fixture_through_gpu(ctx, golden_dir):
    """4 ch x 50 frames of the committed fixture: GPU vs values derived from audioop (not our oracle)."""
    g = np.load(os.path.join(golden_dir, "config1_4ch_50f.npz"))
    st, _, _ = gu.run_decode_meter(ctx, g["payload"], g["codec"])
    assert np.array_equal(st["sumsq"], g["sumsq"])
    assert np.array_equal(st["peak"].astype(np.int64), g["audioop_peak"])
    assert np.array_equal(st["byte_mean"], g["byte_mean"])
    ref = np.sqrt(g["sumsq"].astype(np.float64) / 160.0)
    assert np.all(np.abs(st["rms"] - ref) <= 1e-5 * ref + 1e-30)


def test_empty_batches_are_accepted(ctx):
    torch = gu.torch_cuda()
    d = gu.dev_zeros(16)
    ctx.decode_meter(d, d, 0, 5, 160, d)
    ctx.decode_meter(d, d, 5, 0, 160, d)
    ctx.encode(d, d, 0, 0, 160, d)
    torch.cuda.synchronize()


def test_error_codes(ctx):
    d = gu.dev_zeros(64 * 160)
    L = ctx.L
    assert L.igdsp_decode_meter(ctx.h, None, d.data_ptr(), None, 4, 1, 160, d.data_ptr(), None, None, 0, None) == -22
    assert L.igdsp_decode_meter(ctx.h, d.data_ptr(), d.data_ptr(), None, 4, 1, 0, d.data_ptr(), None, None, 0, None) == -22
    assert L.igdsp_decode_meter(ctx.h, d.data_ptr(), d.data_ptr(), None, 4, 1, 257, d.data_ptr(), None, None, 0, None) == -22
    assert L.igdsp_decode_meter(ctx.h, d.data_ptr(), d.data_ptr(), None, 4, 1, 160, d.data_ptr(), None, None, 8, None) == -22
    assert L.igdsp_decode_meter(None, d.data_ptr(), d.data_ptr(), None, 4, 1, 160, d.data_ptr(), None, None, 0, None) == -22
    assert L.igdsp_encode(ctx.h, d.data_ptr(), d.data_ptr(), 4, 1, 160, d.data_ptr(), 7, None) == -22
    assert L.igdsp_roundtrip_peakhold(ctx.h, d.data_ptr(), d.data_ptr(), 33, 1, 160, d.data_ptr(), d.data_ptr(), d.data_ptr(), None, 7, None) == -22   # encoder lineage
    assert L.igdsp_roundtrip_peakhold(ctx.h, d.data_ptr(), d.data_ptr(), 33, 1, 160, d.data_ptr(), d.data_ptr() + 4, d.data_ptr(), None, 0, None) == -22  # record alignment
    assert L.igdsp_hold_update(ctx.h, d.data_ptr(), 4, 1, 0, d.data_ptr(), None, None) == -22 and L.igdsp_hold_update(ctx.h, d.data_ptr(), 4, 1, 257, d.data_ptr(), None, None) == -22
    assert L.igdsp_destroy(None) == 0           # NULL tolerated like the reference's setters
    assert L.igdsp_map_call(ctx.h, 1, 1 << 30) == -34
    assert ctx.on_rtp_frame(4242, 0, b"\x00" * 160) == -2      # unmapped call id
    assert ctx.on_rtp_frame(4242, 123, b"") == 0               # keep-alive: accepted, ignored
    ctx.map_call(77, 0)
    assert ctx.on_rtp_frame(77, 0, b"\x00" * 257) == -22
    ctx.unmap_call(77)


# ----------------------------------------------------------------------------- a2
@pytest.mark.parametrize("variant", [capi.ENC_SUN16, capi.ENC_G191])
def test_encode_exhaustive(ctx, orc, golden_dir, variant):
    """All 65 536 int16 inputs, both laws, both encoder lineages: GPU == oracle, and the
    G191 lineage == the frozen CPython-audioop table."""
    torch = gu.torch_cuda()
    aud = np.load(os.path.join(golden_dir, "g711_audioop.npz"))
    C_, F_, n = 2, 256, 256
    pcm = np.zeros((F_, C_, n), "<i2")
    pcm[:, 0, :] = np.arange(-32768, 32768, dtype=np.int32).reshape(F_, n).astype("<i2")
    pcm[:, 1, :] = pcm[:, 0, :]
    codec = np.array([0, 8], np.uint8)
    d_out = gu.dev_zeros(F_ * C_ * n, 0xEE)
    ctx.encode(gu.to_dev(pcm), gu.to_dev(codec), C_, F_, n, d_out, variant=variant, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = gu.to_host(d_out, np.uint8, (F_, C_, n))
    exp = orc.encode(pcm, codec, variant)
    assert np.array_equal(got, exp)
    if variant == capi.ENC_G191:
        assert np.array_equal(got[:, 0, :].reshape(-1), aud["ulaw_encode_g191"])
        assert np.array_equal(got[:, 1, :].reshape(-1), aud["alaw_encode_g191"])


@pytest.mark.parametrize("variant", [capi.ENC_SUN16, capi.ENC_G191])
def test_table_driven_compressor_exhaustive(ctx, orc, variant):
    """The LDS cell table the fused round-trip kernel compresses with (2 laws x 16 384 cells) against the
    oracle on all 65 536 int16 inputs: the cells are exact for ANY PCM value, not only decoder outputs."""
    import ctypes as C

    torch = gu.torch_cuda()
    fn = ctx.L.igdsp_internal_encode_table
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
    C_, F_, n = 2, 256, 256
    pcm = np.zeros((F_, C_, n), "<i2")
    pcm[:, 0, :] = np.arange(-32768, 32768, dtype=np.int32).reshape(F_, n).astype("<i2")
    pcm[:, 1, :] = pcm[:, 0, :]
    codec = np.array([0, 8], np.uint8)
    d_out = gu.dev_zeros(F_ * C_ * n, 0xEE)
    assert fn(ctx.h, gu.to_dev(pcm).data_ptr(), gu.to_dev(codec).data_ptr(), C_, F_, n, d_out.data_ptr(), variant, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(gu.to_host(d_out, np.uint8, (F_, C_, n)), orc.encode(pcm, codec, variant))


@pytest.mark.parametrize("variant", [capi.ENC_SUN16, capi.ENC_G191])
def test_encode_large_batch_table_path(ctx, orc, variant):
    """Batches of >= 4 M samples take the table-driven encode kernel: every int16 value x both laws, 64 times over."""
    torch = gu.torch_cuda()
    C_, F_, n = 64, 512, 256                       # 8.4 M samples
    base = np.arange(-32768, 32768, dtype=np.int32).astype("<i2")
    pcm = np.tile(base, C_ * F_ * n // base.size).reshape(F_, C_, n)
    codec = np.where(np.arange(C_) % 2, 8, 0).astype(np.uint8)
    d_out = gu.dev_zeros(F_ * C_ * n, 0xEE)
    ctx.encode(gu.to_dev(pcm), gu.to_dev(codec), C_, F_, n, d_out, variant=variant)
    torch.cuda.synchronize()
    assert np.array_equal(gu.to_host(d_out, np.uint8, (F_, C_, n)), orc.encode(pcm, codec, variant))


@pytest.mark.parametrize("variant", [capi.ENC_SUN16, capi.ENC_G191])
@pytest.mark.parametrize("C_,F_,n", [(64, 2048, 256), (96, 2200, 160), (7, 30001, 160)])
def test_encode_huge_batch_full_table_path(ctx, orc, variant, C_, F_, n):
    """Batches of >= 32 M samples take k_encode_lut16 (full 16-bit table in LDS, incremental frame/channel bookkeeping):
    every int16 value, both laws, channel counts that are not powers of two."""
    torch = gu.torch_cuda()
    total = C_ * F_ * n
    assert total >= 1 << 25
    base = np.arange(-32768, 32768, dtype=np.int32).astype("<i2")
    pcm = np.resize(np.concatenate([base, base[::-1][:65521]]), total).reshape(F_, C_, n)     # period coprime to the frame size
    codec = np.where(np.arange(C_) % 3 == 1, 8, 0).astype(np.uint8)
    d_out = gu.dev_zeros(total, 0xEE)
    ctx.encode(gu.to_dev(pcm), gu.to_dev(codec), C_, F_, n, d_out, variant=variant)
    torch.cuda.synchronize()
    assert np.array_equal(gu.to_host(d_out, np.uint8, (F_, C_, n)), orc.encode(pcm, codec, variant))


@pytest.mark.parametrize("n", [160, 7, 200])
def test_encode_shapes(ctx, orc, n):
    torch = gu.torch_cuda()
    C_, F_ = 19, 3
    rng = np.random.default_rng(5)
    pcm = rng.integers(-32768, 32768, size=(F_, C_, n)).astype("<i2")
    codec = np.where(np.arange(C_) % 3 == 0, 8, 0).astype(np.uint8)
    for variant in (0, 1):
        d_out = gu.dev_zeros(F_ * C_ * n, 0xEE)
        ctx.encode(gu.to_dev(pcm), gu.to_dev(codec), C_, F_, n, d_out, variant=variant, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(gu.to_host(d_out, np.uint8, (F_, C_, n)), orc.encode(pcm, codec, variant))


# ----------------------------------------------------------------------------- config #5
@pytest.mark.parametrize("F_", [12, 64])     # 64 frames: the launcher splits the window into 8 segments merged by atomics
@pytest.mark.parametrize("variant", [capi.ENC_SUN16, capi.ENC_G191])
def test_roundtrip_peakhold_vs_oracle(ctx, orc, variant, F_):
    torch = gu.torch_cuda()
    C_, n = 256, 160
    codec = np.where(np.arange(C_) & 1, 8, 0).astype(np.uint8)
    payload = orc.gen_speech(C_, F_, n, codec)
    payload[3, 10] = 0x7F                     # mu-law negative zero: the one code that does not round-trip
    payload[4, 11] = 0xD5
    payload[5, 12] = 0x00
    gate = (np.arange(C_) % 5 != 0).astype(np.uint8)
    hold0 = gu.new_hold(C_)
    hold0["peak_hold"][7] = 30000             # pre-existing state must be folded, not overwritten
    hold0["count"][7] = 5
    d_out, d_st, d_hold = gu.dev_zeros(F_ * C_ * n, 0xEE), gu.dev_zeros(F_ * C_ * 16, 0xEE), gu.to_dev(hold0)
    s = torch.cuda.current_stream().cuda_stream
    ctx.roundtrip_peakhold(gu.to_dev(payload), gu.to_dev(codec), C_, F_, n, d_out, d_st, d_hold, gate=gu.to_dev(gate), variant=variant, stream=s)
    torch.cuda.synchronize()
    ehold = hold0.copy().view(orc.CHAN_HOLD)
    eout, est, ehold = orc.roundtrip_peakhold(payload, codec, ehold, gate=gate, variant=variant)
    assert np.array_equal(gu.to_host(d_out, np.uint8, (F_, C_, n)), eout)
    gu.assert_stats_equal(gu.to_host(d_st, capi.FRAME_STATS, (F_, C_)), est, n=n)
    ghold = gu.to_host(d_hold, capi.CHAN_HOLD)
    for f in capi.CHAN_HOLD.names:
        assert np.array_equal(ghold[f], ehold[f]), f
    # closed-set property: output == input except mu-law 0x7F -> 0xFF
    exp = payload.copy()
    mu = np.broadcast_to((codec == 0)[None, :, None], payload.shape)
    exp[(payload == 0x7F) & mu] = 0xFF
    assert np.array_equal(eout, exp)


@pytest.mark.parametrize("kernel", [0, 4])            # 0: compressor folded into the expansion LUT (default); 4: compressor cell table
@pytest.mark.parametrize("C_,F_,n", [(4, 50, 160), (33, 5, 160), (64, 9, 160), (100, 7, 160), (200, 3, 164), (7, 4, 24), (65, 2, 255),
                                     (130, 70, 160), (1, 1, 1), (3, 2, 159), (700, 2, 160), (130, 70, 164), (128, 9, 240), (64, 12, 24),
                                     (192, 33, 80), (65, 10, 168), (256, 5, 20), (128, 4, 172), (128, 4, 96)])
@pytest.mark.parametrize("blk", ["0", "1"])
def test_roundtrip_every_shape_vs_oracle(ctx, orc, monkeypatch, kernel, C_, F_, n, blk):
    """igdsp_roundtrip_peakhold serves every geometry: whole groups of 64 channels of 160-byte frames through the fused
    kernels, the C % 64 left-over channels and every other n (164, 24, ... roip_ed137.cpp:6561-6562) / BASELINE config #1's
    4 channels through the general wave-per-channel kernel; codes, records and hold equal the oracle's, with gates and
    pre-existing hold state.  blk: the fused kernels' two work distributions — 0 = a wave walks a segment of one group's frames
    (windows in registers), 1 = a block owns groups and hands out single frames (windows in LDS); the launcher's own rule only
    takes the second where its blocks fill the chip."""
    torch = gu.torch_cuda()
    monkeypatch.setenv("IGDSP_RT_BLK", blk)
    rng = np.random.default_rng(C_ * 1000 + F_ * 10 + n)
    codec = rng.choice(np.array([0, 8], np.uint8), size=C_)
    payload = orc.gen_uniform(F_ * C_ * n, seed=C_ + n).reshape(F_, C_, n).copy()
    payload[0, 0, :] = 0x7F
    if C_ > 2:
        payload[F_ - 1, C_ - 1, :] = 0xD5
        payload[F_ // 2, C_ // 2, :] = rng.choice([0x00, 0x80, 0x2A, 0xAA, 0xFF])
    gate = (rng.integers(0, 4, C_) != 0).astype(np.uint8)
    hold0 = gu.new_hold(C_)
    hold0["peak_hold"][C_ - 1] = 31000
    hold0["count"][0] = 7
    hold0["level_min"][0] = 3
    for variant in (capi.ENC_SUN16, capi.ENC_G191):
        d_out, d_st, d_hold = gu.dev_zeros(F_ * C_ * n, 0xEE), gu.dev_zeros(F_ * C_ * 16, 0xEE), gu.to_dev(hold0)
        ctx.set_variant(kernel)
        try:
            ctx.roundtrip_peakhold(gu.to_dev(payload), gu.to_dev(codec), C_, F_, n, d_out, d_st, d_hold, gate=gu.to_dev(gate), variant=variant)
            torch.cuda.synchronize()
        finally:
            ctx.set_variant(0)
        eout, est, ehold = orc.roundtrip_peakhold(payload, codec, hold0.copy().view(orc.CHAN_HOLD), gate=gate, variant=variant)
        assert np.array_equal(gu.to_host(d_out, np.uint8, (F_, C_, n)), eout)
        gu.assert_stats_equal(gu.to_host(d_st, capi.FRAME_STATS, (F_, C_)), est, n=n)
        ghold = gu.to_host(d_hold, capi.CHAN_HOLD)
        for f in capi.CHAN_HOLD.names:
            assert np.array_equal(ghold[f], ehold[f]), (f, variant)


@pytest.mark.parametrize("gpb,C_,F_,n", [("4", 512, 37, 160), ("2", 384, 50, 160), ("4", 256, 21, 164), ("2", 128, 40, 240), ("4", 256, 30, 80),
                                          ("4", 256, 64, 24), ("1", 192, 3, 160), ("4", 256, 1, 160)])
def test_roundtrip_block_form_groups_per_block(ctx, orc, monkeypatch, gpb, C_, F_, n):
    """The block-owned round trip at 4 / 2 / 1 channel groups per block (odd blocks start in the middle of the frames; F = 1 and
    odd F included), every fused frame size, against the oracle and byte for byte against the static form."""
    torch = gu.torch_cuda()
    rng = np.random.default_rng(C_ + F_ + n)
    codec = rng.choice(np.array([0, 8], np.uint8), size=C_)
    payload = orc.gen_uniform(F_ * C_ * n, seed=C_ + F_).reshape(F_, C_, n).copy()
    payload[F_ // 2, ::5, :] = 0xD5
    gate = (rng.integers(0, 5, C_) != 0).astype(np.uint8)
    hold0 = gu.new_hold(C_)
    hold0["peak_hold"][::7] = 20000
    hold0["count"][::3] = 11
    outs = []
    for blk in ("1", "0"):
        monkeypatch.setenv("IGDSP_RT_BLK", blk)
        monkeypatch.setenv("IGDSP_RT_GPB", gpb)
        d_out, d_st, d_hold = gu.dev_zeros(F_ * C_ * n, 0xEE), gu.dev_zeros(F_ * C_ * 16, 0xEE), gu.to_dev(hold0)
        ctx.roundtrip_peakhold(gu.to_dev(payload), gu.to_dev(codec), C_, F_, n, d_out, d_st, d_hold, gate=gu.to_dev(gate), variant=capi.ENC_G191)
        torch.cuda.synchronize()
        outs.append((gu.to_host(d_out, np.uint8).tobytes(), gu.to_host(d_st, np.uint8).tobytes(), gu.to_host(d_hold, np.uint8).tobytes()))
    assert outs[0] == outs[1]
    eout, est, ehold = orc.roundtrip_peakhold(payload, codec, hold0.copy().view(orc.CHAN_HOLD), gate=gate, variant=capi.ENC_G191)
    assert outs[0][0] == eout.tobytes()
    assert np.frombuffer(outs[0][2], capi.CHAN_HOLD).tobytes() == np.ascontiguousarray(ehold).tobytes()


@pytest.mark.parametrize("variant", [capi.ENC_SUN16, capi.ENC_G191])
def test_roundtrip_every_code_as_the_peak(ctx, orc, variant):
    """Fused round trip on frames that are one code repeated (every code x both laws) and on uniform random codes: the
    kernel derives the frame peak from max (|x|/4)^2 with a float square root, so every one of the 256 magnitudes has to
    come back exactly; codes, records and hold must equal the oracle's."""
    torch = gu.torch_cuda()
    C_, n = 512, 160
    codec = np.where(np.arange(C_) >= 256, 8, 0).astype(np.uint8)
    const = np.repeat((np.arange(C_) & 255).astype(np.uint8)[None, :, None], n, axis=2)          # [1][C][n]
    payload = np.concatenate([const, orc.gen_uniform(3 * C_ * n, seed=5).reshape(3, C_, n)], axis=0)
    F_ = payload.shape[0]
    d_out, d_st, d_hold = gu.dev_zeros(F_ * C_ * n, 0xEE), gu.dev_zeros(F_ * C_ * 16, 0xEE), gu.to_dev(gu.new_hold(C_))
    ctx.roundtrip_peakhold(gu.to_dev(payload), gu.to_dev(codec), C_, F_, n, d_out, d_st, d_hold, variant=variant)
    torch.cuda.synchronize()
    eout, est, ehold = orc.roundtrip_peakhold(payload, codec, gu.new_hold(C_).view(orc.CHAN_HOLD), variant=variant)
    gst = gu.to_host(d_st, capi.FRAME_STATS, (F_, C_))
    assert np.array_equal(gst["peak"], est["peak"])
    assert len(np.unique(est["peak"][0])) >= 240          # 128 + 128 magnitudes, a few shared by the two laws
    gu.assert_stats_equal(gst, est, n=n)
    assert np.array_equal(gu.to_host(d_out, np.uint8, (F_, C_, n)), eout)
    ghold = gu.to_host(d_hold, capi.CHAN_HOLD)
    for f in capi.CHAN_HOLD.names:
        assert np.array_equal(ghold[f], ehold[f]), f


def test_hold_update_and_reset(ctx, orc):
    torch = gu.torch_cuda()
    C_, F_, n = 300, 9, 160
    payload = orc.gen_uniform(F_ * C_ * n, seed=11).reshape(F_, C_, n)
    codec = np.where(np.arange(C_) % 4 == 0, 8, 0).astype(np.uint8)
    est = orc.decode_meter(payload, codec)
    gate = (np.arange(C_) % 3 != 1).astype(np.uint8)
    d_hold = gu.to_dev(gu.new_hold(C_))
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(2):                        # state persists across launches
        ctx.hold_update(gu.to_dev(est), C_, F_, n, d_hold, gate=gu.to_dev(gate), stream=s)
    torch.cuda.synchronize()
    eh = orc.hold_new(C_)
    for _ in range(2):
        orc.hold_update(est, n, eh, gate=gate)
    gh = gu.to_host(d_hold, capi.CHAN_HOLD)
    for f in capi.CHAN_HOLD.names:
        assert np.array_equal(gh[f], eh[f]), f
    mask = (np.arange(C_) % 2).astype(np.uint8)
    ctx.hold_reset(d_hold, C_, mask=gu.to_dev(mask), stream=s)
    torch.cuda.synchronize()
    gh2 = gu.to_host(d_hold, capi.CHAN_HOLD)
    assert np.all(gh2["count"][mask == 1] == 0) and np.all(gh2["level_min"][mask == 1] == 255)
    assert np.array_equal(gh2[mask == 0], gh[mask == 0])


# ----------------------------------------------------------------------------- generators
def test_gen_uniform_matches_oracle(ctx, orc):
    torch = gu.torch_cuda()
    for nbytes, first in ((4096, 0), (1000, 777), (13, 5), (160 * 64, 160 * 64 * 3)):
        d = gu.dev_zeros(nbytes + 16, 0xEE)
        ctx.gen_uniform(d, nbytes, seed=orc.SEED, first_byte=first, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = gu.to_host(d, np.uint8)
        assert np.array_equal(got[:nbytes], orc.gen_uniform(nbytes, first_byte=first))
        assert np.all(got[nbytes:] == 0xEE)


# ----------------------------------------------------------------------------- single-frame path
def test_staging_flush_poll_mirror_of_setIncomingRTP(ctx, orc):
    """igdsp_on_rtp_frame takes exactly what setIncomingRTP reads from tp_adapter (callID,
    payload_buff, payload_bufSize, pt).  trx->IncomingRTP == byte_mean must be bit-exact
    with the restated loop (roip_ed137.cpp:6564-6568); percent follows audiometer.cpp:30-31."""
    n = 160
    calls = {5: 0, 9: 1, 70000: 2, -3: 3}       # incl. ids outside the direct table
    for cid, ch in calls.items():
        ctx.map_call(cid, ch)
    ctx.reset_hold()
    codec = {5: 0, 9: 8, 70000: 0, -3: 8}
    frames = 6
    hold = orc.hold_new(4)
    for f in range(frames):
        batch = {}
        for cid, ch in calls.items():
            if f == 2 and cid == 9:
                assert ctx.on_rtp_frame(cid, 123, b"") == 0       # R2S keep-alive instead of audio
                continue
            ln = n if cid != -3 else 24 + f                        # short payloads (reference anticipates 24 / 164)
            pl = orc.gen_uniform(ln, seed=1000 * f + ch)
            assert ctx.on_rtp_frame(cid, codec[cid], pl.tobytes()) == 0
            batch[ch] = (pl, codec[cid])
        assert ctx.flush() == len(batch)
        for cid, ch in calls.items():
            lv = ctx.poll_call(cid)
            if ch not in batch:
                continue
            pl, pt = batch[ch]
            est = orc.decode_meter(pl.reshape(1, 1, -1), [pt])
            assert lv.byte_mean == int(est["byte_mean"][0, 0]) == orc.byte_mean(pl)
            assert lv.peak == int(est["peak"][0, 0])
            ref = np.sqrt(float(est["sumsq"][0, 0]) / pl.size)
            assert abs(lv.rms - ref) <= 1e-5 * ref + 1e-30
            assert lv.percent == orc.percent(np.float32(lv.rms))
            tmp = orc.hold_new(1)
            orc.hold_update(est, pl.size, tmp)
            hold["peak_hold"][ch] = max(hold["peak_hold"][ch], tmp["peak_hold"][0])
            hold["count"][ch] += 1
            hold["level_sum"][ch] += int(est["byte_mean"][0, 0])
            hold["samples"][ch] += pl.size
            assert lv.peak_hold == hold["peak_hold"][ch]
    assert ctx.flush() == 0                                         # nothing staged: nothing processed
    for cid, ch in calls.items():
        h = ctx.get_hold(ch)
        assert int(h["count"]) == int(hold["count"][ch]) and int(h["level_sum"]) == int(hold["level_sum"][ch])
        assert int(h["samples"]) == int(hold["samples"][ch])
        assert ctx.poll(ch).frames == hold["count"][ch]
    ctx.reset_hold(1)
    assert int(ctx.get_hold(1)["count"]) == 0 and int(ctx.get_hold(0)["count"]) == frames
    for cid in calls:
        ctx.unmap_call(cid)


@pytest.mark.parametrize("nch", [5, 200])
def test_staging_ring_meters_every_frame(orc, nch):
    """20 ms frames against a 40 ms tick (roip_ed137.cpp:1756): 2-3 frames are staged per call between two flushes.  The
    reference's hook runs on EVERY frame (TransportAdapter.cpp:303), so hold.count / level_sum / sumsq_acc / peak_hold /
    n_silent must equal the oracle's fold over ALL frames (keeplogAudioLevel per frame, Functions.cpp:2126-2145), the polled
    level is the NEWEST frame's, lengths other than 160 and a PT change mid-call ride along, and with >= 64 whole frames
    staged the records come from the tuned chunk kernel (nch = 200)."""
    c = capi.Context(device=0, max_channels=nch)
    try:
        for ch in range(nch):
            c.map_call(100 + ch, ch)
        rng = np.random.default_rng(nch)
        hold = orc.hold_new(nch)
        total = np.zeros(nch, np.int64)
        last = {}
        for tick in range(7):
            staged = 0
            for ch in range(nch):
                k = int(rng.integers(0, 4)) if ch else 3                      # 0..3 frames this tick; channel 0 always 3
                for j in range(k):
                    ln = 160 if (ch % 7) else int(rng.choice([24, 164, 160, 1, 255]))   # every 7th channel: odd lengths too
                    pt = 8 if (ch % 3 == 0 and tick >= 3) else 0              # law change mid-call
                    pl = orc.gen_uniform(ln, seed=10000 * tick + 10 * ch + j)
                    if ch == 1 and j == 0:
                        pl = np.full(ln, 0xFF, np.uint8)                       # digital silence
                    assert c.on_rtp_frame(100 + ch, pt, pl.tobytes()) == 0
                    est = orc.decode_meter(pl.reshape(1, 1, -1), [pt])
                    orc.hold_update(est, ln, hold[ch:ch + 1])
                    last[ch] = (est, ln)
                    staged += 1
                    total[ch] += 1
            assert c.flush() == staged
            for ch in range(nch):
                if ch not in last:
                    continue
                lv, (est, ln) = c.poll(ch), last[ch]
                assert (lv.byte_mean, lv.peak, lv.flags) == (int(est["byte_mean"][0, 0]), int(est["peak"][0, 0]), int(est["flags"][0, 0])), (tick, ch)
                ref = np.sqrt(float(est["sumsq"][0, 0]) / ln)
                assert abs(lv.rms - ref) <= 1e-5 * ref + 1e-30
                assert lv.frames == total[ch] and lv.dropped == 0
        for ch in range(nch):
            h = c.get_hold(ch)
            for f in capi.CHAN_HOLD.names:
                assert int(h[f]) == int(hold[f][ch]), (f, ch)
        # overflow: the ring holds IGDSP_STAGE_DEPTH frames; the 9th overwrites the oldest, says so, and is counted
        before = int(c.get_hold(0)["count"])
        pls = [orc.gen_uniform(160, seed=777 + j) for j in range(capi.STAGE_DEPTH + 2)]
        rcs = [c.on_rtp_frame(100, 0, p.tobytes()) for p in pls]
        assert rcs == [0] * capi.STAGE_DEPTH + [-16, -16]
        assert c.flush() == capi.STAGE_DEPTH
        lv = c.poll(0)
        assert lv.dropped == 2 and int(c.get_hold(0)["count"]) == before + capi.STAGE_DEPTH
        assert lv.byte_mean == orc.byte_mean(pls[-1])                          # the newest frame survived
        exp = orc.hold_new(1)
        for p in pls[2:]:
            orc.hold_update(orc.decode_meter(p.reshape(1, 1, -1), [0]), 160, exp)
        c.reset_hold(0)
    finally:
        c.close()


# ----------------------------------------------------------------------------- full-size properties
@pytest.fixture(scope="module")
def big(ctx):
    """BASELINE configs[2]: 65 536 ch x 128 frames, mu-law, D-uniform generated on the device."""
    torch = gu.torch_cuda()
    C_, F_, n = 65536, 128, 160
    d_pl = torch.empty((F_ * C_ * n,), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ctx.gen_uniform(d_pl, F_ * C_ * n, stream=s)
    d_cd = torch.zeros((C_,), dtype=torch.uint8, device="cuda")
    d_st = gu.dev_zeros(F_ * C_ * 16, 0xEE)
    d_agg = gu.dev_zeros(capi.AGGREGATE.itemsize)
    ctx.agg_reset(d_agg, stream=s)
    ctx.decode_meter(d_pl, d_cd, C_, F_, n, d_st, agg=d_agg, rank=0, stream=s)
    torch.cuda.synchronize()
    return dict(C=C_, F=F_, n=n, d_pl=d_pl, d_cd=d_cd, d_st=d_st, agg=gu.to_host(d_agg, capi.AGGREGATE)[0])


def test_full_size_checksum_of_checksums(big):
    """The launch aggregate (device atomics) equals the sum over the per-frame records."""
    st = gu.to_host(big["d_st"], capi.FRAME_STATS)
    agg = big["agg"]
    assert int(agg["frames"]) == st.size == big["C"] * big["F"]
    assert int(agg["samples"]) == st.size * big["n"]
    assert int(agg["sumsq"]) == int(st["sumsq"].sum(dtype=np.uint64))   # <= 8.4e6 * 1.66e11 < 2^64
    assert int(agg["byte_mean_sum"]) == int(st["byte_mean"].astype(np.int64).sum())
    assert int(agg["peak_slot"][0]) == int(st["peak"].max())
    assert int(agg["n_silent"]) == int((st["flags"] & 1).astype(np.int64).sum())
    assert int(agg["n_clipped"]) == int(((st["flags"] >> 2) & 1).astype(np.int64).sum())
    ref = np.sqrt(st["sumsq"].astype(np.float64) / big["n"])
    assert np.all(np.abs(st["rms"] - ref) <= 1e-5 * ref + 1e-30)


def test_full_size_sampled_frames_vs_oracle(big, orc):
    """Random frames (plus first/last chunks) of the 1.34 GB batch re-done by the oracle from the
    shard-invariant generator — no 1.3 GB host copy needed."""
    C_, F_, n = big["C"], big["F"], big["n"]
    st = gu.to_host(big["d_st"], capi.FRAME_STATS)
    rng = np.random.default_rng(3)
    idx = np.unique(np.concatenate([np.arange(64), np.arange(C_ * F_ - 64, C_ * F_), rng.integers(0, C_ * F_, 3000)]))
    for fi in idx:
        pl = orc.gen_uniform(n, first_byte=int(fi) * n)
        e = orc.decode_meter(pl.reshape(1, 1, n), [0])[0, 0]
        g = st[fi]
        assert (int(g["sumsq"]), int(g["peak"]), int(g["byte_mean"]), int(g["flags"])) == \
               (int(e["sumsq"]), int(e["peak"]), int(e["byte_mean"]), int(e["flags"])), fi


def test_full_size_variants_agree(ctx, big):
    """wave-per-frame (variant 1) and chunk32 (variant 2) produce identical records at full size."""
    torch = gu.torch_cuda()
    d_st1, d_st3 = gu.dev_zeros(big["F"] * big["C"] * 16, 0xEE), gu.dev_zeros(big["F"] * big["C"] * 16, 0xEE)
    ctx.set_variant(1)
    ctx.decode_meter(big["d_pl"], big["d_cd"], big["C"], big["F"], big["n"], d_st1, stream=torch.cuda.current_stream().cuda_stream)
    ctx.set_variant(3)
    ctx.decode_meter(big["d_pl"], big["d_cd"], big["C"], big["F"], big["n"], d_st3, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.set_variant(0)
    assert torch.equal(d_st3, big["d_st"])                     # the two chunk64 forms share every instruction that forms a record
    a, b = gu.to_host(d_st1, capi.FRAME_STATS), gu.to_host(big["d_st"], capi.FRAME_STATS)
    for f in ("sumsq", "peak", "byte_mean", "flags"):          # every integer field bit-identical
        assert np.array_equal(a[f], b[f]), f
    # rms: IEEE divide+sqrt (variant 1) vs multiply + v_sqrt_f32 (tuned path): within 4 ulp of each other,
    # both inside the 1e-5 contract (checked against float64 in test_full_size_checksum_of_checksums)
    assert np.all(np.abs(a["rms"].view(np.int32).astype(np.int64) - b["rms"].view(np.int32).astype(np.int64)) <= 4)


def test_full_size_roundtrip_idempotence_config5(ctx, big, orc):
    """BASELINE configs[4]: 65 536 ch mixed A-law/mu-law, fused decode->stats->encode + peak hold.
    Properties: codes reproduce (except mu 0x7F->0xFF); running the pass twice doubles the window
    sums and leaves peak-hold / max / min unchanged; hold equals a fold of the per-frame records."""
    torch = gu.torch_cuda()
    C_, F_, n = big["C"], 16, big["n"]
    d_pl = big["d_pl"][: F_ * C_ * n]
    codec = np.where(np.arange(C_) & 1, 8, 0).astype(np.uint8)
    d_cd = gu.to_dev(codec)
    d_out, d_st = torch.empty_like(d_pl), gu.dev_zeros(F_ * C_ * 16, 0xEE)
    d_hold = gu.to_dev(gu.new_hold(C_))
    s = torch.cuda.current_stream().cuda_stream
    ctx.roundtrip_peakhold(d_pl, d_cd, C_, F_, n, d_out, d_st, d_hold, stream=s)
    torch.cuda.synchronize()
    h1 = gu.to_host(d_hold, capi.CHAN_HOLD).copy()
    src = d_pl.view(F_, C_, n)
    mu = torch.from_numpy(codec == 0).cuda()[None, :, None]
    exp = torch.where((src == 0x7F) & mu, torch.full_like(src, 0xFF), src)
    assert torch.equal(d_out.view(F_, C_, n), exp)
    st = gu.to_host(d_st, capi.FRAME_STATS, (F_, C_))
    assert np.array_equal(h1["peak_hold"], st["peak"].max(axis=0))
    assert np.array_equal(h1["level_max"], st["byte_mean"].max(axis=0))
    assert np.array_equal(h1["level_min"], st["byte_mean"].min(axis=0))
    assert np.array_equal(h1["level_sum"], st["byte_mean"].astype(np.uint32).sum(axis=0))
    assert np.array_equal(h1["sumsq_acc"], st["sumsq"].sum(axis=0))
    assert np.all(h1["count"] == F_)
    d_out2 = torch.empty_like(d_out)
    ctx.roundtrip_peakhold(d_out, d_cd, C_, F_, n, d_out2, d_st, d_hold, stream=s)   # second pass over its own output
    torch.cuda.synchronize()
    assert torch.equal(d_out2, d_out)                                                 # idempotent after one pass
    h2 = gu.to_host(d_hold, capi.CHAN_HOLD)
    assert np.all(h2["count"] == 2 * F_) and np.array_equal(h2["sumsq_acc"], 2 * h1["sumsq_acc"])
    assert np.array_equal(h2["peak_hold"], h1["peak_hold"])
    # the decode_meter kernel sees the same frames identically
    d_st2 = gu.dev_zeros(F_ * C_ * 16, 0xEE)
    ctx.decode_meter(d_out, d_cd, C_, F_, n, d_st2, stream=s)
    torch.cuda.synchronize()
    st2 = gu.to_host(d_st2, capi.FRAME_STATS, (F_, C_))
    for f in ("sumsq", "peak", "flags"):
        assert np.array_equal(st2[f], st[f]), f
    # a sample of mixed-law frames against the oracle
    rng = np.random.default_rng(9)
    for fi in rng.integers(0, C_ * F_, 500):
        f, c = divmod(int(fi), C_)
        pl = orc.gen_uniform(n, first_byte=int(fi) * n)
        e = orc.decode_meter(pl.reshape(1, 1, n), [int(codec[c])])[0, 0]
        assert (int(st[f, c]["sumsq"]), int(st[f, c]["peak"]), int(st[f, c]["byte_mean"])) == \
               (int(e["sumsq"]), int(e["peak"]), int(e["byte_mean"]))


# ----------------------------------------------------------------------------- randomized shapes
def test_fuzz_shapes_against_oracle(ctx, orc):
    """120 random (C, F, n, law mix, ragged?, pcm?, agg?) cases, incl. the 64-frame super-chunk boundary,
    channel wrap inside a super-chunk and tails handed to the general kernel."""
    rng = np.random.default_rng(20241218)
    for case in range(120):
        n = int(rng.choice([160, 160, 160, 160, 24, 164, 96, 255, 1]))
        C_ = int(rng.choice([1, 3, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200]))
        F_ = int(rng.integers(1, 9))
        if rng.integers(0, 4) == 0:
            C_, F_ = int(rng.integers(60, 700)), int(rng.integers(1, 4))
        ragged = n != 160 and rng.integers(0, 2) == 1
        want_pcm, want_agg = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        payload = orc.gen_uniform(F_ * C_ * n, seed=1000 + case).reshape(F_, C_, n).copy()
        if rng.integers(0, 3) == 0:                                   # digital silence / full scale rows
            payload[rng.integers(0, F_), rng.integers(0, C_)] = rng.choice([0xFF, 0xD5, 0x00, 0x2A, 0x7F])
        codec = rng.choice(np.array([0, 8], np.uint8), size=C_)
        length = rng.integers(0, n + 1, size=(F_, C_)).astype(np.uint16) if ragged else None
        ctx.set_variant(int(rng.choice([0, 0, 1])))
        st, pcm, agg = gu.run_decode_meter(ctx, payload, codec, length=length, want_pcm=want_pcm, want_agg=want_agg, rank=case % 8)
        res = orc.decode_meter(payload, codec, length=length, want_pcm=want_pcm, want_agg=want_agg, rank=case % 8)
        res = res if isinstance(res, tuple) else (res,)
        gu.assert_stats_equal(st, res[0], n=length if ragged else n)
        k = 1
        if want_pcm:
            assert np.array_equal(pcm, res[k]), case
            k += 1
        if want_agg:
            for f in ("sumsq", "samples", "frames", "n_silent", "n_clipped", "byte_mean_sum"):
                assert int(agg[f]) == int(res[k][f]), (case, f)
            assert agg["peak_slot"].tolist() == res[k]["peak_slot"].tolist(), case
    ctx.set_variant(0)


def test_fuzz_roundtrip_shapes_against_oracle(ctx, orc):
    """60 random (C, F, n, law mix, gates, pre-existing hold, encoder lineage, fused-kernel form) cases of
    igdsp_roundtrip_peakhold: channel counts around the 64-channel group boundary, frame counts around the segment split,
    n = 160 and the other reference sizes."""
    torch = gu.torch_cuda()
    rng = np.random.default_rng(77)
    for case in range(60):
        n = int(rng.choice([160, 160, 160, 164, 24, 80, 7, 256]))
        C_ = int(rng.choice([1, 4, 63, 64, 65, 127, 128, 129, 192, 300, 640]))
        F_ = int(rng.choice([1, 2, 7, 8, 9, 16, 33, 70]))
        codec = rng.choice(np.array([0, 8], np.uint8), size=C_)
        payload = orc.gen_uniform(F_ * C_ * n, seed=5000 + case).reshape(F_, C_, n).copy()
        if rng.integers(0, 2):
            payload[rng.integers(0, F_), rng.integers(0, C_)] = rng.choice([0xFF, 0xD5, 0x00, 0x2A, 0x7F, 0x80])
        gate = (rng.integers(0, 3, C_) != 0).astype(np.uint8) if rng.integers(0, 2) else None
        hold0 = gu.new_hold(C_)
        hold0["count"] = rng.integers(0, 5, C_)
        hold0["peak_hold"] = rng.integers(0, 32000, C_)
        hold0["level_min"] = rng.integers(0, 256, C_)
        variant, kernel = int(rng.integers(0, 2)), int(rng.choice([0, 0, 4, 1]))
        d_out, d_st, d_hold = gu.dev_zeros(F_ * C_ * n, 0xEE), gu.dev_zeros(F_ * C_ * 16, 0xEE), gu.to_dev(hold0)
        ctx.set_variant(kernel)
        try:
            ctx.roundtrip_peakhold(gu.to_dev(payload), gu.to_dev(codec), C_, F_, n, d_out, d_st, d_hold,
                                   gate=None if gate is None else gu.to_dev(gate), variant=variant)
            torch.cuda.synchronize()
        finally:
            ctx.set_variant(0)
        eout, est, ehold = orc.roundtrip_peakhold(payload, codec, hold0.copy().view(orc.CHAN_HOLD), gate=gate, variant=variant)
        assert np.array_equal(gu.to_host(d_out, np.uint8, (F_, C_, n)), eout), case
        gu.assert_stats_equal(gu.to_host(d_st, capi.FRAME_STATS, (F_, C_)), est, n=n)
        ghold = gu.to_host(d_hold, capi.CHAN_HOLD)
        for f in capi.CHAN_HOLD.names:
            assert np.array_equal(ghold[f], ehold[f]), (case, f)


# ----------------------------------------------------------------------------- sharding (config #4 shape)
def test_channel_sharding_invariance(ctx, orc):
    """BASELINE configs[3] logic on one GPU: the G ranks' shards (contiguous channel ranges of the global
    [F][C][160] array, generated shard-invariantly) processed one after another give exactly the records of the
    unsharded run, and their aggregates SUM to its aggregate with each rank's peak alone in its slot."""
    from igate4xsoftphonedsp_amd import dist as igdist

    torch = gu.torch_cuda()
    C_, F_, n, G = 4096 + 64, 6, 160, 4
    codec = np.where((np.arange(C_) // 3) & 1, 8, 0).astype(np.uint8)
    full = orc.gen_uniform(F_ * C_ * n).reshape(F_, C_, n)
    st_full, _, agg_full = gu.run_decode_meter(ctx, full, codec, want_agg=True, rank=0)
    vec = np.zeros((capi.AGG_WORDS,), np.uint64)
    for g in range(G):
        lo, hi = igdist.channel_range(C_, g, G)
        d_pl = torch.empty((F_, hi - lo, n), dtype=torch.uint8, device="cuda")
        for f in range(F_):                                    # what bench.py does per rank
            ctx.gen_uniform(d_pl[f], (hi - lo) * n, first_byte=(f * C_ + lo) * n)
        torch.cuda.synchronize()
        shard = d_pl.cpu().numpy()
        assert np.array_equal(shard, full[:, lo:hi, :])
        st, _, agg = gu.run_decode_meter(ctx, shard, codec[lo:hi], want_agg=True, rank=g)
        for fld in ("sumsq", "peak", "byte_mean", "flags"):
            assert np.array_equal(st[fld], st_full[fld][:, lo:hi]), (g, fld)
        vec += np.frombuffer(agg.tobytes(), np.uint64)        # the all-reduce(SUM) of SURVEY 8(e)
    node = igdist.node_view(torch.from_numpy(vec.view(np.int64)))
    assert node["sumsq"] == int(agg_full["sumsq"]) and node["frames"] == C_ * F_ and node["samples"] == C_ * F_ * n
    assert node["peak"] == int(st_full["peak"].max()) and node["byte_mean_sum"] == int(agg_full["byte_mean_sum"])
    assert sorted(int(x) for x in vec[6 * capi.AGG_LINE_WORDS:6 * capi.AGG_LINE_WORDS + G]) == sorted(int(st_full["peak"][:, slice(*igdist.channel_range(C_, g, G))].max()) for g in range(G))


def test_half_million_channels_one_launch(ctx, orc):
    """524 288 channels (BASELINE configs[3] total) in one launch on one GPU: 32-bit frame indexing, channel wrap
    and the work queue at 8x the headline channel count; sampled frames against the oracle."""
    torch = gu.torch_cuda()
    C_, F_, n = 524288, 16, 160
    d_pl = torch.empty((F_ * C_ * n,), dtype=torch.uint8, device="cuda")
    ctx.gen_uniform(d_pl, d_pl.numel(), seed=5)
    codec = np.where(np.arange(C_) % 5 == 0, 8, 0).astype(np.uint8)
    d_st, d_agg = gu.dev_zeros(F_ * C_ * 16, 0xEE), gu.dev_zeros(capi.AGGREGATE.itemsize)
    ctx.decode_meter(d_pl, gu.to_dev(codec), C_, F_, n, d_st, agg=d_agg)
    torch.cuda.synchronize()
    st = gu.to_host(d_st, capi.FRAME_STATS)
    agg = gu.to_host(d_agg, capi.AGGREGATE)[0]
    assert int(agg["frames"]) == C_ * F_ and int(agg["sumsq"]) == int(st["sumsq"].sum(dtype=np.uint64))
    rng = np.random.default_rng(1)
    for fi in np.unique(np.concatenate([[0, C_ * F_ - 1], rng.integers(0, C_ * F_, 1500)])):
        c = int(fi) % C_
        e = orc.decode_meter(orc.gen_uniform(n, seed=5, first_byte=int(fi) * n).reshape(1, 1, n), [int(codec[c])])[0, 0]
        g = st[fi]
        assert (int(g["sumsq"]), int(g["peak"]), int(g["byte_mean"]), int(g["flags"])) == (int(e["sumsq"]), int(e["peak"]), int(e["byte_mean"]), int(e["flags"])), fi


def test_probe_placement(ctx):
    """igdsp_probe_placement: a positive per-launch time of the bare read + record stream, with a scratch or a
    caller-supplied record buffer; argument rules."""
    import ctypes as C
    torch = gu.torch_cuda()
    nbytes = 64 << 20
    buf = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    rec = torch.empty((nbytes // 10 + 4096,), dtype=torch.uint8, device="cuda")
    for out in (None, rec):
        ms = ctx.probe_placement(buf, nbytes, out=out, reps=5)
        assert 0.0 < ms < 5.0                                 # 64 MiB at >= 15 GB/s even on a throttled box
    out = C.c_float(0)
    fn = ctx.L.igdsp_probe_placement
    assert fn(ctx.h, buf.data_ptr(), nbytes, None, 0, C.byref(out), None) == -22                 # reps == 0
    assert fn(ctx.h, buf.data_ptr() + 4, nbytes - 4, None, 5, C.byref(out), None) == -22         # alignment
    assert fn(ctx.h, buf.data_ptr(), nbytes, rec.data_ptr() + 8, 5, C.byref(out), None) == -22   # alignment of the output
    assert fn(ctx.h, buf.data_ptr(), 100, None, 5, C.byref(out), None) == -22                    # < one item
    assert fn(ctx.h, None, nbytes, None, 5, C.byref(out), None) == -22


def test_dev_alloc_far(ctx):
    """igdsp_dev_alloc_far: returns a usable output buffer whose probe time is never worse than the plain first
    allocation's (on a box with room it is ~10 % better); argument rules."""
    import ctypes as C
    torch = gu.torch_cuda()
    nbytes = 256 << 20
    src = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    ptr, t0, t1 = C.c_void_p(), C.c_float(0), C.c_float(0)
    fn = ctx.L.igdsp_dev_alloc_far
    rc = fn(ctx.h, C.byref(ptr), 64 << 20, src.data_ptr(), nbytes, 12, 8 << 30, C.byref(t0), C.byref(t1))
    assert rc == 0 and ptr.value
    assert 0 < t1.value <= t0.value * 1.0001
    assert ctx.L.igdsp_dev_memset(ctx.h, ptr, 0x5A, 64 << 20) == 0             # the buffer is real
    torch.cuda.synchronize()
    assert ctx.L.igdsp_dev_free(ctx.h, ptr) == 0
    assert fn(ctx.h, C.byref(ptr), 0, src.data_ptr(), nbytes, 4, 0, None, None) == -22
    assert fn(ctx.h, C.byref(ptr), 1 << 20, None, nbytes, 4, 0, None, None) == -22
    assert fn(ctx.h, C.byref(ptr), 1 << 20, src.data_ptr(), nbytes, 0, 0, None, None) == -22


def test_io_alloc_places_buffers_and_they_work(ctx, orc):
    """igdsp_io_alloc (the placement that round 1 kept in bench.py, now in the product): one call for a config-#5-shaped buffer
    set at the headline size.  (i) the buffers behave like any device memory: the fused round trip on them equals the run on
    plain torch buffers byte for byte, and sampled frames equal the oracle; (ii) when the box shows more than one class of
    device memory, the bare read + record stream from the placed input into the placed record buffer is >= 8 % faster than the
    same stream writing into the input's OWN class (what consecutive plain allocations normally give); (iii) small sets are
    served without probing; argument rules."""
    torch = gu.torch_cuda()
    C_, F_, n = 65536, 128, 160
    B = F_ * C_ * n
    s = torch.cuda.current_stream().cuda_stream
    ioset, (p_in, p_st, p_out), rep = ctx.io_alloc([(B, capi.IO_INPUT), (F_ * C_ * 16, capi.IO_RECORD), (B, capi.IO_BULK)])
    try:
        assert p_in and p_st and p_out and p_in % (2 << 20) == 0 and rep["chunk_bytes"] >= (2 << 20)
        d_pl, d_st, d_out = capi.as_tensor(p_in, B), capi.as_tensor(p_st, F_ * C_ * 16), capi.as_tensor(p_out, B)
        ctx.gen_uniform(d_pl, B, stream=s)
        codec = np.where(np.arange(C_) & 1, 8, 0).astype(np.uint8)
        d_cd = gu.to_dev(codec)
        hold_a, hold_b = gu.to_dev(gu.new_hold(C_)), gu.to_dev(gu.new_hold(C_))
        ctx.roundtrip_peakhold(d_pl, d_cd, C_, F_, n, d_out, d_st, hold_a, stream=s)
        t_pl = d_pl.clone()
        t_st, t_out = torch.empty_like(d_st), torch.empty_like(d_out)
        ctx.roundtrip_peakhold(t_pl, d_cd, C_, F_, n, t_out, t_st, hold_b, stream=s)
        torch.cuda.synchronize()
        assert torch.equal(d_out, t_out) and torch.equal(d_st, t_st) and torch.equal(hold_a, hold_b)
        st = gu.to_host(d_st, capi.FRAME_STATS)
        rng = np.random.default_rng(3)
        for fi in np.unique(np.concatenate([[0, C_ * F_ - 1], rng.integers(0, C_ * F_, 400)])):
            e = orc.decode_meter(orc.gen_uniform(n, first_byte=int(fi) * n).reshape(1, 1, n), [int(codec[int(fi) % C_])])[0, 0]
            assert (int(st[fi]["sumsq"]), int(st[fi]["peak"]), int(st[fi]["byte_mean"])) == (int(e["sumsq"]), int(e["peak"]), int(e["byte_mean"]))
        if rep["classes_found"] >= 2:
            assert rep["placed"] == 1 and rep["probe_ms_other"] <= 0.92 * rep["probe_ms_same"]
            # the call waits until the driver has cleared what the search gave back: bounded, and part of setup_ms
            assert 0.0 < rep["settle_ms"] <= 9000.0 and rep["settle_ms"] <= rep["setup_ms"]
            # The library's two levels come from its own probe stream on freshly created (zero) memory; with real data the same
            # stream runs ~4 % slower at either level, so the placed pair is compared, on the same data, with (i) a pair the
            # library builds in ONE class on purpose (both buffers given the INPUT role: what consecutive plain allocations
            # normally amount to) and (ii), for the record, a naive pair of plain consecutive allocations through the ABI.
            same_set, (s_in, s_st), _ = ctx.io_alloc([(B, capi.IO_INPUT), (F_ * C_ * 16, capi.IO_INPUT)])
            n_in, n_st = ctx.dev_alloc(B), ctx.dev_alloc(F_ * C_ * 16)
            try:
                ctx.gen_uniform(s_in, B, stream=s)
                ctx.gen_uniform(n_in, B, stream=s)
                for _ in range(12):                                                 # clocks, and the driver's clearing of the memory freed above
                    ctx.probe_placement(d_pl, B, out=d_st, reps=10, stream=s)
                t_placed = min(ctx.probe_placement(d_pl, B, out=d_st, reps=10, stream=s) for _ in range(3))
                t_same = min(ctx.probe_placement(s_in, B, out=s_st, reps=10, stream=s) for _ in range(3))
                t_naive = min(ctx.probe_placement(n_in, B, out=n_st, reps=10, stream=s) for _ in range(3))
            finally:
                ctx.dev_free(n_in)
                ctx.dev_free(n_st)
                same_set.close()
            print(f"bare stream, whole batch -> records: placed {t_placed:.4f} ms, one class on purpose {t_same:.4f} ms, naive {t_naive:.4f} ms, report {rep}")
            assert t_placed <= 1.03 * t_naive, (t_placed, t_naive)                  # never worse than what a host would get by itself
            assert t_placed <= 0.97 * t_same, (t_placed, t_same, rep)               # measured 5-10 % (0.227-0.234 vs 0.247-0.255 ms); 13-20 % for bulk outputs
    finally:
        ioset.close()
    # small inputs: nothing to place, nothing probed
    ioset, ptrs, rep = ctx.io_alloc([(1 << 20, capi.IO_INPUT), (4096, capi.IO_RECORD)])
    assert all(ptrs) and rep["placed"] == 0 and rep["probes"] == 0
    t = capi.as_tensor(ptrs[1], 4096)
    t.fill_(7)
    torch.cuda.synchronize()
    assert int(t.sum().item()) == 7 * 4096
    ioset.close()
    # argument rules
    arr = (capi.IoBuf * 1)()
    arr[0].bytes, arr[0].role = 0, capi.IO_INPUT
    import ctypes as C
    st_, r_ = C.c_void_p(), capi.IoReport()
    assert ctx.L.igdsp_io_alloc(ctx.h, arr, 1, 0, C.byref(st_), C.byref(r_)) == -22
    arr[0].bytes, arr[0].role = 4096, 9
    assert ctx.L.igdsp_io_alloc(ctx.h, arr, 1, 0, C.byref(st_), C.byref(r_)) == -22
    assert ctx.L.igdsp_io_alloc(ctx.h, arr, 0, 0, C.byref(st_), C.byref(r_)) == -22
    assert ctx.L.igdsp_io_free(ctx.h, None) == 0


def test_flush_gates_by_ed137_word_and_follows_the_silence_run(orc):
    """The drop-in path with the reference's third hook: igdsp_set_ed137 (= setIncomingED137Value, roip_ed137.h:273) gives a call
    its current ED-137 word, igdsp_set_gate_mode picks the gate, and every flush folds each staged frame into the call's window
    only if the word it was staged under passes (PTT / SQU masks Functions.cpp:1136, 1160); the consecutive-silence run
    (adapter->rtpFalse, TransportAdapter.cpp:657-673) follows EVERY frame in arrival order — also when 160-byte and other frames
    of one call alternate inside a flush.  Against the oracle's window restatement over all frames; begin / end split; poll
    while a flush is open."""
    nch = 70
    c = capi.Context(device=0, max_channels=nch)
    try:
        for ch in range(nch):
            c.map_call(500 + ch, ch)
        rng = np.random.default_rng(5)
        words = {}                                                        # the calls' current ED-137 words persist across the modes
        for mode in (capi.GATE_SQU, capi.GATE_PTT, capi.GATE_SQU_OR_PTT, capi.GATE_ALWAYS):
            c.set_gate_mode(mode)
            c.reset_hold()
            hold = orc.hold_new(nch)
            probe = np.zeros(nch, orc.CHAN_PROBE)
            for ch in range(nch):
                p = c.get_probe(ch)
                probe["run"][ch], probe["alarms"][ch] = p.run, p.alarms          # the run carries over from the previous mode's frames
            last = {}
            for tick in range(9):
                staged = 0
                for ch in range(nch):
                    for j in range(int(rng.integers(0, 4))):
                        if rng.integers(0, 3) == 0:
                            word = int(rng.integers(0, 1 << 32)) if rng.integers(0, 2) else 0
                            c.set_ed137(500 + ch, word)
                            words[ch] = word
                        word = words.get(ch, 0)
                        ln = 160 if rng.integers(0, 4) else int(rng.choice([24, 48, 52, 164, 255]))
                        pl = np.full(ln, 0xD5, np.uint8) if rng.integers(0, 2) else orc.gen_uniform(ln, seed=tick * 100000 + ch * 10 + j)
                        assert c.on_rtp_frame(500 + ch, 8, pl.tobytes()) == 0
                        est = orc.decode_meter(pl.reshape(1, 1, -1), [8])
                        info = np.zeros((1, 1), orc.RTP_INFO)
                        info["ed137"], info["payload_len"] = word, ln
                        orc.window_update(est, hold[ch:ch + 1], info=info, n=256, gate_mode=mode, probe=probe[ch:ch + 1])
                        last[ch] = est
                        staged += 1
                if tick % 2:
                    assert c.flush() == staged
                else:                                                    # the non-blocking pair, with a poll in between
                    assert c.flush_begin() == staged
                    c.poll(0)
                    assert c.flush_end(wait=True) == 0
                for ch in range(nch):
                    if ch in last:
                        lv = c.poll(ch)
                        assert (lv.byte_mean, lv.peak, lv.flags) == (int(last[ch]["byte_mean"][0, 0]), int(last[ch]["peak"][0, 0]), int(last[ch]["flags"][0, 0]))
            for ch in range(nch):
                h, p = c.get_hold(ch), c.get_probe(ch)
                for f in capi.CHAN_HOLD.names:
                    assert int(h[f]) == int(hold[f][ch]), (mode, f, ch)
                assert (p.run, p.alarms) == (int(probe["run"][ch]), int(probe["alarms"][ch])), (mode, ch)
            if mode != capi.GATE_ALWAYS:
                assert 0 < int(hold["count"].sum()) < int(sum(c.poll(ch).frames for ch in range(nch)))
        assert c.L.igdsp_set_gate_mode(c.h, 9) == -22 and c.L.igdsp_set_ed137(c.h, 9999, 0) == -2
    finally:
        c.close()


def test_io_alloc_later_calls_are_served_from_spares(orc):
    """What a search learnt stays with the context: chunks of known class that the first igdsp_io_alloc did not need (and the
    chunks of a set given back with igdsp_io_free) are kept as spares, and a later set that they cover is mapped without a
    single probe, in well under 100 ms, with nothing released (no settle wait) — and is placed like the first."""
    torch = gu.torch_cuda()
    c = capi.Context(device=0, max_channels=64)
    try:
        C_, F_, n = 65536, 128, 160
        B = F_ * C_ * n
        s = torch.cuda.current_stream().cuda_stream
        spec = [(B, capi.IO_INPUT), (F_ * C_ * 16, capi.IO_RECORD)]
        set1, p1, rep1 = c.io_alloc(spec)
        if rep1["classes_found"] < 2:
            set1.close()
            pytest.skip("one class of device memory on this box")
        assert rep1["placed"] == 1 and rep1["probes"] > 0
        set2, p2, rep2 = c.io_alloc(spec)                                  # while the first set is alive: from the search's leftovers
        print("first", rep1, "second", rep2)
        assert rep2["placed"] == 1 and rep2["probes"] == 0 and rep2["chunks_explored"] == 0 and rep2["settle_ms"] == 0.0
        assert rep2["setup_ms"] < 100.0, rep2
        assert set(p1).isdisjoint(p2)
        for p in (p1, p2):
            c.gen_uniform(p[0], B, stream=s)
        for _ in range(10):
            c.probe_placement(p1[0], B, out=p1[1], reps=10, stream=s)
        t1 = min(c.probe_placement(p1[0], B, out=p1[1], reps=10, stream=s) for _ in range(3))
        t2 = min(c.probe_placement(p2[0], B, out=p2[1], reps=10, stream=s) for _ in range(3))
        t_cross = min(c.probe_placement(p1[0], B, out=p2[0], reps=10, stream=s) for _ in range(3))   # input -> the other set's INPUT: one class
        print(f"placed pair of the searched set {t1:.4f} ms, of the set from spares {t2:.4f} ms, input -> input (one class) {t_cross:.4f} ms")
        assert t2 <= 1.03 * t1 and t2 <= 0.97 * t_cross
        # records through the set from spares equal the oracle (the one-class probe above wrote into this set's input: fill it again)
        c.gen_uniform(p2[0], B, stream=s)
        d_st = capi.as_tensor(p2[1], F_ * C_ * 16)
        c.decode_meter(capi.as_tensor(p2[0], B), torch.zeros((C_,), dtype=torch.uint8, device="cuda"), C_, F_, n, d_st, stream=s)
        torch.cuda.synchronize()
        st = gu.to_host(d_st, capi.FRAME_STATS)
        for fi in (0, 12345, C_ * F_ - 1):
            e = orc.decode_meter(orc.gen_uniform(n, first_byte=int(fi) * n).reshape(1, 1, n), [0])[0, 0]
            assert (int(st[fi]["sumsq"]), int(st[fi]["peak"]), int(st[fi]["byte_mean"])) == (int(e["sumsq"]), int(e["peak"]), int(e["byte_mean"]))
        set1.close()
        set2.close()
        set3, p3, rep3 = c.io_alloc(spec)                                  # the chunks the two sets gave back serve the next one
        assert rep3["placed"] == 1 and rep3["probes"] == 0 and rep3["setup_ms"] < 100.0, rep3
        set3.close()
    finally:
        c.close()
