"""-m gpu: every kernel instantiation behind igdsp_decode_meter and igdsp_roundtrip_peakhold (tests/kernel_matrix.py), against
the C oracle.  Records, PCM, re-encoded codes, hold windows and the launch aggregate bit-exact; fp32 RMS within 1e-5 relative of
the float64 definition.

- small: every row once, the meter rows without and with the aggregate, the round-trip rows with both encoder lineages;
- cross-check: every fast meter row again through the general kernels (IGDSP_NO_TINY / IGDSP_NO_STRIDED): the same outputs;
- full chip: every fast instantiation at 65 536 channels (grid == 256, several queue batches per wave), one case at 65 519
  channels, and closed-form silence / full-scale launches that check the counters without the oracle;
- one stream: different persistent kernels back to back without a host sync, with the device work queue and with the
  static schedule — a kernel that re-armed the stream's queue pair wrongly would make the next one skip or repeat work."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import kernel_matrix as km  # noqa: E402

RANK = 5
GUARD = 64
AGG_FIELDS = ("sumsq", "samples", "frames", "n_silent", "n_clipped", "byte_mean_sum")
FAST_ROWS = [r for r in km.METER_ROWS if r.fast != "none"]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=4096)
    yield c
    c.close()


class _Env:
    """IGDSP_* knobs for the launches inside the block (the launchers read them on every call)."""

    def __init__(self, knobs):
        self.knobs = dict(knobs)

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.knobs}
        os.environ.update(self.knobs)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _buf(nbytes, off, fill=0xEE):
    """A device buffer of nbytes at `off` bytes past a 256-byte aligned address, with guard bytes on both sides."""
    raw = gu.dev_zeros(nbytes + 256 + GUARD, fill)
    start = (-raw.data_ptr()) % 256 + off
    v = raw[start:start + nbytes]
    assert v.data_ptr() % 256 == off
    return raw, start, v


def _guards_intact(raw, start, nbytes, fill=0xEE):
    return bool(np.all(raw[:start].cpu().numpy() == fill) and np.all(raw[start + nbytes:].cpu().numpy() == fill))


def _codec(C_, salt=0):
    return np.where((np.arange(C_) * 7 + salt) % 5 < 2, 8, 0).astype(np.uint8)


def _edge_frames(n):
    ramp = (np.arange(n) & 0xFF).astype(np.uint8)
    return [np.full(n, 0xFF, np.uint8), np.full(n, 0xD5, np.uint8), np.full(n, 0x00, np.uint8),
            np.full(n, 0x80, np.uint8), np.full(n, 0x7F, np.uint8), np.full(n, 0x2A, np.uint8),
            np.full(n, 0xAA, np.uint8), ramp, ramp[::-1].copy()]


def _small_payload(orc, n, seed):
    """SMALL_C x SMALL_F frames: uniform codes, the edge frames on channels of both laws, and every code once in a row of
    consecutive bytes (one frame of n >= 256, the frames after it otherwise) on channel 17."""
    C_, F_ = km.SMALL_C, km.SMALL_F
    payload = orc.gen_uniform(F_ * C_ * n, seed=seed).reshape(F_, C_, n).copy()
    for k, fr in enumerate(_edge_frames(n)):
        payload[k % F_, (13 * k + 1) % C_] = fr
        payload[(k + 3) % F_, (29 * k + 2) % C_] = fr
    flat = payload.reshape(-1)
    start = (3 * C_ + 17) * n
    flat[start:start + 256] = np.arange(256, dtype=np.uint8)
    return payload


# ----------------------------------------------------------------------------- meter: one launch and its checks
def _run_meter(ctx, row, payload, codec, length, agg, C_, F_, d_payload=None, knobs=None, stream=None):
    """One igdsp_decode_meter launch with the row's buffers; returns (records, pcm | None, aggregate | None) on the host."""
    torch = gu.torch_cuda()
    n = row.n
    nb = F_ * C_ * n
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    if d_payload is None:
        _, _, d_payload = _buf(nb, row.payload_off)
        d_payload.copy_(torch.from_numpy(np.ascontiguousarray(payload).reshape(-1)))
    assert d_payload.data_ptr() % 16 == row.payload_off % 16
    st_raw, st_at, d_st = _buf(F_ * C_ * 16, row.stats_off)
    pcm = row.pcm_off is not None
    if pcm:
        pcm_raw, pcm_at, d_pcm = _buf(nb * 2, row.pcm_off)
    d_agg = gu.dev_zeros(capi.AGGREGATE.itemsize) if agg else None
    d_len = gu.to_dev(np.asarray(length, dtype="<u2")) if length is not None else None
    torch.cuda.synchronize()
    if agg:
        ctx.agg_reset(d_agg, stream=s)
    ctx.set_variant(row.variant)
    try:
        with _Env(row.knobs if knobs is None else knobs):
            ctx.decode_meter(d_payload, gu.to_dev(codec), C_, F_, n, d_st, pcm=d_pcm if pcm else None, length=d_len, agg=d_agg,
                             rank=RANK, stream=s)
        torch.cuda.synchronize()
    finally:
        ctx.set_variant(0)
    assert _guards_intact(st_raw, st_at, F_ * C_ * 16), f"{row.id}: bytes around the records were written"
    if pcm:
        assert _guards_intact(pcm_raw, pcm_at, nb * 2), f"{row.id}: bytes around the PCM were written"
    return (gu.to_host(d_st, capi.FRAME_STATS, (F_, C_)), gu.to_host(d_pcm, "<i2", (F_, C_, n)) if pcm else None,
            gu.to_host(d_agg, capi.AGGREGATE)[0] if agg else None)


def _check_meter(row, got, exp, n):
    st, pcm, agg = got
    est, epcm, eagg = exp
    gu.assert_stats_equal(st, est, n=n)
    if pcm is not None:
        assert np.array_equal(pcm, epcm), f"{row.id}: PCM differs at {np.argwhere(pcm != epcm)[:3].tolist()}"
    if agg is not None:
        for f in AGG_FIELDS:
            assert int(agg[f]) == int(eagg[f]), (row.id, f, int(agg[f]), int(eagg[f]))
        assert agg["peak_slot"].tolist() == eagg["peak_slot"].tolist(), row.id
        assert int(agg["peak_slot"][RANK]) > 0


def _oracle_meter(orc, payload, codec, length, want_pcm):
    if want_pcm:
        return orc.decode_meter(payload, codec, length=length, want_pcm=True, want_agg=True, rank=RANK)
    est, eagg = orc.decode_meter(payload, codec, length=length, want_agg=True, rank=RANK)
    return est, None, eagg


def _small_meter_case(orc, row):
    payload = _small_payload(orc, row.n, seed=row.n * 11 + row.payload_off)
    codec = _codec(km.SMALL_C)
    length = None
    if row.has_len:
        rng = np.random.default_rng(row.n)
        length = rng.integers(0, row.n + 1, size=(km.SMALL_F, km.SMALL_C)).astype(np.uint16)
        length[0, :8] = [0, 1, 2, 3, row.n, row.n - 1, 49, 48]
    return payload, codec, length


# ----------------------------------------------------------------------------- a. every row, small
@pytest.mark.parametrize("agg", [0, 1], ids=["noagg", "agg"])
@pytest.mark.parametrize("row", km.METER_ROWS, ids=[r.id for r in km.METER_ROWS])
def test_small_meter_row(ctx, orc, row, agg):
    payload, codec, length = _small_meter_case(orc, row)
    exp = _oracle_meter(orc, payload, codec, length, row.pcm_off is not None)
    got = _run_meter(ctx, row, payload, codec, length, agg, km.SMALL_C, km.SMALL_F)
    _check_meter(row, got, exp, length if row.has_len else row.n)


# ----------------------------------------------------------------------------- b. the same input through the general kernels
@pytest.mark.parametrize("row", FAST_ROWS, ids=[r.id for r in FAST_ROWS])
def test_fast_meter_row_equals_general_kernels(ctx, orc, row):
    """IGDSP_NO_TINY, IGDSP_NO_STRIDED and both: k_meter_tiny / k_meter_strided give way to the strided or the general kernels
    (k_meter_image, k_meter_wave_per_frame).  Every integer field of every record, the PCM and the aggregate must equal the
    fast kernel's; RMS of both against the float64 definition."""
    payload, codec, length = _small_meter_case(orc, row)
    fast = _run_meter(ctx, row, payload, codec, length, 1, km.SMALL_C, km.SMALL_F)
    for knobs in ((("IGDSP_NO_TINY", "1"),), (("IGDSP_NO_STRIDED", "1"),), (("IGDSP_NO_TINY", "1"), ("IGDSP_NO_STRIDED", "1"))):
        other = _run_meter(ctx, row, payload, codec, length, 1, km.SMALL_C, km.SMALL_F, knobs=row.knobs + knobs)
        for f in ("sumsq", "peak", "byte_mean", "flags"):
            assert np.array_equal(other[0][f], fast[0][f]), (row.id, knobs, f)
        gu.assert_stats_equal(other[0], fast[0], n=row.n)
        if fast[1] is not None:
            assert np.array_equal(other[1], fast[1]), (row.id, knobs)
        assert other[2].tobytes() == fast[2].tobytes(), (row.id, knobs)


# ----------------------------------------------------------------------------- c. full chip
FULL_NS = sorted({r.n for r in FAST_ROWS if r.full})


def _full_meter(ctx, orc, rows, C_, F_, seed):
    torch = gu.torch_cuda()
    n = rows[0].n
    codec = _codec(C_, salt=n)
    nb = F_ * C_ * n
    exp = _oracle_meter(orc, orc.gen_uniform(nb, seed=seed).reshape(F_, C_, n), codec, None, any(r.pcm_off is not None for r in rows))
    for row in rows:
        _, _, d_pl = _buf(nb, row.payload_off)
        ctx.gen_uniform(d_pl, nb, seed=seed, stream=torch.cuda.current_stream().cuda_stream)
        got = _run_meter(ctx, row, None, codec, None, 1, C_, F_, d_payload=d_pl)
        del d_pl
        _check_meter(row, got, (exp[0], exp[1] if row.pcm_off is not None else None, exp[2]), n)
        assert int(got[2]["frames"]) == C_ * F_


@pytest.mark.parametrize("n", FULL_NS)
def test_full_chip_meter(ctx, orc, n):
    """Every fast instantiation of frame size n at 65 536 channels (64 frames for n <= 32, 16 otherwise), with the aggregate:
    every record, and the PCM of the storing rows, against the oracle on the same generator."""
    _full_meter(ctx, orc, [r for r in FAST_ROWS if r.full and r.n == n], km.FULL_C, km.meter_full_f(n), seed=7000 + n)


@pytest.mark.parametrize("fast,key,store", [("strided", 21, False), ("tiny", 6, False), ("strided", 30, True)])
def test_full_chip_meter_channels_not_a_multiple_of_64(ctx, orc, fast, key, store):
    """65 519 channels: super-chunks straddle channels all through the launch, and the < 64-frame tail goes to the rest kernel."""
    row = next(r for r in FAST_ROWS if (r.fast, r.key, r.store) == (fast, key, store))
    _full_meter(ctx, orc, [row], km.FULL_C_ODD, km.meter_full_f(row.n), seed=9000 + row.n)


FULL_SCALE = {0: (0x80, 32124), 8: (0xAA, 32256)}      # law -> (code, |x|)
SILENCE = {0: (0xFF, 0), 8: (0xD5, 8)}


@pytest.mark.parametrize("kind", ["silence", "full_scale"])
@pytest.mark.parametrize("row", [r for r in FAST_ROWS if r.id in ("tiny-k6-n24", "chunk-n160", "strided-k21-n164", "strided-k30-store-n240")],
                         ids=lambda r: r.id)
def test_full_chip_meter_closed_form(ctx, row, kind):
    """Every frame one code repeated, both laws: digital silence (mu 0xFF, A 0xD5) or full scale (mu 0x80, A 0xAA).  The records
    and the aggregate follow by integer arithmetic: frames = C F, n_silent or n_clipped = frames, sumsq = F n (C_mu 32124^2 +
    C_A 32256^2) at full scale."""
    torch = gu.torch_cuda()
    C_, F_, n = km.FULL_C, km.meter_full_f(row.n), row.n
    codec = np.where(np.arange(C_) % 3 == 1, 8, 0).astype(np.uint8)
    table = SILENCE if kind == "silence" else FULL_SCALE
    per_ch = np.where(codec == 8, table[8][0], table[0][0]).astype(np.uint8)
    mag = np.where(codec == 8, table[8][1], table[0][1]).astype(np.int64)
    _, _, d_pl = _buf(F_ * C_ * n, row.payload_off)
    d_pl.view(F_, C_, n).copy_(gu.to_dev(per_ch).view(1, C_, 1).expand(F_, C_, n))
    st, pcm, agg = _run_meter(ctx, row, None, codec, None, 1, C_, F_, d_payload=d_pl)
    frames = C_ * F_
    assert int(agg["frames"]) == frames and int(agg["samples"]) == frames * n
    assert int(agg["sumsq"]) == F_ * n * int((mag * mag).sum())
    assert int(agg["n_silent"]) == (frames if kind == "silence" else 0)
    assert int(agg["n_clipped"]) == (frames if kind == "full_scale" else 0)
    assert int(agg["byte_mean_sum"]) == F_ * int(per_ch.astype(np.int64).sum())
    assert int(agg["peak_slot"][RANK]) == int(mag.max()) and sum(int(x) for x in agg["peak_slot"]) == int(mag.max())
    assert np.array_equal(st["sumsq"], np.broadcast_to(n * mag * mag, (F_, C_)))
    assert np.array_equal(st["peak"], np.broadcast_to(mag, (F_, C_)))
    assert np.array_equal(st["byte_mean"], np.broadcast_to(per_ch, (F_, C_)))
    probe = (per_ch == 0xD5) & (n > 48)
    flags = np.where(probe, 2, 0) | (1 if kind == "silence" else 4)
    assert np.array_equal(st["flags"], np.broadcast_to(flags, (F_, C_)))
    assert np.all(np.abs(st["rms"].astype(np.float64) - mag) <= 1e-5 * mag)
    if pcm is not None:                                 # every one of these codes decodes to +|x|: mu 0x80, A 0xAA, A 0xD5 (and mu 0xFF to 0)
        assert np.array_equal(pcm, np.broadcast_to(mag.astype(np.int16)[None, :, None], (F_, C_, n)))


# ----------------------------------------------------------------------------- round trip
def _rt_payload(orc, C_, F_, n, seed):
    payload = orc.gen_uniform(F_ * C_ * n, seed=seed).reshape(F_, C_, n).copy()
    payload[0, 0, :] = 0x7F                                 # mu-law negative zero: the one code that does not come back
    payload[F_ - 1, C_ - 1, :] = 0xD5
    payload[F_ // 2, C_ // 2, :] = 0x80
    return payload


def _rt_state(C_, seed):
    rng = np.random.default_rng(seed)
    gate = (rng.integers(0, 4, C_) != 0).astype(np.uint8)
    hold0 = gu.new_hold(C_)
    hold0["peak_hold"][C_ - 1] = 31000
    hold0["count"][0] = 7
    hold0["level_min"][0] = 3
    return gate, hold0


def _run_rt(ctx, row, d_pl, codec, gate, hold0, C_, F_, lineage, stream=None):
    torch = gu.torch_cuda()
    n = row.n
    nb = F_ * C_ * n
    out_raw, out_at, d_out = _buf(nb, row.out_off)
    st_raw, st_at, d_st = _buf(F_ * C_ * 16, 0)
    d_hold = gu.to_dev(hold0)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    ctx.set_variant(row.variant)
    try:
        with _Env(row.knobs):
            ctx.roundtrip_peakhold(d_pl, gu.to_dev(codec), C_, F_, n, d_out, d_st, d_hold, gate=gu.to_dev(gate), variant=lineage, stream=s)
        torch.cuda.synchronize()
    finally:
        ctx.set_variant(0)
    assert _guards_intact(out_raw, out_at, nb) and _guards_intact(st_raw, st_at, F_ * C_ * 16), f"{row.id}: guard bytes written"
    return gu.to_host(d_out, np.uint8, (F_, C_, n)), gu.to_host(d_st, capi.FRAME_STATS, (F_, C_)), gu.to_host(d_hold, capi.CHAN_HOLD)


def _check_rt(row, got, exp):
    out, st, hold = got
    eout, est, ehold = exp
    assert np.array_equal(out, eout), f"{row.id}: codes differ at {np.argwhere(out != eout)[:3].tolist()}"
    gu.assert_stats_equal(st, est, n=row.n)
    for f in capi.CHAN_HOLD.names:
        assert np.array_equal(hold[f], ehold[f]), (row.id, f)


@pytest.mark.parametrize("lineage", [capi.ENC_SUN16, capi.ENC_G191], ids=["sun16", "g191"])
@pytest.mark.parametrize("row", km.RT_ROWS, ids=[r.id for r in km.RT_ROWS])
def test_small_roundtrip_row(ctx, orc, row, lineage):
    C_, F_, n = km.SMALL_C, km.SMALL_F, row.n
    payload = _rt_payload(orc, C_, F_, n, seed=n * 3 + lineage)
    payload.reshape(-1)[(2 * C_ + 5) * n:(2 * C_ + 5) * n + 256] = np.arange(256, dtype=np.uint8)
    codec = _codec(C_, salt=1)
    gate, hold0 = _rt_state(C_, n)
    _, _, d_pl = _buf(F_ * C_ * n, row.payload_off)
    d_pl.copy_(gu.torch_cuda().from_numpy(payload.reshape(-1)))
    got = _run_rt(ctx, row, d_pl, codec, gate, hold0, C_, F_, lineage)
    _check_rt(row, got, orc.roundtrip_peakhold(payload, codec, hold0.copy().view(orc.CHAN_HOLD), gate=gate, variant=lineage))


RT_FULL_NS = sorted({r.n for r in km.RT_ROWS if r.full})


@pytest.mark.parametrize("n", RT_FULL_NS)
def test_full_chip_roundtrip(ctx, orc, n):
    """Every fused round-trip form of frame size n (block form and register form) at 65 536 channels x 24 frames: codes,
    records and hold against the oracle.  One encoder lineage per size, alternating (both are covered by the small tests)."""
    torch = gu.torch_cuda()
    C_, F_ = km.FULL_C, km.RT_FULL_F
    lineage = capi.ENC_G191 if RT_FULL_NS.index(n) % 2 == 0 else capi.ENC_SUN16
    codec = _codec(C_, salt=2)
    gate, hold0 = _rt_state(C_, n + 1)
    seed = 11000 + n
    payload = orc.gen_uniform(F_ * C_ * n, seed=seed).reshape(F_, C_, n)
    exp = orc.roundtrip_peakhold(payload, codec, hold0.copy().view(orc.CHAN_HOLD), gate=gate, variant=lineage)
    del payload
    for row in [r for r in km.RT_ROWS if r.full and r.n == n]:
        _, _, d_pl = _buf(F_ * C_ * n, row.payload_off)
        ctx.gen_uniform(d_pl, F_ * C_ * n, seed=seed, stream=torch.cuda.current_stream().cuda_stream)
        got = _run_rt(ctx, row, d_pl, codec, gate, hold0, C_, F_, lineage)
        del d_pl
        _check_rt(row, got, exp)


# ----------------------------------------------------------------------------- d. different kernels back to back on one stream
# (kind, n, F): every launch has a grid of 256 blocks; the meter launches carry the aggregate
SEQUENCE = [("meter", 160, 16, None),           # k_meter_chunk64
            ("meter", 24, 64, None),            # k_meter_tiny<6>
            ("meter", 164, 16, None),           # k_meter_strided<10, true>
            ("meter", 240, 8, 0),               # k_meter_strided<15, false, STORE>
            ("encode", 160, 4, None),           # k_encode_lut16
            ("meter", 160, 8, 0),               # k_meter_chunk64<STORE>
            ("meter", 32, 64, None),            # k_meter_tiny<8>
            ("roundtrip", 164, 16, None)]       # k_roundtrip_strided<10, true, BLK>


@pytest.fixture(scope="module")
def sequence(orc):
    """Inputs on the device and expected outputs of SEQUENCE."""
    torch = gu.torch_cuda()
    C_ = km.FULL_C
    jobs = []
    for i, (kind, n, F_, pcm_off) in enumerate(SEQUENCE):
        seed = 20000 + i
        codec = _codec(C_, salt=i)
        nb = F_ * C_ * n
        j = {"kind": kind, "n": n, "F": F_, "pcm": pcm_off is not None, "codec": gu.to_dev(codec)}
        if kind == "encode":
            j["pl"] = torch.empty((nb * 2,), dtype=torch.uint8, device="cuda")
            pcm = orc.gen_uniform(nb * 2, seed=seed).view("<i2").reshape(F_, C_, n)
            j["e"] = orc.encode(pcm, codec, capi.ENC_G191)
            del pcm
        else:
            j["pl"] = torch.empty((nb,), dtype=torch.uint8, device="cuda")
            payload = orc.gen_uniform(nb, seed=seed).reshape(F_, C_, n)
            if kind == "meter":
                j["e"] = _oracle_meter(orc, payload, codec, None, pcm_off is not None)
            else:
                j["gate"], j["hold0"] = _rt_state(C_, seed)
                j["e"] = orc.roundtrip_peakhold(payload, codec, j["hold0"].copy().view(orc.CHAN_HOLD), gate=j["gate"], variant=capi.ENC_SUN16)
            del payload
        jobs.append((j, seed))
    return jobs


@pytest.mark.parametrize("global_queue", [1, 0], ids=["device_queue", "static_schedule"])
def test_different_kernels_back_to_back_on_one_stream(orc, sequence, global_queue):
    """chunk64 -> tiny -> strided -> strided + PCM -> encode (lut16) -> chunk64 + PCM -> tiny -> round trip (strided, block form),
    enqueued on one stream without a host sync, then every output against the oracle.  The persistent kernels share the stream's
    work-counter pair; IGDSP_GLOBAL_QUEUE=0 (read by igdsp_create) runs the static schedule instead."""
    torch = gu.torch_cuda()
    with _Env((("IGDSP_GLOBAL_QUEUE", str(global_queue)),)):
        ctx = capi.Context(device=0, max_channels=4096)
    try:
        C_ = km.FULL_C
        outs = []
        for j, seed in sequence:
            n, F_ = j["n"], j["F"]
            ctx.gen_uniform(j["pl"], j["pl"].numel(), seed=seed, stream=torch.cuda.current_stream().cuda_stream)
            o = {"st": gu.dev_zeros(F_ * C_ * 16, 0xEE)}
            if j["kind"] == "meter":
                o["agg"] = gu.dev_zeros(capi.AGGREGATE.itemsize)
                o["pcm"] = gu.dev_zeros(F_ * C_ * n * 2, 0xEE) if j["pcm"] else None
            elif j["kind"] == "encode":
                o["out"] = gu.dev_zeros(F_ * C_ * n, 0xEE)
            else:
                o["out"] = gu.dev_zeros(F_ * C_ * n, 0xEE)
                o["hold"], o["gate"] = gu.to_dev(j["hold0"]), gu.to_dev(j["gate"])
            outs.append(o)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        hs = stream.cuda_stream
        for (j, _), o in zip(sequence, outs):
            n, F_ = j["n"], j["F"]
            if j["kind"] == "meter":
                ctx.agg_reset(o["agg"], stream=hs)
                ctx.decode_meter(j["pl"], j["codec"], C_, F_, n, o["st"], pcm=o["pcm"], agg=o["agg"], rank=RANK, stream=hs)
            elif j["kind"] == "encode":
                ctx.encode(j["pl"], j["codec"], C_, F_, n, o["out"], variant=capi.ENC_G191, stream=hs)
            else:
                ctx.roundtrip_peakhold(j["pl"], j["codec"], C_, F_, n, o["out"], o["st"], o["hold"], gate=o["gate"],
                                       variant=capi.ENC_SUN16, stream=hs)
        stream.synchronize()
        for (j, _), o in zip(sequence, outs):
            n, F_ = j["n"], j["F"]
            what = (j["kind"], n, F_, global_queue)
            if j["kind"] == "meter":
                est, epcm, eagg = j["e"]
                gu.assert_stats_equal(gu.to_host(o["st"], capi.FRAME_STATS, (F_, C_)), est, n=n)
                if epcm is not None:
                    assert np.array_equal(gu.to_host(o["pcm"], "<i2", (F_, C_, n)), epcm), what
                agg = gu.to_host(o["agg"], capi.AGGREGATE)[0]
                for f in AGG_FIELDS:
                    assert int(agg[f]) == int(eagg[f]), (what, f)
                assert agg["peak_slot"].tolist() == eagg["peak_slot"].tolist(), what
            elif j["kind"] == "encode":
                assert np.array_equal(gu.to_host(o["out"], np.uint8, (F_, C_, n)), j["e"]), what
            else:
                eout, est, ehold = j["e"]
                assert np.array_equal(gu.to_host(o["out"], np.uint8, (F_, C_, n)), eout), what
                gu.assert_stats_equal(gu.to_host(o["st"], capi.FRAME_STATS, (F_, C_)), est, n=n)
                assert gu.to_host(o["hold"], capi.CHAN_HOLD).tobytes() == np.ascontiguousarray(ehold).tobytes(), what
        del outs
        assert ctx.L.igdsp_last_error(ctx.h) in (b"", None)
    finally:
        ctx.close()
