// igdsp_capi_bench.hip — calibration, measurement and diagnostic entries: bare traffic kernels the tools compare the real ones
// against, the DIAG instantiation of the headline kernel, the table-driven compressor on its own and native staging loops.  Apart from
// igdsp_probe_placement they are not in include/igdsp.h.  Their argument rules are a null and an alignment check, kept inline.
#include "igdsp_args.h"
#include "igdsp_ctx.h"

using namespace igdsp;
using igdsp::args::misaligned;

extern "C" {

int igdsp_probe_placement(igdsp_ctx *ctx, const void *d_in, size_t bytes, void *d_out, uint32_t reps, float *ms_per_launch, void *stream)
{
    if (!ctx || !d_in || !ms_per_launch || reps == 0 || bytes < 10240u || misaligned(16, {d_in, d_out})) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    void *scratch = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    if (!d_out) {
        if (hipMalloc(&scratch, bytes / 10u + 4096u) != hipSuccess) return fail(ctx, IGDSP_ENOMEM, "probe scratch");
        d_out = scratch;
    }
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = launch_stream_rw(cfg_of(ctx, s), d_in, bytes, d_out, s);
    if (e == hipSuccess) e = hipEventRecord(a, s);
    for (uint32_t i = 0; i < reps && e == hipSuccess; ++i) e = launch_stream_rw(cfg_of(ctx, s), d_in, bytes, d_out, s);
    if (e == hipSuccess) e = hipEventRecord(b, s);
    if (e == hipSuccess) e = hipEventSynchronize(b);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    if (scratch) (void)hipFree(scratch);
    if (e != hipSuccess) return fail(ctx, IGDSP_EDEVICE, "igdsp_probe_placement", e);
    *ms_per_launch = ms / (float)reps;
    return IGDSP_OK;
}

// Measurement / test helper (not in include/igdsp.h): what `n_calls` media threads do between two ticks, in one native loop —
// `frames_per_call` calls of igdsp_on_rtp_frame for each of the calls first_call .. first_call + n_calls - 1, frame f of call k
// taken from payloads[(f * n_calls + k) % n_payloads][payloadlen].  Returns the number of calls that did not return IGDSP_OK.
int igdsp_internal_stage_many(igdsp_ctx *ctx, int32_t first_call, uint32_t n_calls, uint32_t frames_per_call, uint8_t pt,
                              const uint8_t *payloads, uint32_t n_payloads, uint32_t payloadlen)
{
    if (!ctx || !payloads || n_payloads == 0) return IGDSP_EINVAL;
    int bad = 0;
    for (uint32_t f = 0; f < frames_per_call; ++f)
        for (uint32_t k = 0; k < n_calls; ++k)
            if (igdsp_on_rtp_frame(ctx, first_call + (int32_t)k, pt, payloads + (size_t)((f * n_calls + k) % n_payloads) * payloadlen, payloadlen) != IGDSP_OK) ++bad;
    return bad;
}

// Test-only (not in include/igdsp.h): the table-driven compressor the fused round-trip kernel uses, on arbitrary PCM.
int igdsp_internal_encode_table(igdsp_ctx *ctx, const int16_t *d_pcm, const uint8_t *d_codec, uint32_t C, uint32_t F, uint32_t n,
                                uint8_t *d_out, int variant, void *stream)
{
    if (!ctx || !d_pcm || !d_codec || !d_out || (variant != IGDSP_ENC_SUN16 && variant != IGDSP_ENC_G191)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_encode_table(cfg_of(ctx, pick(ctx, stream)), d_pcm, d_codec, C, F, n, d_out, variant, pick(ctx, stream)));
    return IGDSP_OK;
}

// Calibration-only (not in include/igdsp.h): bare load/store kernel with the meter kernel's exact traffic
// (10 KiB read + 1 KiB record store per super-chunk); d_dst needs bytes / 10 bytes.
int igdsp_internal_stream_rw(igdsp_ctx *ctx, const void *d_src, size_t bytes, void *d_dst, void *stream)
{
    if (!ctx || !d_src || !d_dst || misaligned(16, {d_src, d_dst})) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_rw(cfg_of(ctx, pick(ctx, stream)), d_src, bytes, d_dst, pick(ctx, stream)));
    return IGDSP_OK;
}

// Calibration-only (not in include/igdsp.h): the meter's 10 : 1 traffic with the record stores of k consecutive super-chunks clustered
int igdsp_internal_stream_cluster(igdsp_ctx *ctx, const void *d_src, size_t bytes, void *d_dst, int k, void *stream)
{
    if (!ctx || !d_src || !d_dst || misaligned(16, {d_src, d_dst})) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_cluster(cfg_of(ctx, pick(ctx, stream)), d_src, bytes, d_dst, k, pick(ctx, stream)));
    return IGDSP_OK;
}

// Calibration-only (not in include/igdsp.h): the dword-aligned piece pattern of the packed packet / strided kernels, no per-sample work
// (launch_stream_pieces).  src needs n_items * 64 * stride + 16 bytes, dst n_items KiB, dst2 (optional) n_items * 512 bytes.
int igdsp_internal_stream_pieces(igdsp_ctx *ctx, const void *d_src, uint32_t n_items, uint32_t stride, uint32_t hdr, int mode, int rows, void *d_dst, void *d_dst2, void *stream)
{
    if (!ctx || !d_src || !d_dst || (stride & 3u) || stride < 16u * (uint32_t)(rows - (mode == 0 ? 2 : 1))) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_pieces(cfg_of(ctx, pick(ctx, stream)), d_src, n_items, stride, hdr, mode, rows, d_dst, d_dst2, pick(ctx, stream)));
    return IGDSP_OK;
}

// Calibration-only (not in include/igdsp.h): the packed-packet piece stream in the channel-group-major order of the fused window kernel
int igdsp_internal_stream_walk(igdsp_ctx *ctx, const void *d_src, uint32_t n_items, uint32_t stride, uint32_t hdr, uint32_t groups, uint32_t n_seg,
                               uint32_t trickle, void *d_dst, void *d_dst2, void *stream)
{
    if (!ctx || !d_src || !d_dst || (stride & 3u) || n_seg == 0 || (groups && n_items % groups)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_walk(cfg_of(ctx, pick(ctx, stream)), d_src, n_items, stride, hdr, groups, n_seg, trickle, d_dst, d_dst2, pick(ctx, stream)));
    return IGDSP_OK;
}

// Calibration-only (not in include/igdsp.h): bare read : write mix, r and w 1 KiB pieces per wave item
// (pairs built: 0:8, 8:8, 8:4, 4:8, 10:1, 10:0, 8:1, 8:2, 20:2, 5:1; `waves` per block 1..16); src needs n_items * r KiB, dst n_items * w KiB.
int igdsp_internal_stream_mix(igdsp_ctx *ctx, const void *d_src, void *d_dst, uint32_t n_items, int r, int w, int waves, void *stream)
{
    // the source may be only dword aligned: that is what the calibration of misaligned 16-byte loads needs
    if (!ctx || !d_src || !d_dst || misaligned(4, {d_src}) || misaligned(16, {d_dst})) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_mix(cfg_of(ctx, pick(ctx, stream)), d_src, d_dst, n_items, r, w, waves, pick(ctx, stream)));
    return IGDSP_OK;
}

// same, odd items write into a second window (d_dst2 addressed like d_dst) and, if d_src2 is given, read from a second one
int igdsp_internal_stream_mix2(igdsp_ctx *ctx, const void *d_src, void *d_dst, void *d_dst2, uint32_t n_items, int r, int w, int waves, void *stream,
                               const void *d_src2)
{
    if (!ctx || !d_src || !d_dst || !d_dst2 || misaligned(16, {d_src, d_src2, d_dst, d_dst2})) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_mix(cfg_of(ctx, pick(ctx, stream)), d_src, d_dst, n_items, r, w, waves, pick(ctx, stream), d_dst2, d_src2));
    return IGDSP_OK;
}

// Diagnostic-only (not in include/igdsp.h): stamps of the headline kernel's DIAG instantiation, kDiagWords = 16 x u64 per wavefront
// (d_diag holds 16 x 8 bytes per wave of the grid): {t_begin, t_lut_ready, t_end, sum setup, sum half X, iterations, sum half Y, xcc id,
// realtime begin, realtime end, sum frame-reduce, wave, t_prologue_loads_issued, realtime of the last batch draw, realtime of the
// first draw past the end of the work, block}.
int igdsp_internal_diag_chunk32(igdsp_ctx *ctx, const uint8_t *d_payload, const uint8_t *d_codec, uint32_t C, uint32_t F,
                                igdsp_frame_stats *d_stats, uint64_t *d_diag, void *stream)
{
    if (!ctx || !d_payload || !d_codec || !d_stats || !d_diag || C < 32) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_diag_chunk32(cfg_of(ctx, pick(ctx, stream)), d_payload, d_codec, C, F, d_stats, d_diag, pick(ctx, stream)));
    return IGDSP_OK;
}

}  // extern "C"
