// igdsp_capi_spec.hip — the spectrum entries of include/igdsp.h: igdsp_spectrum and its compute-free yardstick
// igdsp_internal_spec_move, and the host-only igdsp_spec_frame / igdsp_spec_tables, which run the rule of igdsp_spec.h that k_spec runs.
// igdsp_spectrum reads as every batched entry does (igdsp_capi.hip): null ctx, the argument rule of igdsp_args.h, hipSetDevice, the
// stream and its launch configuration, the launch.
#include "igdsp_args.h"
#include "igdsp_ctx.h"
#include "igdsp_spec.h"

using namespace igdsp;

static int spec_entry(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, uint32_t C, uint32_t F, uint32_t n,
                      const igdsp_spec_cfg *cfg, igdsp_spec_state *d_state, igdsp_spec_rec *d_rec, float *d_avg, float *d_raw, void *stream,
                      bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_spectrum", args::spec_run(d_g711, d_codec, d_pcm, C, F, n, cfg, d_state, d_rec, d_avg, d_raw));
    const igdsp_spec_cfg k = spec_cfg_or_default(cfg);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_spectrum(cfg_of(ctx, s), d_g711, d_codec, d_pcm, C, F, n, k.hop_frames, k.alpha, d_state, d_rec, d_avg, d_raw, yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- the spectrum graph the reference declares and never computes (initSpectrumGraph, roip_ed137.cpp:6350-6365) ----
int igdsp_spectrum(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, uint32_t n_channels, uint32_t n_frames,
                   uint32_t samples_per_frame, const igdsp_spec_cfg *cfg, igdsp_spec_state *d_state, igdsp_spec_rec *d_rec, float *d_avg,
                   float *d_raw, void *stream)
{
    return spec_entry(ctx, d_g711, d_codec, d_pcm, n_channels, n_frames, samples_per_frame, cfg, d_state, d_rec, d_avg, d_raw, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick (tools/spec_bench.py) — the same rows into the history, the same
// ring loads, tile exchanges and global stores at every hop, no window, butterfly, twiddle, split, log or average.  Arguments as
// igdsp_spectrum.  It stores the bytes igdsp_spectrum stores; the state's history, since and hops come out as by igdsp_spectrum, its
// averaged array as it was read (-70 dBFS from a reset state); a hop's record carries IGDSP_SPEC_HOP, bin 0 and 0.0; d_avg is the
// averaged array as read; d_raw's values are not specified.
int igdsp_internal_spec_move(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, uint32_t n_channels,
                             uint32_t n_frames, uint32_t samples_per_frame, const igdsp_spec_cfg *cfg, igdsp_spec_state *d_state,
                             igdsp_spec_rec *d_rec, float *d_avg, float *d_raw, void *stream)
{
    return spec_entry(ctx, d_g711, d_codec, d_pcm, n_channels, n_frames, samples_per_frame, cfg, d_state, d_rec, d_avg, d_raw, stream, true);
}

// Host only: one frame of one channel, the state advanced
int igdsp_spec_frame(igdsp_spec_state *st, const int16_t *row, uint32_t samples_per_frame, const igdsp_spec_cfg *cfg, igdsp_spec_rec *rec,
                     float *raw)
{
    if (!st || !row || !spec_n_ok(samples_per_frame) || !args::spec_cfg_ok(cfg)) return IGDSP_EINVAL;
    spec_frame_run(*st, row, samples_per_frame, spec_cfg_or_default(cfg), rec, raw);
    return IGDSP_OK;
}

// Host only: the committed tables
int igdsp_spec_tables(const float **window, const float **twiddle)
{
    if (window) *window = kSpecWin;
    if (twiddle) *twiddle = kSpecTw;
    return IGDSP_OK;
}

}  // extern "C"
