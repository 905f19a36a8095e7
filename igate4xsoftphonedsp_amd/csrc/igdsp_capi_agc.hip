// igdsp_capi_agc.hip — the level control's entries of include/igdsp.h: igdsp_agc_run and its compute-free yardstick
// igdsp_internal_agc_move, and the host-only igdsp_agc_cfg_default / igdsp_agc_frame, which run the rule of igdsp_agc.h that k_agc runs.
// igdsp_agc_run reads as every batched entry does (igdsp_capi.hip): null ctx, the argument rule of igdsp_args.h, hipSetDevice, the
// stream and its launch configuration, the launch.
#include "igdsp_args.h"
#include "igdsp_ctx.h"
#include "igdsp_agc.h"

using namespace igdsp;

static int agc_entry(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const uint8_t *d_ctl, const igdsp_agc_cfg *cfg,
                     uint32_t C, uint32_t F, uint32_t n, igdsp_agc_state *d_state, int16_t *d_out, igdsp_agc_rec *d_rec, igdsp_frame_stats *d_stats,
                     void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_agc_run", args::agc_run(d_g711, d_codec, d_pcm, d_ctl, cfg, C, F, n, d_state, d_out, d_rec, d_stats));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_agc(cfg_of(ctx, s), d_g711, d_codec, d_pcm, d_ctl, agc_cfg_or_default(cfg), C, F, n, d_state, d_out, d_rec, d_stats, yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- the level control: a slow gain toward a target level and a peak limiter, per channel ----
int igdsp_agc_run(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const uint8_t *d_ctl, const igdsp_agc_cfg *cfg,
                  uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, igdsp_agc_state *d_state, int16_t *d_out, igdsp_agc_rec *d_rec,
                  igdsp_frame_stats *d_stats, void *stream)
{
    return agc_entry(ctx, d_g711, d_codec, d_pcm, d_ctl, cfg, n_channels, n_frames, samples_per_frame, d_state, d_out, d_rec, d_stats, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick (tools/agc_bench.py) — the same row loads and decode, state load
// and store, row, record and PCM-record stores with their reductions; no block peak, division, recurrence or gain.  Arguments as
// igdsp_agc_run; d_ctl is not read.  Rows, records and PCM records are the bytes igdsp_agc_run stores with every channel at
// IGDSP_AGC_BYPASS; the state, which a bypass leaves alone, is written as it was read (gain clamped; another tag: the RESET state) with
// the tag, flags IGDSP_AGC_BYPASSED and reserved 0.
int igdsp_internal_agc_move(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const uint8_t *d_ctl,
                            const igdsp_agc_cfg *cfg, uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, igdsp_agc_state *d_state,
                            int16_t *d_out, igdsp_agc_rec *d_rec, igdsp_frame_stats *d_stats, void *stream)
{
    return agc_entry(ctx, d_g711, d_codec, d_pcm, d_ctl, cfg, n_channels, n_frames, samples_per_frame, d_state, d_out, d_rec, d_stats, stream, true);
}

// ---- host only
void igdsp_agc_cfg_default(igdsp_agc_cfg *out)
{
    if (out) *out = agc_cfg_default();
}

int igdsp_agc_frame(const igdsp_agc_cfg *cfg, igdsp_agc_state *st, const int16_t *pcm, uint32_t samples_per_frame, uint32_t ctl, int16_t *out,
                    igdsp_agc_rec *rec)
{
    if (!st || !pcm || !agc_n_ok(samples_per_frame) || !agc_cfg_ok(cfg)) return IGDSP_EINVAL;
    agc_frame_run(agc_cfg_or_default(cfg), *st, pcm, samples_per_frame, ctl, out, rec);
    return IGDSP_OK;
}

}  // extern "C"
