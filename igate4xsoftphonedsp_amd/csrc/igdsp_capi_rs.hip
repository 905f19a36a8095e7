// igdsp_capi_rs.hip — the rate converter entries of include/igdsp.h: igdsp_resample and its compute-free yardstick
// igdsp_internal_rs_copy, and the host-only igdsp_rs_frame / igdsp_rs_taps, which run the constexpr rules of igdsp_route.h that k_rs
// runs.  igdsp_resample reads as every batched entry does (igdsp_capi.hip): null ctx, the argument rule of igdsp_args.h, hipSetDevice,
// the stream and its launch configuration, the launch.
#include "igdsp_args.h"
#include "igdsp_ctx.h"

using namespace igdsp;

static int rs_entry(igdsp_ctx *ctx, uint32_t dir, uint32_t factor, uint32_t layout, const uint8_t *d_payload, const uint8_t *d_codec,
                    const int16_t *d_pcm, const uint16_t *d_len, igdsp_rs_state *d_state, uint32_t C, uint32_t F, uint32_t n, uint32_t rows_narrow,
                    uint32_t rows_wide, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_resample", args::resample(dir, factor, layout, d_payload, d_codec, d_pcm, d_len, d_state, C, F, n, rows_narrow, rows_wide,
                                                   d_out, d_stats));
    if (yardstick && !d_out) return IGDSP_EINVAL;                                 // the yardstick writes the rows
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_rs(cfg_of(ctx, s), dir, factor, layout, d_payload, d_codec, d_pcm, d_len, d_state, C, F, n, rows_narrow, rows_wide, d_out,
                           d_stats, yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- the port resampling of pjmedia's bridge when media_cfg.clock_rate is not 8 000 (roip_ed137.cpp:3031-3032) ----
int igdsp_resample(igdsp_ctx *ctx, uint32_t direction, uint32_t factor, uint32_t layout, const uint8_t *d_payload, const uint8_t *d_codec,
                   const int16_t *d_pcm, const uint16_t *d_len, igdsp_rs_state *d_state, uint32_t n_channels, uint32_t n_frames,
                   uint32_t samples_per_frame, uint32_t rows_narrow, uint32_t rows_wide, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return rs_entry(ctx, direction, factor, layout, d_payload, d_codec, d_pcm, d_len, d_state, n_channels, n_frames, samples_per_frame, rows_narrow,
                    rows_wide, d_out, d_stats, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick (tools/rs_bench.py) — the same items in the same order, the
// same loads, tile traffic and stores, an xor in place of the filter, zero records.  Arguments as igdsp_resample; d_out is required,
// the state is neither read nor written.
int igdsp_internal_rs_copy(igdsp_ctx *ctx, uint32_t direction, uint32_t factor, uint32_t layout, const uint8_t *d_payload, const uint8_t *d_codec,
                           const int16_t *d_pcm, const uint16_t *d_len, igdsp_rs_state *d_state, uint32_t n_channels, uint32_t n_frames,
                           uint32_t samples_per_frame, uint32_t rows_narrow, uint32_t rows_wide, int16_t *d_out, igdsp_frame_stats *d_stats,
                           void *stream)
{
    return rs_entry(ctx, direction, factor, layout, d_payload, d_codec, d_pcm, d_len, d_state, n_channels, n_frames, samples_per_frame, rows_narrow,
                    rows_wide, d_out, d_stats, stream, true);
}

// Host only: one frame of one channel, the state advanced
int igdsp_rs_frame(igdsp_rs_state *st, uint32_t direction, uint32_t factor, const int16_t *in, uint32_t n_in, int16_t *out)
{
    if (!st || !in || !out || !rs_dir_ok(direction) || !rs_factor_ok(factor) || n_in == 0) return IGDSP_EINVAL;
    if (direction == IGDSP_RS_UP ? n_in > IGDSP_MAX_PAYLOAD : (n_in % factor != 0 || n_in / factor > IGDSP_MAX_PAYLOAD)) return IGDSP_EINVAL;
    rs_frame_run(*st, direction, factor, in, n_in, out);
    return IGDSP_OK;
}

// Host only: the table of a direction and factor
int igdsp_rs_taps(uint32_t direction, uint32_t factor, const int16_t **taps, uint32_t *count)
{
    const int16_t *tab = rs_table(direction, factor);
    if (!taps || !count || !tab) return IGDSP_EINVAL;
    *taps = tab;
    *count = kRsTaps * factor;
    return IGDSP_OK;
}

}  // extern "C"
