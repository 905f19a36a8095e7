// igdsp_capi_dbuf.hip — the delay buffer entries of include/igdsp.h: igdsp_dbuf_run and its compute-free yardstick
// igdsp_internal_dbuf_move, and the host-only igdsp_dbuf_step, which runs the constexpr rule of igdsp_dbuf.h that k_dbuf runs.
// igdsp_dbuf_run reads as every batched entry does (igdsp_capi.hip): null ctx, the argument rule of igdsp_args.h, hipSetDevice, the
// stream and its launch configuration, the launch.
#include "igdsp_args.h"
#include "igdsp_ctx.h"
#include "igdsp_dbuf.h"

using namespace igdsp;

static int dbuf_entry(igdsp_ctx *ctx, const uint8_t *d_ops, const int16_t *d_in, uint32_t C, uint32_t T, uint32_t n, uint32_t M, igdsp_dbuf_state *d_state,
                      int16_t *d_out, uint8_t *d_flags_out, uint16_t *d_len_out, uint16_t *d_fill, igdsp_frame_stats *d_stats, void *stream,
                      bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_dbuf_run", args::dbuf_run(d_ops, d_in, C, T, n, M, d_state, d_out, d_flags_out, d_len_out, d_fill, d_stats));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_dbuf_run(cfg_of(ctx, s), d_ops, d_in, C, T, n, M, d_state, d_out, d_flags_out, d_len_out, d_fill, d_stats, yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- the delay buffer of pjmedia's splitcomb reverse channels (initSlaveSoundCard, roip_ed137.cpp:3314-3435) ----
int igdsp_dbuf_run(igdsp_ctx *ctx, const uint8_t *d_ops, const int16_t *d_in, uint32_t n_channels, uint32_t n_steps, uint32_t samples_per_frame,
                   uint32_t max_samples, igdsp_dbuf_state *d_state, int16_t *d_out, uint8_t *d_flags_out, uint16_t *d_len_out, uint16_t *d_fill,
                   igdsp_frame_stats *d_stats, void *stream)
{
    return dbuf_entry(ctx, d_ops, d_in, n_channels, n_steps, samples_per_frame, max_samples, d_state, d_out, d_flags_out, d_len_out, d_fill, d_stats,
                      stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick (tools/dbuf_bench.py) — every step taken as PUT|GET at a fixed
// fill of n: the same rows through the ring, the same stores, no update, search, blend or record arithmetic.  Arguments as
// igdsp_dbuf_run; d_ops is not read.
int igdsp_internal_dbuf_move(igdsp_ctx *ctx, const uint8_t *d_ops, const int16_t *d_in, uint32_t n_channels, uint32_t n_steps,
                             uint32_t samples_per_frame, uint32_t max_samples, igdsp_dbuf_state *d_state, int16_t *d_out, uint8_t *d_flags_out,
                             uint16_t *d_len_out, uint16_t *d_fill, igdsp_frame_stats *d_stats, void *stream)
{
    return dbuf_entry(ctx, d_ops, d_in, n_channels, n_steps, samples_per_frame, max_samples, d_state, d_out, d_flags_out, d_len_out, d_fill, d_stats,
                      stream, true);
}

// Host only: one step of one channel, the state advanced
int igdsp_dbuf_step(igdsp_dbuf_state *st, uint32_t op, const int16_t *in, uint32_t samples_per_frame, uint32_t max_samples, int16_t *out,
                    uint32_t *flag)
{
    if (!st || op > (uint32_t)(IGDSP_DBUF_PUT | IGDSP_DBUF_GET) || !dbuf_shape_ok(samples_per_frame, max_samples)) return IGDSP_EINVAL;
    if (((op & IGDSP_DBUF_PUT) && !in) || ((op & IGDSP_DBUF_GET) && !out)) return IGDSP_EINVAL;
    const uint32_t f = dbuf_step_run(*st, op, in, samples_per_frame, max_samples, out);
    if (flag) *flag = f;
    return IGDSP_OK;
}

}  // extern "C"
