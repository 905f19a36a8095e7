// igdsp_capi_ec.hip — the echo canceller's entries of include/igdsp.h: igdsp_echo_cancel and its compute-free yardstick
// igdsp_internal_ec_move, and the host-only igdsp_ec_cfg_default / igdsp_ec_frame, which run the rule of igdsp_ec.h that k_ec runs.
// igdsp_echo_cancel reads as every batched entry does (igdsp_capi.hip): null ctx, the argument rule of igdsp_args.h, hipSetDevice, the
// stream and its launch configuration, the launch.
#include "igdsp_args.h"
#include "igdsp_ctx.h"
#include "igdsp_ec.h"

using namespace igdsp;

static int ec_entry(igdsp_ctx *ctx, const uint8_t *d_near_g711, const uint8_t *d_codec, const int16_t *d_near_pcm, const int16_t *d_far_pcm,
                    uint32_t n_far_rows, const uint32_t *d_far_of, const uint8_t *d_ctl, const igdsp_ec_cfg *cfg, uint32_t C, uint32_t F, uint32_t n,
                    igdsp_ec_state *d_state, int16_t *d_out, igdsp_ec_rec *d_rec, igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_echo_cancel",
             args::ec_run(d_near_g711, d_codec, d_near_pcm, d_far_pcm, n_far_rows, d_far_of, d_ctl, cfg, C, F, n, d_state, d_out, d_rec, d_stats));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_echo_cancel(cfg_of(ctx, s), d_near_g711, d_codec, d_near_pcm, d_far_pcm, n_far_rows, d_far_of, d_ctl, ec_cfg_or_default(cfg), C, F, n,
                                    d_state, d_out, d_rec, d_stats, yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- the echo canceller pjmedia hangs on the sound port and the reference switches off (ec_tail_len = 0) ----
int igdsp_echo_cancel(igdsp_ctx *ctx, const uint8_t *d_near_g711, const uint8_t *d_codec, const int16_t *d_near_pcm, const int16_t *d_far_pcm,
                      uint32_t n_far_rows, const uint32_t *d_far_of, const uint8_t *d_ctl, const igdsp_ec_cfg *cfg, uint32_t n_channels,
                      uint32_t n_frames, uint32_t samples_per_frame, igdsp_ec_state *d_state, int16_t *d_out, igdsp_ec_rec *d_rec,
                      igdsp_frame_stats *d_stats, void *stream)
{
    return ec_entry(ctx, d_near_g711, d_codec, d_near_pcm, d_far_pcm, n_far_rows, d_far_of, d_ctl, cfg, n_channels, n_frames, samples_per_frame, d_state,
                    d_out, d_rec, d_stats, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick (tools/ec_bench.py) — the same row loads, buffer stores, history
// moves, records, row and state stores, no window read, dot product, reduction or update.  Arguments as igdsp_echo_cancel; d_ctl is not
// read.  It stores the bytes igdsp_echo_cancel stores with every channel at IGDSP_EC_BYPASS: the output is the near row, the weights and
// hang are the entry's (a state of another tag: the RESET state), the history is the entry's.
int igdsp_internal_ec_move(igdsp_ctx *ctx, const uint8_t *d_near_g711, const uint8_t *d_codec, const int16_t *d_near_pcm, const int16_t *d_far_pcm,
                           uint32_t n_far_rows, const uint32_t *d_far_of, const uint8_t *d_ctl, const igdsp_ec_cfg *cfg, uint32_t n_channels,
                           uint32_t n_frames, uint32_t samples_per_frame, igdsp_ec_state *d_state, int16_t *d_out, igdsp_ec_rec *d_rec,
                           igdsp_frame_stats *d_stats, void *stream)
{
    return ec_entry(ctx, d_near_g711, d_codec, d_near_pcm, d_far_pcm, n_far_rows, d_far_of, d_ctl, cfg, n_channels, n_frames, samples_per_frame, d_state,
                    d_out, d_rec, d_stats, stream, true);
}

// ---- host only
void igdsp_ec_cfg_default(uint32_t tail, igdsp_ec_cfg *out)
{
    if (out) *out = ec_cfg_default(tail);
}

int igdsp_ec_frame(const igdsp_ec_cfg *cfg, igdsp_ec_state *st, const int16_t *near_pcm, const int16_t *far_pcm, uint32_t samples_per_frame,
                   uint32_t ctl, int16_t *out, igdsp_ec_rec *rec)
{
    if (!st || !near_pcm || !ec_n_ok(samples_per_frame) || !ec_cfg_ok(cfg)) return IGDSP_EINVAL;
    ec_frame_run(ec_cfg_or_default(cfg), *st, near_pcm, far_pcm, samples_per_frame, ctl, out, rec);
    return IGDSP_OK;
}

}  // extern "C"
