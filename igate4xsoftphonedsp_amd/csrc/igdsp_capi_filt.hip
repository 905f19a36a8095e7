// igdsp_capi_filt.hip — the filter's entries of include/igdsp.h: igdsp_filt_run and its compute-free yardstick igdsp_internal_filt_move,
// and the host-only igdsp_filt_frame / _plan_check / _design / _plan_preset, which run the rule and the designs of igdsp_filt.h that
// k_filt runs.  igdsp_filt_run reads as every batched entry does (igdsp_capi.hip): null ctx, the argument rule of igdsp_args.h,
// hipSetDevice, the stream and its launch configuration, the launch.
#include "igdsp_args.h"
#include "igdsp_ctx.h"
#include "igdsp_filt.h"

using namespace igdsp;

static int filt_entry(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const uint8_t *d_ctl, const igdsp_filt_plan *d_plans,
                      uint32_t n_plans, const uint16_t *d_plan_of, uint32_t max_sections, uint32_t C, uint32_t F, uint32_t n, igdsp_filt_state *d_state,
                      int16_t *d_out, igdsp_filt_rec *d_rec, igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_filt_run", args::filt_run(d_g711, d_codec, d_pcm, d_ctl, d_plans, n_plans, d_plan_of, max_sections, C, F, n, d_state, d_out, d_rec, d_stats));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_filt(cfg_of(ctx, s), d_g711, d_codec, d_pcm, d_ctl, d_plans, n_plans, d_plan_of, max_sections, C, F, n, d_state, d_out, d_rec, d_stats,
                             yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- a chain of second-order sections per channel, for a batch ----
int igdsp_filt_run(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const uint8_t *d_ctl, const igdsp_filt_plan *d_plans,
                   uint32_t n_plans, const uint16_t *d_plan_of, uint32_t max_sections, uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame,
                   igdsp_filt_state *d_state, int16_t *d_out, igdsp_filt_rec *d_rec, igdsp_frame_stats *d_stats, void *stream)
{
    return filt_entry(ctx, d_g711, d_codec, d_pcm, d_ctl, d_plans, n_plans, d_plan_of, max_sections, n_channels, n_frames, samples_per_frame, d_state, d_out,
                      d_rec, d_stats, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick (tools/filt_bench.py) — the same row loads and decode, tile
// stores, the lane's read and write of its row with the peak fold, tile reads, state load and store, row, record and stats stores; no
// section runs.  Arguments as igdsp_filt_run; d_ctl is not read, of a plan only its first dword.  It stores the bytes igdsp_filt_run
// stores with every channel at IGDSP_FILT_BYPASS, except that the state, which a bypass leaves alone, is written back as it was read (e
// masked; another tag: zero histories), with the tag, flags as read and reserved 0.
int igdsp_internal_filt_move(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const uint8_t *d_ctl,
                             const igdsp_filt_plan *d_plans, uint32_t n_plans, const uint16_t *d_plan_of, uint32_t max_sections, uint32_t n_channels,
                             uint32_t n_frames, uint32_t samples_per_frame, igdsp_filt_state *d_state, int16_t *d_out, igdsp_filt_rec *d_rec,
                             igdsp_frame_stats *d_stats, void *stream)
{
    return filt_entry(ctx, d_g711, d_codec, d_pcm, d_ctl, d_plans, n_plans, d_plan_of, max_sections, n_channels, n_frames, samples_per_frame, d_state, d_out,
                      d_rec, d_stats, stream, true);
}

// ---- host only
int igdsp_filt_frame(const igdsp_filt_plan *plan, igdsp_filt_state *st, const int16_t *pcm, uint32_t samples_per_frame, uint32_t ctl, int16_t *out,
                     igdsp_filt_rec *rec)
{
    if (!st || !pcm || !filt_n_ok(samples_per_frame)) return IGDSP_EINVAL;
    filt_frame_run(plan, *st, pcm, samples_per_frame, ctl, out, rec);
    return IGDSP_OK;
}

int igdsp_filt_plan_check(const igdsp_filt_plan *plan) { return plan && filt_plan_ok(*plan) ? IGDSP_OK : IGDSP_EINVAL; }

int igdsp_filt_design(uint32_t kind, uint32_t clock_rate, double f0_hz, double q, double gain_db, int16_t *out)
{
    int16_t c[5];
    if (!out || !filt_design(kind, clock_rate, f0_hz, q, gain_db, c)) return IGDSP_EINVAL;
    for (int i = 0; i < 5; ++i) out[i] = c[i];
    return IGDSP_OK;
}

int igdsp_filt_plan_preset(uint32_t preset, uint32_t clock_rate, igdsp_filt_plan *plan)
{
    igdsp_filt_plan p;
    if (!plan || !filt_preset(preset, clock_rate, p)) return IGDSP_EINVAL;
    *plan = p;
    return IGDSP_OK;
}

}  // extern "C"
