// igdsp_capi_tdet.hip — the tone detector's entries of include/igdsp.h: igdsp_tone_detect and its compute-free yardstick
// igdsp_internal_tdet_move, and the host-only igdsp_tdet_plan_build / _plan_dtmf / _digit / _table / _frame / _work_bytes, which run
// the rule of igdsp_tdet.h that k_tdet runs.  igdsp_tone_detect reads as every batched entry does (igdsp_capi.hip): null ctx, the
// argument rule of igdsp_args.h, hipSetDevice, the stream and its launch configuration, the launch.
#include "igdsp_args.h"
#include "igdsp_ctx.h"
#include "igdsp_tdet.h"

using namespace igdsp;

static int tdet_entry(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const igdsp_tdet_plan *d_plans,
                      uint32_t n_plans, const uint16_t *d_plan_of, uint32_t C, uint32_t F, uint32_t n, uint32_t event_mask, igdsp_tdet_state *d_state,
                      igdsp_tdet_rec *d_rec, igdsp_tdet_event *d_events, uint32_t event_cap, uint32_t *d_event_count, void *d_work, void *stream,
                      bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_tone_detect",
             args::tdet_run(d_g711, d_codec, d_pcm, d_plans, n_plans, d_plan_of, C, F, n, d_state, d_rec, d_events, event_cap, d_event_count, d_work));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_tone_detect(cfg_of(ctx, s), d_g711, d_codec, d_pcm, d_plans, n_plans, d_plan_of, C, F, n, event_mask, d_state, d_rec, d_events,
                                    event_cap, d_event_count, d_work, yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- in-band signalling the reference never hears: pjmedia reports digits only from telephone-event packets ----
int igdsp_tone_detect(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const igdsp_tdet_plan *d_plans,
                      uint32_t n_plans, const uint16_t *d_plan_of, uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame,
                      uint32_t event_mask, igdsp_tdet_state *d_state, igdsp_tdet_rec *d_rec, igdsp_tdet_event *d_events, uint32_t event_cap,
                      uint32_t *d_event_count, void *d_work, void *stream)
{
    return tdet_entry(ctx, d_g711, d_codec, d_pcm, d_plans, n_plans, d_plan_of, n_channels, n_frames, samples_per_frame, event_mask, d_state, d_rec,
                      d_events, event_cap, d_event_count, d_work, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick (tools/tdet_bench.py) — the same row loads, buffer stores and
// history moves, the same record, state and list passes, no table, pair read, dot product, decision or debounce.  Arguments as
// igdsp_tone_detect.  It stores the bytes igdsp_tone_detect stores: every record all-zero, the state's history as by igdsp_tone_detect,
// its debounce fields as they were (reserved 0), the list empty with both counts 0.
int igdsp_internal_tdet_move(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const igdsp_tdet_plan *d_plans,
                             uint32_t n_plans, const uint16_t *d_plan_of, uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame,
                             uint32_t event_mask, igdsp_tdet_state *d_state, igdsp_tdet_rec *d_rec, igdsp_tdet_event *d_events, uint32_t event_cap,
                             uint32_t *d_event_count, void *d_work, void *stream)
{
    return tdet_entry(ctx, d_g711, d_codec, d_pcm, d_plans, n_plans, d_plan_of, n_channels, n_frames, samples_per_frame, event_mask, d_state, d_rec,
                      d_events, event_cap, d_event_count, d_work, stream, true);
}

// ---- host only
int igdsp_tdet_plan_build(uint32_t clock_rate, const uint16_t *freq, uint32_t n_lo, uint32_t n_hi, const igdsp_tdet_thr *thr, igdsp_tdet_plan *out)
{
    if (!out) return IGDSP_EINVAL;
    return tdet_plan_make(clock_rate, freq, n_lo, n_hi, thr, *out) ? IGDSP_OK : IGDSP_EINVAL;
}

int igdsp_tdet_plan_dtmf(uint32_t clock_rate, igdsp_tdet_plan *out)
{
    static const uint16_t f[8] = {697, 770, 852, 941, 1209, 1336, 1477, 1633};
    return igdsp_tdet_plan_build(clock_rate, f, 4, 4, nullptr, out);
}

int igdsp_tdet_digit(uint32_t code) { return code >= 1u && code <= 16u ? "123A456B789C*0#D"[code - 1u] : 0; }

int igdsp_tdet_table(const igdsp_tdet_plan *plan, uint32_t n, int16_t *out)
{
    if (!plan || !out || !tdet_n_ok(n)) return IGDSP_EINVAL;
    const uint32_t nf = tdet_nlo(*plan) + tdet_nhi(*plan);
    for (uint32_t k = 0; k < nf; ++k)
        for (uint32_t i = 0; i < n; ++i) {
            out[(2u * k) * n + i] = (int16_t)tdet_wc(kToneSin, plan->step[k], i);
            out[(2u * k + 1u) * n + i] = (int16_t)tdet_ws(kToneSin, plan->step[k], i);
        }
    return IGDSP_OK;
}

int igdsp_tdet_frame(const igdsp_tdet_plan *plan, igdsp_tdet_state *st, const int16_t *row, uint32_t samples_per_frame, igdsp_tdet_rec *rec)
{
    if (!plan || !st || !row || !tdet_n_ok(samples_per_frame)) return IGDSP_EINVAL;
    tdet_frame_run(*plan, *st, row, samples_per_frame, rec);
    return IGDSP_OK;
}

size_t igdsp_tdet_work_bytes(uint32_t n_channels, uint32_t n_frames, int with_rec) { return (size_t)tdet_work_bytes(n_channels, n_frames, with_rec != 0); }

}  // extern "C"
