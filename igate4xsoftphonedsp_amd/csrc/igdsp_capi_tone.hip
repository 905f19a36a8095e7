// igdsp_capi_tone.hip — the tone generator entries of include/igdsp.h: igdsp_tone_generate and its compute-free yardstick
// igdsp_internal_tone_fill, and the host-only igdsp_tone_plan_build / igdsp_tone_frame, which run the constexpr rules of igdsp_route.h
// that k_tone runs.  igdsp_tone_generate reads as every batched entry does (igdsp_capi.hip): null ctx, the argument rule of
// igdsp_args.h, hipSetDevice, the stream and its launch configuration, the launch.
#include "igdsp_args.h"
#include "igdsp_ctx.h"

using namespace igdsp;

static int tone_entry(igdsp_ctx *ctx, const igdsp_tone_plan *d_plans, uint32_t n_plans, const uint16_t *d_plan_of, const uint8_t *d_cmd,
                      igdsp_tone_state *d_state, uint32_t P, uint32_t F, uint32_t n, uint32_t rows_per_frame, int16_t *d_pcm, uint16_t *d_len,
                      igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_tone_generate", args::tone_generate(d_plans, n_plans, d_plan_of, d_cmd, d_state, P, F, n, rows_per_frame, d_pcm, d_len, d_stats));
    if (yardstick && !d_pcm) return IGDSP_EINVAL;                                 // the yardstick writes the rows
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_tone(cfg_of(ctx, s), d_plans, n_plans, d_plan_of, d_cmd, d_state, P, F, n, rows_per_frame, d_pcm, d_len, d_stats, yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- the tonegen port of init_ringTone (Functions.cpp:532-571) ----
int igdsp_tone_generate(igdsp_ctx *ctx, const igdsp_tone_plan *d_plans, uint32_t n_plans, const uint16_t *d_plan_of, const uint8_t *d_cmd,
                        igdsp_tone_state *d_state, uint32_t n_ports, uint32_t n_frames, uint32_t samples_per_frame, uint32_t rows_per_frame,
                        int16_t *d_pcm, uint16_t *d_len, igdsp_frame_stats *d_stats, void *stream)
{
    return tone_entry(ctx, d_plans, n_plans, d_plan_of, d_cmd, d_state, n_ports, n_frames, samples_per_frame, rows_per_frame, d_pcm, d_len, d_stats,
                      stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick (tools/tone_bench.py) — the same items in the same order, the
// same rows, lengths and records stored, no plan, no state, no oscillator.  Arguments as igdsp_tone_generate; d_pcm is required, the
// state is neither read nor written, the rows hold a pattern and the records are the len-0 record.
int igdsp_internal_tone_fill(igdsp_ctx *ctx, const igdsp_tone_plan *d_plans, uint32_t n_plans, const uint16_t *d_plan_of, const uint8_t *d_cmd,
                             igdsp_tone_state *d_state, uint32_t n_ports, uint32_t n_frames, uint32_t samples_per_frame,
                             uint32_t rows_per_frame, int16_t *d_pcm, uint16_t *d_len, igdsp_frame_stats *d_stats, void *stream)
{
    return tone_entry(ctx, d_plans, n_plans, d_plan_of, d_cmd, d_state, n_ports, n_frames, samples_per_frame, rows_per_frame, d_pcm, d_len, d_stats,
                      stream, true);
}

// Host only
int igdsp_tone_plan_build(const igdsp_tone_desc *tones, uint32_t count, uint32_t clock_rate, uint32_t options, igdsp_tone_plan *out)
{
    if (!out) return IGDSP_EINVAL;
    return tone_plan_make(tones, count, clock_rate, options, *out) ? IGDSP_OK : IGDSP_EINVAL;
}

// Host only: one frame of one port, the state advanced
int igdsp_tone_frame(const igdsp_tone_plan *plan, igdsp_tone_state *st, uint32_t cmd, uint32_t samples_per_frame, int16_t *out, uint16_t *len)
{
    const uint32_t n = samples_per_frame;
    if (!plan || !st || !out || !len || n == 0 || n > IGDSP_MAX_PAYLOAD) return IGDSP_EINVAL;
    const igdsp_tone_state s = tone_cmd(*st, cmd);
    const bool hold = (cmd & IGDSP_TONE_CMD_HOLD) != 0u;
    const bool live = !hold && tone_plays(*plan, s) && tone_live(*plan, s.pos);
    for (uint32_t i = 0; i < n; ++i) out[i] = live ? (int16_t)tone_frame_sample(kTonePairs.w, *plan, s.pos, i) : (int16_t)0;
    *len = (uint16_t)(live ? n : 0u);
    *st = hold ? s : tone_advance(*plan, s, n);
    return IGDSP_OK;
}

}  // extern "C"
