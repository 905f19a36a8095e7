// igdsp_capi_cng.hip — the comfort-noise generator's entries of include/igdsp.h: igdsp_cng_run and its compute-free yardstick
// igdsp_internal_cng_move, and the host-only igdsp_cng_table / _gain / _frame, which run the rule of igdsp_cng.h that k_cng runs.
// igdsp_cng_run reads as every batched entry does (igdsp_capi.hip): null ctx, the argument rule of igdsp_args.h, hipSetDevice, the
// stream and its launch configuration, the launch.
#include "igdsp_args.h"
#include "igdsp_cng.h"
#include "igdsp_ctx.h"

using namespace igdsp;

static int cng_entry(igdsp_ctx *ctx, const uint8_t *d_kind, const uint8_t *d_sid, const uint8_t *d_sid_len, const uint8_t *d_g711, const uint8_t *d_codec,
                     const int16_t *d_pcm, const uint8_t *d_ctl, const uint32_t *d_seed, uint32_t C, uint32_t F, uint32_t n, igdsp_cng_state *d_state,
                     int16_t *d_out, uint16_t *d_len_out, igdsp_cng_rec *d_rec, igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_cng_run", args::cng_run(d_kind, d_sid, d_sid_len, d_g711, d_codec, d_pcm, d_ctl, d_seed, C, F, n, d_state, d_out, d_len_out, d_rec, d_stats));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_cng(cfg_of(ctx, s), d_kind, d_sid, d_sid_len, d_g711, d_codec, d_pcm, d_ctl, d_seed, C, F, n, d_state, d_out, d_len_out, d_rec, d_stats,
                            yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- the receive side of DTX: PT 13 payloads back into rows for the bridge, for a batch ----
int igdsp_cng_run(igdsp_ctx *ctx, const uint8_t *d_kind, const uint8_t *d_sid, const uint8_t *d_sid_len, const uint8_t *d_g711, const uint8_t *d_codec,
                  const int16_t *d_pcm, const uint8_t *d_ctl, const uint32_t *d_seed, uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame,
                  igdsp_cng_state *d_state, int16_t *d_out, uint16_t *d_len_out, igdsp_cng_rec *d_rec, igdsp_frame_stats *d_stats, void *stream)
{
    return cng_entry(ctx, d_kind, d_sid, d_sid_len, d_g711, d_codec, d_pcm, d_ctl, d_seed, n_channels, n_frames, samples_per_frame, d_state, d_out, d_len_out,
                     d_rec, d_stats, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick (tools/cng_bench.py) — the same kind, length and voice-row loads
// and decode, tile stores and reads, state load and store, row, length, record and stats stores; no excitation, lattice, gain step or
// SID step.  Arguments as igdsp_cng_run; d_ctl and d_sid's payloads are not read.  It stores the bytes igdsp_cng_run stores with every
// channel at IGDSP_CNG_BYPASS, except that the state, which a bypass leaves alone, is written back as it was read, clamped (b, kq, g,
// g_tgt clamped, have its bit 0; another tag: the RESET state with d_seed's seed), with the tag, flags as read and reserved 0.
int igdsp_internal_cng_move(igdsp_ctx *ctx, const uint8_t *d_kind, const uint8_t *d_sid, const uint8_t *d_sid_len, const uint8_t *d_g711,
                            const uint8_t *d_codec, const int16_t *d_pcm, const uint8_t *d_ctl, const uint32_t *d_seed, uint32_t n_channels,
                            uint32_t n_frames, uint32_t samples_per_frame, igdsp_cng_state *d_state, int16_t *d_out, uint16_t *d_len_out,
                            igdsp_cng_rec *d_rec, igdsp_frame_stats *d_stats, void *stream)
{
    return cng_entry(ctx, d_kind, d_sid, d_sid_len, d_g711, d_codec, d_pcm, d_ctl, d_seed, n_channels, n_frames, samples_per_frame, d_state, d_out, d_len_out,
                     d_rec, d_stats, stream, true);
}

// ---- host only
int igdsp_cng_table(uint32_t out[128])
{
    if (!out) return IGDSP_EINVAL;
    for (uint32_t d = 0; d < 128u; ++d) out[d] = kCngG[d];
    return IGDSP_OK;
}

int igdsp_cng_gain(const uint8_t *payload, uint32_t len, uint32_t *g_tgt)
{
    if (!payload || !g_tgt || len == 0u || len > 16u) return IGDSP_EINVAL;
    *g_tgt = cng_gain_host(payload, len);
    return IGDSP_OK;
}

int igdsp_cng_frame(igdsp_cng_state *st, uint32_t kind, const uint8_t *sid, uint32_t sid_len, const int16_t *voice, uint32_t samples_per_frame,
                    uint32_t ctl, uint32_t seed, int16_t *out, igdsp_cng_rec *rec)
{
    if (!st || !out || !cng_n_ok(samples_per_frame)) return IGDSP_EINVAL;
    if (!sid && kind == (uint32_t)IGDSP_VAD_SID && sid_len != 0u) return IGDSP_EINVAL;
    return (int)cng_frame_run(*st, kind, sid, sid_len, voice, samples_per_frame, ctl, seed, out, rec);
}

}  // extern "C"
