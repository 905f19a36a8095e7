// igdsp_capi_snd.hip — the sound-card splitter / combiner entries of include/igdsp.h (igdsp_snd_combine, igdsp_snd_split), their
// compute-free yardstick igdsp_internal_snd_copy and the host-only igdsp_snd_vu.  The entries read as every batched entry does
// (igdsp_capi.hip): null ctx, the argument rule of igdsp_args.h, hipSetDevice, the stream and its launch configuration, the launch.
#include "igdsp_args.h"
#include "igdsp_ctx.h"

#include <cmath>

using namespace igdsp;

// one direction, or with yardstick its compute-free twin
static int snd_entry(igdsp_ctx *ctx, const char *entry, int dir, const int16_t *d_in, uint32_t D, uint32_t K, uint32_t F, uint32_t n,
                     int16_t *d_bulk, igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, entry, dir == kSndCombine ? args::snd_combine(d_in, D, K, F, n, d_bulk, d_stats) : args::snd_split(d_in, D, K, F, n, d_bulk, d_stats));
    if (yardstick && !d_bulk) return IGDSP_EINVAL;                                // the yardstick moves the bulk bytes only
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_snd(cfg_of(ctx, s), dir, d_in, D, K, F, n, d_bulk, d_stats, yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- the splitcomb of initSlaveSoundCard (roip_ed137.cpp:3314-3435) ----
int igdsp_snd_combine(igdsp_ctx *ctx, const int16_t *d_pcm, uint32_t n_cards, uint32_t card_channels, uint32_t n_frames,
                      uint32_t samples_per_frame, int16_t *d_frames, igdsp_frame_stats *d_stats, void *stream)
{
    return snd_entry(ctx, "igdsp_snd_combine", kSndCombine, d_pcm, n_cards, card_channels, n_frames, samples_per_frame, d_frames, d_stats, stream, false);
}

int igdsp_snd_split(igdsp_ctx *ctx, const int16_t *d_frames, uint32_t n_cards, uint32_t card_channels, uint32_t n_frames,
                    uint32_t samples_per_frame, int16_t *d_pcm, igdsp_frame_stats *d_stats, void *stream)
{
    return snd_entry(ctx, "igdsp_snd_split", kSndSplit, d_frames, n_cards, card_channels, n_frames, samples_per_frame, d_pcm, d_stats, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of both directions (tools/snd_bench.py) — the same items, the
// same bytes read and written in memory order, no transpose and no records.  Arguments as igdsp_snd_combine; d_out is required and
// d_stats is not written.
int igdsp_internal_snd_copy(igdsp_ctx *ctx, const int16_t *d_in, uint32_t n_cards, uint32_t card_channels, uint32_t n_frames,
                            uint32_t samples_per_frame, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return snd_entry(ctx, "igdsp_snd_combine", kSndCombine, d_in, n_cards, card_channels, n_frames, samples_per_frame, d_out, d_stats, stream, true);
}

// Host only: the broadcastVUMeter numbers of one record (percent as igdsp_poll's, audiometer.cpp:30-31)
int igdsp_snd_vu(const igdsp_frame_stats *st, igdsp_snd_vu_t *out)
{
    if (!st || !out) return IGDSP_EINVAL;
    out->percent = (int32_t)(float)(((double)st->rms * 100.0) / (double)IGDSP_METER_FULL_SCALE);
    out->reserved = 0;
    out->db = st->rms > 0.f ? 20.0 * std::log10((double)st->rms / 32768.0) : IGDSP_SND_DB_FLOOR;
    return IGDSP_OK;
}

}  // extern "C"
