// igdsp_capi_ns.hip — the noise suppressor's entries of include/igdsp.h: igdsp_ns_run and its compute-free yardstick
// igdsp_internal_ns_move, and the host-only igdsp_ns_cfg_default / igdsp_ns_tables / igdsp_ns_frame, which run the rule of igdsp_ns.h
// that k_ns runs.  igdsp_ns_run reads as every batched entry does (igdsp_capi.hip): null ctx, the argument rule of igdsp_args.h,
// hipSetDevice, the stream and its launch configuration, the launch.
#include "igdsp_args.h"
#include "igdsp_ctx.h"
#include "igdsp_ns.h"

using namespace igdsp;

static int ns_entry(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const uint8_t *d_ctl, const igdsp_ns_cfg *cfg,
                    uint32_t C, uint32_t F, uint32_t n, igdsp_ns_state *d_state, int16_t *d_out, igdsp_ns_rec *d_rec, igdsp_frame_stats *d_stats, void *stream,
                    bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_ns_run", args::ns_run(d_g711, d_codec, d_pcm, d_ctl, cfg, C, F, n, d_state, d_out, d_rec, d_stats));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_ns(cfg_of(ctx, s), d_g711, d_codec, d_pcm, d_ctl, *cfg, C, F, n, d_state, d_out, d_rec, d_stats, yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- a spectral gain per channel and hop, for a batch ----
int igdsp_ns_run(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const uint8_t *d_ctl, const igdsp_ns_cfg *cfg,
                 uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, igdsp_ns_state *d_state, int16_t *d_out, igdsp_ns_rec *d_rec,
                 igdsp_frame_stats *d_stats, void *stream)
{
    return ns_entry(ctx, d_g711, d_codec, d_pcm, d_ctl, cfg, n_channels, n_frames, samples_per_frame, d_state, d_out, d_rec, d_stats, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick (tools/ns_bench.py) — the same row loads and decode, row
// stores into LDS, state load and store, the delay's pass over the row, the energy and PCM-record folds, row, record and stats stores;
// no transform and no band runs.  Arguments as igdsp_ns_run; d_ctl is not read.  It stores the bytes igdsp_ns_run stores with every
// channel at IGDSP_NS_BYPASS.
int igdsp_internal_ns_move(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const uint8_t *d_ctl, const igdsp_ns_cfg *cfg,
                           uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, igdsp_ns_state *d_state, int16_t *d_out, igdsp_ns_rec *d_rec,
                           igdsp_frame_stats *d_stats, void *stream)
{
    return ns_entry(ctx, d_g711, d_codec, d_pcm, d_ctl, cfg, n_channels, n_frames, samples_per_frame, d_state, d_out, d_rec, d_stats, stream, true);
}

// ---- host only
void igdsp_ns_cfg_default(igdsp_ns_cfg *out)
{
    if (out) ns_cfg_default(*out);
}

int igdsp_ns_tables(const int16_t **window, const int32_t **twiddle)
{
    if (window) *window = kNsWin;
    if (twiddle) *twiddle = kNsTw;
    return IGDSP_OK;
}

int igdsp_ns_frame(const igdsp_ns_cfg *cfg, igdsp_ns_state *st, const int16_t *pcm, uint32_t samples_per_frame, uint32_t ctl, int16_t *out, igdsp_ns_rec *rec)
{
    if (!cfg || !st || !pcm || !ns_n_ok(samples_per_frame) || !ns_cfg_ok(*cfg)) return IGDSP_EINVAL;
    ns_frame_run(*cfg, *st, pcm, samples_per_frame, ctl, out, rec);
    return IGDSP_OK;
}

}  // extern "C"
