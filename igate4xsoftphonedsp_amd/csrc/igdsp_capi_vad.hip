// igdsp_capi_vad.hip — the voice detector's entries of include/igdsp.h: igdsp_vad_run and its compute-free yardstick
// igdsp_internal_vad_move, and the host-only igdsp_vad_cfg_default / _table / _frame / _work_bytes and igdsp_sid_decode, which run the
// rule of igdsp_vad.h that k_vad runs.  igdsp_vad_run reads as every batched entry does (igdsp_capi.hip): null ctx, the argument rule
// of igdsp_args.h, hipSetDevice, the stream and its launch configuration, the launch.
#include "igdsp_args.h"
#include "igdsp_ctx.h"
#include "igdsp_vad.h"

using namespace igdsp;

static int vad_entry(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const uint8_t *d_ctl, const igdsp_vad_cfg *cfg,
                     uint32_t C, uint32_t F, uint32_t n, uint32_t event_mask, igdsp_vad_state *d_state, uint8_t *d_kind, igdsp_vad_rec *d_rec,
                     uint8_t *d_sid, uint8_t *d_txctl, igdsp_vad_event *d_events, uint32_t event_cap, uint32_t *d_event_count, void *d_work,
                     void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_vad_run",
             args::vad_run(d_g711, d_codec, d_pcm, d_ctl, cfg, C, F, n, d_state, d_kind, d_rec, d_sid, d_txctl, d_events, event_cap, d_event_count, d_work));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_vad(cfg_of(ctx, s), d_g711, d_codec, d_pcm, d_ctl, vad_cfg_or_default(cfg), C, F, n, event_mask, d_state, d_kind, d_rec, d_sid,
                            d_txctl, d_events, event_cap, d_event_count, d_work, yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- the stream's silence detector, which the reference switches off (media_cfg.no_vad = 1), for a batch ----
int igdsp_vad_run(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const uint8_t *d_ctl, const igdsp_vad_cfg *cfg,
                  uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, uint32_t event_mask, igdsp_vad_state *d_state, uint8_t *d_kind,
                  igdsp_vad_rec *d_rec, uint8_t *d_sid, uint8_t *d_txctl, igdsp_vad_event *d_events, uint32_t event_cap, uint32_t *d_event_count,
                  void *d_work, void *stream)
{
    return vad_entry(ctx, d_g711, d_codec, d_pcm, d_ctl, cfg, n_channels, n_frames, samples_per_frame, event_mask, d_state, d_kind, d_rec, d_sid, d_txctl,
                     d_events, event_cap, d_event_count, d_work, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick (tools/vad_bench.py) — the same row loads and decode, LDS stores,
// state load and store, kind, record, payload and control-byte stores and list passes; no lag sum, level, decision, noise model or
// recursion.  Arguments as igdsp_vad_run; d_ctl is not read.  It stores the bytes igdsp_vad_run stores with every channel at
// IGDSP_VAD_BYPASS, except that a record's ms is 0 and its level 127; the state, which a bypass leaves alone, is written as it was read
// (nf and A clamped; another tag: the RESET state) with the tag, flags IGDSP_VAD_F_BYPASSED and reserved 0.
int igdsp_internal_vad_move(igdsp_ctx *ctx, const uint8_t *d_g711, const uint8_t *d_codec, const int16_t *d_pcm, const uint8_t *d_ctl,
                            const igdsp_vad_cfg *cfg, uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, uint32_t event_mask,
                            igdsp_vad_state *d_state, uint8_t *d_kind, igdsp_vad_rec *d_rec, uint8_t *d_sid, uint8_t *d_txctl, igdsp_vad_event *d_events,
                            uint32_t event_cap, uint32_t *d_event_count, void *d_work, void *stream)
{
    return vad_entry(ctx, d_g711, d_codec, d_pcm, d_ctl, cfg, n_channels, n_frames, samples_per_frame, event_mask, d_state, d_kind, d_rec, d_sid, d_txctl,
                     d_events, event_cap, d_event_count, d_work, stream, true);
}

// ---- host only
void igdsp_vad_cfg_default(igdsp_vad_cfg *out)
{
    if (out) *out = vad_cfg_default();
}

int igdsp_vad_table(uint64_t out[128])
{
    if (!out) return IGDSP_EINVAL;
    for (uint32_t d = 0; d < 128u; ++d) out[d] = kVadT8[d];
    return IGDSP_OK;
}

int igdsp_vad_frame(const igdsp_vad_cfg *cfg, igdsp_vad_state *st, const int16_t *pcm, uint32_t samples_per_frame, uint32_t ctl, igdsp_vad_rec *rec,
                    uint8_t sid[16])
{
    if (!st || !pcm || !vad_n_ok(samples_per_frame) || !vad_cfg_ok(cfg)) return IGDSP_EINVAL;
    return (int)vad_frame_run(vad_cfg_or_default(cfg), *st, pcm, samples_per_frame, ctl, rec, sid);
}

int igdsp_sid_decode(const uint8_t *payload, uint32_t len, uint8_t *level_dbov, int16_t k_q15[10])
{
    if (!payload || len == 0u) return IGDSP_EINVAL;
    if (level_dbov) *level_dbov = payload[0];
    if (k_q15)
        for (uint32_t i = 0; i < (uint32_t)IGDSP_VAD_ORDER; ++i) k_q15[i] = (int16_t)(i + 1u < len ? vad_dequant(payload[i + 1u]) : 0);
    return IGDSP_OK;
}

size_t igdsp_vad_work_bytes(uint32_t n_channels, uint32_t n_frames, int with_rec) { return (size_t)vad_work_bytes(n_channels, n_frames, with_rec != 0); }

}  // extern "C"
