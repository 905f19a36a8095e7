// igdsp_capi.hip — the batched device entries of include/igdsp.h over the gfx950 kernels, their compute-free yardstick twins
// (igdsp_internal_*_copy) and the host-only companions of each (work sizes, table builders, reports).  An entry reads: null ctx, its
// argument rule (igdsp_args.h: host-only, tested without a device), hipSetDevice, the stream and its launch configuration, the launch.
// There is NO CPU compute path here: when the HIP runtime or a gfx950 device is missing every entry fails with IGDSP_ENODEV.
// Context, routing, flush, poll, memory and timers are in igdsp_capi_ctx.hip, the staged send path in igdsp_capi_tx.hip, calibration
// and diagnostic entries in igdsp_capi_bench.hip.
#include "igdsp_ctx.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

using namespace igdsp;

extern "C" {

// ---------------------------------------------------------------- payload entries
int igdsp_decode_meter(igdsp_ctx *ctx, const uint8_t *d_payload, const uint8_t *d_codec, const uint16_t *d_len,
                       uint32_t C, uint32_t F, uint32_t n, igdsp_frame_stats *d_stats, int16_t *d_pcm,
                       igdsp_aggregate *d_agg, uint32_t rank, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_decode_meter", args::decode_meter(d_payload, d_codec, d_len, C, F, n, d_stats, d_pcm, d_agg, rank));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_decode_meter(cfg_of(ctx, s), ctx->variant, d_payload, d_codec, d_len, C, F, n, d_stats, d_pcm, d_agg, rank, s));
    return IGDSP_OK;
}

// The context's 16-bit compressor table of one lineage (tab[law << 16 | uint16(v)]), built on the device the first time a large
// batch asks for it; nullptr if that failed (the kernels then evaluate the table themselves).
static const uint8_t *enc_table(igdsp_ctx *ctx, int variant)
{
    const int v = variant == IGDSP_ENC_G191 ? 1 : 0;
    std::call_once(ctx->enc_once[v], [&]() {
        uint8_t *t = nullptr;
        hipStream_t bs = nullptr;
        bool ok = hipMalloc((void **)&t, 2u * 65536u) == hipSuccess && hipStreamCreateWithFlags(&bs, hipStreamNonBlocking) == hipSuccess;
        ok = ok && igdsp::launch_build_enc_table(variant, t, bs) == hipSuccess && hipStreamSynchronize(bs) == hipSuccess;
        if (bs) (void)hipStreamDestroy(bs);
        if (ok) ctx->d_enc_tab[v] = t;                          // complete before any launch that reads it is enqueued
        else { if (t) (void)hipFree(t); (void)hipGetLastError(); }   // the kernel evaluates the table itself, as before
    });
    return ctx->d_enc_tab[v];
}

int igdsp_encode(igdsp_ctx *ctx, const int16_t *d_pcm, const uint8_t *d_codec, uint32_t C, uint32_t F, uint32_t n,
                 uint8_t *d_out, int variant, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_encode", args::encode(d_pcm, d_codec, C, F, n, d_out, variant));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    igdsp::LaunchCfg cfg = cfg_of(ctx, s);
    if (encode_wants_table(encode_route(C, F, n, reinterpret_cast<uintptr_t>(d_pcm), reinterpret_cast<uintptr_t>(d_out), (uint32_t)cfg.compute_units)))
        cfg.enc_tab = enc_table(ctx, variant);
    HIP_TRY(ctx, launch_encode(cfg, d_pcm, d_codec, C, F, n, d_out, variant, s));
    return IGDSP_OK;
}

int igdsp_roundtrip_peakhold(igdsp_ctx *ctx, const uint8_t *d_payload, const uint8_t *d_codec, uint32_t C, uint32_t F,
                             uint32_t n, uint8_t *d_out, igdsp_frame_stats *d_stats, igdsp_chan_hold *d_hold,
                             const uint8_t *d_gate, int variant, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_roundtrip_peakhold", args::roundtrip_peakhold(d_payload, d_codec, C, F, n, d_out, d_stats, d_hold, d_gate, variant));
    // every shape is served: whole groups of 64 channels of 160-byte frames by the fused channel-group-major kernel,
    // the remaining channels and every other geometry by the general wave-per-channel kernel (launch_roundtrip)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    igdsp::LaunchCfg cfg = cfg_of(ctx, s);
    cfg.out_spread = ctx->is_spread(d_out);
    HIP_TRY(ctx, launch_roundtrip(cfg, ctx->variant, d_payload, d_codec, C, F, n, d_out, d_stats, d_hold, d_gate, variant, s));
    return IGDSP_OK;
}

int igdsp_hold_update(igdsp_ctx *ctx, const igdsp_frame_stats *d_stats, uint32_t C, uint32_t F, uint32_t n,
                      igdsp_chan_hold *d_hold, const uint8_t *d_gate, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_hold_update", args::hold_update(d_stats, C, F, n, d_hold, d_gate));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_hold_update(d_stats, nullptr, C, F, n, d_hold, d_gate, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_hold_reset(igdsp_ctx *ctx, igdsp_chan_hold *d_hold, uint32_t C, const uint8_t *d_mask, void *stream)
{
    if (!ctx || (!d_hold && C)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_hold_reset(d_hold, C, d_mask, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_agg_reset(igdsp_ctx *ctx, igdsp_aggregate *d_agg, void *stream)
{
    if (!ctx || !d_agg) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(d_agg, 0, sizeof(igdsp_aggregate), pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_depayload(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_radio, uint32_t C,
                    uint32_t F, uint32_t pkt_stride, uint32_t n, uint8_t *d_payload_out, uint16_t *d_len_out,
                    igdsp_rtp_info *d_info_out, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_depayload", args::depayload(d_packets, d_sizes, d_radio, C, F, pkt_stride, n, d_payload_out, d_len_out, d_info_out));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_depayload(cfg_of(ctx, s), d_packets, d_sizes, d_radio, C, F, pkt_stride, n, d_payload_out, d_len_out, d_info_out, s));
    return IGDSP_OK;
}

// ---------------------------------------------------------------- fused packet entries
int igdsp_decode_meter_rtp(igdsp_ctx *ctx, const uint8_t *d_slots, const uint8_t *d_codec, uint32_t C, uint32_t F,
                           igdsp_frame_stats *d_stats, igdsp_rtp_info *d_info, igdsp_aggregate *d_agg, uint32_t rank, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_decode_meter_rtp", args::decode_meter_rtp(d_slots, d_codec, C, F, d_stats, d_info, d_agg, rank));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_decode_meter_rtp(cfg_of(ctx, s), d_slots, nullptr, d_codec, C, F, 0, 20, d_stats, d_info, d_agg, rank, s));
    return IGDSP_OK;
}

int igdsp_decode_meter_packets(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_codec, uint32_t C,
                               uint32_t F, uint32_t pkt_stride, uint32_t hdr_bytes, igdsp_frame_stats *d_stats,
                               igdsp_rtp_info *d_info, igdsp_aggregate *d_agg, uint32_t rank, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_decode_meter_packets",
             args::decode_meter_packets(d_packets, d_sizes, d_codec, C, F, pkt_stride, hdr_bytes, d_stats, d_info, d_agg, rank));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_decode_meter_rtp(cfg_of(ctx, s), d_packets, d_sizes, d_codec, C, F, pkt_stride, hdr_bytes, d_stats, d_info, d_agg, rank, s));
    return IGDSP_OK;
}

int igdsp_decode_meter_packets_mixed(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_codec,
                                     const uint8_t *d_radio, uint32_t C, uint32_t F, uint32_t pkt_stride, igdsp_frame_stats *d_stats,
                                     igdsp_rtp_info *d_info, igdsp_aggregate *d_agg, uint32_t rank, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_decode_meter_packets_mixed",
             args::decode_meter_packets_mixed(d_packets, d_sizes, d_codec, d_radio, C, F, pkt_stride, d_stats, d_info, d_agg, rank));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_decode_meter_rtp(cfg_of(ctx, s), d_packets, d_sizes, d_codec, C, F, pkt_stride, 12, d_stats, d_info, d_agg, rank, s, d_radio));
    return IGDSP_OK;
}

// ---------------------------------------------------------------- ED-137 gated window (last clause)
size_t igdsp_window_work_bytes(uint32_t n_channels) { return (size_t)kWinMaxSeg * 3u * n_channels * sizeof(uint4); }

int igdsp_window_update(igdsp_ctx *ctx, const igdsp_frame_stats *d_stats, const igdsp_rtp_info *d_info, const uint16_t *d_len,
                        uint32_t C, uint32_t F, uint32_t n, const igdsp_window *win, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_window_update", args::window_update(d_stats, d_info, d_len, C, F, n, win));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_window_update(d_stats, d_info, d_len, C, F, n, win->gate_mode, win->probe_alarm ? win->probe_alarm : IGDSP_PROBE_ALARM,
                                      win->d_hold, win->d_gate, win->d_probe, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_decode_meter_window(igdsp_ctx *ctx, uint32_t layout, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_codec,
                              const uint8_t *d_radio, uint32_t C, uint32_t F, uint32_t pkt_stride, uint32_t hdr_bytes,
                              igdsp_frame_stats *d_stats, igdsp_rtp_info *d_info, igdsp_aggregate *d_agg, uint32_t rank,
                              const igdsp_window *win, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_decode_meter_window",
             args::decode_meter_window(layout, d_packets, d_sizes, d_codec, d_radio, C, F, pkt_stride, hdr_bytes, d_stats, d_info, d_agg, rank, win));
    // what the launcher is told of each layout: slots have no stride and no sizes, only MIXED reads the radio flags
    const bool slots = layout == IGDSP_PKT_SLOTS;
    const uint32_t stride = slots ? 0 : pkt_stride, hdr = layout == IGDSP_PKT_PACKED ? hdr_bytes : slots ? 20 : 12;
    const uint16_t *sizes = slots ? nullptr : d_sizes;
    const uint8_t *radio = layout == IGDSP_PKT_MIXED ? d_radio : nullptr;
    const uint32_t alarm = win->probe_alarm ? win->probe_alarm : IGDSP_PROBE_ALARM;
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (args::window_fused(C, win)) {   // channel-group-major fused kernel with the window folded in (launch_decode_meter_window)
        bool too_long = false;
        HIP_TRY(ctx, launch_decode_meter_window(cfg_of(ctx, s), d_packets, sizes, d_codec, C, F, stride, hdr, radio, d_stats, d_info, d_agg, rank, *win,
                                                &too_long, s));
        if (too_long) return fail(ctx, IGDSP_ERANGE, "decode_meter_window: more than 8 x 65535 frames per launch");
        return IGDSP_OK;
    }
    // other channel counts: the plain fused kernel, then the record-wise window fold on the same stream
    HIP_TRY(ctx, launch_decode_meter_rtp(cfg_of(ctx, s), d_packets, sizes, d_codec, C, F, stride, hdr, d_stats, d_info, d_agg, rank, s, radio));
    HIP_TRY(ctx, launch_window_update(d_stats, d_info, nullptr, C, F, IGDSP_SAMPLES_PER_FRAME, win->gate_mode, alarm, win->d_hold, win->d_gate, win->d_probe, s));
    return IGDSP_OK;
}

int igdsp_wav_expand(igdsp_ctx *ctx, const uint8_t *d_payload, uint32_t C, uint32_t F, uint32_t n, uint32_t rate,
                     uint8_t *d_files, uint64_t file_stride, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_wav_expand", args::wav_expand(d_payload, C, F, n, rate, d_files, file_stride));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_wav_expand(cfg_of(ctx, s), d_payload, C, F, n, rate, d_files, file_stride, s));
    return IGDSP_OK;
}

// ---- ED-137 TX packetizer (transport_send_rtp, TransportAdapter.cpp:635-874) ----
int igdsp_tx_calltype_bits(const char *ct)
{
    if (!ct) return 0;
    int b = 0;
    if (std::strstr(ct, "Idle")) b |= IGDSP_TX_CT_IDLE;                                   // :675
    if (std::strstr(ct, "Rxonly") || std::strcmp(ct, "Rx") == 0) b |= IGDSP_TX_CT_RX;     // :795, :811
    if (std::strstr(ct, "Tx") || std::strstr(ct, "TRx")) b |= IGDSP_TX_CT_TX;             // :816, :821
    return b;
}

int igdsp_tx_chan_init(igdsp_tx_chan *h, const char *calltype, int call_in, uint8_t pt, uint32_t ssrc, uint16_t seq0, uint32_t ts0,
                       int32_t keepalive_ms, uint64_t now_ms)
{
    if (!h || pt > 127u) return IGDSP_EINVAL;
    std::memset(h, 0, sizeof *h);                          // PJ_POOL_ZALLOC_T (TransportAdapter.cpp:97)
    h->seq = seq0;
    h->ts = ts0;
    h->ssrc = ssrc;
    h->pt = pt;
    h->call_in = call_in ? 1 : 0;                          // :111
    h->keepalive_ms = keepalive_ms;                        // :115
    h->calltype = (uint8_t)igdsp_tx_calltype_bits(calltype);   // :118
    h->r2s_send_ms = now_ms;                               // :123
    h->first_r2s = 1;                                      // :124 (packetCnt 0, callRecorder / slave enables false: :125-128)
    return IGDSP_OK;
}

int igdsp_tx_packetize(igdsp_ctx *ctx, const int16_t *d_pcm, const uint8_t *d_g711, const uint8_t *d_ctl, uint32_t C, uint32_t F,
                       uint32_t n, uint64_t t0_ms, uint32_t frame_ms, igdsp_tx_chan *d_state, uint8_t *d_last_payload, uint8_t *d_packets,
                       uint32_t pkt_stride, uint16_t *d_sizes, igdsp_tx_info *d_info, int variant, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_tx_packetize", args::tx_packetize(d_pcm, d_g711, d_ctl, C, F, n, t0_ms, frame_ms, d_state, d_last_payload, d_packets,
                                                           pkt_stride, d_sizes, d_info, variant));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    igdsp::LaunchCfg cfg = cfg_of(ctx, s);
    if (tx_wants_table(d_pcm != nullptr, C, F, n)) cfg.enc_tab = enc_table(ctx, variant);
    HIP_TRY(ctx, launch_tx_packetize(cfg, d_pcm, d_g711, d_ctl, C, F, n, t0_ms, frame_ms, d_state, d_last_payload, d_packets, pkt_stride,
                                     d_sizes, d_info, variant, s));
    return IGDSP_OK;
}

// Calibration-only (not in include/igdsp.h): the compute-free packet writer that moves the bytes of an all-audio igdsp_tx_packetize launch
// in the same traversal and the same grid (tx_copy_route) (tools/tx_bench.py --ab).  Exactly one of d_pcm / d_g711; n % 4 == 0.
int igdsp_internal_tx_copy(igdsp_ctx *ctx, const int16_t *d_pcm, const uint8_t *d_g711, uint32_t C, uint32_t F, uint32_t n, uint8_t *d_packets,
                           uint32_t pkt_stride, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_internal_tx_copy", args::tx_copy(d_pcm, d_g711, C, F, n, d_packets, pkt_stride));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_tx_copy_ab(cfg_of(ctx, s), d_pcm, d_g711, C, F, n, d_packets, pkt_stride, s));
    return IGDSP_OK;
}

// ---- conference mix: pjmedia's bridge step as the reference drives it (pjsua_conf_connect roip_ed137.cpp:4907-4917, Functions.cpp:718-740;
// pjsua_conf_adjust_rx_level in setSlotVolume roip_ed137.cpp:5190-5233, setvolumeSiteTone roip_ed137.cpp:6869-6878) ----
int igdsp_conf_level_q7(float level)
{
    if (!(level == level)) return IGDSP_EINVAL;                                               // NaN
    const float adj = (level - 1.0f) * 128.0f;                                                // float, as pjsua does it
    if (!(adj > -1.0e6f && adj < 1.0e6f)) return IGDSP_EINVAL;                                // (int) of it must be defined
    const int q = 128 + (int)adj;                                                             // (int): toward zero
    return (q < 0 || q > 65535) ? IGDSP_EINVAL : q;
}

int igdsp_conf_build(const uint32_t *channel, const uint32_t *port, uint32_t n_conn, uint32_t n_channels, uint32_t n_ports,
                     uint32_t *port_ptr, uint32_t *members, uint32_t *n_members)
{
    if (!port_ptr || !n_members || (n_conn && (!channel || !port || !members))) return IGDSP_EINVAL;
    std::vector<uint64_t> key;
    try { key.resize(n_conn); } catch (...) { return IGDSP_ENOMEM; }
    for (uint32_t i = 0; i < n_conn; ++i) {
        if (channel[i] >= n_channels || port[i] >= n_ports) return IGDSP_EINVAL;
        key[i] = (uint64_t)port[i] << 32 | channel[i];
    }
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    uint32_t j = 0;
    for (uint32_t p = 0; p <= n_ports; ++p) {
        while (j < key.size() && (key[j] >> 32) < p) ++j;
        port_ptr[p] = j;
    }
    for (size_t i = 0; i < key.size(); ++i) members[i] = (uint32_t)key[i];
    *n_members = (uint32_t)key.size();
    return IGDSP_OK;
}

// igdsp_conf_mix, or with yardstick its compute-free twin igdsp_internal_conf_copy
static int conf_mix(igdsp_ctx *ctx, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm, const uint16_t *d_len,
                    const uint16_t *d_gain, const uint32_t *d_port_ptr, const uint32_t *d_members, uint32_t n_members, uint32_t C, uint32_t P,
                    uint32_t F, uint32_t n, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_conf_mix", args::conf_mix(d_payload, d_codec, d_pcm, d_len, d_gain, d_port_ptr, d_members, n_members, C, P, F, n, d_out, d_stats));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_conf_mix(cfg_of(ctx, s), d_payload, d_codec, d_pcm, d_len, d_gain, d_port_ptr, d_members, n_members, C, P, F, n, d_out, d_stats,
                                 yardstick, s));
    return IGDSP_OK;
}

int igdsp_conf_mix(igdsp_ctx *ctx, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm, const uint16_t *d_len,
                   const uint16_t *d_gain, const uint32_t *d_port_ptr, const uint32_t *d_members, uint32_t n_members, uint32_t C, uint32_t P,
                   uint32_t F, uint32_t n, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return conf_mix(ctx, d_payload, d_codec, d_pcm, d_len, d_gain, d_port_ptr, d_members, n_members, C, P, F, n, d_out, d_stats, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of igdsp_conf_mix (tools/conf_bench.py) — the same traversal,
// the same bytes read and written, no decode / scale / clamp / stats.  Arguments as igdsp_conf_mix.
int igdsp_internal_conf_copy(igdsp_ctx *ctx, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm, const uint16_t *d_len,
                             const uint16_t *d_gain, const uint32_t *d_port_ptr, const uint32_t *d_members, uint32_t n_members, uint32_t C,
                             uint32_t P, uint32_t F, uint32_t n, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return conf_mix(ctx, d_payload, d_codec, d_pcm, d_len, d_gain, d_port_ptr, d_members, n_members, C, P, F, n, d_out, d_stats, stream, true);
}

// ---- best signal selection: the receiver vote of checkEvents (roip_ed137.cpp:5985-6119; get_IPRadioSquelch / get_IPRadioBss,
// Functions.cpp:1001-1022; setvolume, Functions.cpp:1664-1705) ----
// igdsp_bss_select, or with yardstick its compute-free twin igdsp_internal_bss_copy
static int bss_select(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                      const uint16_t *d_len, const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members, uint32_t n_members,
                      const uint8_t *d_mute, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t vote_frames, igdsp_bss_state *d_state,
                      uint32_t *d_words, int32_t *d_sel, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_bss_select", args::bss_select(d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, d_mute, C, G,
                                                       F, n, vote_frames, d_state, d_words, d_sel, d_out, d_stats));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_bss_select(cfg_of(ctx, s), d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, d_mute, C, G, F,
                                   n, vote_frames, d_state, d_words, d_sel, d_out, d_stats, yardstick, s));
    return IGDSP_OK;
}

int igdsp_bss_select(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                     const uint16_t *d_len, const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members, uint32_t n_members,
                     const uint8_t *d_mute, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t vote_frames, igdsp_bss_state *d_state,
                     uint32_t *d_words, int32_t *d_sel, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return bss_select(ctx, d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, d_mute, C, G, F, n, vote_frames,
                      d_state, d_words, d_sel, d_out, d_stats, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of igdsp_bss_select (tools/bss_bench.py) — the same traversal,
// the same bytes read and written, no decode / scale / clamp / stats / state machine (every non-empty group "selects" its first
// member).  Arguments as igdsp_bss_select; the group state is not touched, the stored words are written as by a launch (the words
// pass runs behind the yardstick too), and sel / out / stats hold raw bytes.
int igdsp_internal_bss_copy(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                            const uint16_t *d_len, const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members,
                            uint32_t n_members, const uint8_t *d_mute, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t vote_frames,
                            igdsp_bss_state *d_state, uint32_t *d_words, int32_t *d_sel, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return bss_select(ctx, d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, d_mute, C, G, F, n, vote_frames,
                      d_state, d_words, d_sel, d_out, d_stats, stream, true);
}

// ---- PTT priority arbitration: the CLIENT-mode block of checkEvents (roip_ed137.cpp:6124-6231; get_IPRadioPttStatus,
// Functions.cpp:1045-1139; the PTT id, Functions.cpp:1141-1151) ----
// igdsp_ptt_arbitrate, or with yardstick its compute-free twin igdsp_internal_ptt_copy
static int ptt_arbitrate(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                         const uint16_t *d_len, const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members,
                         uint32_t n_members, const uint8_t *d_rxonly, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t release_frames,
                         igdsp_ptt_state *d_state, igdsp_ptt_slot *d_slots, int32_t *d_sel, igdsp_ptt_tick *d_tick, uint8_t *d_ctl_out,
                         int16_t *d_out, igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_ptt_arbitrate", args::ptt_arbitrate(d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, d_rxonly,
                                                             C, G, F, n, release_frames, d_state, d_slots, d_sel, d_tick, d_ctl_out, d_out, d_stats));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_ptt_arbitrate(cfg_of(ctx, s), d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, d_rxonly, C, G,
                                      F, n, release_frames, d_state, d_slots, d_sel, d_tick, d_ctl_out, d_out, d_stats, yardstick, s));
    return IGDSP_OK;
}

int igdsp_ptt_arbitrate(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                        const uint16_t *d_len, const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members,
                        uint32_t n_members, const uint8_t *d_rxonly, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t release_frames,
                        igdsp_ptt_state *d_state, igdsp_ptt_slot *d_slots, int32_t *d_sel, igdsp_ptt_tick *d_tick, uint8_t *d_ctl_out,
                        int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return ptt_arbitrate(ctx, d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, d_rxonly, C, G, F, n,
                         release_frames, d_state, d_slots, d_sel, d_tick, d_ctl_out, d_out, d_stats, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of igdsp_ptt_arbitrate (tools/ptt_bench.py) — the same
// traversal (info records, ops passes, the first member of every group emitted undecoded), the same bytes in and out, no debounce,
// arbitration, decode or records.  Arguments as igdsp_ptt_arbitrate; the group state is not touched, the slots are stepped as by a
// launch, and sel / out / stats hold raw bytes (tick and ctl_out are not written).
int igdsp_internal_ptt_copy(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                            const uint16_t *d_len, const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members,
                            uint32_t n_members, const uint8_t *d_rxonly, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t release_frames,
                            igdsp_ptt_state *d_state, igdsp_ptt_slot *d_slots, int32_t *d_sel, igdsp_ptt_tick *d_tick, uint8_t *d_ctl_out,
                            int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return ptt_arbitrate(ctx, d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, d_rxonly, C, G, F, n,
                         release_frames, d_state, d_slots, d_sel, d_tick, d_ctl_out, d_out, d_stats, stream, true);
}

// ---- R2S link supervision and the device event list: the body of detectR2SPacketAndReconn (roip_ed137.cpp:1764-1780, :2009-2040) and
// the rtpAudio edge of transport_rtp_cb (TransportAdapter.cpp:286-315) ----
size_t igdsp_link_work_bytes(uint32_t n_channels, uint32_t n_ticks) { return (size_t)link_work_bytes(n_channels, n_ticks); }

// igdsp_link_watch, or with yardstick its compute-free twin igdsp_internal_link_copy
static int link_watch(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint16_t *d_sizes, const uint8_t *d_up, const uint16_t *d_period_ms,
                      uint32_t C, uint32_t T, uint32_t S, uint64_t t0_ms, uint32_t tick_ms, uint32_t miss_ticks, uint32_t event_mask,
                      igdsp_link_state *d_state, uint8_t *d_kind, igdsp_link_event *d_events, uint32_t event_cap, uint32_t *d_event_count,
                      void *d_work, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_link_watch", args::link_watch(d_info, d_sizes, d_up, d_period_ms, C, T, S, t0_ms, tick_ms, miss_ticks, event_mask, d_state, d_kind,
                                                       d_events, event_cap, d_event_count, d_work));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_link_watch(cfg_of(ctx, s), d_info, d_sizes, d_up, d_period_ms, C, T, S, t0_ms, tick_ms, miss_ticks, event_mask, d_state, d_kind,
                                   d_events, event_cap, d_event_count, d_work, yardstick, s));
    return IGDSP_OK;
}

int igdsp_link_watch(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint16_t *d_sizes, const uint8_t *d_up, const uint16_t *d_period_ms,
                     uint32_t n_channels, uint32_t n_ticks, uint32_t slots_per_tick, uint64_t t0_ms, uint32_t tick_ms, uint32_t miss_ticks,
                     uint32_t event_mask, igdsp_link_state *d_state, uint8_t *d_kind, igdsp_link_event *d_events, uint32_t event_cap,
                     uint32_t *d_event_count, void *d_work, void *stream)
{
    return link_watch(ctx, d_info, d_sizes, d_up, d_period_ms, n_channels, n_ticks, slots_per_tick, t0_ms, tick_ms, miss_ticks, event_mask, d_state,
                      d_kind, d_events, event_cap, d_event_count, d_work, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of igdsp_link_watch (tools/link_bench.py) — the same passes
// (count, scan and write with a list, one pass without), the same records and sizes read, the state stored as it was read, kind bytes
// of 0 and an empty list; no state machine.  Arguments as igdsp_link_watch.
int igdsp_internal_link_copy(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint16_t *d_sizes, const uint8_t *d_up, const uint16_t *d_period_ms,
                             uint32_t n_channels, uint32_t n_ticks, uint32_t slots_per_tick, uint64_t t0_ms, uint32_t tick_ms, uint32_t miss_ticks,
                             uint32_t event_mask, igdsp_link_state *d_state, uint8_t *d_kind, igdsp_link_event *d_events, uint32_t event_cap,
                             uint32_t *d_event_count, void *d_work, void *stream)
{
    return link_watch(ctx, d_info, d_sizes, d_up, d_period_ms, n_channels, n_ticks, slots_per_tick, t0_ms, tick_ms, miss_ticks, event_mask, d_state,
                      d_kind, d_events, event_cap, d_event_count, d_work, stream, true);
}

// ---- jitter buffer: the pjmedia stream behind adapter->stream_rtp_cb (TransportAdapter.cpp:301): RFC 3550 A.1 / A.3 / A.8 and playout ----
size_t igdsp_jb_ring_bytes(uint32_t n_channels, uint32_t samples_per_frame)
{
    if (samples_per_frame == 0 || samples_per_frame > IGDSP_MAX_PAYLOAD) return 0;
    return (size_t)jb_ring_bytes(n_channels, samples_per_frame);
}

int igdsp_jb_report(const igdsp_jb_state *s, igdsp_jb_prior *prior, igdsp_jb_rr *out)
{
    if (!s || !prior || !out) return IGDSP_EINVAL;
    *out = igdsp_jb_rr{};
    if (!(s->flags & IGDSP_JB_HEARD)) return IGDSP_OK;
    const uint32_t ext = s->cycles + s->max_seq;
    const uint32_t expected = ext - s->base_seq + 1u;
    const int64_t lost = (int64_t)expected - (int64_t)s->received;
    const bool same = prior->epoch == s->epoch;                                 // init_seq zeroes the priors
    const uint32_t exp_int = expected - (same ? prior->expected_prior : 0u), rec_int = s->received - (same ? prior->received_prior : 0u);
    const int64_t lost_int = (int64_t)exp_int - (int64_t)rec_int;
    out->ssrc = s->ssrc;
    out->ext_max_seq = ext;
    out->cum_lost = (int32_t)std::min<int64_t>(std::max<int64_t>(lost, -0x800000), 0x7FFFFF);
    out->jitter = s->jitter >> 4;
    out->fraction_lost = (exp_int == 0u || lost_int <= 0) ? 0u : (uint8_t)std::min<int64_t>((lost_int << 8) / exp_int, 255);
    out->valid = 1;
    prior->expected_prior = expected;
    prior->received_prior = s->received;
    prior->epoch = s->epoch;
    return IGDSP_OK;
}

void igdsp_jb_adapt_cfg_default(igdsp_jb_adapt_cfg *cfg)
{
    if (cfg) *cfg = args::jb_adapt_cfg_or_default(nullptr);
}

int igdsp_jb_adapt_next(const igdsp_jb_adapt_cfg *cfg, uint32_t jitter_q4, uint32_t samples_per_frame, igdsp_jb_adapt *a)
{
    const igdsp_jb_adapt_cfg c = args::jb_adapt_cfg_or_default(cfg);
    if (!a || !jb_adapt_cfg_ok(c) || samples_per_frame == 0 || samples_per_frame > IGDSP_MAX_PAYLOAD) return IGDSP_EINVAL;
    return (int)jb_adapt_start(c, jitter_q4, samples_per_frame, *a);
}

// igdsp_jb_receive, or with yardstick its compute-free twin igdsp_internal_jb_copy (which leaves d_pkt_status alone)
static int jb_receive(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_radio, const uint32_t *d_arrival,
                      uint32_t C, uint32_t T, uint32_t S, uint32_t stride, uint32_t n, uint32_t delay, igdsp_jb_state *d_state, void *d_ring,
                      uint8_t *d_payload, uint16_t *d_len, igdsp_rtp_info *d_info, uint8_t *d_tick_flags, uint8_t *d_pkt_status, void *stream,
                      bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_jb_receive", args::jb_receive(d_packets, d_sizes, d_radio, d_arrival, C, T, S, stride, n, delay, d_state, d_ring, d_payload, d_len,
                                                       d_info, d_tick_flags, d_pkt_status));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_jb_receive(cfg_of(ctx, s), d_packets, d_sizes, d_radio, d_arrival, C, T, S, stride, n, delay, d_state, d_ring, d_payload, d_len,
                                   d_info, d_tick_flags, yardstick ? nullptr : d_pkt_status, yardstick, s));
    return IGDSP_OK;
}

int igdsp_jb_receive(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_radio, const uint32_t *d_arrival,
                     uint32_t C, uint32_t T, uint32_t S, uint32_t pkt_stride, uint32_t n, uint32_t delay_frames, igdsp_jb_state *d_state,
                     void *d_ring, uint8_t *d_payload_out, uint16_t *d_len_out, igdsp_rtp_info *d_info_out, uint8_t *d_tick_flags,
                     uint8_t *d_pkt_status, void *stream)
{
    return jb_receive(ctx, d_packets, d_sizes, d_radio, d_arrival, C, T, S, pkt_stride, n, delay_frames, d_state, d_ring, d_payload_out, d_len_out,
                      d_info_out, d_tick_flags, d_pkt_status, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of igdsp_jb_receive (tools/jb_bench.py) — the rows of an
// in-order lossless launch (arrival slot 0 of every tick copied as igdsp_depayload would), with no header walk, state machine or ring
// store.  Arguments as igdsp_jb_receive; the state, the ring and d_pkt_status are not touched.
int igdsp_internal_jb_copy(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_radio, const uint32_t *d_arrival,
                           uint32_t C, uint32_t T, uint32_t S, uint32_t pkt_stride, uint32_t n, uint32_t delay_frames, igdsp_jb_state *d_state,
                           void *d_ring, uint8_t *d_payload_out, uint16_t *d_len_out, igdsp_rtp_info *d_info_out, uint8_t *d_tick_flags,
                           uint8_t *d_pkt_status, void *stream)
{
    return jb_receive(ctx, d_packets, d_sizes, d_radio, d_arrival, C, T, S, pkt_stride, n, delay_frames, d_state, d_ring, d_payload_out, d_len_out,
                      d_info_out, d_tick_flags, d_pkt_status, stream, true);
}

int igdsp_jb_receive_adaptive(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_radio, const uint32_t *d_arrival,
                              uint32_t C, uint32_t T, uint32_t S, uint32_t stride, uint32_t n, const igdsp_jb_adapt_cfg *cfg, igdsp_jb_state *d_state,
                              void *d_ring, igdsp_jb_adapt *d_adapt, uint8_t *d_payload, uint16_t *d_len, igdsp_rtp_info *d_info,
                              uint8_t *d_tick_flags, uint8_t *d_pkt_status, uint8_t *d_delay_out, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_jb_receive_adaptive", args::jb_receive_adaptive(d_packets, d_sizes, d_radio, d_arrival, C, T, S, stride, n, cfg, d_state, d_ring,
                                                                         d_adapt, d_payload, d_len, d_info, d_tick_flags, d_pkt_status, d_delay_out));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_jb_adaptive(cfg_of(ctx, s), d_packets, d_sizes, d_radio, d_arrival, C, T, S, stride, n, args::jb_adapt_cfg_or_default(cfg), d_state,
                                    d_ring, d_adapt, d_payload, d_len, d_info, d_tick_flags, d_pkt_status, d_delay_out, s));
    return IGDSP_OK;
}

// ---- packet loss concealment between the jitter buffer and the bridge (the pjmedia stream's PLC; G.711 Appendix I's structure) ----
// igdsp_plc_conceal, or with yardstick its compute-free twin igdsp_internal_plc_copy
static int plc_conceal(igdsp_ctx *ctx, const uint8_t *d_tick_flags, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                       const uint16_t *d_len, uint32_t C, uint32_t T, uint32_t n, igdsp_plc_state *d_state, int16_t *d_out, uint16_t *d_len_out,
                       igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_plc_conceal", args::plc_conceal(d_tick_flags, d_payload, d_codec, d_pcm, d_len, C, T, n, d_state, d_out, d_len_out, d_stats));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_plc_conceal(cfg_of(ctx, s), d_tick_flags, d_payload, d_codec, d_pcm, d_len, C, T, n, d_state, d_out, d_len_out, d_stats, yardstick, s));
    return IGDSP_OK;
}

int igdsp_plc_conceal(igdsp_ctx *ctx, const uint8_t *d_tick_flags, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                      const uint16_t *d_len, uint32_t C, uint32_t T, uint32_t n, igdsp_plc_state *d_state, int16_t *d_out, uint16_t *d_len_out,
                      igdsp_frame_stats *d_stats, void *stream)
{
    return plc_conceal(ctx, d_tick_flags, d_payload, d_codec, d_pcm, d_len, C, T, n, d_state, d_out, d_len_out, d_stats, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of igdsp_plc_conceal (tools/plc_bench.py) — the same
// traversal with every tick taken as PLAIN: the input bits widened to the output, no decode, pitch search, synthesis or stats (the
// records carry only the length); the state's ring and scalars are written.  Arguments as igdsp_plc_conceal.
int igdsp_internal_plc_copy(igdsp_ctx *ctx, const uint8_t *d_tick_flags, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                            const uint16_t *d_len, uint32_t C, uint32_t T, uint32_t n, igdsp_plc_state *d_state, int16_t *d_out,
                            uint16_t *d_len_out, igdsp_frame_stats *d_stats, void *stream)
{
    return plc_conceal(ctx, d_tick_flags, d_payload, d_codec, d_pcm, d_len, C, T, n, d_state, d_out, d_len_out, d_stats, stream, true);
}

// ---------------------------------------------------------------- byte streams
int igdsp_g726_reorder(igdsp_ctx *ctx, const uint8_t *d_in, uint8_t *d_out, uint64_t n_bytes, int mode, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_g726_reorder", args::g726_reorder(d_in, d_out, n_bytes, mode));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_g726(cfg_of(ctx, s), d_in, d_out, n_bytes, mode, s));
    return IGDSP_OK;
}

int igdsp_gen_uniform(igdsp_ctx *ctx, uint8_t *d_out, uint64_t n_bytes, uint64_t seed, uint64_t first_byte, void *stream)
{
    if (!ctx || (!d_out && n_bytes)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_gen_uniform(d_out, n_bytes, seed, first_byte, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_stream_read(igdsp_ctx *ctx, const void *d_src, size_t bytes, uint64_t *d_sink, void *stream)
{
    if (!ctx || !d_src || !d_sink || args::misaligned(16, {d_src})) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_stream_read(cfg_of(ctx, s), d_src, bytes, d_sink, s));
    return IGDSP_OK;
}

}  // extern "C"
