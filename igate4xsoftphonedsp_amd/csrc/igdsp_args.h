// igdsp_args.h — the argument rules of the batched C entries as plain host functions: no HIP, no context, no stream, so that
// tests/route/args_driver.cpp runs every rule with g++ alone (tests/test_args_cpu.py, from the table in tests/args_cases.py) and
// tests/test_gpu_args.py replays the same table through the library.
//
// One function per entry, taking the entry's own arguments with every pointer as const void *.  A pointer is only compared and
// masked, never dereferenced; the two host structs (igdsp_window, igdsp_jb_adapt_cfg) are read.  The order of the clauses is part of
// the contract: it decides which code wins when several apply (IGDSP_ERANGE against IGDSP_EINVAL) and which clauses still apply when
// there is nothing to do.  A yardstick twin (igdsp_internal_*_copy) takes its public entry's rule.
#pragma once
#include <cstdint>
#include <initializer_list>

#include "igdsp.h"
#include "igdsp_agc.h"
#include "igdsp_cng.h"
#include "igdsp_filt.h"
#include "igdsp_ns.h"
#include "igdsp_route.h"
#include "igdsp_vad.h"

namespace igdsp::args {

// run: launch.  !run && rc == IGDSP_OK: nothing to do.  why: the rule as igdsp_last_error shows it (behind the entry's name), or nullptr.
struct Verdict {
    int rc;
    bool run;
    const char *why;
};
constexpr Verdict kRun{IGDSP_OK, true, nullptr};
constexpr Verdict kNothing{IGDSP_OK, false, nullptr};
constexpr Verdict reject(int rc, const char *why = nullptr) { return Verdict{rc, false, why}; }
constexpr Verdict kInvalid{IGDSP_EINVAL, false, nullptr};

using P = const void *;

// ---- the helpers every rule is made of
inline bool any_null(std::initializer_list<P> ps)
{
    for (P p : ps) if (!p) return true;
    return false;
}
// one of ps is not a multiple of k (a power of two); NULL is aligned to everything, so optional buffers go in as they are
inline bool misaligned(uintptr_t k, std::initializer_list<P> ps)
{
    uintptr_t a = 0;
    for (P p : ps) a |= reinterpret_cast<uintptr_t>(p);
    return (a & (k - 1)) != 0;
}
constexpr bool exactly_one(P a, P b) { return (a == nullptr) != (b == nullptr); }
constexpr bool at_most_one(P a, P b) { return !(a && b); }
constexpr bool empty(uint32_t a, uint32_t b) { return (uint64_t)a * b == 0; }
constexpr bool lineage_ok(int variant) { return variant == IGDSP_ENC_SUN16 || variant == IGDSP_ENC_G191; }
// packet slots: at least `floor` bytes (the header, or the header and what the entry reads behind it), dword-granular (so header
// words and payload dwords are aligned), at most `cap`
constexpr bool stride_ok(uint32_t stride, uint32_t floor, uint32_t cap = 2048u) { return stride >= floor && !(stride & 3u) && stride <= cap; }
// C channels x F frames (or ticks) of n samples: frame indices are 32-bit on the device
constexpr int check_shape(uint32_t C, uint32_t F, uint32_t n)
{
    if (n == 0 || n > IGDSP_MAX_PAYLOAD) return IGDSP_EINVAL;
    if ((uint64_t)C * F >= 0xFFFFFFE0ull) return IGDSP_ERANGE;
    return IGDSP_OK;
}
// C channels x T ticks x S arrival slots: slot indices and counts are 32-bit on the device
constexpr bool slots_fit(uint32_t C, uint32_t T, uint32_t S) { return (uint64_t)C * T * S < 0xFFFFFFE0ull; }
constexpr bool slots_per_tick_ok(uint32_t S) { return S != 0 && S <= IGDSP_STAGE_DEPTH; }
constexpr bool hdr_ok(uint32_t hdr_bytes) { return hdr_bytes == 12u || hdr_bytes == 20u; }

constexpr igdsp_jb_adapt_cfg jb_adapt_cfg_or_default(const igdsp_jb_adapt_cfg *cfg)
{
    return cfg ? *cfg
               : igdsp_jb_adapt_cfg{IGDSP_JB_ADAPT_MIN, IGDSP_JB_ADAPT_MAX, IGDSP_JB_DELAY, IGDSP_JB_ADAPT_MULT, IGDSP_JB_ADAPT_LATE_RESTART, {0, 0, 0}};
}

// ---- payload entries
inline Verdict decode_meter(P d_payload, P d_codec, P, uint32_t C, uint32_t F, uint32_t n, P d_stats, P, P, uint32_t rank)
{
    if (empty(C, F)) return kNothing;
    if (any_null({d_payload, d_codec, d_stats})) return kInvalid;
    if (int rc = check_shape(C, F, n)) return reject(rc);
    if (rank >= IGDSP_AGG_MAX_RANKS) return kInvalid;
    return kRun;
}

inline Verdict encode(P d_pcm, P d_codec, uint32_t C, uint32_t F, uint32_t n, P d_out, int variant)
{
    if (empty(C, F)) return kNothing;
    if (any_null({d_pcm, d_codec, d_out}) || !lineage_ok(variant)) return kInvalid;
    if (int rc = check_shape(C, F, n)) return reject(rc);
    return kRun;
}

inline Verdict roundtrip_peakhold(P d_payload, P d_codec, uint32_t C, uint32_t F, uint32_t n, P d_out, P d_stats, P d_hold, P, int variant)
{
    if (empty(C, F)) return kNothing;
    if (any_null({d_payload, d_codec, d_out, d_stats, d_hold}) || !lineage_ok(variant)) return kInvalid;
    if (int rc = check_shape(C, F, n)) return reject(rc);
    if (misaligned(8, {d_stats, d_hold})) return kInvalid;                                   // natural struct alignment
    return kRun;
}

inline Verdict hold_update(P d_stats, uint32_t C, uint32_t F, uint32_t n, P d_hold, P)
{
    if (empty(C, F)) return kNothing;
    if (any_null({d_stats, d_hold})) return kInvalid;
    if (int rc = check_shape(C, F, n)) return reject(rc);
    return kRun;
}

inline Verdict depayload(P d_packets, P, P d_radio, uint32_t C, uint32_t F, uint32_t pkt_stride, uint32_t n, P d_payload_out, P d_len_out,
                         P d_info_out)
{
    if (empty(C, F)) return kNothing;
    if (any_null({d_packets, d_radio, d_payload_out, d_len_out, d_info_out})) return kInvalid;
    if (int rc = check_shape(C, F, n)) return reject(rc);
    if (!stride_ok(pkt_stride, 20u) || misaligned(4, {d_packets})) return kInvalid;
    return kRun;
}

// ---- the fused packet entries.  What follows the range check is one rule for igdsp_decode_meter_rtp (IGDSP_PKT_SLOTS),
// igdsp_decode_meter_packets (PACKED), igdsp_decode_meter_packets_mixed (MIXED) and igdsp_decode_meter_window (any of the three):
// 16-byte aligned 180-byte slots, or dword-aligned packets at a stride that holds the header the layout reads and 160 samples, whose
// dword offsets stay 32-bit; whole super-chunks of 64 frames; naturally aligned records.  Other shapes take the two-step route
// (igdsp_depayload + igdsp_decode_meter): rejected rather than silently re-routed.
inline Verdict packet_layout(uint32_t layout, P d_packets, P d_sizes, uint32_t C, uint32_t F, uint32_t pkt_stride, uint32_t hdr_bytes, P d_stats,
                             P d_info)
{
    if (layout == IGDSP_PKT_SLOTS) {
        if (misaligned(16, {d_packets})) return reject(IGDSP_EINVAL, "slots need 16-byte alignment");
    } else {
        if (layout == IGDSP_PKT_PACKED && !hdr_ok(hdr_bytes)) return kInvalid;
        const uint32_t floor = (layout == IGDSP_PKT_MIXED ? 20u : hdr_bytes) + IGDSP_SAMPLES_PER_FRAME;
        if (!stride_ok(pkt_stride, floor) || (uint64_t)C * F * pkt_stride > 0xFFFFFFFFull * 4ull) return kInvalid;
        if (misaligned(4, {d_packets}) || misaligned(2, {d_sizes})) return reject(IGDSP_EINVAL, "needs dword-aligned packets, 2-byte aligned sizes");
    }
    if (((uint64_t)C * F) % 64u || misaligned(16, {d_stats}) || misaligned(8, {d_info}))
        return reject(IGDSP_EINVAL, "needs C*F % 64 == 0, 16-byte aligned stats, 8-byte aligned info");
    return kRun;
}

inline Verdict decode_meter_rtp(P d_slots, P d_codec, uint32_t C, uint32_t F, P d_stats, P d_info, P, uint32_t rank)
{
    if (empty(C, F)) return kNothing;
    if (any_null({d_slots, d_codec, d_stats}) || rank >= IGDSP_AGG_MAX_RANKS) return kInvalid;
    if (int rc = check_shape(C, F, IGDSP_SAMPLES_PER_FRAME)) return reject(rc);
    return packet_layout(IGDSP_PKT_SLOTS, d_slots, nullptr, C, F, 0, 20, d_stats, d_info);
}

inline Verdict decode_meter_packets(P d_packets, P d_sizes, P d_codec, uint32_t C, uint32_t F, uint32_t pkt_stride, uint32_t hdr_bytes, P d_stats,
                                    P d_info, P, uint32_t rank)
{
    if (empty(C, F)) return kNothing;
    if (any_null({d_packets, d_codec, d_stats}) || rank >= IGDSP_AGG_MAX_RANKS) return kInvalid;
    if (!hdr_ok(hdr_bytes)) return kInvalid;                                                 // here ahead of the range check
    if (int rc = check_shape(C, F, IGDSP_SAMPLES_PER_FRAME)) return reject(rc);
    return packet_layout(IGDSP_PKT_PACKED, d_packets, d_sizes, C, F, pkt_stride, hdr_bytes, d_stats, d_info);
}

inline Verdict decode_meter_packets_mixed(P d_packets, P d_sizes, P d_codec, P d_radio, uint32_t C, uint32_t F, uint32_t pkt_stride, P d_stats,
                                          P d_info, P, uint32_t rank)
{
    if (empty(C, F)) return kNothing;
    if (any_null({d_packets, d_codec, d_radio, d_stats}) || rank >= IGDSP_AGG_MAX_RANKS) return kInvalid;
    if (int rc = check_shape(C, F, IGDSP_SAMPLES_PER_FRAME)) return reject(rc);
    return packet_layout(IGDSP_PKT_MIXED, d_packets, d_sizes, C, F, pkt_stride, 12, d_stats, d_info);
}

// ---- ED-137 gated window.  The window is checked ahead of the nothing-to-do return.
inline Verdict window(const igdsp_window *win)
{
    if (!win || !win->d_hold || win->gate_mode > IGDSP_GATE_SQU_OR_PTT) return kInvalid;
    if (misaligned(8, {win->d_hold}) || misaligned(4, {win->d_probe}) || misaligned(16, {win->d_work}))
        return reject(IGDSP_EINVAL, "igdsp_window: d_hold 8-byte, d_probe 4-byte, d_work 16-byte aligned");
    return kRun;
}

inline Verdict window_update(P d_stats, P, P, uint32_t C, uint32_t F, uint32_t n, const igdsp_window *win)
{
    if (const Verdict v = window(win); !v.run) return v;
    if (empty(C, F)) return kNothing;
    if (!d_stats) return kInvalid;
    if (int rc = check_shape(C, F, n)) return reject(rc);
    return kRun;
}

// the fused path of igdsp_decode_meter_window: whole groups of 64 channels and a window with d_work (only read once the window passed)
inline bool window_fused(uint32_t C, const igdsp_window *win) { return C % 64u == 0u && win->d_work != nullptr; }

inline Verdict decode_meter_window(uint32_t layout, P d_packets, P d_sizes, P d_codec, P d_radio, uint32_t C, uint32_t F, uint32_t pkt_stride,
                                   uint32_t hdr_bytes, P d_stats, P d_info, P, uint32_t rank, const igdsp_window *win)
{
    if (layout > IGDSP_PKT_MIXED) return kInvalid;
    if (const Verdict v = window(win); !v.run) return v;
    if (empty(C, F)) return kNothing;
    if (any_null({d_packets, d_codec}) || rank >= IGDSP_AGG_MAX_RANKS) return kInvalid;
    if (layout == IGDSP_PKT_MIXED && !d_radio) return kInvalid;
    const bool fused = window_fused(C, win);
    if (!d_stats && !fused) return reject(IGDSP_EINVAL, "d_stats may only be NULL on the fused path (n_channels % 64 == 0, d_work given)");
    if (int rc = check_shape(C, F, IGDSP_SAMPLES_PER_FRAME)) return reject(rc);
    if (const Verdict v = packet_layout(layout, d_packets, d_sizes, C, F, pkt_stride, hdr_bytes, d_stats, d_info); !v.run) return v;
    if (!d_info && !fused) return reject(IGDSP_EINVAL, "channel counts that are not multiples of 64 (or a window without d_work) need d_info");
    return kRun;
}

inline Verdict wav_expand(P d_payload, uint32_t C, uint32_t F, uint32_t n, uint32_t, P d_files, uint64_t file_stride)
{
    if (empty(C, F)) return kNothing;
    if (any_null({d_payload, d_files})) return kInvalid;
    if (int rc = check_shape(C, F, n)) return reject(rc);
    if (file_stride < 44ull + 2ull * F * n || 2ull * F * n > 0xFFFFFFFFull - 36ull) return kInvalid;   // the header's sizes are 32-bit
    return kRun;
}

// ---- ED-137 TX packetizer
inline Verdict tx_packetize(P d_pcm, P d_g711, P, uint32_t C, uint32_t F, uint32_t n, uint64_t, uint32_t, P d_state, P d_last_payload, P d_packets,
                            uint32_t pkt_stride, P d_sizes, P d_info, int variant)
{
    if (empty(C, F)) return kNothing;
    if (!exactly_one(d_pcm, d_g711)) return kInvalid;
    if (any_null({d_state, d_last_payload, d_packets, d_sizes, d_info})) return kInvalid;
    if (d_pcm && !lineage_ok(variant)) return kInvalid;
    if (int rc = check_shape(C, F, n)) return reject(rc);
    if (!stride_ok(pkt_stride, 20u + n) || misaligned(4, {d_packets})) return kInvalid;
    if (misaligned(8, {d_state}) || misaligned(4, {d_info}) || misaligned(2, {d_sizes, d_pcm})) return kInvalid;
    if ((uint64_t)F * n >= 0x80000000ull) return reject(IGDSP_ERANGE);                         // ts + f * n and frame indices stay 32-bit
    return kRun;
}

// igdsp_internal_tx_copy: every clause ahead of the nothing-to-do return; n % 4 == 0; no upper bound on the stride
inline Verdict tx_copy(P d_pcm, P d_g711, uint32_t C, uint32_t F, uint32_t n, P d_packets, uint32_t pkt_stride)
{
    if (!exactly_one(d_pcm, d_g711) || !d_packets || (n & 3u) || n == 0 || n > IGDSP_MAX_PAYLOAD || !stride_ok(pkt_stride, 20u + n, 0xFFFFFFFFu) ||
        misaligned(4, {d_packets, d_g711}) || misaligned(8, {d_pcm}))
        return kInvalid;
    if (empty(C, F)) return kNothing;
    if (int rc = check_shape(C, F, n)) return reject(rc);
    return kRun;
}

inline Verdict g726_reorder(P d_in, P d_out, uint64_t n_bytes, int mode)
{
    if (mode < 1 || mode > 4) return kInvalid;
    if (n_bytes == 0) return kNothing;
    if (any_null({d_in, d_out})) return kInvalid;
    if (n_bytes % (mode == 2 ? 3u : mode == 4 ? 5u : 1u)) return kInvalid;                     // the reference over-reads on partial groups
    return kRun;
}

// ---- conference mix
inline Verdict conf_mix(P d_payload, P d_codec, P d_pcm, P d_len, P d_gain, P d_port_ptr, P d_members, uint32_t n_members, uint32_t C, uint32_t P_,
                        uint32_t F, uint32_t n, P d_out, P d_stats)
{
    if (empty(P_, F)) return kNothing;                                                       // nothing to write
    if (!exactly_one(d_payload, d_pcm) || (d_payload && !d_codec)) return kInvalid;
    if (!d_out && !d_stats) return kInvalid;
    if (any_null({d_gain, d_port_ptr}) || (n_members && !d_members)) return kInvalid;
    if (int rc = check_shape(C, F, n)) return reject(rc);
    if (int rc = check_shape(P_, F, n)) return reject(rc);
    if (misaligned(2, {d_pcm, d_len, d_gain, d_out}) || misaligned(4, {d_port_ptr, d_members}) || misaligned(8, {d_stats})) return kInvalid;
    return kRun;
}

// ---- the vote (igdsp_bss_select) and the arbiter (igdsp_ptt_arbitrate): C channels in G groups of members with a per-member record
// (d_per_member: the vote's words, the arbiter's slots), optional audio in at most one form, optional outputs per group.  d_more: the
// entry's further 4-byte aligned outputs.
inline Verdict group_audio(P d_info, P d_payload, P d_codec, P d_pcm, P d_len, P d_gain, P d_group_ptr, P d_members, uint32_t n_members, uint32_t C,
                           uint32_t G, uint32_t F, uint32_t n, P d_state, P d_per_member, P d_sel, P d_more, P d_out, P d_stats)
{
    if (any_null({d_info, d_group_ptr, d_state})) return kInvalid;
    if (n_members && (!d_members || !d_per_member)) return kInvalid;
    if (n_members > (1u << 24)) return kInvalid;                                             // positions are 24-bit in the vote key
    if (!at_most_one(d_payload, d_pcm)) return kInvalid;
    if (d_payload && !d_codec) return kInvalid;
    if ((d_out || d_stats) && !d_payload && !d_pcm) return kInvalid;                         // audio outputs need audio
    if (int rc = check_shape(C, F, n)) return reject(rc);
    if (int rc = check_shape(G, F, n)) return reject(rc);
    if (misaligned(2, {d_pcm, d_len, d_gain, d_out}) || misaligned(4, {d_info, d_group_ptr, d_members, d_state, d_per_member, d_sel, d_more}) ||
        misaligned(8, {d_stats}))
        return kInvalid;
    return kRun;
}

inline Verdict bss_select(P d_info, P d_payload, P d_codec, P d_pcm, P d_len, P d_gain, P d_group_ptr, P d_members, uint32_t n_members, P,
                          uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t, P d_state, P d_words, P d_sel, P d_out, P d_stats)
{
    if (empty(G, F)) return kNothing;
    return group_audio(d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, C, G, F, n, d_state, d_words, d_sel,
                       nullptr, d_out, d_stats);
}

inline Verdict ptt_arbitrate(P d_info, P d_payload, P d_codec, P d_pcm, P d_len, P d_gain, P d_group_ptr, P d_members, uint32_t n_members, P,
                             uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t release_frames, P d_state, P d_slots, P d_sel, P d_tick, P,
                             P d_out, P d_stats)
{
    if (n == 0 || n > IGDSP_MAX_PAYLOAD || n_members > (1u << 24) || release_frames > 255u) return kInvalid;   // always checked
    if (empty(G, F)) return kNothing;
    return group_audio(d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, C, G, F, n, d_state, d_slots, d_sel,
                       d_tick, d_out, d_stats);
}

// ---- R2S link supervision.  Everything but the two work-dependent clauses is checked whether or not there is work; a launch with an
// event list and no work still runs (it writes the two counts).
inline Verdict link_watch(P d_info, P d_sizes, P, P d_period_ms, uint32_t C, uint32_t T, uint32_t S, uint64_t, uint32_t tick_ms, uint32_t miss_ticks,
                          uint32_t, P d_state, P, P d_events, uint32_t event_cap, P d_event_count, P d_work)
{
    if (!slots_per_tick_ok(S) || tick_ms == 0 || miss_ticks > 65535u) return kInvalid;
    if (!d_events && event_cap) return kInvalid;
    const bool list = d_event_count != nullptr;
    if (list && (!d_work || misaligned(16, {d_work}))) return kInvalid;
    if (misaligned(2, {d_sizes, d_period_ms}) || misaligned(4, {d_info, d_events, d_event_count}) || misaligned(8, {d_state})) return kInvalid;
    const bool work = !empty(C, T);
    if (work && any_null({d_info, d_state})) return kInvalid;
    if (!slots_fit(C, T, S)) return reject(IGDSP_ERANGE);                                     // list indices and counts are 32-bit
    return work || list ? kRun : kNothing;
}

// ---- jitter buffer: one rule for igdsp_jb_receive (a fixed delay) and igdsp_jb_receive_adaptive (a cfg, NULL = the defaults, and a
// per-channel d_adapt)
inline Verdict jb_rule(P d_packets, P d_sizes, P d_radio, P d_arrival, uint32_t C, uint32_t T, uint32_t S, uint32_t pkt_stride, uint32_t n,
                       bool adaptive, uint32_t delay_frames, const igdsp_jb_adapt_cfg *cfg, P d_state, P d_ring, P d_adapt, P d_payload, P d_len,
                       P d_info)
{
    if (empty(C, T)) return kNothing;
    if (any_null({d_packets, d_radio, d_state, d_ring, d_payload, d_len, d_info}) || (adaptive && !d_adapt)) return kInvalid;
    const bool delay_ok = adaptive ? jb_adapt_cfg_ok(jb_adapt_cfg_or_default(cfg)) : delay_frames < IGDSP_JB_DEPTH;
    if (!slots_per_tick_ok(S) || !delay_ok) return kInvalid;
    if (!stride_ok(pkt_stride, 20u)) return kInvalid;
    if (int rc = check_shape(C, T, n)) return reject(rc);
    if (!slots_fit(C, T, S)) return reject(IGDSP_ERANGE);
    if (misaligned(2, {d_sizes, d_len}) || misaligned(4, {d_packets, d_arrival, d_state, d_adapt}) || misaligned(8, {d_info}) ||
        misaligned(16, {d_ring}))
        return kInvalid;
    return kRun;
}

inline Verdict jb_receive(P d_packets, P d_sizes, P d_radio, P d_arrival, uint32_t C, uint32_t T, uint32_t S, uint32_t pkt_stride, uint32_t n,
                          uint32_t delay_frames, P d_state, P d_ring, P d_payload, P d_len, P d_info, P, P)
{
    return jb_rule(d_packets, d_sizes, d_radio, d_arrival, C, T, S, pkt_stride, n, false, delay_frames, nullptr, d_state, d_ring, nullptr, d_payload,
                   d_len, d_info);
}

inline Verdict jb_receive_adaptive(P d_packets, P d_sizes, P d_radio, P d_arrival, uint32_t C, uint32_t T, uint32_t S, uint32_t pkt_stride, uint32_t n,
                                   const igdsp_jb_adapt_cfg *cfg, P d_state, P d_ring, P d_adapt, P d_payload, P d_len, P d_info, P, P, P)
{
    return jb_rule(d_packets, d_sizes, d_radio, d_arrival, C, T, S, pkt_stride, n, true, 0, cfg, d_state, d_ring, d_adapt, d_payload, d_len, d_info);
}

// ---- packet loss concealment
inline Verdict plc_conceal(P d_tick_flags, P d_payload, P d_codec, P d_pcm, P d_len, uint32_t C, uint32_t T, uint32_t n, P d_state, P d_out,
                           P d_len_out, P d_stats)
{
    if (empty(C, T)) return kNothing;
    if (any_null({d_tick_flags, d_state, d_out})) return kInvalid;
    if (!exactly_one(d_payload, d_pcm) || (d_payload && !d_codec)) return kInvalid;
    if (int rc = check_shape(C, T, n)) return reject(rc);
    if (misaligned(2, {d_pcm, d_len, d_out, d_len_out}) || misaligned(4, {d_state}) || misaligned(8, {d_stats})) return kInvalid;
    return kRun;
}

// ---- sound-card splitter / combiner: one rule for both directions (d_in, d_bulk: d_pcm and d_frames in the entry's direction)
inline Verdict snd_rule(P d_in, uint32_t D, uint32_t K, uint32_t F, uint32_t n, P d_bulk, P d_stats)
{
    if (empty(D, F)) return kNothing;
    if (!d_in || (!d_bulk && !d_stats)) return kInvalid;
    if (K == 0 || K > IGDSP_SND_MAX_CHANNELS) return kInvalid;
    // check_shape(D * K, F, n) with the row count D * K taken in 64 bits (< 2^35, so the product with F is taken only where it fits)
    if (n == 0 || n > IGDSP_MAX_PAYLOAD) return kInvalid;
    const uint64_t rows = (uint64_t)D * K;
    if (rows >= 0xFFFFFFE0ull || rows * F >= 0xFFFFFFE0ull) return reject(IGDSP_ERANGE);
    if (misaligned(2, {d_in, d_bulk}) || misaligned(8, {d_stats})) return kInvalid;
    if (d_in == d_bulk) return reject(IGDSP_EINVAL, "the output must not be the input");
    return kRun;
}

inline Verdict snd_combine(P d_pcm, uint32_t D, uint32_t K, uint32_t F, uint32_t n, P d_frames, P d_stats)
{
    return snd_rule(d_pcm, D, K, F, n, d_frames, d_stats);
}

inline Verdict snd_split(P d_frames, uint32_t D, uint32_t K, uint32_t F, uint32_t n, P d_pcm, P d_stats)
{
    return snd_rule(d_frames, D, K, F, n, d_pcm, d_stats);
}

// ---- tone generator (rows_per_frame 0 = n_ports; the rows of a frame that count are the larger of the two)
inline Verdict tone_generate(P d_plans, uint32_t n_plans, P d_plan_of, P d_cmd, P d_state, uint32_t ports, uint32_t F, uint32_t n,
                             uint32_t rows_per_frame, P d_pcm, P d_len, P d_stats)
{
    if (empty(ports, F)) return kNothing;
    if (any_null({d_plans, d_state}) || n_plans == 0 || (!d_pcm && !d_stats)) return kInvalid;
    if (rows_per_frame != 0 && rows_per_frame < ports) return kInvalid;
    if (int rc = check_shape(rows_per_frame ? rows_per_frame : ports, F, n)) return reject(rc);
    if (misaligned(2, {d_pcm, d_len, d_plan_of}) || misaligned(4, {d_plans, d_state}) || misaligned(8, {d_stats})) return kInvalid;
    for (P out : {d_pcm, d_len, d_stats})
        for (P in : {d_plans, d_plan_of, d_cmd, d_state})
            if (out && out == in) return reject(IGDSP_EINVAL, "an output must not be an input or the state");
    return kRun;
}

// ---- rate converter.  The direction, the factor and the layout are checked whether or not there is work.  rows_narrow / rows_wide
// 0 = n_channels; the rows that count on a side are its stride times its frames (n_frames, times the factor for a wide side in sub-frames)
inline Verdict resample(uint32_t dir, uint32_t factor, uint32_t layout, P d_payload, P d_codec, P d_pcm, P d_len, P d_state, uint32_t C, uint32_t F,
                        uint32_t n, uint32_t rows_narrow, uint32_t rows_wide, P d_out, P d_stats)
{
    if (!rs_dir_ok(dir) || !rs_factor_ok(factor) || layout > IGDSP_RS_SUBFRAMES) return kInvalid;
    if (empty(C, F)) return kNothing;
    if (dir == IGDSP_RS_UP ? (!exactly_one(d_payload, d_pcm) || (d_payload && !d_codec)) : (!d_pcm || d_payload)) return kInvalid;
    if (!d_state || (!d_out && !d_stats)) return kInvalid;
    if ((rows_narrow != 0 && rows_narrow < C) || (rows_wide != 0 && rows_wide < C)) return kInvalid;
    if (n == 0 || n > IGDSP_MAX_PAYLOAD) return kInvalid;
    const uint64_t wide_frames = (uint64_t)F * (layout == IGDSP_RS_SUBFRAMES ? factor : 1u);
    if ((uint64_t)(rows_narrow ? rows_narrow : C) * F >= 0xFFFFFFE0ull || (uint64_t)(rows_wide ? rows_wide : C) * wide_frames >= 0xFFFFFFE0ull)
        return reject(IGDSP_ERANGE);
    if (misaligned(2, {d_pcm, d_len, d_out}) || misaligned(4, {d_state}) || misaligned(8, {d_stats})) return kInvalid;
    for (P out : {d_out, d_stats})
        for (P in : {d_payload, d_codec, d_pcm, d_len, d_state})
            if (out && out == in) return reject(IGDSP_EINVAL, "an output must not be an input or the state");
    return kRun;
}

// ---- delay buffer.  The frame and the maximum are checked whether or not there is work.  The buffers' extents are known from the
// shape, so "no output may overlap" is a test of byte ranges: every output against every input, the state and every other output
inline bool ranges_overlap(P a, uint64_t a_bytes, P b, uint64_t b_bytes)
{
    const uint64_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + b_bytes && y < x + a_bytes;
}
inline Verdict dbuf_run(P d_ops, P d_in, uint32_t C, uint32_t T, uint32_t n, uint32_t M, P d_state, P d_out, P d_flags_out, P d_len_out, P d_fill,
                        P d_stats)
{
    if (n == 0 || n > IGDSP_MAX_PAYLOAD || M < 2u * n || M > IGDSP_DBUF_CAP) return kInvalid;
    if (empty(C, T)) return kNothing;
    if (any_null({d_ops, d_in, d_state, d_out})) return kInvalid;
    if ((uint64_t)C * T >= 0xFFFFFFE0ull) return reject(IGDSP_ERANGE);
    if (misaligned(2, {d_in, d_out, d_len_out, d_fill}) || misaligned(4, {d_state}) || misaligned(8, {d_stats})) return kInvalid;
    const uint64_t steps = (uint64_t)C * T;
    struct Buf { P p; uint64_t bytes; };
    const Buf ins[3] = {{d_ops, steps}, {d_in, steps * n * 2u}, {d_state, (uint64_t)C * sizeof(igdsp_dbuf_state)}};
    const Buf outs[5] = {{d_out, steps * n * 2u}, {d_flags_out, steps}, {d_len_out, steps * 2u}, {d_fill, steps * 2u}, {d_stats, steps * 16u}};
    for (int i = 0; i < 5; ++i) {
        for (const Buf &b : ins)
            if (ranges_overlap(outs[i].p, outs[i].bytes, b.p, b.bytes)) return reject(IGDSP_EINVAL, "an output must not overlap an input or the state");
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes)) return reject(IGDSP_EINVAL, "two outputs must not overlap");
    }
    return kRun;
}

// ---- spectrum.  The frame and the cfg (NULL = the defaults) are checked whether or not there is work.  The state is read and written:
// like the outputs it may overlap neither an input nor an output
constexpr bool spec_cfg_ok(const igdsp_spec_cfg *cfg)
{
    return !cfg || (cfg->hop_frames >= 1u && cfg->alpha > 0.0f && cfg->alpha <= 1.0f);        // (a NaN alpha fails)
}
inline Verdict spec_run(P d_g711, P d_codec, P d_pcm, uint32_t C, uint32_t F, uint32_t n, const igdsp_spec_cfg *cfg, P d_state, P d_rec, P d_avg,
                        P d_raw)
{
    if (n == 0 || n > IGDSP_MAX_PAYLOAD || !spec_cfg_ok(cfg)) return kInvalid;
    if (empty(C, F)) return kNothing;
    if (!exactly_one(d_g711, d_pcm) || (d_g711 && !d_codec) || !d_state) return kInvalid;
    if ((uint64_t)C * F >= 0xFFFFFFE0ull) return reject(IGDSP_ERANGE);
    if (misaligned(2, {d_pcm}) || misaligned(4, {d_state, d_avg, d_raw}) || misaligned(8, {d_rec})) return kInvalid;
    const uint64_t frames = (uint64_t)C * F;
    struct Buf { P p; uint64_t bytes; };
    const Buf ins[3] = {{d_g711, frames * n}, {d_g711 ? d_codec : nullptr, C}, {d_pcm, frames * n * 2u}};
    const Buf outs[4] = {{d_state, (uint64_t)C * sizeof(igdsp_spec_state)}, {d_rec, frames * sizeof(igdsp_spec_rec)},
                         {d_avg, (uint64_t)C * IGDSP_SPEC_BINS * 4u}, {d_raw, (uint64_t)C * IGDSP_SPEC_BINS * 4u}};
    for (int i = 0; i < 4; ++i) {
        for (const Buf &b : ins)
            if (ranges_overlap(outs[i].p, outs[i].bytes, b.p, b.bytes)) return reject(IGDSP_EINVAL, "the state and the outputs must not overlap an input");
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return reject(IGDSP_EINVAL, "the state and the outputs must not overlap each other");
    }
    return kRun;
}

// ---- tone detector.  The frame length is checked whether or not there is work.  Nothing to do with a list still writes the counts, so
// d_event_count's own rules apply before the shape's
inline Verdict tdet_run(P d_g711, P d_codec, P d_pcm, P d_plans, uint32_t n_plans, P d_plan_of, uint32_t C, uint32_t F, uint32_t n, P d_state,
                        P d_rec, P d_events, uint32_t event_cap, P d_event_count, P d_work)
{
    if (n < 2u || n > IGDSP_MAX_PAYLOAD || (n & 1u)) return kInvalid;
    if (misaligned(4, {d_event_count}) || misaligned(16, {d_work}) || (d_event_count && !d_work)) return kInvalid;
    if (d_event_count && event_cap != 0u && !d_events) return kInvalid;
    if (empty(C, F)) return d_event_count ? kRun : kNothing;              // the counts are written as 0
    if (!exactly_one(d_g711, d_pcm) || (d_g711 && !d_codec) || !d_state || !d_plans || n_plans == 0u) return kInvalid;
    if ((uint64_t)C * F >= 0xFFFFFFE0ull) return reject(IGDSP_ERANGE);
    // the kernel reads a row two samples at a time (n is even, so every row starts as the buffer does) and stores an event as 16 bytes
    if (misaligned(2, {d_g711, d_plan_of}) || misaligned(4, {d_pcm, d_plans, d_state}) || misaligned(8, {d_rec}) || misaligned(16, {d_events})) return kInvalid;
    const uint64_t frames = (uint64_t)C * F;
    const bool list = d_event_count != nullptr;
    struct Buf { P p; uint64_t bytes; };
    const Buf ins[5] = {{d_g711, frames * n}, {d_g711 ? d_codec : nullptr, C}, {d_pcm, frames * n * 2u},
                        {d_plans, (uint64_t)n_plans * sizeof(igdsp_tdet_plan)}, {d_plan_of, (uint64_t)C * 2u}};
    const Buf outs[5] = {{d_state, (uint64_t)C * sizeof(igdsp_tdet_state)}, {d_rec, frames * sizeof(igdsp_tdet_rec)},
                         {list ? d_events : nullptr, (uint64_t)event_cap * sizeof(igdsp_tdet_event)}, {d_event_count, 8u},
                         {list ? d_work : nullptr, tdet_work_bytes(C, F, d_rec != nullptr)}};
    for (int i = 0; i < 5; ++i) {
        for (const Buf &b : ins)
            if (ranges_overlap(outs[i].p, outs[i].bytes, b.p, b.bytes)) return reject(IGDSP_EINVAL, "the state and the outputs must not overlap an input");
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return reject(IGDSP_EINVAL, "the state and the outputs must not overlap each other");
    }
    return kRun;
}

// ---- echo canceller.  The frame length and the cfg (NULL = the defaults) are checked whether or not there is work
constexpr bool ec_cfg_ok(const igdsp_ec_cfg *cfg) { return !cfg || ((cfg->tail == 128u || cfg->tail == 256u) && cfg->mu_shift <= 6u); }
inline Verdict ec_run(P d_near_g711, P d_codec, P d_near_pcm, P d_far_pcm, uint32_t n_far, P d_far_of, P d_ctl, const igdsp_ec_cfg *cfg, uint32_t C,
                      uint32_t F, uint32_t n, P d_state, P d_out, P d_rec, P d_stats)
{
    if (n < 2u || n > IGDSP_MAX_PAYLOAD || (n & 1u) || !ec_cfg_ok(cfg)) return kInvalid;
    if (empty(C, F)) return kNothing;
    if (!exactly_one(d_near_g711, d_near_pcm) || (d_near_g711 && !d_codec) || !d_state || (n_far != 0u && !d_far_pcm)) return kInvalid;
    if ((uint64_t)C * F >= 0xFFFFFFE0ull || (uint64_t)n_far * F >= 0xFFFFFFE0ull) return reject(IGDSP_ERANGE);
    // rows are read and stored two samples at a time (n is even, so every row starts as its buffer does), weights and records as 16 bytes
    if (misaligned(2, {d_near_g711}) || misaligned(4, {d_near_pcm, d_far_pcm, d_far_of, d_out}) || misaligned(8, {d_stats}) ||
        misaligned(16, {d_state, d_rec})) return kInvalid;
    const uint64_t frames = (uint64_t)C * F;
    struct Buf { P p; uint64_t bytes; };
    const Buf ins[6] = {{d_near_g711, frames * n}, {d_near_g711 ? d_codec : nullptr, C}, {d_near_pcm, frames * n * 2u},
                        {d_far_pcm, (uint64_t)n_far * F * n * 2u}, {d_far_of, (uint64_t)C * 4u}, {d_ctl, C}};
    const Buf outs[4] = {{d_state, (uint64_t)C * sizeof(igdsp_ec_state)}, {d_out, frames * n * 2u}, {d_rec, frames * sizeof(igdsp_ec_rec)},
                         {d_stats, frames * sizeof(igdsp_frame_stats)}};
    for (int i = 0; i < 4; ++i) {
        for (const Buf &b : ins)
            if (ranges_overlap(outs[i].p, outs[i].bytes, b.p, b.bytes)) return reject(IGDSP_EINVAL, "the state and the outputs must not overlap an input");
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return reject(IGDSP_EINVAL, "the state and the outputs must not overlap each other");
    }
    return kRun;
}

// ---- level control.  The frame length and the cfg (NULL = the defaults) are checked whether or not there is work
inline Verdict agc_run(P d_g711, P d_codec, P d_pcm, P d_ctl, const igdsp_agc_cfg *cfg, uint32_t C, uint32_t F, uint32_t n, P d_state, P d_out,
                       P d_rec, P d_stats)
{
    if (!agc_n_ok(n) || !agc_cfg_ok(cfg)) return kInvalid;
    if (empty(C, F)) return kNothing;
    if (!exactly_one(d_g711, d_pcm) || (d_g711 && !d_codec) || !d_state || !(d_out || d_rec || d_stats)) return kInvalid;
    if ((uint64_t)C * F >= 0xFFFFFFE0ull) return reject(IGDSP_ERANGE);
    // a block of 8 samples is one load (8 bytes of codes, 16 of PCM) and one 16-byte store; the state and a record are 16 bytes
    if (misaligned(8, {d_g711, d_stats}) || misaligned(16, {d_pcm, d_state, d_out, d_rec})) return kInvalid;
    const uint64_t frames = (uint64_t)C * F;
    struct Buf { P p; uint64_t bytes; };
    const Buf ins[4] = {{d_g711, frames * n}, {d_g711 ? d_codec : nullptr, C}, {d_pcm, frames * n * 2u}, {d_ctl, C}};
    const Buf outs[4] = {{d_state, (uint64_t)C * sizeof(igdsp_agc_state)}, {d_out, frames * n * 2u}, {d_rec, frames * sizeof(igdsp_agc_rec)},
                         {d_stats, frames * sizeof(igdsp_frame_stats)}};
    for (int i = 0; i < 4; ++i) {
        for (const Buf &b : ins)
            if (ranges_overlap(outs[i].p, outs[i].bytes, b.p, b.bytes)) return reject(IGDSP_EINVAL, "the state and the outputs must not overlap an input");
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return reject(IGDSP_EINVAL, "the state and the outputs must not overlap each other");
    }
    return kRun;
}

// ---- voice activity.  The frame length and the cfg (NULL = the defaults) are checked whether or not there is work.  Nothing to do with
// a list still writes the counts, so d_event_count's own rules apply before the shape's
inline Verdict vad_run(P d_g711, P d_codec, P d_pcm, P d_ctl, const igdsp_vad_cfg *cfg, uint32_t C, uint32_t F, uint32_t n, P d_state, P d_kind,
                       P d_rec, P d_sid, P d_txctl, P d_events, uint32_t event_cap, P d_event_count, P d_work)
{
    if (!vad_n_ok(n) || !vad_cfg_ok(cfg)) return kInvalid;
    if (misaligned(4, {d_event_count}) || misaligned(16, {d_work}) || (d_event_count && !d_work)) return kInvalid;
    if (d_event_count && event_cap != 0u && !d_events) return kInvalid;
    if (empty(C, F)) return d_event_count ? kRun : kNothing;              // the counts are written as 0
    if (!exactly_one(d_g711, d_pcm) || (d_g711 && !d_codec) || !d_state || !(d_kind || d_rec || d_sid || d_txctl || d_event_count)) return kInvalid;
    if ((uint64_t)C * F >= 0xFFFFFFE0ull) return reject(IGDSP_ERANGE);
    // a piece of 8 samples is one load (8 bytes of codes, 16 of PCM); the state is read as dwords and 8-byte sums, a record, a payload
    // and an event are one 16-byte store each
    if (misaligned(8, {d_g711}) || misaligned(16, {d_pcm, d_state, d_rec, d_sid, d_events})) return kInvalid;
    const uint64_t frames = (uint64_t)C * F;
    const bool list = d_event_count != nullptr;
    struct Buf { P p; uint64_t bytes; };
    const Buf ins[4] = {{d_g711, frames * n}, {d_g711 ? d_codec : nullptr, C}, {d_pcm, frames * n * 2u}, {d_ctl, C}};
    const Buf outs[8] = {{d_state, (uint64_t)C * sizeof(igdsp_vad_state)}, {d_kind, frames}, {d_rec, frames * sizeof(igdsp_vad_rec)}, {d_sid, frames * 16u},
                         {d_txctl, frames}, {list ? d_events : nullptr, (uint64_t)event_cap * sizeof(igdsp_vad_event)}, {d_event_count, 8u},
                         {list ? d_work : nullptr, vad_work_bytes(C, F, d_rec != nullptr)}};
    for (int i = 0; i < 8; ++i) {
        for (const Buf &b : ins)
            if (ranges_overlap(outs[i].p, outs[i].bytes, b.p, b.bytes)) return reject(IGDSP_EINVAL, "the state and the outputs must not overlap an input");
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return reject(IGDSP_EINVAL, "the state and the outputs must not overlap each other");
    }
    return kRun;
}

// ---- comfort noise.  The frame length is checked whether or not there is work
inline Verdict cng_run(P d_kind, P d_sid, P d_sid_len, P d_g711, P d_codec, P d_pcm, P d_ctl, P d_seed, uint32_t C, uint32_t F, uint32_t n, P d_state,
                       P d_out, P d_len_out, P d_rec, P d_stats)
{
    if (!cng_n_ok(n)) return kInvalid;
    if (empty(C, F)) return kNothing;
    if (any_null({d_kind, d_sid, d_state, d_out}) || !at_most_one(d_g711, d_pcm) || (d_g711 && !d_codec)) return kInvalid;
    if ((uint64_t)C * F >= 0xFFFFFFE0ull) return reject(IGDSP_ERANGE);
    // a piece of 8 samples is one load (8 bytes of codes, 16 of PCM) and one 16-byte store; the state goes as six 16-byte pieces, a
    // payload, a record and a stats record as one
    if (misaligned(8, {d_g711}) || misaligned(16, {d_sid, d_pcm, d_state, d_out, d_rec, d_stats})) return kInvalid;
    const uint64_t frames = (uint64_t)C * F;
    struct Buf { P p; uint64_t bytes; };
    const Buf ins[8] = {{d_kind, frames}, {d_sid, frames * 16u}, {d_sid_len, frames}, {d_g711, frames * n}, {d_g711 ? d_codec : nullptr, C},
                        {d_pcm, frames * n * 2u}, {d_ctl, C}, {d_seed, (uint64_t)C * 4u}};
    const Buf outs[5] = {{d_state, (uint64_t)C * sizeof(igdsp_cng_state)}, {d_out, frames * n * 2u}, {d_len_out, frames * 2u},
                         {d_rec, frames * sizeof(igdsp_cng_rec)}, {d_stats, frames * sizeof(igdsp_frame_stats)}};
    for (int i = 0; i < 5; ++i) {
        for (const Buf &b : ins)
            if (ranges_overlap(outs[i].p, outs[i].bytes, b.p, b.bytes)) return reject(IGDSP_EINVAL, "the state and the outputs must not overlap an input");
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return reject(IGDSP_EINVAL, "the state and the outputs must not overlap each other");
    }
    return kRun;
}

// ---- filter.  The frame length and max_sections are checked whether or not there is work
inline Verdict filt_run(P d_g711, P d_codec, P d_pcm, P d_ctl, P d_plans, uint32_t n_plans, P d_plan_of, uint32_t max_sections, uint32_t C, uint32_t F,
                        uint32_t n, P d_state, P d_out, P d_rec, P d_stats)
{
    if (!filt_n_ok(n) || max_sections > kFiltMaxSections) return kInvalid;
    if (empty(C, F)) return kNothing;
    if (!exactly_one(d_g711, d_pcm) || (d_g711 && !d_codec) || !d_plans || n_plans == 0u || !d_state || !(d_out || d_rec || d_stats)) return kInvalid;
    if ((uint64_t)C * F >= 0xFFFFFFE0ull) return reject(IGDSP_ERANGE);
    // a piece of 8 samples is one load (8 bytes of codes, 16 of PCM) and one 16-byte store; the state goes as three 16-byte pieces, a
    // record and a PCM record as one, a plan as dwords, a plan index as a half-word
    if (misaligned(2, {d_plan_of}) || misaligned(4, {d_plans}) || misaligned(8, {d_g711}) || misaligned(16, {d_pcm, d_state, d_out, d_rec, d_stats}))
        return kInvalid;
    const uint64_t frames = (uint64_t)C * F;
    struct Buf { P p; uint64_t bytes; };
    const Buf ins[6] = {{d_g711, frames * n}, {d_g711 ? d_codec : nullptr, C}, {d_pcm, frames * n * 2u}, {d_ctl, C},
                        {d_plans, (uint64_t)n_plans * sizeof(igdsp_filt_plan)}, {d_plan_of, (uint64_t)C * 2u}};
    const Buf outs[4] = {{d_state, (uint64_t)C * sizeof(igdsp_filt_state)}, {d_out, frames * n * 2u}, {d_rec, frames * sizeof(igdsp_filt_rec)},
                         {d_stats, frames * sizeof(igdsp_frame_stats)}};
    for (int i = 0; i < 4; ++i) {
        for (const Buf &b : ins)
            if (ranges_overlap(outs[i].p, outs[i].bytes, b.p, b.bytes)) return reject(IGDSP_EINVAL, "the state and the outputs must not overlap an input");
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return reject(IGDSP_EINVAL, "the state and the outputs must not overlap each other");
    }
    return kRun;
}

// ---- noise suppression.  The frame length and cfg are checked whether or not there is work
inline Verdict ns_run(P d_g711, P d_codec, P d_pcm, P d_ctl, const igdsp_ns_cfg *cfg, uint32_t C, uint32_t F, uint32_t n, P d_state, P d_out, P d_rec,
                      P d_stats)
{
    if (!ns_n_ok(n) || !cfg || !ns_cfg_ok(*cfg)) return kInvalid;
    if (empty(C, F)) return kNothing;
    if (!exactly_one(d_g711, d_pcm) || (d_g711 && !d_codec) || !d_state || !(d_out || d_rec || d_stats)) return kInvalid;
    if ((uint64_t)C * F >= 0xFFFFFFE0ull) return reject(IGDSP_ERANGE);
    // a piece of 8 samples is one load (8 bytes of codes, 16 of PCM) and one 16-byte store; the state goes as 67 16-byte pieces, a
    // record and a PCM record as one
    if (misaligned(8, {d_g711}) || misaligned(16, {d_pcm, d_state, d_out, d_rec, d_stats})) return kInvalid;
    const uint64_t frames = (uint64_t)C * F;
    struct Buf { P p; uint64_t bytes; };
    const Buf ins[4] = {{d_g711, frames * n}, {d_g711 ? d_codec : nullptr, C}, {d_pcm, frames * n * 2u}, {d_ctl, C}};
    const Buf outs[4] = {{d_state, (uint64_t)C * sizeof(igdsp_ns_state)}, {d_out, frames * n * 2u}, {d_rec, frames * sizeof(igdsp_ns_rec)},
                         {d_stats, frames * sizeof(igdsp_frame_stats)}};
    for (int i = 0; i < 4; ++i) {
        for (const Buf &b : ins)
            if (ranges_overlap(outs[i].p, outs[i].bytes, b.p, b.bytes)) return reject(IGDSP_EINVAL, "the state and the outputs must not overlap an input");
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return reject(IGDSP_EINVAL, "the state and the outputs must not overlap each other");
    }
    return kRun;
}

// ---- SRTP: one rule for igdsp_srtp_protect and igdsp_srtp_unprotect.  The strides are checked whether or not there is work.  In place
// is the one overlap allowed: d_out == d_packets with equal strides, d_sizes_out == d_sizes
inline Verdict srtp_run(P d_ctl, P d_packets, P d_sizes, uint32_t C, uint32_t F, uint32_t pkt_stride, P d_state, P d_out, uint32_t out_stride, P d_sizes_out,
                        P d_rec, uint64_t state_bytes = sizeof(igdsp_srtp_state))
{
    if (!stride_ok(pkt_stride, 12u) || !stride_ok(out_stride, 12u)) return kInvalid;
    if (empty(C, F)) return kNothing;
    if (!d_sizes) return reject(IGDSP_EINVAL, "d_sizes is required: a protected packet never fills its slot");
    if (any_null({d_packets, d_state, d_out, d_sizes_out})) return kInvalid;
    if ((uint64_t)C * F >= 0xFFFFFFE0ull) return reject(IGDSP_ERANGE);
    // a packet goes as 16-byte pieces at dword alignment, a record as one 8-byte store, the state as 16-byte pieces
    if (misaligned(2, {d_sizes, d_sizes_out}) || misaligned(4, {d_packets, d_out}) || misaligned(8, {d_rec}) || misaligned(16, {d_state})) return kInvalid;
    const uint64_t frames = (uint64_t)C * F;
    struct Buf { P p; uint64_t bytes; };
    const Buf ins[3] = {{d_ctl, frames}, {d_packets, frames * pkt_stride}, {d_sizes, frames * 2u}};
    const Buf outs[4] = {{d_state, (uint64_t)C * state_bytes}, {d_out, frames * out_stride}, {d_sizes_out, frames * 2u},
                         {d_rec, frames * sizeof(igdsp_srtp_rec)}};
    for (int i = 0; i < 4; ++i) {
        for (int k = 0; k < 3; ++k) {
            const bool in_place = (i == 1 && k == 1 && d_out == d_packets && out_stride == pkt_stride) || (i == 2 && k == 2 && d_sizes_out == d_sizes);
            if (!in_place && ranges_overlap(outs[i].p, outs[i].bytes, ins[k].p, ins[k].bytes))
                return reject(IGDSP_EINVAL, "the state and the outputs must not overlap an input, except in place");
        }
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return reject(IGDSP_EINVAL, "the state and the outputs must not overlap each other");
    }
    return kRun;
}

// ---- SRTCP: igdsp_srtcp_protect and igdsp_srtcp_unprotect take SRTP's arguments under SRTP's rule
inline Verdict srtcp_run(P d_ctl, P d_packets, P d_sizes, uint32_t C, uint32_t F, uint32_t pkt_stride, P d_state, P d_out, uint32_t out_stride, P d_sizes_out,
                         P d_rec)
{
    return srtp_run(d_ctl, d_packets, d_sizes, C, F, pkt_stride, d_state, d_out, out_stride, d_sizes_out, d_rec);
}

// ---- SRTP with AES-GCM: igdsp_srtp_gcm_protect and igdsp_srtp_gcm_unprotect take SRTP's arguments under SRTP's rule; the state is the
// larger igdsp_srtp_gcm_state
inline Verdict srtp_gcm_run(P d_ctl, P d_packets, P d_sizes, uint32_t C, uint32_t F, uint32_t pkt_stride, P d_state, P d_out, uint32_t out_stride, P d_sizes_out,
                            P d_rec)
{
    return srtp_run(d_ctl, d_packets, d_sizes, C, F, pkt_stride, d_state, d_out, out_stride, d_sizes_out, d_rec, sizeof(igdsp_srtp_gcm_state));
}

// ---- RTCP.  The stride is checked whether or not there is work.  Build writes its packets, sizes, records and the state; parse its
// records and the state: none of them may overlap an input or another of them
inline Verdict rtcp_build(P d_ctl, P d_jb, P d_src, P d_now, P d_cname, P d_cname_len, uint32_t C, uint32_t F, P d_state, P d_packets, uint32_t pkt_stride,
                          P d_sizes, P d_rec)
{
    if (!stride_ok(pkt_stride, (uint32_t)IGDSP_RTCP_MAX_BUILT)) return kInvalid;
    if (empty(C, F)) return kNothing;
    if (any_null({d_ctl, d_src, d_now, d_state, d_packets, d_sizes})) return kInvalid;
    if ((d_cname == nullptr) != (d_cname_len == nullptr)) return reject(IGDSP_EINVAL, "d_cname and d_cname_len come together");
    if ((uint64_t)C * F >= 0xFFFFFFE0ull) return reject(IGDSP_ERANGE);
    // a packet goes as 16-byte pieces at dword alignment, a record as one 8-byte store, the states, a source and a CNAME as 16-byte pieces
    if (misaligned(2, {d_sizes}) || misaligned(4, {d_packets}) || misaligned(8, {d_now, d_rec}) || misaligned(16, {d_jb, d_src, d_cname, d_state})) return kInvalid;
    const uint64_t frames = (uint64_t)C * F;
    struct Buf { P p; uint64_t bytes; };
    const Buf ins[6] = {{d_ctl, frames}, {d_jb, (uint64_t)C * sizeof(igdsp_jb_state)}, {d_src, frames * sizeof(igdsp_rtcp_src)}, {d_now, (uint64_t)F * 8u},
                        {d_cname, (uint64_t)C * IGDSP_RTCP_CNAME_MAX}, {d_cname_len, C}};
    const Buf outs[4] = {{d_state, (uint64_t)C * sizeof(igdsp_rtcp_state)}, {d_packets, frames * pkt_stride}, {d_sizes, frames * 2u},
                         {d_rec, frames * sizeof(igdsp_rtcp_built)}};
    for (int i = 0; i < 4; ++i) {
        for (const Buf &b : ins)
            if (ranges_overlap(outs[i].p, outs[i].bytes, b.p, b.bytes)) return reject(IGDSP_EINVAL, "the state and the outputs must not overlap an input");
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return reject(IGDSP_EINVAL, "the state and the outputs must not overlap each other");
    }
    return kRun;
}
inline Verdict rtcp_parse(P d_packets, P d_sizes, P d_arrival, P d_local_ssrc, uint32_t C, uint32_t F, uint32_t pkt_stride, P d_state, P d_rec)
{
    if (!stride_ok(pkt_stride, 8u)) return kInvalid;
    if (empty(C, F)) return kNothing;
    if (any_null({d_packets, d_sizes, d_arrival, d_local_ssrc, d_state})) return kInvalid;
    if ((uint64_t)C * F >= 0xFFFFFFE0ull) return reject(IGDSP_ERANGE);
    if (misaligned(2, {d_sizes}) || misaligned(4, {d_packets, d_arrival, d_local_ssrc}) || misaligned(16, {d_state, d_rec})) return kInvalid;
    const uint64_t frames = (uint64_t)C * F;
    struct Buf { P p; uint64_t bytes; };
    const Buf ins[4] = {{d_packets, frames * pkt_stride}, {d_sizes, frames * 2u}, {d_arrival, frames * 4u}, {d_local_ssrc, (uint64_t)C * 4u}};
    const Buf outs[2] = {{d_state, (uint64_t)C * sizeof(igdsp_rtcp_state)}, {d_rec, frames * sizeof(igdsp_rtcp_seen)}};
    for (int i = 0; i < 2; ++i) {
        for (const Buf &b : ins)
            if (ranges_overlap(outs[i].p, outs[i].bytes, b.p, b.bytes)) return reject(IGDSP_EINVAL, "the state and the records must not overlap an input");
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes)) return reject(IGDSP_EINVAL, "the state and the records must not overlap each other");
    }
    return kRun;
}

}  // namespace igdsp::args
