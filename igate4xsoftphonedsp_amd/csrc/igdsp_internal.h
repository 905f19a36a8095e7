// Internal launcher declarations shared by the kernel translation units (igdsp_k_*.hip) and the C-ABI ones (igdsp_capi*.hip, igdsp_io.hip).
// Not part of the ABI (include/igdsp.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "igdsp.h"
#include "igdsp_route.h"

namespace igdsp {

struct LaunchCfg {
    int compute_units;   // persistent grid = compute_units blocks
    uint32_t *gqueue;    // device-wide work counter {next batch, blocks done} for this launch, zero on entry
                         // and re-armed by the kernel itself; nullptr = static per-block distribution
    bool out_spread = false;   // the launch's bulk output sits half in one, half in another memory class (igdsp_io_alloc)
    const uint8_t *enc_tab = nullptr;   // igdsp_encode: the context's ready-made compressor table of this lineage (2 x 65 536 bytes), or nullptr
};

// The ED-137 gated window of a fused packet launch (launch_decode_meter_window): work = uint4[n_seg][3][C] unit summaries (window
// words 0, 1 and the silence-run word, k_window_finish); a unit = (one of n_groups = C / 64 channel groups, one of n_seg segments
// of the F frames).
struct WinArgs {
    uint4 *work = nullptr;
    uint32_t gate_mask = 0, alarm = IGDSP_PROBE_ALARM, n_seg = 1, n_groups = 0, F = 0;   // gate_mask: ED-137 bits that open the frame gate (0 = always)
    // block-owned form (gpb != 0): a block owns gpb = 1 << gsh consecutive channel groups for the launch, their windows live in its LDS
    // and it folds them into hold / probe itself; work = uint4[n_groups / gpb][F][gpb] probe / reset masks
    uint32_t gpb = 0, gsh = 0;
    igdsp_chan_hold *hold = nullptr;
    const uint8_t *gate = nullptr;
    igdsp_chan_probe *probe = nullptr;
};
constexpr int kWinRing = 16;                             // frames of a group that may be folded before an earlier one is (power of two)

hipError_t init_device_attributes();       // per-device kernel attributes; igdsp_create calls it with its device current
hipError_t launch_decode_meter(const LaunchCfg &cfg, int variant,
                               const uint8_t *payload, const uint8_t *codec, const uint16_t *len,
                               uint32_t C, uint32_t F, uint32_t n,
                               igdsp_frame_stats *stats, int16_t *pcm,
                               igdsp_aggregate *agg, uint32_t rank, hipStream_t s);
hipError_t launch_decode_meter_rtp(const LaunchCfg &cfg, const uint8_t *slots, const uint16_t *sizes, const uint8_t *codec, uint32_t C,
                                   uint32_t F, uint32_t stride, uint32_t hdr, igdsp_frame_stats *stats, igdsp_rtp_info *info,
                                   igdsp_aggregate *agg, uint32_t rank, hipStream_t s, const uint8_t *radio = nullptr);
// igdsp_decode_meter_window's fused path (C % 64 == 0, win.d_work given): the window folded into the decode + meter pass, in the form
// window_route picks, k_window_finish included.  *too_long: F needs more than kWinMaxSeg segments of 65 535 frames; nothing launched.
hipError_t launch_decode_meter_window(const LaunchCfg &cfg, const uint8_t *packets, const uint16_t *sizes, const uint8_t *codec, uint32_t C,
                                      uint32_t F, uint32_t stride, uint32_t hdr, const uint8_t *radio, igdsp_frame_stats *stats,
                                      igdsp_rtp_info *info, igdsp_aggregate *agg, uint32_t rank, const igdsp_window &win, bool *too_long,
                                      hipStream_t s);
// window fold of records (per-frame ED-137 gates, silence run): igdsp_window_update; and the chaining of a fused launch's per-segment
// run summaries into probe[c]
hipError_t launch_window_update(const igdsp_frame_stats *stats, const igdsp_rtp_info *info, const uint16_t *len, uint32_t C, uint32_t F, uint32_t n,
                                uint32_t gate_mode, uint32_t alarm, igdsp_chan_hold *hold, const uint8_t *gate, igdsp_chan_probe *probe, hipStream_t s);
hipError_t launch_window_finish(const uint4 *work, uint32_t C, uint32_t n_seg, uint32_t alarm, igdsp_chan_hold *hold, const uint8_t *gate,
                                igdsp_chan_probe *probe, hipStream_t s);
hipError_t launch_diag_chunk32(const LaunchCfg &cfg, const uint8_t *payload, const uint8_t *codec, uint32_t C, uint32_t F,
                               igdsp_frame_stats *stats, uint64_t *diag, hipStream_t s);
hipError_t launch_build_enc_table(int variant, uint8_t *tab, hipStream_t s);   // tab[law << 16 | uint16(v)] = enc(v), 131 072 bytes
hipError_t launch_encode(const LaunchCfg &cfg, const int16_t *pcm, const uint8_t *codec,
                         uint32_t C, uint32_t F, uint32_t n, uint8_t *out, int variant, hipStream_t s);
hipError_t launch_encode_table(const LaunchCfg &cfg, const int16_t *pcm, const uint8_t *codec, uint32_t C, uint32_t F, uint32_t n,
                               uint8_t *out, int variant, hipStream_t s);
hipError_t launch_roundtrip(const LaunchCfg &cfg, int kernel_variant, const uint8_t *payload, const uint8_t *codec,
                            uint32_t C, uint32_t F, uint32_t n, uint8_t *out, igdsp_frame_stats *stats,
                            igdsp_chan_hold *hold, const uint8_t *gate, int variant, hipStream_t s);
hipError_t launch_hold_update(const igdsp_frame_stats *stats, const uint16_t *len, uint32_t C, uint32_t F, uint32_t n,
                              igdsp_chan_hold *hold, const uint8_t *gate, hipStream_t s);
hipError_t launch_flush_fold(const igdsp_frame_stats *stA, const igdsp_frame_stats *stB, const uint16_t *lenB, const uint2 *seq, const uint2 *runs,
                             uint32_t n_channels, uint32_t gate_mode, uint32_t alarm, igdsp_chan_hold *hold, igdsp_chan_probe *probe,
                             igdsp_frame_stats *last, hipStream_t s);
hipError_t launch_hold_reset(igdsp_chan_hold *hold, uint32_t C, const uint8_t *mask, hipStream_t s);
hipError_t launch_depayload(const LaunchCfg &cfg, const uint8_t *packets, const uint16_t *sizes, const uint8_t *radio,
                            uint32_t C, uint32_t F, uint32_t stride, uint32_t n, uint8_t *payload, uint16_t *len,
                            igdsp_rtp_info *info, hipStream_t s);
hipError_t launch_tx_copy_ab(const LaunchCfg &cfg, const int16_t *pcm, const uint8_t *g711, uint32_t C, uint32_t F, uint32_t n,
                             uint8_t *packets, uint32_t stride, hipStream_t s);   // compute-free yardstick of launch_tx_packetize
hipError_t launch_tx_packetize(const LaunchCfg &cfg, const int16_t *pcm, const uint8_t *g711, const uint8_t *ctl, uint32_t C, uint32_t F,
                               uint32_t n, uint64_t t0, uint32_t frame_ms, igdsp_tx_chan *state, uint8_t *last, uint8_t *packets,
                               uint32_t stride, uint16_t *sizes, igdsp_tx_info *info, int variant, hipStream_t s);
// igdsp_tx_flush's device step over one compacted upload block (csrc/igdsp_txstage.h's layout): per-frame packets in 256-byte slots,
// igdsp_tx_info per frame, the legs' state (in place and a copy per run for the download) and their send buffers [legs][236].
hipError_t launch_tx_staged(const LaunchCfg &cfg, const void *runs, const void *recs, const uint32_t *stream, uint32_t n_runs,
                            igdsp_tx_chan *state, uint8_t *send_buf, igdsp_tx_info *info, igdsp_tx_chan *chan_out, uint32_t *packets,
                            hipStream_t s);
// igdsp_conf_mix: exactly one of g711 (+ codec) / pcm; out and stats may be nullptr (not both: the C ABI checks).  yardstick: the
// compute-free form, the same traversal, the same bytes read and written, no decode / scale / clamp / stats
hipError_t launch_conf_mix(const LaunchCfg &cfg, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, const uint16_t *len,
                           const uint16_t *gain, const uint32_t *port_ptr, const uint32_t *members, uint32_t n_members, uint32_t C, uint32_t P,
                           uint32_t F, uint32_t n, int16_t *out, igdsp_frame_stats *stats, bool yardstick, hipStream_t s);
// igdsp_bss_select: at most one of g711 (+ codec) / pcm; sel, out, stats may each be nullptr (out and stats need an input: the C ABI
// checks); gain nullptr = 256.  yardstick: the compute-free form, the same traversal and bytes, no decode / scale / clamp / stats /
// state machine
hipError_t launch_bss_select(const LaunchCfg &cfg, const igdsp_rtp_info *info, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm,
                             const uint16_t *len, const uint16_t *gain, const uint32_t *group_ptr, const uint32_t *members, uint32_t n_members,
                             const uint8_t *mute, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t vote_frames, igdsp_bss_state *state,
                             uint32_t *words, int32_t *sel, int16_t *out, igdsp_frame_stats *stats, bool yardstick, hipStream_t s);
// igdsp_ptt_arbitrate: at most one of g711 (+ codec) / pcm; sel, tick, ctl_out, out, stats may each be nullptr (out and stats need an
// input: the C ABI checks); gain nullptr = 256; release_frames 0 = IGDSP_PTT_RELEASE_FRAMES.  yardstick: the compute-free form, the same
// traversal and bytes, no decode / scale / clamp / stats / debounce / arbitration; the group state is not touched, the slots are
// stepped as by a launch
hipError_t launch_ptt_arbitrate(const LaunchCfg &cfg, const igdsp_rtp_info *info, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm,
                                const uint16_t *len, const uint16_t *gain, const uint32_t *group_ptr, const uint32_t *members,
                                uint32_t n_members, const uint8_t *rxonly, uint32_t C, uint32_t G, uint32_t F, uint32_t n,
                                uint32_t release_frames, igdsp_ptt_state *state, igdsp_ptt_slot *slots, int32_t *sel, igdsp_ptt_tick *tick,
                                uint8_t *ctl_out, int16_t *out, igdsp_frame_stats *stats, bool yardstick, hipStream_t s);
// igdsp_link_watch: sizes, up, period, kind may each be nullptr; event_count nullptr = no list (one pass, work unused), else work is
// igdsp_link_work_bytes(C, T) bytes, 16-byte aligned; miss_ticks 0 = IGDSP_LINK_MISS_TICKS, event_mask 0 = IGDSP_LINK_EVENT_DEFAULT.
// C * T == 0 with a list: only the two counts are written (0).  yardstick: the compute-free form, the same passes, the same bytes read
// and written, no state machine: the state is stored as it was read, the kind bytes are 0 and the list is empty
hipError_t launch_link_watch(const LaunchCfg &cfg, const igdsp_rtp_info *info, const uint16_t *sizes, const uint8_t *up, const uint16_t *period,
                             uint32_t C, uint32_t T, uint32_t S, uint64_t t0_ms, uint32_t tick_ms, uint32_t miss_ticks, uint32_t event_mask,
                             igdsp_link_state *state, uint8_t *kind, igdsp_link_event *events, uint32_t event_cap, uint32_t *event_count,
                             void *work, bool yardstick, hipStream_t s);
// igdsp_jb_receive: sizes, arrival, tick, pkt may each be nullptr; ring is igdsp_jb_ring_bytes(C, n) bytes, 16-byte aligned.
// yardstick: the compute-free form, the same rows as an in-order lossless launch (arrival slot k = 0 of every tick played straight from
// the packet), no header walk, state machine or ring store; the state is not touched
hipError_t launch_jb_receive(const LaunchCfg &cfg, const uint8_t *packets, const uint16_t *sizes, const uint8_t *radio, const uint32_t *arrival,
                             uint32_t C, uint32_t T, uint32_t S, uint32_t stride, uint32_t n, uint32_t delay, igdsp_jb_state *state, void *ring,
                             uint8_t *payload, uint16_t *len, igdsp_rtp_info *info, uint8_t *tick, uint8_t *pkt, bool yardstick, hipStream_t s);
// igdsp_jb_receive_adaptive: as launch_jb_receive with the channel's delay from adapt [C] and cfg (checked by the C ABI); delay_out may
// be nullptr.  No yardstick form: igdsp_internal_jb_copy is the yardstick of both entries
hipError_t launch_jb_adaptive(const LaunchCfg &cfg, const uint8_t *packets, const uint16_t *sizes, const uint8_t *radio, const uint32_t *arrival,
                              uint32_t C, uint32_t T, uint32_t S, uint32_t stride, uint32_t n, const igdsp_jb_adapt_cfg &acfg, igdsp_jb_state *state,
                              void *ring, igdsp_jb_adapt *adapt, uint8_t *payload, uint16_t *len, igdsp_rtp_info *info, uint8_t *tick, uint8_t *pkt,
                              uint8_t *delay_out, hipStream_t s);
// igdsp_plc_conceal: exactly one of g711 (+ codec) / pcm; len, len_out, stats may each be nullptr.  yardstick: the compute-free form,
// the same traversal with every tick taken as PLAIN, the input bits widened to the output, no decode, pitch search, synthesis or stats
// (records carry only the length); the ring and the scalars are written as by a launch
hipError_t launch_plc_conceal(const LaunchCfg &cfg, const uint8_t *flags, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm,
                              const uint16_t *len, uint32_t C, uint32_t T, uint32_t n, igdsp_plc_state *state, int16_t *out, uint16_t *len_out,
                              igdsp_frame_stats *stats, bool yardstick, hipStream_t s);
// igdsp_snd_combine (dir kSndCombine: in = pcm [F][D * K][n], out = frames [F][D][n][K]) / igdsp_snd_split (kSndSplit: the reverse);
// out and stats may be nullptr (not both: the C ABI checks).  yardstick: the compute-free form, the same items, the same bytes read
// and written in memory order, no transpose and no records; it needs out
hipError_t launch_snd(const LaunchCfg &cfg, int dir, const int16_t *in, uint32_t D, uint32_t K, uint32_t F, uint32_t n, int16_t *out,
                      igdsp_frame_stats *stats, bool yardstick, hipStream_t s);
// igdsp_tone_generate: plan_of, cmd, len may each be nullptr; pcm and stats may be nullptr (not both: the C ABI checks); rows_per_frame 0 =
// P.  yardstick: the compute-free form, the same items and stores, no plan, state or oscillator; it needs pcm
hipError_t launch_tone(const LaunchCfg &cfg, const igdsp_tone_plan *plans, uint32_t n_plans, const uint16_t *plan_of, const uint8_t *cmd,
                       igdsp_tone_state *state, uint32_t P, uint32_t F, uint32_t n, uint32_t rows_per_frame, int16_t *pcm, uint16_t *len,
                       igdsp_frame_stats *stats, bool yardstick, hipStream_t s);
// igdsp_resample: exactly one of g711 (+ codec, UP only) / pcm; len may be nullptr; out and stats may be nullptr (not both: the C ABI
// checks); rows_narrow / rows_wide 0 = C.  yardstick: the compute-free form, the same loads, LDS traffic and stores, no filter, zero
// records, the state neither read nor written
hipError_t launch_rs(const LaunchCfg &cfg, uint32_t dir, uint32_t R, uint32_t layout, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm,
                     const uint16_t *len, igdsp_rs_state *state, uint32_t C, uint32_t F, uint32_t n, uint32_t rows_narrow, uint32_t rows_wide,
                     int16_t *out, igdsp_frame_stats *stats, bool yardstick, hipStream_t s);
// igdsp_dbuf_run: flags, len_out, fill, stats may each be nullptr.  yardstick: the compute-free form, every step taken as PUT|GET at a
// fixed fill of n, the rows through the ring as by a launch, no update, search, blend or record arithmetic (records carry only the
// length); the scalars are written as by a launch
hipError_t launch_dbuf_run(const LaunchCfg &cfg, const uint8_t *ops, const int16_t *in, uint32_t C, uint32_t T, uint32_t n, uint32_t M,
                           igdsp_dbuf_state *state, int16_t *out, uint8_t *flags, uint16_t *len_out, uint16_t *fill, igdsp_frame_stats *stats,
                           bool yardstick, hipStream_t s);
// igdsp_spectrum: exactly one of g711 (with codec) and pcm; rec, avg, raw may each be nullptr.  yardstick: the compute-free form, the same
// rows into the ring, the same ring loads, tile exchanges and stores at a hop, no window, butterfly, twiddle, split, log or average (a
// record carries only IGDSP_SPEC_HOP; the averaged array is stored as it was read)
hipError_t launch_spectrum(const LaunchCfg &cfg, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, uint32_t C, uint32_t F, uint32_t n,
                           uint32_t hop_frames, float alpha, igdsp_spec_state *state, igdsp_spec_rec *rec, float *avg, float *raw, bool yardstick,
                           hipStream_t s);
// the link stage's scan (igdsp_k_link.hip), which launch_event_list launches as well: counts[0 .. N) behind the 16-byte head of
// `head` -> exclusive offsets in place; first: start at 0, else at head[0]; last: event_count = {total, min(total, cap)}.  One block of
// kLinkScanThreads
__global__ void k_link_scan(uint32_t *head, uint64_t N, uint32_t first, uint32_t last, uint32_t cap, uint32_t *event_count);
// The event list behind a stage's dense records (ListRoute; igdsp_tone_detect, igdsp_vad_run), called behind the stage's own kernel;
// event_count nullptr = no list.  pass<false> / pass<true>: the stage's list kernel (event_list_pass, igdsp_lanes.h).  empty: the
// stage launched nothing (C * F == 0) and only the two counts are written (0).  list_records: where the stage's kernel writes the
// records the list reads when the caller gave no d_rec: d_work, behind the counts.  (Defined in igdsp_k_link.hip for the two stages.)
template <class Rec>
inline Rec *list_records(Rec *rec, bool list, void *work, const ListRoute &r) { return list && !rec ? reinterpret_cast<Rec *>(static_cast<uint8_t *>(work) + r.counts_bytes) : rec; }
template <class Rec, class Event>
using ListPass = void (*)(const Rec *rec, uint32_t C, uint32_t F, uint32_t W, uint32_t mask, uint32_t *counts, Event *events, uint32_t cap);
template <class Rec, class Event>
hipError_t launch_event_list(ListPass<Rec, Event> count, ListPass<Rec, Event> store, const ListRoute &r, bool empty, const Rec *rec, uint32_t C,
                             uint32_t F, uint32_t mask, Event *events, uint32_t event_cap, uint32_t *event_count, void *work, hipStream_t s);
// igdsp_tone_detect: exactly one of g711 (with codec) and pcm; plan_of, rec, events may each be nullptr; event_count nullptr = no list
// (work unused), else work is igdsp_tdet_work_bytes bytes, 16-byte aligned; event_mask 0 = IGDSP_TDET_EVENT_DEFAULT.  C * F == 0 with a
// list: only the two counts are written (0).  yardstick: the compute-free form, the same rows into the same buffers, the same records,
// state and list passes, no table, dot product, decision or debounce (records are all-zero, the debounce fields stay as they were)
hipError_t launch_tone_detect(const LaunchCfg &cfg, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, const igdsp_tdet_plan *plans,
                              uint32_t n_plans, const uint16_t *plan_of, uint32_t C, uint32_t F, uint32_t n, uint32_t event_mask,
                              igdsp_tdet_state *state, igdsp_tdet_rec *rec, igdsp_tdet_event *events, uint32_t event_cap, uint32_t *event_count,
                              void *work, bool yardstick, hipStream_t s);
// igdsp_echo_cancel: exactly one of near_g711 (with codec) and near_pcm; far_of, ctl, out, rec, stats may each be nullptr; cfg checked
// by the C ABI.  yardstick: the compute-free form, the same row loads, history moves, state and row stores, no dot product, reduction or
// update (out = the near row, the weights as they were, the history as by a launch; records carry the energies and BYPASSED)
hipError_t launch_echo_cancel(const LaunchCfg &cfg, const uint8_t *near_g711, const uint8_t *codec, const int16_t *near_pcm, const int16_t *far_pcm,
                              uint32_t n_far, const uint32_t *far_of, const uint8_t *ctl, const igdsp_ec_cfg &ec, uint32_t C, uint32_t F, uint32_t n,
                              igdsp_ec_state *state, int16_t *out, igdsp_ec_rec *rec, igdsp_frame_stats *stats, bool yardstick, hipStream_t s);
// igdsp_agc_run: exactly one of g711 (with codec) and pcm; ctl, out, rec, stats may each be nullptr; cfg checked by the C ABI.
// yardstick: the compute-free form, the same row loads, state load and store, row, record and PCM-record stores, no peak, division,
// recurrence or gain (out = the row, the state as read, tagged; records carry the state's gain and env, tmin 4096 and BYPASSED)
hipError_t launch_agc(const LaunchCfg &cfg, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, const uint8_t *ctl, const igdsp_agc_cfg &agc,
                      uint32_t C, uint32_t F, uint32_t n, igdsp_agc_state *state, int16_t *out, igdsp_agc_rec *rec, igdsp_frame_stats *stats,
                      bool yardstick, hipStream_t s);
// igdsp_vad_run: exactly one of g711 (with codec) and pcm; ctl, kind, rec, sid, txctl, events may each be nullptr; cfg checked by the C
// ABI; event_count nullptr = no list (work unused), else work is igdsp_vad_work_bytes bytes, 16-byte aligned; event_mask 0 =
// IGDSP_VAD_EVENT_DEFAULT.  C * F == 0 with a list: only the two counts are written (0).  yardstick: the compute-free form, the same row
// loads, decode, LDS stores, state load and store, output stores and list passes, no lag sum, level, decision, model or recursion: it
// stores the bytes igdsp_vad_run stores with every channel at IGDSP_VAD_BYPASS except ms = 0 and level = 127 in the records, and the
// state, which a bypass leaves alone, as it was read (nf and A clamped; another tag: the RESET state) with the tag, flags
// IGDSP_VAD_F_BYPASSED and reserved 0
hipError_t launch_vad(const LaunchCfg &cfg, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, const uint8_t *ctl, const igdsp_vad_cfg &vad,
                      uint32_t C, uint32_t F, uint32_t n, uint32_t event_mask, igdsp_vad_state *state, uint8_t *kind, igdsp_vad_rec *rec, uint8_t *sid,
                      uint8_t *txctl, igdsp_vad_event *events, uint32_t event_cap, uint32_t *event_count, void *work, bool yardstick, hipStream_t s);
// igdsp_cng_run: kind, sid, state, out required; at most one of g711 (with codec) and pcm; sid_len (nullptr: 11), ctl, seed, len_out, rec,
// stats may each be nullptr.  yardstick: the compute-free form, the same kind, length and voice-row loads, decode, tile stores and reads,
// state load and store and output stores, no excitation, lattice, gain step or SID step: it stores the bytes igdsp_cng_run stores with
// every channel at IGDSP_CNG_BYPASS, and the state, which a bypass leaves alone, as it was read (b, kq, g, g_tgt clamped, have its bit
// 0; another tag: the RESET state with d_seed's seed) with the tag, flags as read and reserved 0; ctl and the payloads are not read
hipError_t launch_cng(const LaunchCfg &cfg, const uint8_t *kind, const uint8_t *sid, const uint8_t *sid_len, const uint8_t *g711, const uint8_t *codec,
                      const int16_t *pcm, const uint8_t *ctl, const uint32_t *seed, uint32_t C, uint32_t F, uint32_t n, igdsp_cng_state *state,
                      int16_t *out, uint16_t *len_out, igdsp_cng_rec *rec, igdsp_frame_stats *stats, bool yardstick, hipStream_t s);
// igdsp_filt_run: exactly one of g711 (with codec) and pcm; plans (n_plans >= 1) and state required; ctl, plan_of, out, rec, stats may
// each be nullptr; max_sections 0..4.  yardstick: the compute-free form, the same row loads, decode, tile stores, reads and writes,
// state load and store and output stores, and the peak fold of a bypassed row; no section runs.  It stores the bytes igdsp_filt_run
// stores with every channel at IGDSP_FILT_BYPASS, and the state, which a bypass leaves alone, as it was read (e masked; another tag:
// zero histories) with the tag, flags as read and reserved 0; ctl is not read, of a plan only its first dword
hipError_t launch_filt(const LaunchCfg &cfg, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, const uint8_t *ctl, const igdsp_filt_plan *plans,
                       uint32_t n_plans, const uint16_t *plan_of, uint32_t max_sections, uint32_t C, uint32_t F, uint32_t n, igdsp_filt_state *state,
                       int16_t *out, igdsp_filt_rec *rec, igdsp_frame_stats *stats, bool yardstick, hipStream_t s);
// igdsp_ns_run: exactly one of g711 (with codec) and pcm; state required; ctl, out, rec, stats may each be nullptr; cfg checked by the
// caller.  yardstick: the compute-free form, the same row loads, decode, row stores into LDS, state load and store, the hop's pass of
// ns_hop_bypass over the row, the energy and PCM-record folds, output stores; no transform, no band runs.  It stores the bytes
// igdsp_ns_run stores with every channel at IGDSP_NS_BYPASS; ctl is not read
hipError_t launch_ns(const LaunchCfg &cfg, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, const uint8_t *ctl, const igdsp_ns_cfg &ns,
                     uint32_t C, uint32_t F, uint32_t n, igdsp_ns_state *state, int16_t *out, igdsp_ns_rec *rec, igdsp_frame_stats *stats, bool yardstick,
                     hipStream_t s);
// igdsp_srtp_protect / igdsp_srtp_unprotect: dir kSrtpDirProtect or kSrtpDirUnprotect; ctl and rec may be nullptr.  yardstick: the
// compute-free form of protect: the same loads, tile traffic, state load and store and stores, the header parse and the size rules, no
// AES round and no compression: a packet goes out as it came with tag_len zero bytes behind it, its record says BYPASSED, the state's
// words are stored as read; ctl is not read
hipError_t launch_srtp(const LaunchCfg &cfg, int dir, const uint8_t *ctl, const uint8_t *packets, const uint16_t *sizes, uint32_t C, uint32_t F,
                       uint32_t pkt_stride, igdsp_srtp_state *state, uint8_t *out, uint32_t out_stride, uint16_t *sizes_out, igdsp_srtp_rec *rec,
                       bool yardstick, hipStream_t s);
// igdsp_srtcp_protect / igdsp_srtcp_unprotect: launch_srtp's arguments and yardstick, RFC 3711 3.4 (the trailer's 14 bytes go out as zeros)
hipError_t launch_srtcp(const LaunchCfg &cfg, int dir, const uint8_t *ctl, const uint8_t *packets, const uint16_t *sizes, uint32_t C, uint32_t F,
                        uint32_t pkt_stride, igdsp_srtp_state *state, uint8_t *out, uint32_t out_stride, uint16_t *sizes_out, igdsp_srtp_rec *rec,
                        bool yardstick, hipStream_t s);
// igdsp_srtp_gcm_protect / igdsp_srtp_gcm_unprotect: launch_srtp's arguments with the GCM state; yardstick as there (the 16 tag bytes go
// out as zeros)
hipError_t launch_srtp_gcm(const LaunchCfg &cfg, int dir, const uint8_t *ctl, const uint8_t *packets, const uint16_t *sizes, uint32_t C, uint32_t F,
                           uint32_t pkt_stride, igdsp_srtp_gcm_state *state, uint8_t *out, uint32_t out_stride, uint16_t *sizes_out, igdsp_srtp_rec *rec,
                           bool yardstick, hipStream_t s);
// igdsp_rtcp_build: jb, rec and (together) cname, cname_len may be nullptr.  igdsp_rtcp_parse: rec may be nullptr.  yardstick: the
// compute-free forms.  Build: the same loads, the size rule, a row of the packet's size filled with one loaded word, the same stores,
// a record with the size and no flag, the state as read.  Parse: the same loads, tile traffic and row reads; the record is the size's
// verdict alone (PARSED, EMPTY or MALFORMED), the state as read
hipError_t launch_rtcp_build(const LaunchCfg &cfg, const uint8_t *ctl, const igdsp_jb_state *jb, const igdsp_rtcp_src *src, const uint64_t *now,
                             const uint8_t *cname, const uint8_t *cname_len, uint32_t C, uint32_t F, igdsp_rtcp_state *state, uint8_t *packets,
                             uint32_t pkt_stride, uint16_t *sizes, igdsp_rtcp_built *rec, bool yardstick, hipStream_t s);
hipError_t launch_rtcp_parse(const LaunchCfg &cfg, const uint8_t *packets, const uint16_t *sizes, const uint32_t *arrival, const uint32_t *local_ssrc, uint32_t C,
                             uint32_t F, uint32_t pkt_stride, igdsp_rtcp_state *state, igdsp_rtcp_seen *rec, bool yardstick, hipStream_t s);
hipError_t launch_wav_expand(const LaunchCfg &cfg, const uint8_t *payload, uint32_t C, uint32_t F, uint32_t n, uint32_t rate,
                             uint8_t *files, uint64_t file_stride, hipStream_t s);
hipError_t launch_g726(const LaunchCfg &cfg, const uint8_t *in, uint8_t *out, uint64_t n_bytes, int mode, hipStream_t s);
hipError_t launch_gen_uniform(uint8_t *out, uint64_t n_bytes, uint64_t seed, uint64_t first_byte, hipStream_t s);
hipError_t launch_stream_rw(const LaunchCfg &cfg, const void *src, size_t bytes, void *dst, hipStream_t s);
hipError_t launch_stream_cluster(const LaunchCfg &cfg, const void *src, size_t bytes, void *dst, int k, hipStream_t s);
hipError_t launch_stream_pieces(const LaunchCfg &cfg, const void *src, uint32_t n_items, uint32_t stride, uint32_t hdr, int mode, int rows, void *dst, void *dst2, hipStream_t s);
hipError_t launch_stream_walk(const LaunchCfg &cfg, const void *src, uint32_t n_items, uint32_t stride, uint32_t hdr, uint32_t groups, uint32_t n_seg,
                              uint32_t trickle, void *dst, void *dst2, hipStream_t s);
hipError_t launch_stream_mix(const LaunchCfg &cfg, const void *src, void *dst, uint32_t n_items, int r, int w, int waves, hipStream_t s, void *dst2 = nullptr, const void *src2 = nullptr);
hipError_t launch_stream_read(const LaunchCfg &cfg, const void *src, size_t bytes, uint64_t *sink, hipStream_t s);

}  // namespace igdsp
