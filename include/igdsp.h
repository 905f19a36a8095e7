/*
 * igdsp.h — C ABI of the MI355X (gfx950) G.711 + level-meter hot path.
 *
 * This is the drop-in boundary for ONE path of piyanon108/iGate4xSoftphoneDSP:
 * the per-20 ms-RTP-frame work done behind the pjmedia transport adapter
 *   transport_rtp_cb  -> RoIP_ED137::setIncomingRTP(tp_adapter*)   (TransportAdapter.cpp:240-316, roip_ed137.cpp:6541-6587)
 *   transport_send_rtp -> RoIP_ED137::setOutgoingRTP(tp_adapter*)  (TransportAdapter.cpp:635-874, roip_ed137.cpp:6500-6536)
 * plus the G.711 decode/encode that pjmedia performs around those hooks
 * (TransportAdapter.cpp:301; codec selection roip_ed137.cpp:3546-3574) and the
 * level-meter contract of audiometer.cpp:30-31 / Functions.cpp:2126-2230.
 *
 * Plain C types only; usable from C99 and C++11 (the reference builds with
 * CONFIG += c++11, iGate4xSoftphoneDSP.pro:2).  No torch / HIP types appear
 * here: device buffers are `void*`-compatible raw pointers, streams are an
 * opaque `void*` (a hipStream_t; NULL is HIP's legacy default stream).
 *
 * Error convention follows the reference (pj_status_t, PJ_SUCCESS == 0,
 * TransportAdapter.cpp:135-223): every entry returns int, 0 == success,
 * negative == IGDSP_E*.  Nothing here throws or aborts the host.
 */
#ifndef IGDSP_H
#define IGDSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: igdsp_io_alloc / igdsp_io_free, igdsp_wav_expand, staging ring (igdsp_level.dropped, IGDSP_STAGE_DEPTH); every round-1 entry is
 * unchanged in signature and meaning.
 * 3: additive again — the ED-137 gated window (igdsp_window, igdsp_decode_meter_window, igdsp_window_update, igdsp_chan_probe),
 * igdsp_set_ed137 / igdsp_set_gate_mode / igdsp_get_probe on the single-frame path, igdsp_flush_begin / igdsp_flush_end.
 *    Later, still additive under 3: the ED-137 TX packetizer (igdsp_tx_chan, igdsp_tx_info, igdsp_tx_chan_init, igdsp_tx_calltype_bits,
 *    igdsp_tx_packetize); the staged send path behind transport_send_rtp (igdsp_tx_open .. igdsp_tx_flush, igdsp_tx_packet); the
 *    conference mix (igdsp_conf_level_q7, igdsp_conf_build, igdsp_conf_mix, IGDSP_FLAG_SATURATED); best signal selection
 *    (igdsp_bss_state, IGDSP_BSS_VOTE_FRAMES, igdsp_bss_select); the jitter buffer (igdsp_jb_state, igdsp_jb_prior, igdsp_jb_rr,
 *    IGDSP_JB_*, igdsp_jb_ring_bytes, igdsp_jb_report, igdsp_jb_receive; igdsp_jb_adapt, igdsp_jb_adapt_cfg, igdsp_jb_receive_adaptive); packet loss concealment (igdsp_plc_state, IGDSP_PLC_*,
 *    IGDSP_FLAG_CONCEALED, igdsp_plc_conceal); PTT priority arbitration (igdsp_ptt_state, igdsp_ptt_slot, igdsp_ptt_tick, IGDSP_PTT_*,
 *    igdsp_ptt_arbitrate); R2S link supervision and the device event list (igdsp_link_state, igdsp_link_event, IGDSP_LINK_*,
 *    igdsp_link_work_bytes, igdsp_link_watch); the sound-card splitter / combiner (IGDSP_SND_*, igdsp_snd_combine, igdsp_snd_split,
 *    igdsp_snd_vu_t, igdsp_snd_vu); the tone generator (IGDSP_TONE_*, igdsp_tone_desc, igdsp_tone_seg, igdsp_tone_plan,
 *    igdsp_tone_state, igdsp_tone_plan_build, igdsp_tone_frame, igdsp_tone_generate); the rate converter (IGDSP_RS_*, igdsp_rs_state,
 *    igdsp_resample, igdsp_rs_frame, igdsp_rs_taps); the sound port's delay buffer (IGDSP_DBUF_*, igdsp_dbuf_state, igdsp_dbuf_run,
 *    igdsp_dbuf_step); the spectrum graph (IGDSP_SPEC_*, igdsp_spec_state, igdsp_spec_cfg, igdsp_spec_rec, igdsp_spectrum,
 *    igdsp_spec_frame, igdsp_spec_tables); the tone detector (IGDSP_TDET_*, igdsp_tdet_*, igdsp_tone_detect); the echo canceller
 *    (IGDSP_EC_*, igdsp_ec_cfg, igdsp_ec_state, igdsp_ec_rec, igdsp_ec_cfg_default, igdsp_ec_frame, igdsp_echo_cancel); the level control
 *    (IGDSP_AGC_*, igdsp_agc_cfg, igdsp_agc_state, igdsp_agc_rec, igdsp_agc_cfg_default, igdsp_agc_frame, igdsp_agc_run); voice
 *    activity, DTX and the RFC 3389 comfort-noise payload (IGDSP_VAD_*, igdsp_vad_cfg, igdsp_vad_state, igdsp_vad_rec, igdsp_vad_event,
 *    igdsp_vad_cfg_default, igdsp_vad_table, igdsp_vad_frame, igdsp_sid_decode, igdsp_vad_work_bytes, igdsp_vad_run); comfort noise from
 *    RFC 3389 SIDs (IGDSP_CNG_*, igdsp_cng_state, igdsp_cng_rec, igdsp_cng_table, igdsp_cng_gain, igdsp_cng_frame, igdsp_cng_run); the
 *    filter (IGDSP_FILT_*, igdsp_filt_plan, igdsp_filt_state, igdsp_filt_rec, igdsp_filt_frame, igdsp_filt_plan_check,
 *    igdsp_filt_design, igdsp_filt_plan_preset, igdsp_filt_run). */
#define IGDSP_ABI_VERSION 3

/* ---- error codes (0 == PJ_SUCCESS-style success) ------------------------- */
#define IGDSP_OK          0
#define IGDSP_EINVAL    (-22)  /* bad argument (NULL, size, alignment, unknown codec)   */
#define IGDSP_ENOMEM    (-12)  /* host or device allocation failed                      */
#define IGDSP_ENODEV    (-19)  /* no usable gfx950 device / HIP runtime error            */
#define IGDSP_ENOENT     (-2)  /* call_id not mapped to a channel (a4 routing miss)      */
#define IGDSP_ERANGE    (-34)  /* channel / frame index out of the context's capacity    */
#define IGDSP_EBUSY     (-16)  /* staging ring of the channel was full: the OLDEST staged frame was overwritten */
#define IGDSP_EDEVICE   (-5)   /* kernel launch / runtime failure (see igdsp_last_error) */

/* ---- codec ids: RTP payload types, as gated at TransportAdapter.cpp:252 ---
 * (WAVE_FORMAT_MULAW 0x0007 / WAVE_FORMAT_ALAW 0x0006 of Codecs.h:33-34 are the
 * container tags; on the wire and in this ABI the RTP PT is the codec id.) */
#define IGDSP_PT_PCMU      0   /* G.711 mu-law */
#define IGDSP_PT_PCMA      8   /* G.711 A-law  */
#define IGDSP_PT_R2S     123   /* ED-137 keep-alive: never metered (TransportAdapter.cpp:299,308) */

/* ---- frame geometry (roip_ed137.h:112,115: CLOCK_RATE 8000, PTIME 20) ----- */
#define IGDSP_CLOCK_RATE          8000
#define IGDSP_PTIME_MS              20
#define IGDSP_SAMPLES_PER_FRAME    160
#define IGDSP_MAX_PAYLOAD          256   /* tp_adapter::payload_buff[256], TransportAdapter.h:66 */
#define IGDSP_STAGE_DEPTH            8   /* frames a channel can stage between two igdsp_flush calls (160 ms of audio) */
#define IGDSP_METER_FULL_SCALE   30000   /* audiometer.cpp:30-31 */

/* ---- G.711 encoder variant -------------------------------------------------
 * Decode is unique (ITU-T G.711 tables).  Two historic encoders exist; they
 * agree on every value a decoder can produce and on ITU decision values, and
 * differ only in rounding of some negative inputs / clipping:
 *   SUN16 : 16-bit-domain Sun g711.c lineage (mu-law: BIAS 0x84 added to the
 *           16-bit magnitude, clip 32635; A-law: "-pcm - 8" with the < 0 clamp).
 *   G191  : 14/13-bit-domain ITU-T G.191 STL lineage (mu-law: pcm >> 2, BIAS 0x21,
 *           clip 8159; A-law: pcm >> 3, "-pcm - 1") — bit-identical to CPython
 *           `audioop`, which pins it exhaustively (tests/golden/g711_audioop.npz).
 * WHICH of the two the reference's pjmedia build carries is UNVERIFIED: pjmedia is
 * a third-party dependency of the reference, unpinned and absent from this tree
 * (SURVEY.md 8c), and the reference holds no G.711 vector.  A maintainer with
 * pjmedia's source picks the variant by reading pjmedia/src/pjmedia/alaw_ulaw.c
 * against the two descriptions above (a ">> 2" / ">> 3" before the segment search
 * = G191; a 16-bit BIAS 0x84 / "- 8" = SUN16).  Every binding and example of this
 * repository defaults to G191, the one an independent implementation pins; the
 * round trip of DECODED codes is identical in both (closed set, tested).
 */
#define IGDSP_ENC_SUN16   0
#define IGDSP_ENC_G191    1

/* ---- per-frame flags ------------------------------------------------------- */
#define IGDSP_FLAG_SILENT   0x01  /* peak <= 8: digital silence (A 0xD5/0x55, mu 0xFF/0x7F/0xFE/0x7E) */
#define IGDSP_FLAG_PROBE_D5 0x02  /* payload[28]==payload[38]==payload[48]==0xD5: the reference's own
                                     TX silence probe on packet bytes 40/50/60 behind a 12-byte RTP
                                     header (TransportAdapter.cpp:657-673) */
#define IGDSP_FLAG_CLIPPED  0x04  /* peak == codec full scale (32124 mu / 32256 A) */
#define IGDSP_FLAG_EMPTY    0x08  /* zero-length frame (missing / keep-alive slot): all fields 0 */

/* Per channel-frame result, 16 bytes, naturally aligned.
 *  sumsq     : exact sum of x^2 over the decoded int16 samples of the frame
 *  rms       : sqrtf((float)sumsq / n)                 (fp32; oracle is float64, rel tol 1e-5)
 *  peak      : max |x|                                  (<= 32256)
 *  byte_mean : (uint8_t)(sum of raw payload bytes / n)  — bit-exact restatement of the
 *              reference's "audioLevel" (roip_ed137.cpp:6564-6568, unsigned-char target)
 *  flags     : IGDSP_FLAG_*                                                          */
typedef struct igdsp_frame_stats {
    uint64_t sumsq;
    float    rms;
    uint16_t peak;
    uint8_t  byte_mean;
    uint8_t  flags;
} igdsp_frame_stats;

/* Per-channel running aggregate / peak-hold, 32 bytes.  Mirrors the PTT-window
 * logger (keeplogAudioLevel Functions.cpp:2126-2145; reset createPTTEventDataLogger
 * Functions.cpp:2155-2167): while a channel's window is open each frame does
 * count++, level_sum += byte_mean, level_max/min update, plus (new) sumsq_acc and
 * peak_hold for the decoded-domain meter.  Reset state: all 0, level_min = 255. */
typedef struct igdsp_chan_hold {
    uint64_t sumsq_acc;   /* sum of frame sumsq over the window                       */
    uint32_t count;       /* frames accumulated (trx::level_in_count)                 */
    uint32_t level_sum;   /* exact sum of byte_mean; reference's uint16 OutgoingRTPSum
                             (roip_ed137.h:741) equals (uint16_t)level_sum             */
    uint32_t samples;     /* samples accumulated (count * n for full frames)          */
    uint16_t peak_hold;   /* running max |x|                                          */
    uint8_t  level_max;   /* trx::OutgoingRTPmax (init 0)                             */
    uint8_t  level_min;   /* trx::OutgoingRTPmin (init 255)                           */
    uint32_t n_silent;    /* frames flagged IGDSP_FLAG_SILENT                         */
    uint32_t n_clipped;   /* frames flagged IGDSP_FLAG_CLIPPED                        */
} igdsp_chan_hold;

/* Node/launch aggregate: the packed vector of SURVEY 8(e).  All u64 so that ONE
 * sum all-reduce (RCCL ncclSum over int64) yields sums AND the max: rank g writes
 * its local peak only into peak_slot[g]; after the sum every rank holds all peaks. */
#define IGDSP_AGG_MAX_RANKS 8
/* Every counter owns a 128-byte line: a persistent launch ends with one device atomic per block per counter, and
 * atomics on ONE line serialise (~95 per microsecond) - seven counters sharing a line cost ~8 us per launch on
 * MI355X, on separate lines ~3 us (tools/agg_ab.py).  The padding is zero, so the struct is still summed as one
 * vector of IGDSP_AGG_WORDS uint64. */
#define IGDSP_AGG_LINE_WORDS 16
typedef struct igdsp_aggregate {
    uint64_t sumsq;         uint64_t pad0[IGDSP_AGG_LINE_WORDS - 1];   /* sum of sumsq over all frames      */
    uint64_t samples;       uint64_t pad1[IGDSP_AGG_LINE_WORDS - 1];   /* samples metered                   */
    uint64_t frames;        uint64_t pad2[IGDSP_AGG_LINE_WORDS - 1];   /* non-empty frames metered          */
    uint64_t n_silent;      uint64_t pad3[IGDSP_AGG_LINE_WORDS - 1];
    uint64_t n_clipped;     uint64_t pad4[IGDSP_AGG_LINE_WORDS - 1];
    uint64_t byte_mean_sum; uint64_t pad5[IGDSP_AGG_LINE_WORDS - 1];   /* sum of byte_mean (checksum-of-checksums) */
    uint64_t peak_slot[IGDSP_AGG_MAX_RANKS];                            /* this rank's peak in slot[rank]    */
    uint64_t pad6[IGDSP_AGG_LINE_WORDS - IGDSP_AGG_MAX_RANKS];
} igdsp_aggregate;
#define IGDSP_AGG_WORDS (7 * IGDSP_AGG_LINE_WORDS)

/* What igdsp_poll returns for one channel: everything host code needs to fill
 * trx::IncomingRTP (roip_ed137.cpp:6570-6585) and feed updateInputLevel(int percent)
 * (roip_ed137.cpp:584-592; scale audiometer.cpp:30-31). */
typedef struct igdsp_level {
    uint8_t  byte_mean;   /* -> trx->radioN->IncomingRTP / OutgoingRTP               */
    uint8_t  flags;
    uint16_t peak;
    float    rms;
    int32_t  percent;     /* int(float(rms*100.0/30000.0)), AudioMeter::onValueChanged */
    uint16_t peak_hold;
    uint16_t dropped;     /* frames overwritten in the staging ring before a flush took them (saturates at 65535) */
    uint32_t frames;      /* frames metered for this channel since create            */
} igdsp_level;

typedef struct igdsp_ctx igdsp_ctx;

/* ---- lifecycle -------------------------------------------------------------- */

/* Create a context on HIP device `device` with staging capacity for
 * `max_channels` concurrent calls.  Allocates the pinned host slab
 * [max_channels][160], its device mirror, result buffers and a private stream.
 * Fails with IGDSP_ENODEV when no gfx950 device/runtime is usable — there is
 * no CPU fallback. */
int igdsp_create(igdsp_ctx **out, int device, uint32_t max_channels);
int igdsp_destroy(igdsp_ctx *ctx);
/* Human-readable text of the last runtime error on this context ("" if none). */
const char *igdsp_last_error(const igdsp_ctx *ctx);
int igdsp_abi_version(void);
/* Device the context is bound to; number of CUs (for grid sizing reports). */
int igdsp_device_info(const igdsp_ctx *ctx, int *device, int *compute_units, char *name, size_t name_len);

/* ---- a4: call-id -> channel routing (roip_ed137.cpp:6519-6534, 6570-6585) ---- */
int igdsp_map_call(igdsp_ctx *ctx, int32_t call_id, uint32_t channel);
int igdsp_unmap_call(igdsp_ctx *ctx, int32_t call_id);

/* ---- (i) single-frame entry, callable from setIncomingRTP/setOutgoingRTP -------
 * Inputs are exactly what those hooks read from tp_adapter: callID, payload
 * pointer, payload length (roip_ed137.cpp:6549-6552) and the RTP PT
 * (TransportAdapter.cpp:252).  Copies `payload` (borrowed; pjmedia owns pkt) into
 * the channel's staging ring (IGDSP_STAGE_DEPTH frames deep: the reference's hook runs on every frame,
 * TransportAdapter.cpp:303, and so every frame reaches the meter) and returns; never blocks on the device.  Safe to
 * call concurrently from several media threads for DIFFERENT channels.  If the owner thread has not flushed for more
 * than IGDSP_STAGE_DEPTH frames the oldest staged frame of the channel is overwritten, counted in igdsp_level.dropped,
 * and the call returns IGDSP_EBUSY (the new frame IS staged).  pt == 123 (R2S keep-alive) and unknown PTs are accepted
 * and ignored (returns 0, nothing staged), like the reference which meters only pt != 123.  payloadlen > 256 ->
 * IGDSP_EINVAL (the reference would overflow payload_buff[256] there, TransportAdapter.cpp:286). */
int igdsp_on_rtp_frame(igdsp_ctx *ctx, int32_t call_id, uint8_t pt,
                       const uint8_t *payload, uint32_t payloadlen);

/* Take every frame staged since the previous flush (all of them, oldest first per channel), upload them compacted in
 * one copy, meter them — whole 160-byte frames through the tuned chunk kernel once 64 or more are staged, everything else
 * through the general kernel — fold EVERY frame into the per-channel hold state (keeplogAudioLevel semantics per frame,
 * Functions.cpp:2126-2145) and make each channel's newest record visible to igdsp_poll.  Called by ONE owner thread per
 * context (e.g. the reference's 40 ms timer, roip_ed137.cpp:1756).  `n_frames_out` (optional) receives the number of
 * staged frames processed. */
int igdsp_flush(igdsp_ctx *ctx, uint32_t *n_frames_out);

/* Non-blocking form of igdsp_flush, for owner threads that must not wait (the reference's hook and its 40 ms timer slot never
 * wait: TransportAdapter.cpp:303, roip_ed137.cpp:1756).  igdsp_flush_begin snapshots the staged frames, enqueues upload, kernels
 * and downloads on the context's stream and returns; igdsp_flush_end waits for that work (normally finished long before the next
 * tick) and publishes the levels for igdsp_poll.  wait == 0: return IGDSP_EBUSY instead of waiting if the device has not finished.
 * igdsp_flush == begin + end(wait = 1).  A begin while the previous flush is still open ends it first (waiting).  igdsp_poll /
 * igdsp_get_hold / igdsp_get_probe read the PUBLISHED snapshot and never wait for a flush in flight. */
int igdsp_flush_begin(igdsp_ctx *ctx, uint32_t *n_frames_out);
int igdsp_flush_end(igdsp_ctx *ctx, int wait);

/* The third hook of the reference's boundary, setIncomingED137Value(uint32_t value, pjsua_acc_id) (roip_ed137.h:273; called by
 * transport_rtp_cb with ntohl(adapter->ed137_value), TransportAdapter.cpp:305,313): records the call's current ED-137 word (host
 * order).  Frames staged by igdsp_on_rtp_frame AFTER it carry that word, and igdsp_flush folds a frame into the call's window only
 * if the word passes the context's gate mode (igdsp_set_gate_mode: IGDSP_GATE_* below; default IGDSP_GATE_ALWAYS = every frame,
 * the round-2 behaviour).  Wait-free for the caller, like igdsp_on_rtp_frame.  igdsp_get_probe: the call's consecutive-silence
 * state (adapter->rtpFalse, TransportAdapter.cpp:657-673) as of the last finished flush. */
int igdsp_set_ed137(igdsp_ctx *ctx, int32_t call_id, uint32_t ed137_value);
int igdsp_set_gate_mode(igdsp_ctx *ctx, uint32_t gate_mode);
struct igdsp_chan_probe;
int igdsp_get_probe(igdsp_ctx *ctx, uint32_t channel, struct igdsp_chan_probe *out);

/* (iii) results poll for one channel (valid after a flush). */
int igdsp_poll(igdsp_ctx *ctx, uint32_t channel, igdsp_level *out);
int igdsp_poll_call(igdsp_ctx *ctx, int32_t call_id, igdsp_level *out);
/* (iv) reset the peak-hold / window aggregate of one channel (PTT press,
 * Functions.cpp:2155-2167). channel == UINT32_MAX resets all. */
int igdsp_reset_hold(igdsp_ctx *ctx, uint32_t channel);
/* Read back the hold state of one channel. */
int igdsp_get_hold(igdsp_ctx *ctx, uint32_t channel, igdsp_chan_hold *out);

/* ---- (ii) batched device entries ----------------------------------------------
 * All d_* pointers are DEVICE pointers on the context's device.  Layout is
 * time-major, as frames arrive: payload[f][c][n] u8, codec[c] u8 (RTP PT 0 / 8),
 * stats[f][c], pcm[f][c][n] i16.  n = samples_per_frame (1..256; 160 is the tuned
 * path).  d_len (optional, may be NULL) gives a per-frame valid length
 * len[f][c] <= n for ragged input; bytes past len are ignored; len 0 marks an
 * empty slot.  Work is enqueued on `stream` (a hipStream_t; NULL = the legacy
 * default stream) and NOT synchronised. */

/* a1+a3+a5+a7: decode + meter.  d_pcm may be NULL (meter-only, the headline).
 * d_agg (optional) is an igdsp_aggregate on the device that this launch ADDS
 * into (zero it first with igdsp_agg_reset); rank selects the peak slot. */
int igdsp_decode_meter(igdsp_ctx *ctx,
                       const uint8_t *d_payload, const uint8_t *d_codec, const uint16_t *d_len,
                       uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame,
                       igdsp_frame_stats *d_stats, int16_t *d_pcm,
                       igdsp_aggregate *d_agg, uint32_t rank, void *stream);

/* a2: encode int16 PCM -> G.711 codes, per-channel law. variant = IGDSP_ENC_*. */
int igdsp_encode(igdsp_ctx *ctx,
                 const int16_t *d_pcm, const uint8_t *d_codec,
                 uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame,
                 uint8_t *d_payload_out, int variant, void *stream);

/* a1+a2+a5+a6 fused (config #5): decode -> stats -> re-encode -> per-channel hold.
 * d_gate[c] (optional): 0 = window closed (frame metered but not folded into
 * hold), non-zero = open.  d_hold[c] persists across launches. */
int igdsp_roundtrip_peakhold(igdsp_ctx *ctx,
                             const uint8_t *d_payload, const uint8_t *d_codec,
                             uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame,
                             uint8_t *d_payload_out, igdsp_frame_stats *d_stats,
                             igdsp_chan_hold *d_hold, const uint8_t *d_gate,
                             int variant, void *stream);

/* Fold stats[f][c] into hold[c] (for callers that ran igdsp_decode_meter). */
int igdsp_hold_update(igdsp_ctx *ctx, const igdsp_frame_stats *d_stats,
                      uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame,
                      igdsp_chan_hold *d_hold, const uint8_t *d_gate, void *stream);
int igdsp_hold_reset(igdsp_ctx *ctx, igdsp_chan_hold *d_hold, uint32_t n_channels,
                     const uint8_t *d_reset_mask, void *stream);

int igdsp_agg_reset(igdsp_ctx *ctx, igdsp_aggregate *d_agg, void *stream);

/* ---- ED-137 RTP depayload + gather on the device ------------------
 * The step BEFORE the path: transport_rtp_cb's header parse and payload copy
 * (TransportAdapter.cpp:240-292; header layout ed137_rtp.h:22-48), batched.
 * Input  : packets[f][c][pkt_stride] raw RTP packets as received (slot of pkt_stride bytes,
 *          pkt_stride % 4 == 0), sizes[f][c] = received size (NULL: every packet fills its slot),
 *          radio[c] != 0 => 20-byte ED-137 header (12 B RTP + ext hdr 0x0167/len 1 + ED-137 word),
 *          else plain 12-byte RTP (TransportAdapter.cpp:270,279).
 * Output : payload[f][c][n] dense (bytes past the payload length zeroed), len[f][c] = metered payload
 *          length (0 for PT 123 keep-alives, non-G.711 PTs, runts, and oversize packets — the
 *          reference drops payloads it cannot buffer, TransportAdapter.cpp:286-291), info[f][c].
 * `len` feeds igdsp_decode_meter's d_len directly. */
typedef struct igdsp_rtp_info {
    uint32_t ed137;        /* ntohl(ED-137 word), 0 on non-radio calls (get_ed137_value, TransportAdapter.cpp:337-346) */
    uint16_t payload_len;  /* size - header, before any clamp (what transport_rtp_cb stores in payload_bufSize)       */
    uint8_t  pt;           /* RTP payload type (7 bits)                                                              */
    uint8_t  flags;        /* IGDSP_RTP_*                                                                            */
} igdsp_rtp_info;
#define IGDSP_RTP_V2        0x01  /* version field == 2                                   */
#define IGDSP_RTP_X         0x02  /* header-extension bit                                 */
#define IGDSP_RTP_MARKER    0x04
#define IGDSP_RTP_ED137_OK  0x08  /* radio call, X set, profile 0x0167, length 1          */
#define IGDSP_RTP_KEEPALIVE 0x10  /* PT 123 (R2S): never metered                          */
#define IGDSP_RTP_METERED   0x20  /* PT 0 or 8 with a usable payload: len[f][c] > 0       */
#define IGDSP_RTP_RUNT      0x40  /* size < header                                        */
#define IGDSP_RTP_OVERSIZE  0x80  /* payload longer than n: dropped                       */
/* ED-137 word fields, masks as the reference extracts them (Functions.cpp:1018,1045,1136,1148) */
#define IGDSP_ED137_PTT_TYPE(v) (((v) & 0xe0000000u) >> 29)
#define IGDSP_ED137_SQU(v)      (((v) & 0x10000000u) >> 28)
#define IGDSP_ED137_PTT_ID(v)   (((v) & 0x0fc00000u) >> 22)
#define IGDSP_ED137_BSS(v)      (((v) & 0x000000f8u) >> 3)

int igdsp_depayload(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_radio,
                    uint32_t n_channels, uint32_t n_frames, uint32_t pkt_stride, uint32_t samples_per_frame,
                    uint8_t *d_payload_out, uint16_t *d_len_out, igdsp_rtp_info *d_info_out, void *stream);

/* ---- Fused fast path: packet slots straight into the meter (depayload + decode + meter in ONE kernel) ----
 * For receivers that deposit radio-call packets (20-byte ED-137 header + 160-byte G.711 payload = 180 bytes,
 * TransportAdapter.cpp:846) into fixed 192-byte slots laid out so the payload is 16-byte aligned:
 *     bytes 0..1   received packet size (uint16 LE)         bytes 2..11  reserved (0)
 *     bytes 12..31 the 20-byte header (custom_rtp_hdr)      bytes 32..191 payload
 * slots[f][c][192].  A frame is metered iff size == 180 and its RTP PT equals codec[c] (0 or 8); every
 * other slot (PT 123 keep-alive, other PT, other size) gets an IGDSP_FLAG_EMPTY record — route those
 * rare frames through igdsp_depayload + igdsp_decode_meter(d_len) if they must be metered.
 * d_info (optional) receives the same igdsp_rtp_info igdsp_depayload would produce. */
#define IGDSP_SLOT_BYTES      192
#define IGDSP_SLOT_HDR_OFFSET  12
#define IGDSP_SLOT_PAYLOAD_OFFSET 32
int igdsp_decode_meter_rtp(igdsp_ctx *ctx, const uint8_t *d_slots, const uint8_t *d_codec,
                           uint32_t n_channels, uint32_t n_frames,
                           igdsp_frame_stats *d_stats, igdsp_rtp_info *d_info,
                           igdsp_aggregate *d_agg, uint32_t rank, void *stream);

/* The same fused kernel over packets packed exactly as igdsp_depayload takes them: packets[f][c][pkt_stride]
 * (pkt_stride % 4 == 0, >= hdr_bytes + 160), sizes[f][c] (NULL: every packet is hdr_bytes + 160 long), ONE header
 * type per launch (hdr_bytes = 20 for ED-137 radio legs, 12 for plain SIP legs).  Piece addresses are only dword
 * aligned here; gfx950 global loads need no more.  Metered iff size == hdr_bytes + 160 and PT == codec[c]. */
int igdsp_decode_meter_packets(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_codec,
                               uint32_t n_channels, uint32_t n_frames, uint32_t pkt_stride, uint32_t hdr_bytes,
                               igdsp_frame_stats *d_stats, igdsp_rtp_info *d_info,
                               igdsp_aggregate *d_agg, uint32_t rank, void *stream);

/* The same again with a PER-CHANNEL header length: d_radio[c] != 0 -> 20-byte ED-137 header, 0 -> 12-byte RTP header
 * (radio legs and plain SIP legs in one launch, as in the reference's process, TransportAdapter.cpp:265-292).
 * pkt_stride >= 180.  Metered iff size == header + 160 and PT == codec[c]; info as igdsp_depayload would give it. */
int igdsp_decode_meter_packets_mixed(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_codec,
                                     const uint8_t *d_radio, uint32_t n_channels, uint32_t n_frames, uint32_t pkt_stride,
                                     igdsp_frame_stats *d_stats, igdsp_rtp_info *d_info,
                                     igdsp_aggregate *d_agg, uint32_t rank, void *stream);

/* ---- SURVEY 8(f) rank 1, last clause: squelch / PTT gating of the meter from the ED-137 word, on the device ---------------------
 * The reference folds a frame's level into the PTT window (keeplogAudioLevel, Functions.cpp:2126-2145) while the window is open,
 * and reads PTT / squelch out of the ED-137 word of the RTP header extension (masks: PTT type Functions.cpp:1136, PTT id :1148,
 * SQU :1160, BSS :1018).  A window here is the per-channel igdsp_chan_hold; a metered frame (f, c) is folded into hold[c] iff
 *     (d_gate == NULL || d_gate[c] != 0)                     the caller's per-channel window state (eventPttSQL_In_LoggingOn)
 *  && frame_gate(gate_mode, ED-137 word of the frame's OWN packet)
 * with frame_gate = 1 (ALWAYS), SQU bit set (SQU), PTT type != 0 (PTT), either (SQU_OR_PTT).  Legs without an ED-137 word
 * (12-byte RTP header: the word reads 0, as get_ed137_value gives it) are therefore never folded under SQU / PTT gating.
 * Independently of the gate, d_probe[c] follows the reference's consecutive-silence counter (adapter->rtpFalse,
 * TransportAdapter.cpp:657-673): a metered frame long enough to hold the probe bytes (payload length > 48) adds 1 to `run` when
 * its IGDSP_FLAG_PROBE_D5 is set and clears `run` when it is not; shorter / empty frames leave it; `alarms` counts how often
 * `run` reached probe_alarm (the reference logs at exactly 500).  Frames of a channel are taken in frame order f = 0 .. F-1. */
#define IGDSP_GATE_ALWAYS      0u
#define IGDSP_GATE_SQU         1u
#define IGDSP_GATE_PTT         2u
#define IGDSP_GATE_SQU_OR_PTT  3u
#define IGDSP_PROBE_ALARM    500u   /* TransportAdapter.cpp:666 */
typedef struct igdsp_chan_probe {
    uint32_t run;        /* consecutive probe-matching frames up to now (adapter->rtpFalse)   */
    uint32_t alarms;     /* times run reached the alarm length                                 */
} igdsp_chan_probe;
typedef struct igdsp_window {
    uint32_t gate_mode;           /* IGDSP_GATE_*                                                                    */
    uint32_t probe_alarm;         /* 0 = IGDSP_PROBE_ALARM                                                           */
    igdsp_chan_hold *d_hold;      /* [C] window aggregate the gated frames are folded into (required)                */
    const uint8_t *d_gate;        /* [C] optional per-channel window state, 0 = closed                               */
    igdsp_chan_probe *d_probe;    /* [C] optional consecutive-silence state                                          */
    void *d_work;                 /* igdsp_window_work_bytes(C) bytes of device scratch, 16-byte aligned (48 B x 8 x C): */
                                  /* igdsp_decode_meter_window's fused kernels need it (the per-segment window / run     */
                                  /* summaries of the form that keeps the windows in registers); not used by             */
                                  /* igdsp_window_update.  One buffer per stream that launches                           */
} igdsp_window;
size_t igdsp_window_work_bytes(uint32_t n_channels);

/* Fold records into the window: the generalisation of igdsp_hold_update to per-FRAME gates.  d_info (optional) = the
 * igdsp_rtp_info[F][C] of igdsp_depayload / the fused packet entries: supplies each frame's ED-137 word (NULL: word 0) and,
 * when d_len is NULL, its length (payload_len clamped to samples_per_frame; NULL as well: samples_per_frame).  EMPTY records
 * are skipped.  One thread per channel walks its F frames in order. */
int igdsp_window_update(igdsp_ctx *ctx, const igdsp_frame_stats *d_stats, const igdsp_rtp_info *d_info, const uint16_t *d_len,
                        uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, const igdsp_window *win, void *stream);

/* The fused packet entries with the window folded in the SAME launch: packets -> records (+ info, aggregate) -> hold[c] and
 * probe[c], one pass over the packets.  layout selects the packet format and which of the arguments apply:
 *   IGDSP_PKT_SLOTS  = igdsp_decode_meter_rtp            (192-byte slots; d_sizes, d_radio, pkt_stride, hdr_bytes ignored)
 *   IGDSP_PKT_PACKED = igdsp_decode_meter_packets        (pkt_stride, hdr_bytes 12 / 20, optional d_sizes; d_radio ignored)
 *   IGDSP_PKT_MIXED  = igdsp_decode_meter_packets_mixed  (pkt_stride, d_radio, optional d_sizes; hdr_bytes ignored)
 * Same argument rules and records as those entries.  With n_channels % 64 == 0 and win->d_work given the windows are kept on
 * the chip during the launch, in one of two forms the library picks by shape: a workgroup owns 64 / 128 / 256 consecutive
 * channels for the launch, keeps their windows and silence runs in its LDS and writes hold[c] / probe[c] itself (launches of
 * more than 255 frames go out in parts on the stream); or a wavefront keeps 64 channels' windows and runs in registers over a
 * segment of the frames, the segments' summaries go through d_work and are folded in frame order by a small second kernel.
 * Integer sums / max / min and an in-order run either way: bit-identical to the sequential fold.  Other channel counts, or
 * d_work == NULL, run the plain fused kernel followed by igdsp_window_update on the same stream; d_info has to be given then
 * (it carries each frame's ED-137 word and length).  On the fused path d_stats may be NULL: a host that only wants the windows
 * (the PTT logger) then pays for no per-frame record at all — the launch reads the packets and writes hold / probe. */
#define IGDSP_PKT_SLOTS   0u
#define IGDSP_PKT_PACKED  1u
#define IGDSP_PKT_MIXED   2u
int igdsp_decode_meter_window(igdsp_ctx *ctx, uint32_t layout, const uint8_t *d_packets, const uint16_t *d_sizes,
                              const uint8_t *d_codec, const uint8_t *d_radio, uint32_t n_channels, uint32_t n_frames,
                              uint32_t pkt_stride, uint32_t hdr_bytes, igdsp_frame_stats *d_stats, igdsp_rtp_info *d_info,
                              igdsp_aggregate *d_agg, uint32_t rank, const igdsp_window *win, void *stream);

/* ---- recorder-compatible output on the device (WavWriter.cpp:63-156) ------------------------------
 * The step AFTER the path.  For every channel c of a batch payload[F][C][n] one complete file image exactly as the
 * reference's recorder would leave it after writeRTPWav(frame 0) ... writeRTPWav(frame F-1), stop():
 *     files + c * file_stride : [ 44-byte header | every payload byte b as the two bytes {b, 0x00} ]   (44 + 2 F n bytes)
 * header = WavWriter::start's (RIFF / WAVE / "fmt " 16, tag 7, "channels" 2, rate, rate * 4, align 4, 16 bits, "data") with
 * the two sizes WavWriter::stop patches in (36 + 2 F n and 2 F n).  file_stride >= 44 + 2 F n; a multiple of 4 (and n % 8
 * == 0) takes the tiled streaming kernel, anything else a byte-wise one.  Fastest (0.77 of the HBM peak instead of 0.70)
 * when (d_files + 44) % 128 == 0 and file_stride % 128 == 0: the payload-derived bytes of every file are then line-aligned.  Byte-identical to the host recorder
 * (igdsp_wav_* in the host mirror) and to the REAL WavWriter.cpp (tests/golden/config1_4ch_50f.npz). */
int igdsp_wav_expand(igdsp_ctx *ctx, const uint8_t *d_payload, uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame,
                     uint32_t rate, uint8_t *d_files, uint64_t file_stride, void *stream);

/* ---- G.726 code-word reorder (RoIP_ED137::changeUplinkOrder, roip_ed137.cpp:6379-6499) ----
 * Repacks G.726 code words between the RFC 3551 and AAL2 bit orders, bug-for-bug as the reference
 * does it on its (unsigned-char) target:
 *   mode 1 (16 kbit/s, 2-bit): the four 2-bit fields of every byte are reversed          (:6382-6389)
 *   mode 2 (24 kbit/s, 3-bit): 3-byte groups through the reference's bit-field struct   (:6390-6441)
 *   mode 3 (32 kbit/s, 4-bit): nibbles swapped                                           (:6442-6449)
 *   mode 4 (40 kbit/s, 5-bit): 5-byte groups; the reference's 2-bit field S2_ receives
 *          `(b0 >> 5) & 0x04`, which never fits, so those two output bits are always 0  (:6450-6498)
 * n_bytes must be a multiple of the group size (1, 3, 1, 5): the reference over-reads otherwise. */
int igdsp_g726_reorder(igdsp_ctx *ctx, const uint8_t *d_in, uint8_t *d_out, uint64_t n_bytes, int g726UplinkBitrate, void *stream);

/* ---- ED-137 TX packetizer: transport_send_rtp on the device (TransportAdapter.cpp:635-874) --------------------------------
 * The send half of the adapter, batched: a launch's worth of outgoing frames in, the packets transport_send_rtp hands to
 * pjmedia_transport_send_rtp out, bit for bit, plus what the reference derives on the way (ED-137 word, keep-alive choice,
 * marker, audioLevel).  Radio legs only (adapter->radiostatus, :641).  Frame f of channel c is one call of transport_send_rtp at
 * now = t0_ms + f * frame_ms, frames of a channel in order:
 *   1 stream packet (what pjmedia encodes before the adapter sees it): 0x80, M << 7 | pt, seq, ts, ssrc (network order), then
 *     the frame's n G.711 bytes.  Frame f carries seq + f (mod 2^16) and ts + f * n; every frame advances them, sent or not.
 *   2 TX silence run (:657-673): only if 12 + n > 60; stream bytes 40, 50, 60 all 0xD5 -> run++ (qint16), else run = 0.
 *   3 Idle-in zeroing (:675-679): calltype contains "Idle" and callIn -> sql = ptt = 0 (persists).
 *   4 gate (:680-706): (ptt && !callIn) || (sql && callIn) copies the payload into the send buffer (d_last_payload, persists);
 *     otherwise (uint64)(now - r2sSendtime) < (uint64)keepAlivePeroid && !firstR2SPacket -> NOT SENT (size 0, nothing else
 *     changes), and a difference >= the period sets r2sSendtime = now (the quint64 wrap of now < r2sSendtime included).
 *   5 header (:712-796, custom_rtp_hdr ed137_rtp.h:22-48): 0x90 (x = 1), m = firstR2SPacket && packetCnt == 0, profile 0x0167,
 *     length 1; word = slave-enable debounce base (steady: 00 -> 0, 11 -> 0x131c0, rx -> 0x13140, tx -> 0x13180; changing: copy,
 *     count = min(count + 1, 5), 00 -> 0x13100) | sql ? 1 << 28 | bssi << 3 & 0xf8 : !ptt ? 1 << 22 : 0 | ptt ? pttid << 22 &
 *     0x0fc00000 | pttpriority << 29 & 0xe0000000 : 0; pt = 123 on an Rx leg with !callIn.
 *   6 size / PT ladder (:804-839) as written: 20 bytes with pt 123, or 20 + n.  A 20 + n packet whose frame the gate did not
 *     copy carries the send buffer's STALE payload (the last gated frame, zeros before any).
 *   7 counters (:849-856): packetCnt / firstR2SPacket after every sent frame.
 *   8 audioLevel (roip_ed137.cpp:6510-6517): sent with pt != 123 -> (uint8_t)(sum of the first n STREAM-packet bytes as signed
 *     char / (int)n), header bytes included.
 * The calltype predicates (case-sensitive QString::contains) are evaluated once on the host into IGDSP_TX_CT_* bits. */
#define IGDSP_TX_CT_IDLE   0x01   /* contains "Idle"                     */
#define IGDSP_TX_CT_RX     0x02   /* contains "Rxonly" or equals "Rx"    */
#define IGDSP_TX_CT_TX     0x04   /* contains "Tx" or contains "TRx"     */
/* Per-channel persistent state (device-resident, 64 bytes): tp_adapter's send-side fields (TransportAdapter.h:40-93).  Host code
 * may change fields between launches: those are the setters setAdapterPtt / setTxRxSlaveEnable / setAdapterQslOn / setAdapterPttId /
 * setcallRecorder (TransportAdapter.cpp:136-210); setTxRxSlaveEnable writes *_changed and zeroes slave_count. */
typedef struct igdsp_tx_chan {
    uint64_t r2s_send_ms;       /* adapter->r2sSendtime (ms)                                        */
    uint32_t ts;                /* stream RTP timestamp of the next frame                           */
    uint32_t ssrc;
    int32_t  keepalive_ms;      /* adapter->keepAlivePeroid                                         */
    int32_t  packet_cnt;        /* adapter->packetCnt                                               */
    uint16_t seq;               /* stream RTP sequence number of the next frame                     */
    uint8_t  pt;                /* stream RTP payload type (0 mu-law, 8 A-law)                      */
    uint8_t  first_r2s;         /* adapter->firstR2SPacket                                          */
    uint8_t  tx_slave, rx_slave, tx_slave_changed, rx_slave_changed;
    int32_t  slave_count;       /* adapter->trxSlaveEnableChangedCount                              */
    uint8_t  ptt, sql, call_in, call_recorder;
    uint8_t  pttid, pttpriority, bssi, calltype;   /* calltype = IGDSP_TX_CT_* bits                 */
    int16_t  tx_run;            /* adapter->rtpFalse (qint16)                                       */
    uint8_t  level;             /* last outgoing audioLevel (OutgoingRTP)                           */
    uint8_t  reserved0;
    uint32_t reserved[4];
} igdsp_tx_chan;
/* Per-frame output, 8 bytes. */
typedef struct igdsp_tx_info {
    uint32_t ed137;             /* the ED-137 word, host order (0 when not sent)                    */
    uint16_t size;              /* bytes handed to pjmedia_transport_send_rtp: 0 (not sent), 20, 20 + n */
    uint8_t  flags;             /* IGDSP_TX_*                                                       */
    uint8_t  level;             /* audioLevel when IGDSP_TX_LEVEL_VALID, else 0                     */
} igdsp_tx_info;
#define IGDSP_TX_SENT          0x01
#define IGDSP_TX_KEEPALIVE_PT  0x02   /* pt 123 on the wire                                         */
#define IGDSP_TX_MARKER        0x04
#define IGDSP_TX_STALE_PAYLOAD 0x08   /* 20 + n bytes carrying the send buffer, not this frame      */
#define IGDSP_TX_LEVEL_VALID   0x10   /* setOutgoingRTP ran: level is the new OutgoingRTP           */
/* d_ctl[f][c] bits (optional array). */
#define IGDSP_TX_CTL_PTT   0x01
#define IGDSP_TX_CTL_SQL   0x02
#define IGDSP_TX_CTL_MARK  0x04   /* the stream header's M bit                                     */
#define IGDSP_TX_CTL_SET   0x80   /* setAdapterPtt / setAdapterQslOn before this frame: ptt = bit 0, sql = bit 1 */

/* transport_adapter_create's defaults (TransportAdapter.cpp:108-127, zalloc for the rest): first_r2s = 1, r2s_send_ms = now_ms,
 * keepalive_ms, call_in, calltype bits; seq / ts / ssrc / pt are the stream's.  Host-only, no GPU needed.  pt > 127 -> EINVAL. */
int igdsp_tx_chan_init(igdsp_tx_chan *h, const char *calltype, int call_in, uint8_t pt, uint32_t ssrc, uint16_t seq0,
                       uint32_t ts0, int32_t keepalive_ms, uint64_t now_ms);
/* IGDSP_TX_CT_* bits of a calltype string (NULL -> 0).  Host-only. */
int igdsp_tx_calltype_bits(const char *calltype);
/* Exactly one of d_pcm[f][c][n] (int16, encoded on the fly, law from the channel's pt: 8 A-law, else mu-law; variant =
 * IGDSP_ENC_*) or d_g711[f][c][n] (already encoded).  d_ctl[f][c] optional.  d_state[c], d_last_payload[c][n] persist across
 * launches (zero the payloads once).  d_packets[f][c][pkt_stride]: pkt_stride % 4 == 0, >= 20 + n, <= 2048, the layout
 * igdsp_depayload reads; bytes past sizes[f][c] are never written, and an unsent frame leaves its slot untouched.
 * d_sizes[f][c], d_info[f][c] required. */
int igdsp_tx_packetize(igdsp_ctx *ctx, const int16_t *d_pcm, const uint8_t *d_g711, const uint8_t *d_ctl,
                       uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, uint64_t t0_ms, uint32_t frame_ms,
                       igdsp_tx_chan *d_state, uint8_t *d_last_payload, uint8_t *d_packets, uint32_t pkt_stride,
                       uint16_t *d_sizes, igdsp_tx_info *d_info, int variant, void *stream);

/* ---- Staged ED-137 send path: transport_send_rtp as pjmedia calls it (TransportAdapter.cpp:635-874) ------------------------
 * The drop-in form of the packetizer above.  pjmedia calls transport_send_rtp(tp, pkt, size) once per leg per frame, on the
 * conference bridge's clock, with the stream packet it has already encoded; the adapter setters change the leg between calls from
 * other threads.  Here the call stages the packet (igdsp_on_tx_frame), the setters stage their values, and the owner thread
 * packetises everything staged once per bridge tick on the device (igdsp_tx_flush), then hands each packet to
 * pjmedia_transport_send_rtp itself.  Radio legs only (adapter->radiostatus, :641).
 *
 * Each staged frame is exactly one call of the reference's transport_send_rtp at currenttime = now_ms, for its leg, in staging
 * order, with the eight steps of igdsp_tx_packetize, except that bytes 2..11 of the output header, and the stream bytes the
 * audioLevel sum and the silence probe read (byte 1 with the stream's M bit included), are the staged packet's own, and
 * n = size - 12 is per frame (1 <= n <= 236: send_pkt_buff[256] holds 20 + n, TransportAdapter.h:69).  The send buffer is one
 * persistent 236-byte region per leg: a gated frame overwrites [0, n) of it, so a stale packet carries older bytes past a shorter
 * copy, as the reference does.
 *
 * Legs: igdsp_tx_open opens one on the channel igdsp_map_call gave call_id, with transport_adapter_create's defaults
 * (:108-127); the first igdsp_tx_open of a context allocates the TX staging and device state (RX-only users pay nothing).  A
 * second igdsp_tx_open of the same channel starts over from the defaults; igdsp_tx_close drops the leg's staged frames (counted in
 * igdsp_tx_counts' dropped).  A producer must not stage on a leg while it is opened or closed.
 * Staging (igdsp_on_tx_frame): wait-free for the caller — a single-producer ring per leg, IGDSP_STAGE_DEPTH frames deep (one
 * producer per leg: pjmedia serialises send_rtp per stream).  A full ring refuses the NEW frame with IGDSP_EBUSY (counted in
 * refused).  Rejected with IGDSP_EINVAL: NULL, a packet that is not RTP V = 2 with P = X = 0 and CC = 0, n outside [1, 236]
 * (pjmedia's own stream never produces them; the reference would read them undefined).  No open leg: IGDSP_ENOENT.
 * Setters: igdsp_tx_set_* are the adapter setters (:135-223).  Wait-free too; each changes only the fields it names.  They apply in
 * happens-before order with the same leg's igdsp_on_tx_frame: one that returned before frame k was staged takes effect before
 * frame k's step; one racing with the staging of frame k lands on k or on k + 1, never lost or torn; one after the last staged
 * frame carries over to the next.  The device's own changes (Idle-in zeroing of ptt / sql) survive setters of other fields.
 * igdsp_tx_set_sql: bssi < 0 is the 3-argument overload (bssi unchanged); priority is accepted and unused, as sqlpriority is
 * zeroed before every use (:739).  igdsp_tx_set_slave zeroes the debounce count, as setTxRxSlaveEnable does.
 * Flush (igdsp_tx_flush, ONE owner thread; may run concurrently with igdsp_flush / igdsp_flush_begin on another thread, it has its
 * own stream and buffers): takes every staged frame, packetises them in one upload / kernel / download, and returns when the
 * results are readable.  igdsp_tx_results: one entry per processed frame, legs in channel order and frames in staging order,
 * unsent frames (size 0) included; valid until the next igdsp_tx_flush.  igdsp_tx_get_chan: the leg's state as of the last
 * finished flush (staged setters not yet applied). */
typedef struct igdsp_tx_packet {
    const uint8_t *pkt;         /* `size` bytes for pjmedia_transport_send_rtp; valid until the next igdsp_tx_flush          */
    int32_t  call_id;
    uint32_t ed137;             /* host order, 0 when not sent                                                              */
    uint16_t size;              /* 0 (keep-alive rate limit: not sent), 20, or 20 + n                                       */
    uint8_t  flags;             /* IGDSP_TX_* as in igdsp_tx_info                                                           */
    uint8_t  level;             /* OutgoingRTP when IGDSP_TX_LEVEL_VALID                                                    */
} igdsp_tx_packet;
#define IGDSP_TX_MAX_N     236   /* largest payload of a staged frame                                               */
int igdsp_tx_open(igdsp_ctx *ctx, int32_t call_id, const char *calltype, int call_in, int32_t keepalive_ms, uint64_t now_ms);
int igdsp_tx_close(igdsp_ctx *ctx, int32_t call_id);
int igdsp_tx_set_ptt(igdsp_ctx *ctx, int32_t call_id, int ptt, int priority, int user_rec);   /* setAdapterPtt       */
int igdsp_tx_set_sql(igdsp_ctx *ctx, int32_t call_id, int sql, int priority, int32_t bssi);  /* setAdapterQslOn     */
int igdsp_tx_set_ptt_id(igdsp_ctx *ctx, int32_t call_id, int pttid);                         /* setAdapterPttId     */
int igdsp_tx_set_slave(igdsp_ctx *ctx, int32_t call_id, int rx, int tx);                     /* setTxRxSlaveEnable  */
int igdsp_tx_set_recorder(igdsp_ctx *ctx, int32_t call_id, int on);                          /* setcallRecorder     */
int igdsp_tx_set_calltype(igdsp_ctx *ctx, int32_t call_id, const char *calltype);            /* setCallType         */
/* the body of transport_send_rtp: stage pjmedia's stream packet (12-byte RTP header + n G.711 bytes); now_ms = currenttime */
int igdsp_on_tx_frame(igdsp_ctx *ctx, int32_t call_id, const void *pkt, uint32_t size, uint64_t now_ms);
int igdsp_tx_flush(igdsp_ctx *ctx, uint32_t *n_frames_out);
int igdsp_tx_results(igdsp_ctx *ctx, const igdsp_tx_packet **out, uint32_t *n_out);
int igdsp_tx_get_chan(igdsp_ctx *ctx, int32_t call_id, igdsp_tx_chan *out);
/* frames of the call's leg refused by a full ring / dropped by igdsp_tx_close, since its igdsp_tx_open (either pointer may be NULL) */
int igdsp_tx_counts(igdsp_ctx *ctx, int32_t call_id, uint32_t *refused, uint32_t *dropped);

/* ---- Conference mix: the bridge step after RX decode (pjmedia's conference bridge as the reference drives it) -------------------
 * Every call's conference slot is connected to the sound-card channel slots (on_call_media_state, roip_ed137.cpp:4907-4917, through
 * connectPort / disconnectPort, Functions.cpp:718-740), and each call's receive level is set with pjsua_conf_adjust_rx_level(conf_slot,
 * SLOT_VOLUME) (setSlotVolume, roip_ed137.cpp:5190-5233): steps of 0.1f within [0, 2] (roip_ed137.h:246-247), 2.0 at start
 * (roip_ed137.cpp:210), 2.0 / 0.0 for the PTT-priority unmute / mute (roip_ed137.cpp:6140-6320), the sidetone level or 0.5 while the
 * local operator transmits (setvolumeSiteTone, roip_ed137.cpp:6869-6878; Functions.cpp:1660-1700).  The bridge scales each source by
 * its level, sums the sources connected to an output port and plays the result.
 *
 * igdsp_conf_mix does that step for a batch of frames: a PORT is an output (a sound-card channel, a console, a recorder), its members
 * are channels, given as CSR: members[port_ptr[p] .. port_ptr[p + 1]).  For frame f, port p, sample s:
 *   x   = the decoded sample of member m (the G.711 tables of igdsp_decode_meter; with d_pcm the PCM value); 0 when s >= len[f][m]
 *   a   = clamp16(trunc(x * gain[m] / 128))          C integer division, toward zero (an arithmetic >> 7 differs for negative x)
 *   S   = the exact sum of a over the port's members (64-bit; member order does not matter)
 *   out[f][p][s] = clamp16(S)
 * Records [f][p] over out, as igdsp_frame_stats: sumsq exact, rms = sqrtf((float)sumsq / n), peak = max |out| (up to 32768),
 * byte_mean 0, flags IGDSP_FLAG_SILENT (peak <= 8) | IGDSP_FLAG_SATURATED (a clamp of either stage fired in this port-frame).
 * EMPTY: the port has no member < n_channels with len > 0 in this frame (no members, members >= n_channels only, or every member's
 * len 0): out is zeros and the record is igdsp_decode_meter's len-0 record (all 0, IGDSP_FLAG_EMPTY).  EMPTY depends on membership
 * and len only, never on the gain: a muted member keeps the frame live.
 * A bad table is safe: members >= n_channels contribute nothing and are never dereferenced, port_ptr values are clamped to n_members,
 * a port with port_ptr[p + 1] < port_ptr[p] is empty, and a member listed twice is mixed twice (igdsp_conf_build removes duplicates).
 *
 * Fidelity.  The Q7 rule is pjmedia's receive-level adjustment as it is commonly published (itemp = itemp * adj / 128, clamped to
 * int16), and pjsua's float level -> adj mapping is (int)((level - 1) * 128) with adj = 128 + that (igdsp_conf_level_q7).  Both are
 * UNVERIFIED here: pjmedia is a third-party dependency of the reference and is not in this tree.  pjmedia's adaptive normalisation
 * of a sum of several transmitters is deliberately NOT restated: the mix saturates instead; the two agree whenever at most one
 * member of a port contributes (the PTT arbitration's usual state: one call unmuted, the others at level 0).  A port row that must
 * not clip goes through igdsp_agc_run ("Level control" below) behind the mix. */
#define IGDSP_FLAG_SATURATED 0x10  /* igdsp_conf_mix: a per-member or the final int16 clamp fired in this port-frame */
/* Q7 receive level of a float slot volume: 128 + (int)((level - 1.0f) * 128.0f) in float arithmetic, as pjsua converts it
 * (0.0 -> 0, 0.1f -> 13, 0.5 -> 64, 1.0 -> 128, 2.0 -> 256).  IGDSP_EINVAL for NaN, a negative result (an adjustment below -128)
 * or a result above 65535.  Host-only, no GPU needed. */
int igdsp_conf_level_q7(float level);
/* The CSR of a connection list: n_conn (channel[i], port[i]) pairs -> port_ptr[n_ports + 1] and members[] (room for n_conn entries),
 * *n_members written.  Members sorted by port, then channel; duplicate connections removed (pjsua_conf_connect of an existing
 * connection is a no-op).  A channel >= n_channels or port >= n_ports -> IGDSP_EINVAL, nothing written.  Host-only. */
int igdsp_conf_build(const uint32_t *channel, const uint32_t *port, uint32_t n_conn, uint32_t n_channels, uint32_t n_ports,
                     uint32_t *port_ptr, uint32_t *members, uint32_t *n_members);
/* Exactly one input: d_payload[f][c][n] G.711 with d_codec[c] (RTP PT: 8 A-law, else mu-law), or d_pcm[f][c][n] int16.  d_len[f][c]
 * optional (as igdsp_decode_meter).  d_gain[c] Q7 (128 = unity), d_port_ptr[n_ports + 1], d_members[n_members] (may be NULL when
 * n_members is 0).  At least one of d_out[f][p][n] int16 and d_stats[f][p].  n = 1..256.  n_ports == 0 or n_frames == 0: nothing to
 * do.  Enqueued on `stream`, not synchronised. */
int igdsp_conf_mix(igdsp_ctx *ctx, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm, const uint16_t *d_len,
                   const uint16_t *d_gain, const uint32_t *d_port_ptr, const uint32_t *d_members, uint32_t n_members,
                   uint32_t n_channels, uint32_t n_ports, uint32_t n_frames, uint32_t samples_per_frame,
                   int16_t *d_out, igdsp_frame_stats *d_stats, void *stream);

/* ---- Best signal selection: the ED-137 receiver vote between depayload and the bridge -------------------------------------------
 * A gateway hears one frequency through several receivers; each one's ED-137 word carries its squelch (SQU, bit 28) and a 5-bit BSS
 * quality index (bits 7-3).  The reference (SERVER mode, rxBestSignalEnable, on by default) votes for one receiver in checkEvents
 * (roip_ed137.cpp:5985-6119) over its four radios, from get_IPRadioSquelch / get_IPRadioBss (Functions.cpp:1001-1022), and plays it
 * by slot volume (setvolume, Functions.cpp:1664-1705): every open radio MUTE, the voted one UNMUTE (SLOT_VOLUME 2.0 = Q7 256).
 *
 * igdsp_bss_select runs that vote for n_groups groups (one frequency each) over n_frames frames.  A group's members are channels, as
 * CSR: member slots k in [group_ptr[g], group_ptr[g + 1]); their ORDER is the tie-break order (the reference's fixed trx1.radio1,
 * trx1.radio2, trx2.radio1, trx2.radio2).  Per frame f, in order:
 *   1. Words.  For EVERY slot k < n_members with c = members[k] < n_channels: words[k] = info[f][c].ed137 iff the frame carries a
 *      stored word, i.e. !(info.flags & IGDSP_RTP_RUNT) and info.pt is 0, 8, 18 or 123 (transport_rtp_cb, TransportAdapter.cpp:
 *      247-256, 408-415; 123 is the R2S keep-alive); otherwise words[k] keeps its value.  Words are kept per slot, not per channel:
 *      a channel listed twice is two slots with the same word.
 *   2. Squelch, per member: rx = SQU(words[k]) && c < n_channels && !(d_mute && d_mute[g]); rssi = BSS(words[k]).
 *   3. Step the group's state (count, on, voted):
 *      - if the voted member has rx == 0 (or voted names no slot of the group): count = 0, on = 0, voted = 0;
 *      - if any member has rx: count = min(count + 1, UINT32_MAX); if count >= vote_frames and !on: on = 1, votes += 1 (mod 2^32),
 *        voted = 1 + the position of the FIRST member (in member order) whose rx holds and whose rssi is >= every open member's;
 *      - otherwise count = 0, on = 0, voted = 0.
 *      A vote LATCHES: a stronger receiver that opens later does not take over.  When the voted receiver closes while others stay
 *      open the count restarts in that same frame (it is 1 there) and a new vote follows vote_frames - 1 frames later.
 *   4. Emit.  sel[f][g] = members[b + voted - 1] (a channel < n_channels), or -1 when nothing is voted.  With audio, for the voted
 *      channel c: out[f][g][s] = clamp16(trunc(x * gain[c] / 128)) for s < len[f][c] (x: the decoded sample as igdsp_conf_mix reads
 *      it), 0 past len; the record [f][g] over out as igdsp_conf_mix writes it (sumsq, rms, peak, byte_mean 0, IGDSP_FLAG_SILENT,
 *      IGDSP_FLAG_SATURATED when the clamp fired).  Nothing voted, or the voted member's len 0: out is zeros and the record is
 *      igdsp_decode_meter's len-0 record (all 0, IGDSP_FLAG_EMPTY).  A voted frame equals igdsp_conf_mix of a one-member port.
 * The state (d_state[g]) and the words (d_words[k]) carry the vote across launches: F launches of one frame give the same bits as one
 * launch of F frames.  An all-zero state is the reset state (a memset resets it); zero words are closed receivers.  The state
 * belongs to one table: rebuilding group_ptr / members means resetting the state and the words.  igdsp_conf_build sorts members by
 * channel, so a host that wants a priority order other than channel order builds the CSR itself.
 * An all-zero igdsp_rtp_info is a PT-0 packet with word 0, not a missing frame: a missing frame carries IGDSP_RTP_RUNT, as
 * igdsp_depayload writes it for size 0.
 * A bad table is safe: group_ptr values are clamped to n_members, a group with group_ptr[g + 1] < group_ptr[g] is empty, members
 * >= n_channels are calls that are not up (never read, never open, never voted).
 *
 * Fidelity.  PINNED to the reference: the vote, the latch, the count restart, the tie order and the word rule (step 1).
 * UNVERIFIED: pjmedia's Q7 level arithmetic, as for igdsp_conf_mix.  DIFFERENT ON PURPOSE: (a) the tick is one frame (the reference
 * runs checkEvents on its 40 ms timer and on audio edges), so the threshold is vote_frames (IGDSP_BSS_VOTE_FRAMES = 5 ticks of 40 ms
 * at 20 ms frames); (b) what a receiver plays before the first vote depends on volume history outside the reference's BSS block:
 * here it is silence; (c) a dropped call (member >= n_channels) is a closed receiver, where the reference keeps its stale lastRx.
 * The force-mute / group-PTT rule (roip_ed137.cpp:5630-5655) is d_mute[g], set by the host per launch (its SqlGroupDelay release
 * stays on the host).  The lastRxmsec hold (roip_ed137.cpp:5658-5669) is dead code in the reference and has no counterpart. */
typedef struct igdsp_bss_state {  /* per group, 16 bytes; ALL-ZERO = reset */
    uint32_t count;               /* sqlStatusCount, saturating                                                      */
    uint32_t voted;               /* 1 + position of the voted member in the group's member list, 0 = none (audioSQLOn) */
    uint32_t on;                  /* sqlStatusOn (any non-zero value is on; written back as 0 / 1)                  */
    uint32_t votes;               /* votes taken so far (telemetry, wraps)                                           */
} igdsp_bss_state;
#define IGDSP_BSS_VOTE_FRAMES 10  /* default threshold: 5 ticks of the reference's 40 ms timer at 20 ms frames */
/* d_info[f][c] (igdsp_depayload's records) required.  Audio, at most one: d_payload[f][c][n] G.711 with d_codec[c] (RTP PT: 8 A-law,
 * else mu-law), or d_pcm[f][c][n] int16; d_len[f][c] optional (as igdsp_decode_meter).  d_gain[c] Q7, NULL = 256 (UNMUTE at
 * SLOT_VOLUME 2.0).  d_group_ptr[n_groups + 1] required, d_members[n_members] (n_members <= 2^24; NULL when 0).  d_mute[g] optional.
 * vote_frames 0 = IGDSP_BSS_VOTE_FRAMES.  d_state[n_groups] and d_words[n_members] required (read and written).  Outputs, each
 * optional: d_sel[f][g], d_out[f][g][n] int16, d_stats[f][g]; d_out and d_stats need an audio input.  Without audio only sel, the
 * state and the words are produced (n is then still checked: 1..256).  n_groups == 0 or n_frames == 0: nothing to do.  Enqueued
 * on `stream`, not synchronised. */
int igdsp_bss_select(igdsp_ctx *ctx, const igdsp_rtp_info *d_info,
                     const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm, const uint16_t *d_len,
                     const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members, uint32_t n_members,
                     const uint8_t *d_mute, uint32_t n_channels, uint32_t n_groups, uint32_t n_frames, uint32_t samples_per_frame,
                     uint32_t vote_frames, igdsp_bss_state *d_state, uint32_t *d_words,
                     int32_t *d_sel, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream);

/* ---- PTT priority arbitration: who may key a transmitter, the send-direction twin of the receiver vote ------------------------------
 * Several call-in legs (consoles) may key one frequency.  The reference (inviteMode == CLIENT) arbitrates them in checkEvents
 * (roip_ed137.cpp:6124-6231) by the PTT type of their ED-137 words (get_IPRadioPttStatus, Functions.cpp:1045-1139): the highest type
 * takes the transmitter, every other pressed leg is muted by slot volume, and a release is debounced.  igdsp_ptt_arbitrate runs that
 * loop for n_groups groups (one frequency or transmitter each) over n_frames frames, one tick per frame.
 *
 * A group's members are channels, as CSR: member slots k in [group_ptr[g], group_ptr[g + 1]); their ORDER is the reference's
 * trx_incall order and decides ties.  group_ptr values are clamped to n_members and a descending pair is an empty group, as in
 * igdsp_bss_select.  Persistent: d_state[g] (igdsp_ptt_state) and d_slots[k] (igdsp_ptt_slot); ALL-ZERO is the reset state of both.
 * Both are read defensively, so that a garbage state stays in bounds: a holder larger than the group counts as 0, level is taken
 * & 7, pressed != 0 counts as pressed.
 *
 * Per frame f, first per slot (every slot k < n_members steps once per frame, whichever groups list it):
 *   1. Word.  With c = members[k] < n_channels: slot.word = info[f][c].ed137 iff the frame stores a word; igdsp_bss_select's step 1
 *      verbatim (!(flags & IGDSP_RTP_RUNT) and pt 0, 8, 18 or 123).
 *   2. Skip.  c >= n_channels: the leg has no call; the slot is left untouched and takes no part in the tick (:6131).
 *   3. PTT type.  p = (d_rxonly && d_rxonly[c]) ? 0 : IGDSP_ED137_PTT_TYPE(slot.word)  (TRXMODE_RX, :6134).
 *   4. Release debounce (:6139-6154, bug for bug):
 *      - p != last_tx and p == 0: release_cnt = min(release_cnt + 1, 255); if release_cnt < release_frames then p = 1 (the value 1,
 *        not the old type);
 *      - p != last_tx and p != 0: release_cnt unchanged;
 *      - p == last_tx: release_cnt = 0;
 *      then last_tx = p (the substituted value).
 * then per group, over its members in order (position pos), with the member's p:
 *   5. Takeover (:6157-6177): p > level: level = p, holder = pos + 1, takeovers += 1.
 *   6. Press and release (:6191-6222): p > 0 && !pressed: pressed = 1.  p == 0 && pressed: pressed = 0, holder = 0 if holder ==
 *      pos + 1, and in either case level = 0.  The reference zeroes ptt_level on ANY pressed leg's release, not only the holder's;
 *      another pressed leg then re-takes or steals the transmitter later in the same tick or in the next one.  Kept.
 * After the tick: sel[f][g] = members[b + holder - 1] if a holder exists and that channel is < n_channels, else -1.  tick[f][g]:
 * sel; level; ptt_id = IGDSP_ED137_PTT_ID of the holder's stored word (0 without a holder); flags = IGDSP_PTT_ON (some member with a
 * call is pressed after the tick) | IGDSP_PTT_PRESS (some member went pressed in it) | IGDSP_PTT_RELEASE (some member released in
 * it) | IGDSP_PTT_TAKEOVER (step 5 fired in it); ctl = IGDSP_TX_CTL_SET | (ON ? IGDSP_TX_CTL_PTT : 0).  d_ctl_out[f][g] is the ctl
 * byte alone, dense: with n_channels = n_groups it is a valid d_ctl[f][c] of igdsp_tx_packetize (it holds sql at 0).
 * Audio, optional, exactly as igdsp_bss_select's step 4: for the holder's channel c, out[f][g][s] = clamp16(trunc(x * gain[c] / 128))
 * for s < len[f][c], 0 past it; the record [f][g] over out; zeros and IGDSP_FLAG_EMPTY when nothing is held or len is 0; gain NULL =
 * 256.  The emit depends on holder only: a holder stays audible after another leg's release zeroed level, as the reference's slot
 * volume does.
 * release_frames 0 = IGDSP_PTT_RELEASE_FRAMES; valid 1..255, 1 = no debounce.  F launches of one frame give the same bits (outputs,
 * state, slots) as one launch of F frames.  The state belongs to one table: rebuilding group_ptr / members means resetting both.
 * A slot two groups list (only a bad table does) is one leg seen by both; a slot no group lists still steps, and nothing reads it.
 *
 * Fidelity.  PINNED to the reference: steps 3-6, the substitute value 1, the level reset on any release, member order.
 * DIFFERENT ON PURPOSE: (a) the tick is one frame (the reference's 40 ms timer and audio edges), so IGDSP_PTT_RELEASE_FRAMES = 12 is
 * 6 ticks of 40 ms at 20 ms frames; (b) a leg that was never unmuted is silent, where the reference starts every slot at SLOT_VOLUME
 * 2.0; (c) one holder replaces the per-leg volumes: equivalent from a reset state, where an unmuted leg is always pressed and a
 * takeover mutes every other pressed leg.  UNVERIFIED: pjmedia's Q7 level arithmetic, as for igdsp_conf_mix. */
typedef struct igdsp_ptt_state {  /* per group, 16 bytes; ALL-ZERO = reset */
    uint32_t level;               /* ptt_level: the PTT type that holds the transmitter (read & 7)                    */
    uint32_t holder;              /* 1 + position of the unmuted member in the group's member list, 0 = none          */
    uint32_t takeovers;           /* step 5 firings so far (telemetry, wraps)                                         */
    uint32_t reserved;            /* kept as it is                                                                    */
} igdsp_ptt_state;
typedef struct igdsp_ptt_slot {   /* per member slot, 8 bytes; ALL-ZERO = reset */
    uint32_t word;                /* the slot's stored ED-137 word                                                    */
    uint8_t  last_tx;             /* lastTx: the (substituted) PTT type of the last tick                              */
    uint8_t  release_cnt;         /* lastTxmsec: ticks of the release being debounced, saturating at 255              */
    uint8_t  pressed;             /* m_PttPressed (any non-zero value is pressed; written as 0 / 1 on a change)       */
    uint8_t  reserved;            /* kept as it is                                                                    */
} igdsp_ptt_slot;
typedef struct igdsp_ptt_tick {   /* per (frame, group), 8 bytes */
    int32_t  sel;                 /* the unmuted channel, -1 = none                                                   */
    uint8_t  level;               /* ptt_level after the tick                                                         */
    uint8_t  ptt_id;              /* PTT id of the holder's stored word, 0 = no holder                                */
    uint8_t  flags;               /* IGDSP_PTT_*                                                                      */
    uint8_t  ctl;                 /* IGDSP_TX_CTL_SET | IGDSP_TX_CTL_PTT iff IGDSP_PTT_ON                             */
} igdsp_ptt_tick;
#define IGDSP_PTT_ON        0x01
#define IGDSP_PTT_PRESS     0x02
#define IGDSP_PTT_RELEASE   0x04
#define IGDSP_PTT_TAKEOVER  0x08
#define IGDSP_PTT_RELEASE_FRAMES 12  /* default debounce: 6 ticks of the reference's 40 ms timer at 20 ms frames */
/* d_info[f][c], d_group_ptr[n_groups + 1], d_state[n_groups] and d_slots[n_members] required (d_members and d_slots may be NULL when
 * n_members is 0; n_members <= 2^24).  Audio, at most one: d_payload[f][c][n] G.711 with d_codec[c], or d_pcm[f][c][n]; d_len, d_gain
 * as igdsp_bss_select.  d_rxonly[c] optional.  Outputs, each optional: d_sel[f][g], d_tick[f][g], d_ctl_out[f][g], d_out[f][g][n],
 * d_stats[f][g]; d_out and d_stats need an audio input.  n = 1..256 always.  n_groups == 0 or n_frames == 0: nothing to do.  Enqueued
 * on `stream`, not synchronised. */
int igdsp_ptt_arbitrate(igdsp_ctx *ctx, const igdsp_rtp_info *d_info,
                        const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm, const uint16_t *d_len,
                        const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members, uint32_t n_members,
                        const uint8_t *d_rxonly, uint32_t n_channels, uint32_t n_groups, uint32_t n_frames, uint32_t samples_per_frame,
                        uint32_t release_frames, igdsp_ptt_state *d_state, igdsp_ptt_slot *d_slots,
                        int32_t *d_sel, igdsp_ptt_tick *d_tick, uint8_t *d_ctl_out, int16_t *d_out, igdsp_frame_stats *d_stats,
                        void *stream);

/* ---- R2S link supervision and the device event list: the body of the reference's 40 ms timer ------------------------------------------
 * Every received packet refreshes a leg's timestamp (adapter->r2sPacket, TransportAdapter.cpp:122,289,302,311, read through
 * get_R2SStatus); the reference's timer (detectR2SPacketAndReconn, roip_ed137.cpp:1756) hangs a call up with WG-67 cause 2001
 * "missing R2S KeepAlive" when the timestamp is older than 3 * r2sPeriod for six ticks in a row (roip_ed137.cpp:1764-1780, :2009-2040).
 * The same callback keeps adapter->rtpAudio: the first audio packet after keep-alives, or the first keep-alive after audio, is what
 * makes the reference call setIncomingED137Value -> checkEvents (TransportAdapter.cpp:298-315).  igdsp_link_watch runs both per
 * channel over n_ticks ticks on igdsp_depayload's records and hands back only what changed: a kind byte per (tick, channel) and a
 * compacted list of the (tick, channel) pairs whose kind meets event_mask, small enough to copy back every tick.
 *
 * Layout.  Arrival slots are igdsp_jb_receive's: a = t * slots_per_tick + k, k = 0 .. slots_per_tick - 1 the arrival order within
 * tick t, slots_per_tick = 1 .. IGDSP_STAGE_DEPTH.  d_info[a][c]: the records igdsp_depayload wrote for those slots.  d_sizes[a][c]
 * == 0: no packet in the slot; d_sizes NULL: every slot holds one.  now(t) = t0_ms + (uint64_t)t * tick_ms in wrapping uint64
 * arithmetic; every packet of tick t is stamped now(t).  Persistent: d_state[c] (igdsp_link_state); ALL-ZERO is the reset state (the
 * call is not up).  Bits of flags other than IGDSP_LINK_UP | _AUDIO | _ALARMED, and reserved, are kept as they are.
 *
 * Per tick t and channel c, in tick order, with kind = 0, word = 0, period = d_period_ms ? d_period_ms[c] : IGDSP_LINK_R2S_PERIOD_MS:
 *   1. Up.  d_up && !d_up[c]: clear IGDSP_LINK_UP, leave everything else, and end the tick with kind = 0 (the reference's else branch;
 *      its reconnect counter stays on the host).  Otherwise, if IGDSP_LINK_UP is clear: last_ms = now, count = 0, clear AUDIO and
 *      ALARMED, set UP, kind |= CAME_UP (transport_adapter_create, TransportAdapter.cpp:122 and TransportAdapter.h:91).
 *   2. Arrivals, k in order.  Every slot that holds a packet sets last_ms = now (every return path of transport_rtp_cb refreshes it).
 *      - keep-alive (!(flags & IGDSP_RTP_RUNT) && pt == 123): if AUDIO is set, clear it, kind |= AUDIO_OFF, word = info.ed137;
 *      - audio (!(flags & IGDSP_RTP_RUNT) && pt != 123 && payload_len < 1024, TransportAdapter.cpp:286,298): if AUDIO is clear, set it,
 *        kind |= AUDIO_ON, word = info.ed137;
 *      - anything else (runts, payloads of 1024 or more) only refreshes last_ms.
 *   3. Supervise (roip_ed137.cpp:1767-1780).  diff = (int64_t)(now - last_ms); a last_ms ahead of now gives a negative diff, which is
 *      never late, as with the reference's qint64.  diff > 3 * (int64_t)period: kind |= LATE; if count == miss_ticks - 1 then kind |=
 *      MISSING, set ALARMED, alarms += 1; count = min(count + 1, 65535).  Else: if count > 0 then kind |= RECOVERED; count = 0, clear
 *      ALARMED.  MISSING fires once per outage, exactly where the reference's r2sCount == 5 does with miss_ticks 6 and tick_ms 40.
 *
 * Outputs.  d_kind[t][c] (optional): the kind byte.  (t, c) is an event iff kind & event_mask (event_mask 0 = IGDSP_LINK_EVENT_DEFAULT).
 * Events are written to d_events in tick-major, then ascending channel order; d_event_count[0] = the number of events of the launch,
 * d_event_count[1] = min(that, event_cap), the number stored: the first event_cap events in that order are kept and nothing is ever
 * written past d_events[event_cap).  d_events may be NULL iff event_cap == 0; d_event_count may be NULL, then no list is produced.
 * Each launch starts its list at index 0.
 * State.  n_ticks launches of one tick, t0_ms advanced each time, give the same state bytes, kind bytes and events as one launch of
 * n_ticks ticks (each event's tick shifted by its launch).
 * Arguments.  miss_ticks 0 = IGDSP_LINK_MISS_TICKS, valid 1 .. 65535; tick_ms >= 1; d_work (igdsp_link_work_bytes bytes, 16-byte
 * aligned) is required when a list is requested, and every stream that launches needs its own; d_info and d_state are required
 * unless there is nothing to do.  n_channels == 0 or n_ticks == 0: nothing to do, the counts are written as 0.  Violations return
 * IGDSP_EINVAL before any launch (n_channels * n_ticks * slots_per_tick >= 2^32 - 32: IGDSP_ERANGE).  Enqueued on `stream`, not
 * synchronised.
 *
 * Fidelity.  PINNED to the reference: steps 2 and 3, the refresh on every packet (runts and oversize payloads included), the < 1024
 * rule, the comparison of the count with miss_ticks - 1 before the increment.  DIFFERENT ON PURPOSE: (a) the tick is one frame, so
 * IGDSP_LINK_MISS_TICKS = 12 is 6 ticks of the reference's 40 ms timer at 20 ms frames; (b) packets are stamped with their tick's
 * time, not the wall clock; (c) count saturates at 65535 where r2sCount is an int; (d) non-radio legs follow the same < 1024 rule,
 * where the reference reads a stale static rtphdr; (e) the hang-up itself, a SIP action, stays on the host: MISSING is its cue. */
#define IGDSP_LINK_R2S_PERIOD_MS 200   /* roip_ed137.h:685 */
#define IGDSP_LINK_MISS_TICKS     12   /* 6 ticks of the reference's 40 ms timer at 20 ms frames */
/* kind bits, per (tick, channel) */
#define IGDSP_LINK_AUDIO_ON   0x01     /* rtpAudio 0 -> 1 on an audio packet of this tick   */
#define IGDSP_LINK_AUDIO_OFF  0x02     /* rtpAudio 1 -> 0 on a keep-alive of this tick      */
#define IGDSP_LINK_MISSING    0x04     /* the hang-up condition fired in this tick          */
#define IGDSP_LINK_LATE       0x08     /* diff > 3 * period at this tick's check            */
#define IGDSP_LINK_RECOVERED  0x10     /* count went from > 0 to 0 in this tick             */
#define IGDSP_LINK_CAME_UP    0x20     /* the call came up in this tick                     */
#define IGDSP_LINK_EVENT_DEFAULT 0x37  /* every kind but LATE */
/* state flags */
#define IGDSP_LINK_UP       0x01
#define IGDSP_LINK_AUDIO    0x02
#define IGDSP_LINK_ALARMED  0x04
typedef struct igdsp_link_state {      /* per channel, 16 bytes, ALL-ZERO = reset (call not up) */
    uint64_t last_ms;                  /* adapter->r2sPacket                                   */
    uint32_t alarms;                   /* MISSING firings so far (telemetry, wraps)            */
    uint16_t count;                    /* r2sCount, saturating at 65535                        */
    uint8_t  flags;                    /* IGDSP_LINK_UP | _AUDIO | _ALARMED; other bits kept   */
    uint8_t  reserved;                 /* kept as it is                                        */
} igdsp_link_state;
typedef struct igdsp_link_event {      /* 16 bytes */
    uint32_t channel;
    uint32_t tick;                     /* t within this launch                                 */
    uint32_t word;                     /* ed137 of the tick's last edge packet, else 0         */
    uint16_t count;                    /* state count after the tick                           */
    uint8_t  kind;                     /* the whole kind byte of (tick, channel)               */
    uint8_t  reserved;                 /* 0 */
} igdsp_link_event;
/* bytes of d_work for a launch of this shape (host-only; grows with min(n_ticks, 128) and n_channels / 64) */
size_t igdsp_link_work_bytes(uint32_t n_channels, uint32_t n_ticks);
int igdsp_link_watch(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint16_t *d_sizes,
                     const uint8_t *d_up, const uint16_t *d_period_ms,
                     uint32_t n_channels, uint32_t n_ticks, uint32_t slots_per_tick,
                     uint64_t t0_ms, uint32_t tick_ms, uint32_t miss_ticks, uint32_t event_mask,
                     igdsp_link_state *d_state, uint8_t *d_kind,
                     igdsp_link_event *d_events, uint32_t event_cap, uint32_t *d_event_count,
                     void *d_work, void *stream);

/* ---- Jitter buffer: RTP sequence tracking and playout between depayload and the vote / the bridge ---------------------------------
 * The reference hands every packet but the keep-alives to adapter->stream_rtp_cb (TransportAdapter.cpp:301): the pjmedia stream, which
 * validates the RTP sequence, puts frames back in playout order in its jitter buffer and keeps the RTCP receive statistics.
 * igdsp_jb_receive does that step for a batch: packets in ARRIVAL order in, one playout frame per channel per tick out, in the layout
 * of igdsp_depayload, so that igdsp_decode_meter, igdsp_bss_select and igdsp_conf_mix take the outputs unchanged.
 *
 * Input.  packets[a][c][pkt_stride], sizes[a][c] (NULL: every packet fills its slot), radio[c]: igdsp_depayload's meaning.  Arrival
 * slot a = t * slots_per_tick + k for tick t = 0 .. n_ticks - 1 and k = 0 .. slots_per_tick - 1, the arrival order within the tick
 * (slots_per_tick = 1 .. IGDSP_STAGE_DEPTH).  sizes[a][c] == 0: no packet.  d_arrival[a][c] (optional): the arrival time in RTP clock
 * units (8 kHz), used only for the jitter.
 * Per packet, in arrival order (seq, ts and ssrc are RTP header bytes 2-3, 4-7 and 8-11, network order):
 *   1. No packet: nothing happens (status NONE).
 *   2. Invalid: a runt (size < header) or V != 2: invalid += 1, otherwise ignored (INVALID).
 *   3. Keep-alive: PT 123: keepalives += 1; never enters the sequence logic, as the reference passes no PT 123 to the stream.  Its
 *      record is kept for the tick (KEEPALIVE).
 *   4. New source: if a source has been heard and ssrc differs from the state's, the source part of the state resets (the A.1 / A.8
 *      fields), playout stops and the ring is discarded: discarded += frames in it, restarts += 1.
 *   5. Validation: RFC 3550 Appendix A.1 as written: a new source starts with init_seq(seq), max_seq = seq - 1, probation =
 *      MIN_SEQUENTIAL (2); then update_seq with MAX_DROPOUT 3000, MAX_MISORDER 100, RTP_SEQ_MOD 1 << 16: probation, cycle counting, and
 *      the re-sync after two sequential packets following a large jump.  A packet for which update_seq returns 0 is counted invalid and
 *      not placed (INVALID).  So the FIRST packet of a new source is never played; that is RFC behaviour.  As in A.1's C, "seq ==
 *      max_seq + 1" is an int comparison: during probation 0 does not follow 65535.
 *   6. Jitter (d_arrival given, packet accepted): RFC 3550 A.8 in integer form, all mod 2^32: transit = arrival - ts; unless this is
 *      the source's first accepted packet, d = |transit - last transit| and jitter += d - ((jitter + 8) >> 4) (jitter is scaled by 16).
 *   7. Start or placement.  Start (playout stopped, or update_seq has just run init_seq): discarded += frames in the ring, the ring is
 *      emptied, restarts += 1 if playout was running; head = seq, wait = delay_frames, and the packet goes into the ring (RESTART).
 *      Otherwise d = (int16_t)(seq - head): d < 0: late += 1, dropped (LATE); d >= IGDSP_JB_DEPTH: a Start at this packet, restarts
 *      += 1 (RESTART); else ring slot (head + d) % IGDSP_JB_DEPTH: if it already holds this seq, duplicate += 1 and the first copy is
 *      kept (DUPLICATE), otherwise the packet is placed there (PLACED).
 * Per tick t, after that tick's arrivals:
 *   - stopped, or wait > 0: IDLE (wait -= 1 if it was > 0);
 *   - playing and the head's slot holds seq head: PLAYED: that packet's payload, len and info, bit-identical to what igdsp_depayload
 *     writes for it (bytes past len zeroed, len 0 for PT 18 / other PTs / oversize, IGDSP_RTP_OVERSIZE); the slot is freed, head += 1,
 *     lost_run = 0, played += 1;
 *   - playing and the slot is empty: LOST: head += 1, lost_run += 1, lost += 1; when lost_run reaches IGDSP_JB_DEPTH playout stops and
 *     what is still in the ring is discarded (discarded += frames).  An ED-137 radio stops sending audio when its squelch closes and
 *     sends only keep-alives: its channel goes IDLE 16 ticks later;
 *   - IDLE / LOST ticks: payload zeros, len 0, info = the record of the LAST keep-alive of this tick if there was one (so
 *     igdsp_bss_select still stores its word), else {ed137 0, payload_len 0, pt 0, IGDSP_RTP_RUNT}, the missing-frame record.
 * Outputs: payload[t][c][n], len[t][c], info[t][c] (required); d_tick_flags[t][c] (optional, IGDSP_JB_PLAYED / LOST / IDLE);
 * d_pkt_status[a][c] (optional, IGDSP_JB_PKT_*).
 * State: igdsp_jb_state[c] and the ring (igdsp_jb_ring_bytes(C, n) bytes of device memory, 16-byte aligned) belong to the caller and
 * carry playout across launches: n_ticks launches of one tick give the same outputs and state, and a ring holding the same packets, as
 * one launch of n_ticks ticks.
 * All-zero is the reset state of both; resetting a channel means zeroing its state and its ring slice.  A ring belongs to one n.
 *
 * Fidelity.  PINNED to RFC 3550: A.1 (sequence validation), A.3 (igdsp_jb_report) and A.8 (jitter).  UNVERIFIED: that pjmedia's
 * rtp.c / rtcp.c use the same constants (pjmedia is a third-party dependency of the reference and is not in this tree).  DIFFERENT ON
 * PURPOSE: igdsp_jb_receive has a fixed delay (delay_frames at every playout start), where pjsua's default jbuf adapts
 * (igdsp_jb_receive_adaptive below adapts it per talkspurt); the buffer itself does no concealment, LOST ticks come out as len 0 (igdsp_plc_conceal below fills them in); keep-alive words are not delayed by the
 * buffer. */
#define IGDSP_JB_DEPTH   16      /* ring slots per channel: 320 ms at 20 ms frames */
#define IGDSP_JB_DELAY    3      /* default delay_frames: 60 ms */
#define IGDSP_JB_IDLE     1      /* d_tick_flags */
#define IGDSP_JB_PLAYED   2
#define IGDSP_JB_LOST     3
#define IGDSP_JB_PKT_NONE       0   /* d_pkt_status */
#define IGDSP_JB_PKT_INVALID    1
#define IGDSP_JB_PKT_KEEPALIVE  2
#define IGDSP_JB_PKT_PLACED     3
#define IGDSP_JB_PKT_LATE       4
#define IGDSP_JB_PKT_DUPLICATE  5
#define IGDSP_JB_PKT_RESTART    6   /* placed as the head of a (re)started playout */
#define IGDSP_JB_HEARD      0x01    /* igdsp_jb_state.flags: a source has been heard */
#define IGDSP_JB_PLAYING    0x02    /*   playout running (wait counts the pre-roll)  */
#define IGDSP_JB_TRANSIT    0x04    /*   transit holds the source's last transit     */
typedef struct igdsp_jb_state {     /* per channel, 80 bytes, ALL-ZERO = reset */
    uint32_t ssrc;
    uint32_t cycles;                /* A.1: shifted count of sequence number cycles */
    uint32_t base_seq;
    uint32_t bad_seq;               /* last 'bad' seq + 1 (RTP_SEQ_MOD + 1 = none) */
    uint32_t probation;
    uint32_t received;
    uint32_t transit;               /* A.8: last transit, mod 2^32 */
    uint32_t jitter;                /* scaled by 16 */
    uint32_t epoch;                 /* init_seq calls so far: tells igdsp_jb_report that the A.1 priors were reset */
    uint16_t max_seq;
    uint16_t head;                  /* seq of the next playout tick */
    uint8_t  wait;                  /* pre-roll ticks left */
    uint8_t  lost_run;              /* consecutive LOST ticks */
    uint8_t  flags;                 /* IGDSP_JB_HEARD | IGDSP_JB_PLAYING | IGDSP_JB_TRANSIT */
    uint8_t  reserved0;
    uint32_t played, lost, late, duplicate, invalid, keepalives, discarded, restarts;
    uint32_t reserved1;
} igdsp_jb_state;
/* What igdsp_jb_report remembers between two reports of a channel (A.3's expected_prior / received_prior); all-zero to start. */
typedef struct igdsp_jb_prior {
    uint32_t expected_prior;
    uint32_t received_prior;
    uint32_t epoch;                 /* the state's epoch the priors belong to */
    uint32_t reserved;
} igdsp_jb_prior;
/* The receiver-report fields of RFC 3550 6.4.1 for one channel. */
typedef struct igdsp_jb_rr {
    uint32_t ssrc;
    uint32_t ext_max_seq;           /* cycles + max_seq                                         */
    int32_t  cum_lost;              /* expected - received, clamped to [-0x800000, 0x7FFFFF]     */
    uint32_t jitter;                /* interarrival jitter, RTP clock units (state jitter >> 4)  */
    uint8_t  fraction_lost;         /* (lost_interval << 8) / expected_interval, 0 if none lost  */
    uint8_t  valid;                 /* 1: a source has been heard (else every field is 0)       */
    uint16_t reserved;
} igdsp_jb_rr;
/* Ring bytes for n_channels at n samples per frame: IGDSP_JB_DEPTH tags per channel, then IGDSP_JB_DEPTH slots per channel of a
 * 16-byte record head and the payload rounded up to 16 bytes.  0 for n outside 1..256.  Host-only. */
size_t igdsp_jb_ring_bytes(uint32_t n_channels, uint32_t samples_per_frame);
/* RFC 3550 A.3 over one channel's state: extended highest seq, cumulative lost (24-bit clamp), fraction lost since the report that
 * last advanced *prior (which this call advances; priors of an earlier init_seq epoch count as zero, as init_seq resets them), jitter.
 * A state with no source heard gives an all-zero report.  Host-only, no GPU needed. */
int igdsp_jb_report(const igdsp_jb_state *s, igdsp_jb_prior *prior, igdsp_jb_rr *out);
/* d_packets, d_radio, d_state, d_ring, d_payload_out, d_len_out, d_info_out required; d_sizes, d_arrival, d_tick_flags, d_pkt_status
 * optional.  pkt_stride % 4 == 0, 20 .. 2048; slots_per_tick 1 .. IGDSP_STAGE_DEPTH; delay_frames 0 .. IGDSP_JB_DEPTH - 1; n 1..256.
 * n_channels == 0 or n_ticks == 0: nothing to do.  Enqueued on `stream`, not synchronised. */
int igdsp_jb_receive(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_radio, const uint32_t *d_arrival,
                     uint32_t n_channels, uint32_t n_ticks, uint32_t slots_per_tick, uint32_t pkt_stride, uint32_t samples_per_frame,
                     uint32_t delay_frames, igdsp_jb_state *d_state, void *d_ring, uint8_t *d_payload_out, uint16_t *d_len_out,
                     igdsp_rtp_info *d_info_out, uint8_t *d_tick_flags, uint8_t *d_pkt_status, void *stream);

/* ---- Jitter buffer, adaptive: a playout delay chosen per talkspurt -------------------------------------------------------------------
 * igdsp_jb_receive_adaptive is igdsp_jb_receive with the pre-roll of every playout start taken from the channel's own igdsp_jb_adapt
 * record where igdsp_jb_receive takes delay_frames.  An ED-137 radio sends audio only while its squelch is open, so playout starts
 * again at every talkspurt, and the delay is adapted there: the classic talkspurt rule (Ramjee, Kurose, Towsley, Schulzrinne, INFOCOM
 * 1994: delay = d + 4 v at each talkspurt), with the RFC 3550 A.8 jitter of igdsp_jb_state as the variation estimate v.  No audio is
 * stretched or dropped inside a talkspurt.
 *
 * Everything in igdsp_jb_receive's text above holds, except where delay_frames was used.  Let n = samples_per_frame and
 * J = igdsp_jb_state.jitter (scaled by 16) after the packet's step 6.
 *   Start rule.  It runs at every Start of step 7, whatever caused it: playout stopped, init_seq ran, d >= IGDSP_JB_DEPTH, or the late
 *   re-sync below.  In order:
 *     cur  = (flags & IGDSP_JB_ADAPT_SET) ? delay : init_frames
 *     tj   = min(max_frames, (jitter_mult * J + 16 n - 1) / (16 n)), in 64-bit integer division
 *     want = max(tj, need)
 *     new  = want >= cur ? want : cur - 1          the delay grows at once and shrinks one frame per Start
 *     new  = clamp(new, min_frames, max_frames)
 *     if SET was on and new > delay: grows += 1; if SET was on and new < delay: shrinks += 1 (both saturate at 65535)
 *     delay = new, flags |= SET, need = 0, late_run = 0
 *     the state's wait = new, where igdsp_jb_receive writes delay_frames.
 *   LATE packet (d < 0 while playing, no init_seq): late += 1 as in igdsp_jb_receive; need = max(need, min(delay + (-d), max_frames));
 *   late_run = min(late_run + 1, 255).  If late_restart > 0 and late_run >= late_restart the packet is not dropped: it performs a Start
 *   at its seq (the late re-sync): restarts += 1, the ring is discarded as at any Start, the packet is placed and its status is
 *   RESTART.  Otherwise its status is LATE.
 *   PLACED, DUPLICATE or RESTART: late_run = 0.
 *   Other packets.  Keep-alives, invalid packets and missing slots touch nothing in igdsp_jb_adapt.  A new SSRC resets the source part
 *   of igdsp_jb_state as in igdsp_jb_receive; igdsp_jb_adapt persists, because the path is the same.
 *   d_delay_out[t][c] (optional) is igdsp_jb_adapt.delay after tick t's arrivals; 0 before the channel's first Start.
 *   d_arrival == NULL: J stays 0, so only need drives the delay.
 * Invariants.  With min_frames = max_frames = init_frames = D and late_restart = 0 every output, the state bytes and the ring bytes
 * equal igdsp_jb_receive's with delay_frames = D.  n_ticks launches of one tick equal one launch of n_ticks ticks, d_adapt included.
 * State: igdsp_jb_adapt[c] (device memory, 4-byte aligned) belongs to the caller beside d_state and d_ring; all-zero is its reset state.
 *
 * Fidelity.  PINNED: RFC 3550 A.8 as the variation estimate, and the talkspurt rule's structure (Ramjee et al., multiplier 4).
 * UNVERIFIED: pjmedia's own algorithm (pjmedia is a third-party dependency of the reference and is not in this tree).  DIFFERENT ON
 * PURPOSE: the delay changes only at playout starts, with no stretching or dropping of audio inside a talkspurt, so a continuous stream
 * adapts only through the late re-sync; there is no mean-delay term, because arrivals are quantised to ticks by the caller. */
#define IGDSP_JB_ADAPT_MIN           1
#define IGDSP_JB_ADAPT_MAX          12
#define IGDSP_JB_ADAPT_MULT          4   /* the 4 of d + 4 v */
#define IGDSP_JB_ADAPT_LATE_RESTART  3
#define IGDSP_JB_ADAPT_SET        0x01   /* igdsp_jb_adapt.flags: delay holds a value */
typedef struct igdsp_jb_adapt_cfg {      /* host memory, read during the call; NULL = the defaults */
    uint8_t min_frames, max_frames, init_frames, jitter_mult, late_restart, reserved[3];
} igdsp_jb_adapt_cfg;
typedef struct igdsp_jb_adapt {          /* per channel, 8 bytes, device, ALL-ZERO = reset */
    uint8_t delay, flags, need, late_run;
    uint16_t grows, shrinks;             /* saturate at 65535 */
} igdsp_jb_adapt;
/* The defaults: {IGDSP_JB_ADAPT_MIN, IGDSP_JB_ADAPT_MAX, IGDSP_JB_DELAY, IGDSP_JB_ADAPT_MULT, IGDSP_JB_ADAPT_LATE_RESTART}.  Host-only. */
void igdsp_jb_adapt_cfg_default(igdsp_jb_adapt_cfg *cfg);
/* The Start rule above for one channel: returns the new delay and updates *a exactly as the kernel does.  cfg NULL = the defaults.
 * IGDSP_EINVAL for a NULL a, an invalid cfg or samples_per_frame outside 1..256.  Host-only, no GPU needed. */
int igdsp_jb_adapt_next(const igdsp_jb_adapt_cfg *cfg, uint32_t jitter_q4, uint32_t samples_per_frame, igdsp_jb_adapt *a);
/* Arguments, alignment and limits as igdsp_jb_receive's, without delay_frames.  d_adapt required, 4-byte aligned; d_delay_out
 * optional.  cfg (NULL = the defaults) must satisfy min_frames <= init_frames <= max_frames <= IGDSP_JB_DEPTH - 1 and jitter_mult <=
 * 16, else IGDSP_EINVAL.  n_channels == 0 or n_ticks == 0: nothing to do.  Enqueued on `stream`, not synchronised. */
int igdsp_jb_receive_adaptive(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_radio,
                              const uint32_t *d_arrival, uint32_t n_channels, uint32_t n_ticks, uint32_t slots_per_tick, uint32_t pkt_stride,
                              uint32_t samples_per_frame, const igdsp_jb_adapt_cfg *cfg, igdsp_jb_state *d_state, void *d_ring,
                              igdsp_jb_adapt *d_adapt, uint8_t *d_payload_out, uint16_t *d_len_out, igdsp_rtp_info *d_info_out,
                              uint8_t *d_tick_flags, uint8_t *d_pkt_status, uint8_t *d_delay_out, void *stream);

/* ---- Packet loss concealment: between the jitter buffer and the bridge ------------------------------------------------------------
 * igdsp_plc_conceal turns the jitter buffer's playout ticks into continuous PCM: a LOST tick (or a PLAYED one that carries no audio)
 * repeats the last pitch period of what the channel played, fading out, and the first good tick after a loss fades back in; the
 * structure of G.711 Appendix I.  Per channel it keeps the last IGDSP_PLC_HIST output samples and the pitch cycle of the current run.
 *
 * All arithmetic is integer (Q15 weights, ">> 15" an arithmetic floor shift), so every implementation agrees bit for bit.  Notation:
 *   y[k]   the channel's history, oldest first (k = 0 .. 279): y[k] = hist[(head + k) % IGDSP_PLC_HIST];
 *   x[s]   the tick's input sample: the decoded G.711 sample or d_pcm for s < min(len, n), 0 past that (d_len NULL: len = n);
 *   w(i)   ((i + 1) << 15) / (q + 1), an integer division of positive numbers, for a blend of q samples;
 *   gain(m) max(0, 32768 - max(0, m - IGDSP_PLC_FLAT) * IGDSP_PLC_STEP): full gain for 10 ms, -20 % per 10 ms, silence from 60 ms;
 *   S(m)   the synthetic sample at run index m: (cycle[pos] * gain(m) + 16384) >> 15, then pos = (pos + 1) % pitch.
 * Per tick t and channel c, in tick order (tick flags as igdsp_jb_receive writes them):
 *   1. Good: PLAYED with len > 0.  missing == 0: out = x.  Otherwise the recovery: q = pitch >> 2; for i < min(q, n)
 *      out[i] = (S(missing + i) * (32768 - w(i)) + x[i] * w(i) + 16384) >> 15, out[i] = x[i] past that; then missing = 0.
 *   2. Concealed: LOST, or PLAYED with len == 0 (undecodable PTs, oversize frames).  If missing == 0 a run starts:
 *      - pitch search: D(p) = sum_{i<160} |y[120 + i] - y[120 + i - p]| for p = IGDSP_PLC_PMIN .. IGDSP_PLC_PMAX; p = the smallest D,
 *        the smallest p on ties (the key (D << 7) | p fits 32 bits: one min-reduction gives both rules);
 *      - cycle: q = p >> 2; cycle[i] = y[280 - p + i] for i < p - q; for i = p - q .. p - 1, j = i - (p - q):
 *        cycle[i] = (y[280 - p + i] * (32768 - w(j)) + y[280 - 2p + i] * w(j) + 16384) >> 15; entries >= p are left as they were;
 *      - pitch = p, pos = 0, runs += 1;
 *      - fade-in with no added delay: for i < min(q, n) out[i] = (y[279 - i] * (32768 - w(i)) + S(i) * w(i) + 16384) >> 15 (the
 *        reversed tail blended into the cycle), out[i] = S(i) past that.
 *      Otherwise (a run goes on) out[i] = S(missing + i).  Then missing = min(missing + n, 65535) and concealed += 1.
 *   3. IDLE, or any other flag value: out = 0 and missing = 0.  No recovery fade ever follows an IDLE tick.
 *   4. Every tick appends out[0 .. n) to the ring at head, then head = (head + n) % IGDSP_PLC_HIST (n <= 256 < 280: a tick never
 *      overlaps itself).
 * Every blend is convex, so no clamp is needed and every product fits int32.  The state is read as head % IGDSP_PLC_HIST, pitch
 * clamped to [IGDSP_PLC_PMIN, IGDSP_PLC_PMAX] and pos % pitch, and written back so: a garbage state stays in bounds.
 * Outputs: d_out[t][c][n] int16; d_len_out[t][c] = n, 0 for IDLE ticks; d_stats[t][c] the record igdsp_conf_mix writes, over out
 * (sumsq, rms, peak, byte_mean 0, IGDSP_FLAG_SILENT) plus IGDSP_FLAG_CONCEALED on concealed ticks; IDLE ticks get the len-0 record
 * (all 0, IGDSP_FLAG_EMPTY).  (d_out, d_len_out) feed igdsp_conf_mix / igdsp_bss_select through their d_pcm / d_len inputs unchanged.
 * The state carries concealment across launches: n_ticks launches of one tick give the same outputs and state bytes as one launch of
 * n_ticks ticks.  All-zero is the reset state (its history is silence).  A state belongs to one n.
 *
 * Fidelity.  The reference delegates concealment to pjmedia, which is not in this tree.  UNVERIFIED: which algorithm pjmedia applies.
 * PINNED to G.711 Appendix I's structure: the constants (pitch range 40 .. 120, a 20 ms match window, 10 ms at full gain, -20 % per
 * 10 ms, silence from 60 ms, a quarter-period overlap-add at both edges of a loss).  DIFFERENT ON PURPOSE: no 3.75 ms output delay
 * (the reversed-tail fade-in replaces it); one pitch period throughout, where Appendix I widens to 2 and 3 periods after 10 and
 * 20 ms; an integer AMDF pitch search (average magnitude difference), not a normalised float correlation; Q15 arithmetic. */
#define IGDSP_PLC_PMIN   40    /* shortest pitch period, samples (200 Hz)            */
#define IGDSP_PLC_PMAX  120    /* longest pitch period (66.7 Hz)                     */
#define IGDSP_PLC_SPAN  160    /* samples compared per candidate period (20 ms)      */
#define IGDSP_PLC_HIST  280    /* history kept per channel = SPAN + PMAX             */
#define IGDSP_PLC_FLAT   80    /* concealed samples at full gain (10 ms)             */
#define IGDSP_PLC_STEP   82    /* Q15 gain decrement per sample after that           */
#define IGDSP_FLAG_CONCEALED 0x20  /* record flag: this tick's output is synthetic  */
typedef struct igdsp_plc_state {   /* per channel, 832 bytes, ALL-ZERO = reset */
    int16_t  hist[IGDSP_PLC_HIST]; /* ring: history sample k (0 = oldest) is hist[(head + k) % HIST] */
    int16_t  cycle[IGDSP_PLC_PMAX];/* the pitch cycle of the current / last run   */
    uint16_t head, pitch, pos;     /* ring head; period of the last run; next cycle index */
    uint16_t missing;              /* samples concealed in the current run, saturating at 65535; 0 = no run */
    uint32_t runs, concealed;      /* telemetry, wrapping: runs started, ticks concealed */
    uint32_t reserved[4];
} igdsp_plc_state;
/* d_tick_flags[t][c] (IGDSP_JB_*), d_state[c] and d_out[t][c][n] required.  Exactly one input: d_payload[t][c][n] G.711 with
 * d_codec[c] (RTP PT: 8 A-law, else mu-law; igdsp_decode_meter's tables), or d_pcm[t][c][n] int16.  d_len[t][c], d_len_out[t][c]
 * and d_stats[t][c] optional.  n = 1..256.  n_channels == 0 or n_ticks == 0: nothing to do.  Outputs must not overlap the inputs.
 * Enqueued on `stream`, not synchronised. */
int igdsp_plc_conceal(igdsp_ctx *ctx, const uint8_t *d_tick_flags,
                      const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm, const uint16_t *d_len,
                      uint32_t n_channels, uint32_t n_ticks, uint32_t samples_per_frame,
                      igdsp_plc_state *d_state, int16_t *d_out, uint16_t *d_len_out,
                      igdsp_frame_stats *d_stats, void *stream);

/* ---- Sound-card splitter / combiner: the last step of the tick, between the bridge's ports and the card -------------------------------
 * The reference hands the bridge's audio to its slave sound card through pjmedia's splitter / combiner: initSlaveSoundCard
 * (roip_ed137.cpp:3314-3435) creates a 6-channel pjmedia_splitcomb at 8 kHz, puts the bridge's master port on channel 0, adds a reverse
 * channel per further card channel as the conference ports sc_ch1_slot .. sc_ch5_slot and connects the combiner to the card's player;
 * on_call_audio_state (:4907-4920) connects every call to every one of those ports in both directions.  The ports of igdsp_conf_mix
 * are those card channels.
 *
 * A CARD has K channels, 1 <= K <= IGDSP_SND_MAX_CHANNELS (the reference's has 6).  A card frame is n samples of K interleaved int16:
 * frames[f][d][s][k], n = 1..256.  The mono side is dense: card d, channel k is row d * K + k — port p of igdsp_conf_mix in the
 * playback direction, channel c of a d_pcm input in the capture direction.  There is no map table: igdsp_conf_mix's CSR does the
 * routing, and a port without members already comes out as zeros.
 *   igdsp_snd_combine (playback: the splitcomb's get_frame over its reverse channels' put_frame)
 *       frames[f][d][s][k] = pcm[f][d * K + k][s]
 *   igdsp_snd_split   (capture: the splitcomb's put_frame, the reverse channels' get_frame)
 *       pcm[f][d * K + k][s] = frames[f][d][s][k]
 * Both are bit for bit, so split(combine(x)) == x.  Records [f][d * K + k] over that row's n samples, as igdsp_conf_mix writes them:
 * sumsq exact, rms = sqrtf((float)sumsq / n), peak = max |x| (32768 for -32768), byte_mean 0, flags IGDSP_FLAG_SILENT when peak <= 8
 * and nothing else.  igdsp_snd_combine's records are the OUT VU of the card's channels and igdsp_snd_split's the IN VU: the
 * per-card-channel in1..in4 / out1..out4 numbers the reference receives from an outside process over its WebSocket
 * (roip_ed137.cpp:7686-7716) and folds into the PTT window (keeplogAudioLevel).  Their [F][C] layout is what igdsp_hold_update takes
 * with n_channels = n_cards * card_channels, so a PTT window over a card channel needs nothing new.
 * At least one of the bulk output and d_stats must be given: records only is a pure meter over PCM, bulk only a pure transpose.  The
 * input is required; n_cards == 0 or n_frames == 0: nothing to do.  n_cards * card_channels * n_frames < 2^32 - 32 (IGDSP_ERANGE).
 * d_pcm and d_frames 2-byte, d_stats 8-byte aligned; the output must not be the input, and the buffers must not overlap at all.
 * Enqueued on `stream`, not synchronised.
 *
 * Fidelity.  UNVERIFIED: the interleaving order s * K + k is the standard PCM layout the ALSA card takes; pjmedia's splitcomb.c is not
 * in the reference tree.  DIFFERENT ON PURPOSE: pjmedia's reverse channels carry a delay buffer because the bridge and the card have
 * separate clocks; these two entries buffer nothing, and the delay buffer is a step of its own between them and the bridge
 * (igdsp_dbuf_run, "Delay buffer" below).  The reference opens only a player on this card
 * (pjmedia_snd_port_create_player; the bidirectional pjmedia_snd_port_create is commented out at :3411-3420), so its capture direction
 * carries silence today although both directions are wired; igdsp_snd_split is the step that wiring implies. */
#define IGDSP_SND_MAX_CHANNELS 8
int igdsp_snd_combine(igdsp_ctx *ctx, const int16_t *d_pcm /* [F][D*K][n] */, uint32_t n_cards, uint32_t card_channels,
                      uint32_t n_frames, uint32_t samples_per_frame,
                      int16_t *d_frames /* [F][D][n][K] */, igdsp_frame_stats *d_stats /* [F][D*K] */, void *stream);
int igdsp_snd_split(igdsp_ctx *ctx, const int16_t *d_frames /* [F][D][n][K] */, uint32_t n_cards, uint32_t card_channels,
                    uint32_t n_frames, uint32_t samples_per_frame,
                    int16_t *d_pcm /* [F][D*K][n] */, igdsp_frame_stats *d_stats /* [F][D*K] */, void *stream);

/* Host only, no GPU: the numbers a broadcastVUMeter message carries for one card channel, from its record.  percent is
 * int(float(rms * 100.0 / 30000.0)), exactly igdsp_level.percent; db = 20 * log10(rms / 32768.0) in double, IGDSP_SND_DB_FLOOR for
 * rms == 0.  UNVERIFIED: the outside process's own dB scale is not in the reference tree.  IGDSP_EINVAL for a NULL argument. */
#define IGDSP_SND_DB_FLOOR (-100.0)
typedef struct igdsp_snd_vu_t {
    int32_t percent;
    uint32_t reserved;
    double  db;
} igdsp_snd_vu_t;
int igdsp_snd_vu(const igdsp_frame_stats *st, igdsp_snd_vu_t *out);

/* ---- Tone generator: the bridge's last source, the ring tone --------------------------------------------------------------------------
 * RoIP_ED137::init_ringTone (Functions.cpp:532-571, called at roip_ed137.cpp:3082) creates a pjmedia_tonegen port (8 kHz, mono, 160
 * samples, 16 bit, PJMEDIA_TONEGEN_LOOP), plays a 440 + 480 Hz dual tone of 2 000 ms on / 1 000 ms off and adds the port to the bridge;
 * playRing / stopRing (Functions.cpp:523-531) connect and disconnect it to port 0 and rewind it.  A tone PORT here is one such
 * generator: a row of PCM per frame that igdsp_conf_mix takes as one more d_pcm channel.  Everything is integer.
 *
 * PLAN (igdsp_tone_plan_build, host only, no GPU): count = 1..IGDSP_TONE_MAX descriptors with pjmedia_tone_desc's fields; clock_rate a
 * multiple of 1 000 in 8 000..48 000; freq1 in 1..clock_rate / 2 - 1, freq2 0 (single tone) or in the same range; volume <= 32767,
 * 0 = IGDSP_TONE_VOLUME; reserved 0; options a combination of IGDSP_TONE_LOOP and IGDSP_TONE_NO_FADE.  Per tone i:
 *   on = on_msec * clock_rate / 1000, off likewise (integer division); start_i = sum over j < i of (on_j + off_j);
 *   step(f) = ((f << 32) + clock_rate / 2) / clock_rate in 64 bits, step2 = 0 for a single tone;
 *   fade_in = clock_rate / 1000, fade_out = clock_rate / 500, both 0 with IGDSP_TONE_NO_FADE or when on < fade_in + fade_out.
 * cycle = sum of (on_i + off_i) must be >= 1.  Anything else: IGDSP_EINVAL, nothing written.
 *
 * OSCILLATOR.  T[i] = floor(32767 sin(2 pi i / 1024) + 0.5), i = 0..1023, a list of constants in the source (no libm at run time;
 * T[256] = 32767, T[i] = -T[1024 - i]).  For sample offset k >= 0 inside a tone's ON period, per oscillator:
 *   ph = (uint32_t)(k * step);  i = ph >> 22;  fr = (ph >> 6) & 0xFFFF
 *   osc = T[i] + (((T[(i + 1) & 1023] - T[i]) * fr) >> 16)                  arithmetic shift = floor
 *   single: a = (osc1 * vol) >> 15          dual: a = ((osc1 + osc2) * vol) >> 16
 *   k < fade_in:        a = a * k / fade_in                                 C division, toward zero
 *   k >= on - fade_out: a = a * (on - 1 - k) / fade_out
 * The phase restarts at 0 at every tone start.  Against float64 the oscillator is within 2 of 32767 sin(2 pi ph / 2^32) and the output
 * within 4 of vol sin (single) / vol (sin + sin) / 2 (dual); a step is within clock_rate / 2^33 Hz of its frequency.
 *
 * PORT-FRAME.  Port p, frame f, sample s of a launch of F frames of n samples (n = 1..256).  d_cmd[p], if given, is applied first:
 * IGDSP_TONE_CMD_STOP clears IGDSP_TONE_PLAYING; IGDSP_TONE_CMD_REWIND without STOP sets pos = 0 and PLAYING (pjmedia_tonegen_play and
 * pjmedia_tonegen_rewind); IGDSP_TONE_CMD_HOLD: the bridge does not pull this port in this launch: every frame is EMPTY and pos does not
 * advance (STOP and REWIND still take effect).  A port whose d_plan_of[p] >= n_plans is EMPTY in every frame, its plan is never
 * dereferenced and its state is written back unchanged apart from the cmd.  With PLAYING set, q0 = pos + f * n in 64 bits:
 *   looping:      q = (q0 + s) mod cycle; the frame is always produced;
 *   not looping:  produced when q0 < cycle, with q = q0 + s and samples with q >= cycle 0; EMPTY when q0 >= cycle.
 * In a produced frame the segment with start_i <= q < start_i + on_i + off_i gives k = q - start_i: the oscillator rule when k < on_i,
 * else 0.  EMPTY: zeros, len 0 and igdsp_decode_meter's len-0 record (all 0, IGDSP_FLAG_EMPTY).  Produced: len n and the record as
 * igdsp_conf_mix writes it (sumsq exact, rms = sqrtf((float)sumsq / n), peak, byte_mean 0, IGDSP_FLAG_SILENT when peak <= 8).
 * State after the launch of a port that was not held and is PLAYING: looping pos' = (pos + F * n) mod cycle; not looping
 * pos' = min(pos + F * n, cycle), and PLAYING stays set only while pos' < cycle.  A port that is not PLAYING does not move.  So F frames
 * in one launch, F launches of one frame and any split in between give the same rows and the same final state.
 * A plan that igdsp_tone_plan_build did not make is read as it is and is safe: n_tones above IGDSP_TONE_MAX counts as IGDSP_TONE_MAX, a
 * cycle of 0 plays nothing, a position that no segment holds is silence.
 *
 * igdsp_tone_frame (host only): one frame of one port by the same rule, the state advanced; plan, st, out and len required, cmd as
 * d_cmd[p], samples_per_frame 1..256 (else IGDSP_EINVAL).
 * igdsp_tone_generate: d_plans [n_plans] (n_plans >= 1), d_state [P] required, 4-byte aligned; d_plan_of [P] optional (NULL: plan 0),
 * 2-byte aligned; d_cmd [P] optional.  rows_per_frame is the frame stride of d_pcm and d_len in rows: 0 means n_ports, otherwise
 * >= n_ports; tone rows can so be written beside the calls' rows of a [F][C + P][n] array that igdsp_conf_mix reads with
 * n_channels = C + P; rows outside [0, P) of each frame are not touched.  d_stats is dense [F][P].  At least one of d_pcm and d_stats;
 * d_len optional.  d_pcm and d_len 2-byte, d_stats 8-byte aligned; an output must not be one of the inputs or the state, and the
 * buffers must not overlap at all.  n_ports == 0 or n_frames == 0: nothing to do, the state is untouched.
 * max(rows_per_frame, n_ports) * n_frames < 2^32 - 32 (IGDSP_ERANGE).  Enqueued on `stream`, not synchronised.
 *
 * Fidelity.  UNVERIFIED: pjmedia's tonegen.c is not in the reference tree, so its default amplitude (IGDSP_TONE_VOLUME), the shape and
 * length of its fades and the restart of the phase at every tone are this library's own rules, not compared with it.  The reference
 * fills three descriptors and plays count = 1 (Functions.cpp:542-560): its cadence is 2 s on / 1 s off. */
#define IGDSP_TONE_MAX      8        /* tones per plan */
#define IGDSP_TONE_VOLUME   12288    /* used when a desc's volume is 0 (pjmedia's default amplitude; UNVERIFIED) */
#define IGDSP_TONE_LOOP     1u       /* plan option: PJMEDIA_TONEGEN_LOOP */
#define IGDSP_TONE_NO_FADE  2u       /* plan option */
#define IGDSP_TONE_PLAYING  1u       /* state flag */
#define IGDSP_TONE_CMD_REWIND 1u     /* d_cmd bits, applied before frame 0 of a launch */
#define IGDSP_TONE_CMD_STOP   2u
#define IGDSP_TONE_CMD_HOLD   4u
typedef struct igdsp_tone_desc { uint16_t freq1, freq2, on_msec, off_msec, volume, reserved; } igdsp_tone_desc;   /* pjmedia_tone_desc's fields */
typedef struct igdsp_tone_seg { uint32_t start, on, step1, step2; uint16_t vol, fade_in, fade_out, reserved; } igdsp_tone_seg;   /* 24 bytes */
typedef struct igdsp_tone_plan { uint32_t n_tones, options, cycle, clock_rate; igdsp_tone_seg seg[IGDSP_TONE_MAX]; } igdsp_tone_plan;   /* 208 bytes */
typedef struct igdsp_tone_state { uint32_t pos, flags; } igdsp_tone_state;   /* 8 bytes per port; all-zero: stopped at the start */
int igdsp_tone_plan_build(const igdsp_tone_desc *tones, uint32_t count, uint32_t clock_rate, uint32_t options, igdsp_tone_plan *out);
int igdsp_tone_frame(const igdsp_tone_plan *plan, igdsp_tone_state *st, uint32_t cmd, uint32_t samples_per_frame, int16_t *out,
                     uint16_t *len);
int igdsp_tone_generate(igdsp_ctx *ctx, const igdsp_tone_plan *d_plans, uint32_t n_plans, const uint16_t *d_plan_of /* [P], NULL: plan 0 */,
                        const uint8_t *d_cmd /* [P], optional */, igdsp_tone_state *d_state /* [P], in and out */,
                        uint32_t n_ports, uint32_t n_frames, uint32_t samples_per_frame, uint32_t rows_per_frame,
                        int16_t *d_pcm, uint16_t *d_len, igdsp_frame_stats *d_stats /* [F][P], dense */, void *stream);

/* ---- Rate converter: a bridge that does not run at the streams' 8 kHz ------------------------------------------------------------------
 * initSoftPhone takes the bridge's clock rate from the control command (roip_ed137.cpp:227-241, 7269, 7419) and puts it into
 * media_cfg.clock_rate and media_cfg.snd_clock_rate (:3031-3032); the splitcomb, the player port, the null port and the tone generator
 * all use it (:3318-3424, Functions.cpp:555, 1198), and an older settings line defaulted it to 48 000 (Functions.cpp:503).  G.711
 * streams are always 8 kHz, so with any other bridge rate pjmedia's bridge resamples every call port in both directions at
 * media_cfg.quality = 5 (its large filter).  igdsp_resample is that step for every call of a launch: IGDSP_RS_UP takes a call's rows to
 * the bridge's rate (towards igdsp_conf_mix / igdsp_snd_combine), IGDSP_RS_DOWN takes a port's rows back (towards igdsp_encode /
 * igdsp_tx_packetize).  Everything is integer.
 *
 * RULE.  Factor R in {2, 3, 4, 6} (8 <-> 16, 24, 32, 48 kHz; 16 <-> 48), T = IGDSP_RS_TAPS = 24 taps per phase, prototype length
 * N = 24 R, coefficients Q14.  The prototype is a Kaiser-windowed sinc: c_j = j - (N - 1) / 2,
 *   h[j] = sinc(0.95 c_j / R) * kaiser_N(beta = 6.0)[j],   sinc(x) = sin(pi x) / (pi x)
 * in float64, and fix(v): q = floor(16384 v / sum(v) + 0.5), then 16384 - sum(q) added to the entry of largest |q| (the lowest index
 * on a tie), so that every table sums to exactly 16384 and a constant input reproduces itself.  U_R[p][k] = fix(h[p::R])[k] (p < R,
 * k < 24), D_R[j] = fix(h)[j] (j < N).  The formula is how the constants were made (tools/rs_tables.py); the committed constants of
 * csrc/igdsp_rs_tab.h ARE the definition, and igdsp_rs_taps returns them.
 * A channel's input is one stream x[g], g = f * n_in + s over the launch; x[g] for g < 0 comes from the state's history; with d_len a
 * sample with s >= len of its input row is 0 (as igdsp_conf_mix reads a short row).
 *   UP    narrow row n samples, wide row n R:   y[g R + p] = clamp16((sum_{k < 24} U_R[p][k] x[g - k]           + 8192) >> 14)
 *   DOWN  wide row n R samples, narrow row n:   y[g]       = clamp16((sum_{j < N}  D_R[j]    x[g R + R - 1 - j] + 8192) >> 14)
 * >> is arithmetic (a floor).  DOWN has no lookahead: a frame's last output uses the frame's last input.  With |x| <= 32768 and
 * sum |q| <= 34 960 the sum plus 8192 stays below 2^31: 32-bit accumulators are exact (Q15 would not fit).  The clamp is real: the
 * worst output before it is about 69 900.  The group delay of (N - 1) / 2 wide samples (23.5 at R = 2, 71.5 at R = 6: just under 12
 * narrow samples, 1.5 ms at 8 kHz) is NOT compensated: the output is the delayed signal.  The filter is non-recursive: every frame of
 * a launch depends on the input only, and only inputs with g < 0 come from the state.
 *
 * STATE.  hist is the channel's last IGDSP_RS_HIST = 144 input samples, oldest first (UP uses the last 23, DOWN the last N - 1).  After
 * a launch hist is the last 144 entries of (old hist, the launch's input) and frames += n_frames; flags is reserved and kept as it is.
 * F frames in one launch, F launches of one frame and any split in between give the same outputs and the same final state.
 *
 * LAYOUTS.  samples_per_frame n = 1..256 counts the NARROW side.  The narrow side is [F][rows_narrow][n].  The wide side is
 *   IGDSP_RS_ROWS       [F][rows_wide][n R]
 *   IGDSP_RS_SUBFRAMES  [F R][rows_wide][n]: wide sample q of (f, c) is sample q % n of frame f R + q / n,
 * so that igdsp_conf_mix, igdsp_snd_* and tone ports built at R * 8000 Hz with samples_per_frame = n consume or produce the rows
 * directly.  rows_narrow / rows_wide are each side's frame stride in rows (as rows_per_frame of igdsp_tone_generate): 0 means
 * n_channels, otherwise >= n_channels; rows outside [0, n_channels) are never touched.
 * INPUT.  UP takes exactly one of d_payload ([f][c][n] G.711 with d_codec[c]: PT 8 A-law, anything else mu-law; igdsp_decode_meter's
 * expansion) and d_pcm (int16); DOWN takes d_pcm only.  d_len is optional and is laid out as the input rows are (their frame count
 * and row stride).
 * OUTPUT.  At least one of d_out and d_stats.  d_stats is dense, one record per output row as laid out ([F][C], or [F R][C] for UP into
 * IGDSP_RS_SUBFRAMES) over that row's samples: sumsq exact, rms = sqrtf((float)sumsq / count), peak = max |y| (32768 for -32768),
 * byte_mean 0, flags IGDSP_FLAG_SILENT (peak <= 8) | IGDSP_FLAG_SATURATED (the clamp fired in that row).
 * A bad direction, factor or layout is IGDSP_EINVAL with nothing written.  d_state required, 4-byte aligned; d_pcm, d_len, d_out
 * 2-byte, d_stats 8-byte aligned; an output must not be an input or the state and the buffers must not overlap at all.
 * n_channels == 0 or n_frames == 0: nothing to do, the state is untouched.  max(rows, n_channels) * n_frames * (R in the sub-frame
 * layout) < 2^32 - 32 on both sides (IGDSP_ERANGE).  Enqueued on `stream`, not synchronised.
 *
 * igdsp_rs_frame (host only, no GPU): one frame of one channel by the same rule, the state advanced.  n_in input samples: 1..256 for
 * UP (n_in R written), a multiple of R in R..256 R for DOWN (n_in / R written).  igdsp_rs_taps (host only): the table of a direction and
 * factor (UP: R * 24 values in [p][k] order, DOWN: 24 R) and its length.  Both: IGDSP_EINVAL for a NULL or anything out of range.
 *
 * Fidelity.  UNVERIFIED: pjmedia's resampler (libresample: resample.c / resamplesubs.c, a Kaiser-windowed sinc table with linear
 * interpolation between entries) is third-party and not in the reference tree; the filter length, cutoff, window, rounding and
 * delay above are this library's own rules and are not compared with it. */
#define IGDSP_RS_UP         0u
#define IGDSP_RS_DOWN       1u
#define IGDSP_RS_ROWS       0u       /* wide side [F][rows][n R] */
#define IGDSP_RS_SUBFRAMES  1u       /* wide side [F R][rows][n] */
#define IGDSP_RS_TAPS       24       /* taps per phase */
#define IGDSP_RS_HIST       144      /* history samples per channel: N - 1 = 143 at R = 6, rounded up */
typedef struct igdsp_rs_state {
    int16_t  hist[IGDSP_RS_HIST];    /* the channel's last 144 input samples, oldest first */
    uint32_t flags;                  /* reserved, kept as it is */
    uint32_t frames;                 /* frames converted, wrapping */
} igdsp_rs_state;                    /* 296 bytes; all-zero = silence */
int igdsp_resample(igdsp_ctx *ctx, uint32_t direction, uint32_t factor, uint32_t layout,
                   const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm, const uint16_t *d_len,
                   igdsp_rs_state *d_state /* [C], in and out */, uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame,
                   uint32_t rows_narrow, uint32_t rows_wide, int16_t *d_out, igdsp_frame_stats *d_stats /* dense */, void *stream);
int igdsp_rs_frame(igdsp_rs_state *st, uint32_t direction, uint32_t factor, const int16_t *in, uint32_t n_in, int16_t *out);
int igdsp_rs_taps(uint32_t direction, uint32_t factor, const int16_t **taps, uint32_t *count);

/* ---- Delay buffer: the sound port's two clocks, between the splitter / combiner and the bridge ------------------------------------------
 * initSlaveSoundCard (roip_ed137.cpp:3314-3435) creates five pjmedia_splitcomb_create_rev_channel ports, and each of those carries a
 * delay buffer in both directions: the bridge's tick and the card's crystal are separate clocks, so within one tick of the one side the
 * other has delivered zero, one or two frames.  igdsp_dbuf_run is that buffer for every card channel of a launch, in either direction:
 * igdsp_snd_split -> igdsp_dbuf_run -> igdsp_conf_mix (capture) and igdsp_conf_mix -> igdsp_dbuf_run -> igdsp_snd_combine (playback).
 * Everything is integer.
 *
 * STATE.  A channel buffers len samples, oldest first: y[k] = ring[(head + k) % IGDSP_DBUF_CAP], k < len.  n = samples_per_frame
 * (1..256), M = max_samples (2 n <= M <= IGDSP_DBUF_CAP).  A state is READ as: head %= CAP; if len > M the oldest len - M samples are
 * skipped (head advanced, len = M, not counted); eff == 0 reads as M >> 1, otherwise min(eff, M); last_op other than IGDSP_DBUF_PUT or
 * IGDSP_DBUF_GET reads as 0; since reads as min(since, IGDSP_DBUF_RECALC - 1); and it is written back so: all-zero is the reset state and
 * a garbage state stays in bounds.  The six counters are telemetry and wrap.
 *
 * STEPS.  A launch is T = n_steps steps; step t of channel c has op = d_ops[t][c] & 3.  With both bits set the PUT runs first, then
 * the GET.  Two frames of one side inside one tick of the other are two steps, so any interleaving of the two clocks can be written
 * down.
 *   update(op)  (the burst level, learnt per direction switch)
 *       if last_op == op:  level = min(level + 1, 65535); return
 *       if last_op != 0:   max_level = max(max_level, level); since += level
 *       last_op = op; level = 1
 *       if since >= IGDSP_DBUF_RECALC:
 *           eff = (3 * eff + min(M, (max_level + 1) * n)) >> 2;  max_level = 0;  since = 0
 *   PUT, x = d_in[t][c][0 .. n)
 *       update(PUT); puts += 1
 *       if (len > n + eff || len + n > M) && len >= IGDSP_DBUF_WIN:  shrink()           (at most one per PUT)
 *       d = len + n - M;  if d > 0: head = (head + d) % CAP; len -= d; dropped += d       (the oldest samples)
 *       y[len .. len + n) = x;  len += n
 *   shrink()  drops one pitch period of the newest audio by overlap-add, with the rules of the concealment (igdsp_plc_conceal):
 *       z[k] = y[len - 280 + k];  D(p) = sum_{i<160} |z[120 + i] - z[120 + i - p]| for p = IGDSP_PLC_PMIN .. IGDSP_PLC_PMAX;
 *       p = the smallest D, the smallest p on ties (the key (D << 7) | p);  w(i) = ((i + 1) << 15) / (p + 1);
 *       b[i] = (z[280 - 2 p + i] * (32768 - w(i)) + z[280 - p + i] * w(i) + 16384) >> 15 for i < p   (>> arithmetic: a floor);
 *       the newest 2 p samples are replaced by b[0 .. p);  len -= p; shrinks += 1; shrunk += p.
 *       The blend is convex: no clamp is needed and every product fits int32.
 *   GET
 *       update(GET); gets += 1
 *       if len < n:  out = zeros; head = (head + len) % CAP; len = 0; underruns += 1; flag = IGDSP_JB_LOST
 *       else:        out = y[0 .. n); head = (head + n) % CAP; len -= n;              flag = IGDSP_JB_PLAYED
 *
 * OUTPUTS per step and channel.  d_out[t][c][n] is written on GET steps only (rows of steps without a GET are never written).
 * d_flags_out[t][c] (optional): PLAYED or LOST as above, IGDSP_JB_IDLE without a GET: when every step has a GET, igdsp_plc_conceal
 * takes the flags as they are and conceals the underruns.  d_len_out[t][c] (optional): n on GET, else 0, what igdsp_conf_mix's d_len
 * takes.  d_fill[t][c] (optional): len after the step, the delay in samples; a host reads its drift here.  d_stats[t][c] (optional):
 * the record over the output row as igdsp_conf_mix writes it (sumsq exact, rms = sqrtf((float)sumsq / n), peak, byte_mean 0,
 * IGDSP_FLAG_SILENT when peak <= 8; an underrun row is a row of zeros); steps without a GET get the len-0 record (all 0,
 * IGDSP_FLAG_EMPTY).  Rows of d_in whose step has no PUT are never read.
 *
 * CHAINING.  T launches of one step, one launch of T steps and any split in between give the same outputs and the same state: the
 * same scalars and the same live samples y[0 .. len).  Ring bytes outside the live region are unspecified.
 *
 * ARGUMENTS.  samples_per_frame and max_samples out of range: IGDSP_EINVAL, whether or not there is work.  n_channels == 0 or
 * n_steps == 0: nothing to do, the state is untouched.  d_ops, d_in, d_state and d_out are required.  n_channels * n_steps < 2^32 - 32
 * (IGDSP_ERANGE).  d_in, d_out, d_len_out, d_fill 2-byte, d_state 4-byte, d_stats 8-byte aligned.  No output may overlap an input, the
 * state or another output.  Enqueued on `stream`, not synchronised.
 *
 * igdsp_dbuf_step (host only, no GPU): one step of one channel by the same rule.  op is IGDSP_DBUF_PUT, IGDSP_DBUF_GET, both or 0
 * (the state is only read and written back); in is read on PUT, out (n samples) is written on GET only, *flag (optional) as
 * d_flags_out.  IGDSP_EINVAL for a NULL state, an op above 3, sizes out of range, or a NULL row its op needs.
 *
 * Fidelity.  UNVERIFIED: pjmedia's delaybuf.c and wsola.c are not in the reference tree.  PINNED to their structure: the burst level
 * learnt per direction switch; the effective size smoothed 3 : 1 and re-learnt every IGDSP_DBUF_RECALC half-frames of traffic; a shrink
 * when the fill exceeds a frame plus the effective size or would exceed the maximum; the oldest samples dropped when that is not
 * enough; a zero frame and an emptied buffer on underrun.  DIFFERENT ON PURPOSE: a 128 ms cap instead of pjmedia's 400 ms default,
 * which keeps the state at 2 KiB per channel; one period per PUT, with the concealment's integer pitch search, instead of a windowed
 * float WSOLA loop; mono PCM only (the split runs before the buffer); an underrun is not expanded: the LOST flag hands the gap to
 * igdsp_plc_conceal. */
#define IGDSP_DBUF_CAP     1024   /* ring samples per channel: 128 ms at 8 kHz            */
#define IGDSP_DBUF_WIN      280   /* the shrink's window = IGDSP_PLC_HIST                 */
#define IGDSP_DBUF_RECALC   200   /* burst levels summed between two updates of eff       */
#define IGDSP_DBUF_PUT     0x01   /* d_ops bits */
#define IGDSP_DBUF_GET     0x02
typedef struct igdsp_dbuf_state {
    int16_t  ring[IGDSP_DBUF_CAP];  /* buffered sample k (0 = oldest) is ring[(head + k) % CAP], k < len */
    uint16_t head, len;             /* the live region                                        */
    uint16_t eff;                   /* effective size, samples (0 reads as max_samples >> 1)  */
    uint16_t level, max_level;      /* the current burst, the longest since the last recalc   */
    uint16_t since;                 /* burst levels summed since the last recalc              */
    uint16_t last_op, reserved0;    /* 0, IGDSP_DBUF_PUT or IGDSP_DBUF_GET                    */
    uint32_t underruns, shrinks, shrunk, dropped, puts, gets;   /* telemetry, wrapping       */
    uint32_t reserved[6];
} igdsp_dbuf_state;                 /* 2112 bytes; all-zero = reset */
int igdsp_dbuf_run(igdsp_ctx *ctx, const uint8_t *d_ops /* [T][C] */, const int16_t *d_in /* [T][C][n] */,
                   uint32_t n_channels, uint32_t n_steps, uint32_t samples_per_frame, uint32_t max_samples,
                   igdsp_dbuf_state *d_state /* [C], in and out */, int16_t *d_out /* [T][C][n] */, uint8_t *d_flags_out, uint16_t *d_len_out,
                   uint16_t *d_fill, igdsp_frame_stats *d_stats, void *stream);
int igdsp_dbuf_step(igdsp_dbuf_state *st, uint32_t op, const int16_t *in, uint32_t samples_per_frame,
                    uint32_t max_samples, int16_t *out, uint32_t *flag);

/* ---- Spectrum: the spectrum graph's 1 024-point transform, per channel and hop ------------------------------------------------------------
 * The reference declares a spectrum graph and never computes one: DEFAULT_FFT_SIZE 1024 (roip_ed137.h:118), fftSize, d_realFftData,
 * d_iirFftData, signalInput[1024], d_fftAvg, spectValueChanged(int), spectClear() (roip_ed137.h:510-522); initSpectrumGraph()
 * (roip_ed137.cpp:6350-6365) fills both arrays with -70 dBFS and sets d_fftAvg = 1.0 - 1.0e-2 * 75; the fftw calls of the teardown
 * (roip_ed137.cpp:1705-1710) are commented out.  igdsp_spectrum is that pipeline for every channel of a launch: 1 024 points, a raw
 * dBFS array, and an array averaged in the dB domain that starts at -70 with gain 0.25.  It takes the rows igdsp_plc_conceal leaves
 * (or a port's rows ahead of igdsp_conf_mix), G.711 codes or PCM.  All arithmetic is fp32.
 *
 * STATE.  igdsp_spec_state is opaque to callers: the last 1 024 samples (oldest first), the averaged array, the frames since the last
 * hop, a hop count and a flag that says the averaged array is live.  All-zero is the reset state: its history is silence and its
 * averaged array reads as IGDSP_SPEC_FLOOR_DB in every bin.  A state is READ as: since >= hop_frames reads as hop_frames - 1; only
 * bit IGDSP_SPEC_LIVE of flags counts; and it is written back so (flags = IGDSP_SPEC_LIVE, the averaged array materialised), so a
 * garbage state stays in bounds.  hops is telemetry and wraps.
 *
 * PER FRAME f of channel c, n = samples_per_frame (1..256), cfg = {hop_frames >= 1, alpha in (0, 1]} (NULL: {1, 0.25f}):
 *   1. the row's n samples are decoded (d_g711[f][c][n] with d_codec[c]: IGDSP_PT_PCMA is A-law, anything else mu-law; or
 *      d_pcm[f][c][n]) and appended to the history, the oldest n samples leave;  since += 1
 *   2. if since == hop_frames, a hop:  since = 0;  x[0 .. 1023] = the history, oldest first
 *        y[i]   = (float)x[i] * w[i],  w the periodic Hann window 0.5 - 0.5 cos(2 pi i / 1024)
 *        X[k]   = sum_i y[i] e^(-2 pi i k i / 1024),  k = 0 .. IGDSP_SPEC_BINS - 1   (bins 0 .. 511: the Nyquist bin is dropped)
 *        P[k]   = (re^2 + im^2) * 2^-46        (a full-scale sine on a bin centre: |X| = 32768 * 512 / 2 = 2^23, 0 dBFS)
 *        raw[k] = 10 log10f(P[k] + 1e-20f)
 *        avg[k] += alpha * (raw[k] - avg[k]);  hops += 1
 * The window and the twiddle factors are committed constants (csrc/igdsp_spec_tab.h, igdsp_spec_tables); no sinf / cosf runs.  The
 * transform's order of operations is the library's own (three radix-8 passes over the samples packed as 512 complex points, then a
 * split pass): results agree with a float64 evaluation of the formulas within 0.05 dB on every bin within 60 dB of the frame's total
 * power, not bit for bit with another FFT.  On the device a channel's results are bit for bit the same whatever n_channels, its
 * position, and the way the frames are split over launches.
 *
 * OUTPUTS, each optional (NULL: skipped).  d_rec[f][c]: peak_db / peak_bin = the maximum of raw over the 512 bins (the lowest bin
 * on a tie) and flags = IGDSP_SPEC_HOP when the frame computed a spectrum; a frame without a hop writes an all-zero record.
 * d_avg[c][512]: the averaged array after the launch's last frame.  d_raw[c][512]: the last raw spectrum of the launch, written only
 * for channels that hopped in this launch.
 *
 * ARGUMENTS.  samples_per_frame and cfg out of range: IGDSP_EINVAL, whether or not there is work.  n_channels == 0 or n_frames == 0:
 * nothing to do.  Exactly one of d_g711 (with d_codec) and d_pcm; d_state is required.  n_channels * n_frames < 2^32 - 32
 * (IGDSP_ERANGE).  d_pcm 2-byte, d_state, d_avg, d_raw 4-byte, d_rec 8-byte aligned.  The state and the outputs may overlap neither
 * an input nor each other.  Enqueued on `stream`, not synchronised.
 *
 * igdsp_spec_frame (host only, no GPU): one frame of one channel by the same rule, row = n PCM samples; rec (optional) as d_rec,
 * raw (optional, 512 floats) is written on a hop only.  IGDSP_EINVAL for a NULL state or row, n or cfg out of range.
 * igdsp_spec_tables (host only): the window (1 024 floats) and the twiddle factors t[k] = (cos(2 pi k / 1024), -sin(2 pi k / 1024)),
 * k = 0 .. 1023, as 2 048 floats; either pointer may be NULL.
 *
 * Fidelity.  PINNED to the reference's declarations: 1 024 points, -70 dBFS initial arrays, the gain 0.25 (= 1 - d_fftAvg).
 * UNVERIFIED: the reference computes no spectrum, so window, scaling and the dB-domain average follow the receiver whose constants
 * it copied (a Hann window, dBFS of a full-scale sine, avg += gain * (raw - avg)).  DIFFERENT ON PURPOSE: the rows' own rate only,
 * full rows only (feed concealed PCM), one FFT size. */
#define IGDSP_SPEC_N        1024    /* points = samples of history                              */
#define IGDSP_SPEC_BINS      512    /* bins 0 .. 511; the Nyquist bin is dropped                */
#define IGDSP_SPEC_FLOOR_DB (-70.0f) /* what a reset state's averaged array reads as            */
#define IGDSP_SPEC_HOP    0x0001    /* igdsp_spec_rec.flags: this frame computed a spectrum     */
#define IGDSP_SPEC_LIVE   0x0001    /* igdsp_spec_state.flags: the averaged array is live       */
typedef struct igdsp_spec_state {
    int16_t  hist[IGDSP_SPEC_N];    /* the last 1 024 samples, oldest first                     */
    float    avg[IGDSP_SPEC_BINS];  /* the averaged array, dBFS (valid with IGDSP_SPEC_LIVE)    */
    uint32_t since;                 /* frames since the last hop                                */
    uint32_t hops;                  /* telemetry, wrapping                                      */
    uint32_t flags, reserved;
} igdsp_spec_state;                 /* 4112 bytes; all-zero = reset */
typedef struct igdsp_spec_cfg {
    uint32_t hop_frames;            /* >= 1: a spectrum every hop_frames frames                 */
    float    alpha;                 /* (0, 1]: the average's gain                               */
} igdsp_spec_cfg;
typedef struct igdsp_spec_rec {
    uint16_t peak_bin, flags;
    float    peak_db;
} igdsp_spec_rec;                   /* 8 bytes */
int igdsp_spectrum(igdsp_ctx *ctx, const uint8_t *d_g711 /* [F][C][n] */, const uint8_t *d_codec /* [C] */, const int16_t *d_pcm /* [F][C][n] */,
                   uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, const igdsp_spec_cfg *cfg,
                   igdsp_spec_state *d_state /* [C], in and out */, igdsp_spec_rec *d_rec /* [F][C] */, float *d_avg /* [C][512] */,
                   float *d_raw /* [C][512] */, void *stream);
int igdsp_spec_frame(igdsp_spec_state *st, const int16_t *row, uint32_t samples_per_frame, const igdsp_spec_cfg *cfg,
                     igdsp_spec_rec *rec, float *raw);
int igdsp_spec_tables(const float **window, const float **twiddle);

/* ---- Tone detector: in-band DTMF and single tones, per channel and frame ---------------------------------------------------------------
 * A gateway between SIP telephone legs (isSipCall) and analogue radios gets its signalling in the audio: digits dialled through a
 * G.711 leg, the 440 + 480 Hz ring tone of igdsp_tone_generate, a SELCAL or answer tone on a radio channel.  igdsp_tone_detect hears
 * them in the rows igdsp_plc_conceal, igdsp_snd_split or igdsp_tone_generate leave (G.711 codes with d_codec, or PCM, [F][C][n]).
 * Everything is integer; no libm runs at run time.
 *
 * PLAN (igdsp_tdet_plan_build, host only).  clock_rate as the generator's; n_lo = 1..8 frequencies of the low group, n_hi = 0..8 of
 * the high group, freq[0 .. n_lo) the low group, freq[n_lo .. n_lo + n_hi) the high group, each in 1..clock_rate / 2 - 1 and stored as
 * the generator's 32-bit phase step ((f << 32) + clock_rate / 2) / clock_rate; steps past n_lo + n_hi are 0.  thr (NULL: the defaults)
 * = {min_amp 8..32767 [400], rel_q8 [1024], fwd_q8 [673, 4.2 dB], rev_q8 [1615, 8 dB], frac_q8 [150], min_on 1..255 [3],
 * min_off 1..255 [2]}, the q8 values 1..65535.  Anything else: IGDSP_EINVAL, nothing written.  n_hi == 0 is a single-group plan: one
 * tone out of n_lo, code = index + 1, no twist test; otherwise code = 1 + lo_index * n_hi + hi_index.  igdsp_tdet_plan_dtmf fills the
 * 4 + 4 DTMF plan (697 770 852 941 / 1209 1336 1477 1633 Hz) with the defaults; igdsp_tdet_digit(code) is the character of its code
 * ("123A456B789C*0#D"[code - 1], 0 for any other code).
 *
 * TABLE.  With the generator's T[1024] and osc(ph) = T[i] + (((T[(i + 1) & 1023] - T[i]) * fr) >> 16), i = ph >> 22, fr = (ph >> 6)
 * & 0xFFFF: for window index i = 0..n - 1 and frequency k, ph = (uint32_t)(i * step_k),
 *   ws[k][i] = osc(ph) / 16,  wc[k][i] = osc(ph + 0x40000000) / 16     C division, toward zero: both lie in [-2047, 2047]
 * (the cosine is the sine a quarter turn ahead).  The phase restarts at 0 in every window.  igdsp_tdet_table (host only) writes
 * wc then ws of frequency k at out[(2 k) * n] and out[(2 k + 1) * n], k < n_lo + n_hi.
 *
 * EVALUATION.  n = samples_per_frame even, 2..256 (odd: IGDSP_EINVAL).  Two evaluations per frame over windows of n samples:
 * e = 0 over the state's last n / 2 samples followed by the frame's first n / 2, e = 1 over the frame.  x = the window's samples
 * (G.711 decoded as igdsp_spectrum does: IGDSP_PT_PCMA is A-law, anything else mu-law),
 *   v[i] = x[i] >> 3  (arithmetic),  I_k = sum v[i] wc[k][i],  Q_k = sum v[i] ws[k][i],  P_k = I_k^2 + Q_k^2,  E = sum v[i]^2.
 * |v| <= 4096, |w| <= 2047, n <= 256: |I_k|, |Q_k| <= 4096 * 2047 * 256 = 2 146 435 072 < 2^31, so both fit int32; P_k < 2^63 and
 * E <= 2^32 are uint64.
 *
 * HIT.  Per group the strongest bin by P, the lowest index on a tie: lo (and hi).  S = P >> 16 (part of the rule: it keeps every
 * product below 2^64).  The hit code is the plan's code when ALL of these hold, else 0:
 *   every chosen P >= ((min_amp >> 3) * 2047 * (n / 2))^2;
 *   S_chosen * 256 >= rel_q8 * S_other for every other bin of its group;
 *   two groups only:  S_hi * 256 <= fwd_q8 * S_lo  and  S_lo * 256 <= rev_q8 * S_hi;
 *   (S_lo + S_hi) * 256 >= frac_q8 * ((E * (n / 2) * 2047^2) >> 16)      (S_hi = 0 in a single-group plan).
 *
 * DEBOUNCE.  Per channel cur, cand, run, off (bytes) and len (16 bits).  Per evaluation with hit code h, in this order:
 *   1. cur != 0:  len = min(len + 1, 65535);  h == cur: off = 0;  else off = min(off + 1, 255)
 *   2. candidate: h != 0 && h == cand: run = min(run + 1, 255);  else cand = h, run = h ? 1 : 0.   (h == cur != 0: cand = 0, run = 0)
 *   3. cur != 0 && off >= min_off:  OFF;  len = len > off ? len - off : 0  (the digit's length in evaluations, the trailing misses
 *      taken off);  cur = 0;  off = 0
 *   4. cur == 0 && cand != 0 && run >= min_on:  ON;  cur = cand;  len = run;  off = 0;  cand = 0;  run = 0
 * So the evaluation that ends a digit already counts as a candidate for the next one, and len keeps an ended digit's length until the
 * next ON.
 *
 * STATE.  igdsp_tdet_state: the last 128 values v (the samples >> 3, oldest first) and the debounce fields.  All-zero is the reset state.  Any bytes
 * are a valid state (nothing indexes by them); reserved is written back 0.  F frames in one launch, F launches of one frame and any
 * split in between give the same bytes; a channel's results are the same at any channel count and position.
 *
 * OUTPUTS, each optional.  d_rec[f][c] (igdsp_tdet_rec): the two evaluations' hit codes, cur and len after the frame, flags =
 * IGDSP_TDET_ON0 / _OFF0 / _ON1 / _OFF1, code = the digit the frame's last ON or OFF is about (0: none).  The event list has
 * igdsp_link_watch's contract: (f, c) is an event iff flags & event_mask (0 = IGDSP_TDET_EVENT_DEFAULT), order frame-major then
 * ascending channel, d_event_count[0] = the number of events, [1] = min(that, event_cap) = the number stored, nothing is written past
 * d_events[event_cap); d_events may be NULL iff event_cap == 0; d_event_count NULL: no list.  A list needs d_work of
 * igdsp_tdet_work_bytes(n_channels, n_frames, d_rec != NULL) bytes, 16-byte aligned, one per stream that launches.
 * d_plan_of[C] (optional, NULL: plan 0) with n_plans >= 1 as the generator has; a channel whose plan index is >= n_plans detects
 * nothing: all-zero records, no event, its state untouched.  Four consecutive channels (4 k .. 4 k + 3) are worked on together, once
 * per distinct plan among them: channels interleaved over four plans cost up to four times channels sorted by plan.
 *
 * ARGUMENTS.  An odd or out-of-range samples_per_frame: IGDSP_EINVAL, whether or not there is work.  n_channels == 0 or n_frames == 0:
 * nothing to do, the counts are written as 0.  Exactly one of d_g711 (with d_codec) and d_pcm; d_plans and d_state required.
 * n_channels * n_frames < 2^32 - 32 (IGDSP_ERANGE).  d_g711, d_plan_of 2-byte, d_pcm, d_plans, d_state, d_event_count 4-byte, d_rec
 * 8-byte, d_events, d_work 16-byte aligned (the rows are read two samples, the events stored 16 bytes at a time).  The state and the outputs may overlap neither an input nor each other.  Enqueued on `stream`, not
 * synchronised.
 *
 * igdsp_tdet_frame (host only, no GPU): one frame of one channel by the same rule, row = n PCM samples; rec optional.
 *
 * Fidelity.  This is the library's own rule.  UNVERIFIED against ITU-T Q.24 and against any other detector; what is promised is what
 * the tests show (tests/test_tdet_cpu.py: the 16 digits, twist, frequency offset, talk-off, noise, duration). */
#define IGDSP_TDET_MAX_FREQ 16      /* frequencies per plan, both groups                        */
#define IGDSP_TDET_HIST     128     /* samples of history in the state                          */
#define IGDSP_TDET_ON0   0x01       /* igdsp_tdet_rec.flags: ON raised by evaluation 0          */
#define IGDSP_TDET_OFF0  0x02
#define IGDSP_TDET_ON1   0x04
#define IGDSP_TDET_OFF1  0x08
#define IGDSP_TDET_EVENT_DEFAULT 0x0F
typedef struct igdsp_tdet_thr {
    uint16_t min_amp, rel_q8, fwd_q8, rev_q8, frac_q8;
    uint8_t  min_on, min_off;
} igdsp_tdet_thr;                   /* 12 bytes */
typedef struct igdsp_tdet_plan {
    uint32_t clock_rate;
    uint8_t  n_lo, n_hi, reserved[2];
    igdsp_tdet_thr thr;
    uint32_t step[IGDSP_TDET_MAX_FREQ];
} igdsp_tdet_plan;                  /* 84 bytes */
typedef struct igdsp_tdet_state {
    int16_t  hist[IGDSP_TDET_HIST]; /* the last 128 samples >> 3, oldest first                  */
    uint8_t  cur, cand, run, off;
    uint16_t len, reserved;
} igdsp_tdet_state;                 /* 264 bytes; all-zero = reset */
typedef struct igdsp_tdet_rec {
    uint8_t  hit[2];                /* the raw hit code of evaluations 0 and 1                  */
    uint8_t  cur;                   /* after the frame                                          */
    uint8_t  flags;                 /* IGDSP_TDET_ON0 | _OFF0 | _ON1 | _OFF1                    */
    uint16_t len;                   /* the running length after the frame, saturating           */
    uint8_t  code;                  /* the digit of the frame's last ON or OFF                  */
    uint8_t  reserved;              /* 0 */
} igdsp_tdet_rec;                   /* 8 bytes */
typedef struct igdsp_tdet_event {
    uint32_t channel;
    uint32_t frame;                 /* f within this launch                                     */
    igdsp_tdet_rec rec;             /* d_rec[f][c]                                              */
} igdsp_tdet_event;                 /* 16 bytes */
int igdsp_tdet_plan_build(uint32_t clock_rate, const uint16_t *freq, uint32_t n_lo, uint32_t n_hi, const igdsp_tdet_thr *thr,
                          igdsp_tdet_plan *out);
int igdsp_tdet_plan_dtmf(uint32_t clock_rate, igdsp_tdet_plan *out);
int igdsp_tdet_digit(uint32_t code);
int igdsp_tdet_table(const igdsp_tdet_plan *plan, uint32_t samples_per_frame, int16_t *out /* [2 (n_lo + n_hi)][n] */);
int igdsp_tdet_frame(const igdsp_tdet_plan *plan, igdsp_tdet_state *st, const int16_t *row, uint32_t samples_per_frame, igdsp_tdet_rec *rec);
size_t igdsp_tdet_work_bytes(uint32_t n_channels, uint32_t n_frames, int with_rec);
int igdsp_tone_detect(igdsp_ctx *ctx, const uint8_t *d_g711 /* [F][C][n] */, const uint8_t *d_codec /* [C] */, const int16_t *d_pcm /* [F][C][n] */,
                      const igdsp_tdet_plan *d_plans, uint32_t n_plans, const uint16_t *d_plan_of /* [C], NULL: plan 0 */,
                      uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, uint32_t event_mask,
                      igdsp_tdet_state *d_state /* [C], in and out */, igdsp_tdet_rec *d_rec /* [F][C] */,
                      igdsp_tdet_event *d_events, uint32_t event_cap, uint32_t *d_event_count, void *d_work, void *stream);

/* ---- Echo canceller: the sound port's echo canceller, per channel, as an adaptive FIR filter ---------------------------------------------
 * pjmedia hangs an echo canceller on the pjmedia_snd_port the reference opens and the reference switches it off (ec_tail_len = 0); it
 * then closes every receiver of a group while a transmitter of the group is keyed (groupMute).  igdsp_echo_cancel takes the far end (what
 * the channel's transmitter sends: a PCM row as igdsp_conf_mix writes it per port) out of the near end (what the channel's receiver
 * hears: G.711 codes with d_codec, or PCM, [F][C][n]), so that a receiver stays open, metered and voted on during transmit.
 * Everything is integer; every sum is exact, so no result depends on the order of summation.
 *
 * RULE.  A block-normalised LMS filter with blocks of B = 8 samples and a tail of L = cfg->tail = 128 or 256 taps (one value per
 * launch).  xs = far >> 2 (arithmetic) stands behind the state's history of the last L values xs.  A frame of n samples (even, 2..256)
 * is cut into blocks of 8 from its start; the last block is shorter when n % 8 != 0.  Per block of b samples at positions j:
 *   1. wh[k] = w[k] >> 18                                         (14 bits, Q13; the weights from before the block serve all of it)
 *   2. acc_j = sum over k < L of wh[k] * xs[j - k];  yhat_j = clamp16((acc_j + 1024) >> 11);  out_j = e_j = clamp16(near_j - yhat_j)
 *   3. P = sum of xs^2 over the L most recent values at the block's end
 *   4. xmax = 4 * max |xs| over the last L + b values;  dmax = max |near_j| over the block
 *   5. if 2 * dmax > xmax and dmax >= cfg->dmin:  hang = cfg->hang;   else if hang > 0:  hang = hang - 1
 *   6. only if hang == 0 and P >= cfg->pmin and the channel is not frozen:   es_j = e_j / 4 (C division, toward zero),
 *        g[k] = sum over j of es_j * xs[j - k],   q = the bit length of P,   sh = 31 - cfg->mu_shift - q,
 *        w[k] = sat32(w[k] + (sh >= 0 ? g[k] << sh : g[k] >> -sh))          (in 64 bits; the right shift arithmetic)
 * |wh| <= 2^13 and |xs| <= 2^13: a product is at most 2^26, 16 of them fit 32 bits, a whole tail (2^34) needs 64.  |es| <= 2^13 likewise.
 * igdsp_ec_cfg_default(tail, out) fills {tail, mu_shift 2, pmin 65536, hang 80 blocks, dmin 256}.
 *
 * STATE.  igdsp_ec_state, one per channel, read at the start of a launch and written back at its end.  tag = IGDSP_EC_TAG | L names the
 * layout and the tail the state was run with: a state with any other tag (all-zero included) starts as the RESET state, w, hist, hang
 * and flags 0.  Under the right tag any bytes are a valid state: hist is read clamped to -8192..8191, nothing indexes by a field.  At
 * L = 128 the upper halves of w and hist are written 0.  flags keeps IGDSP_EC_W_SATURATED since the last reset.  F frames in one launch,
 * F launches of one frame and any split in between give the same bytes; a channel's results are the same at any channel count and position.
 *
 * FAR END AND CONTROL.  d_far_pcm is [F][n_far_rows][n]; channel c reads row d_far_of[c] (NULL: row c), so the receivers of a group
 * share their transmitter's row.  An index >= n_far_rows means no far end: the channel runs as IGDSP_EC_BYPASS over a far row of zeros.
 * d_ctl[c] (NULL: IGDSP_EC_RUN; a value above 3 counts as RUN) holds for the launch:
 *   IGDSP_EC_RUN;   IGDSP_EC_FREEZE: filter and detect, never adapt;   IGDSP_EC_BYPASS: out = near, no filter, no detector (hang
 *   stays), the history still advances;   IGDSP_EC_RESET: the state becomes the RESET state before the launch's first frame, then RUN.
 *
 * OUTPUTS, each optional.  d_out[f][c][n] = e.  d_rec[f][c] (igdsp_ec_rec): near_e = (sum near^2) >> 8 and out_e = (sum out^2) >> 8 (the
 * echo return loss enhancement of a frame is 10 log10(near_e / out_e)), flags = IGDSP_EC_ADAPTED (a block adapted), _DOUBLETALK (a
 * block ended with hang > 0), _FAR_ACTIVE (a block had P >= pmin), _W_SATURATED (a weight was clipped in this frame), _BYPASSED;
 * n_adapt and n_dt the counts of such blocks; wmax = max |w[k] >> 18| after the frame.  d_stats[f][c]: the PCM record of out, as
 * igdsp_conf_mix writes it.  With d_out NULL the stage runs for state and records only.
 *
 * ARGUMENTS.  samples_per_frame odd or outside 2..256, cfg->tail not 128 or 256, cfg->mu_shift > 6: IGDSP_EINVAL, whether or not there
 * is work (cfg NULL: the defaults at tail 128).  n_channels == 0 or n_frames == 0: nothing to do.  Exactly one of d_near_g711 (with
 * d_codec) and d_near_pcm; d_far_pcm (unless n_far_rows == 0) and d_state required.  n_channels * n_frames and n_far_rows * n_frames
 * < 2^32 - 32 (IGDSP_ERANGE).  d_near_g711 2-byte, d_near_pcm, d_far_pcm, d_far_of, d_out 4-byte, d_stats 8-byte, d_state, d_rec
 * 16-byte aligned (rows are read and stored two samples, weights and records 16 bytes at a time).  The state and the outputs may
 * overlap neither an input nor each other.  Enqueued on `stream`, not synchronised.
 *
 * igdsp_ec_frame (host only, no GPU): one frame of one channel by the same rule; near is PCM, far NULL = no far end, out and rec
 * optional.  IGDSP_EINVAL for what the entry rejects.
 *
 * Fidelity.  This is the library's own rule.  UNVERIFIED against ITU-T G.168, against speex, WebRTC and any other canceller; what is
 * promised is what the tests show (tests/test_ec_cpu.py: integer against float64, single talk, double talk, the controls). */
#define IGDSP_EC_MAX_TAIL 256
#define IGDSP_EC_BLOCK    8
#define IGDSP_EC_TAG      0xEC010000u /* | L: igdsp_ec_state.tag                                 */
#define IGDSP_EC_RUN      0           /* d_ctl                                                    */
#define IGDSP_EC_FREEZE   1
#define IGDSP_EC_BYPASS   2
#define IGDSP_EC_RESET    3
#define IGDSP_EC_ADAPTED     0x01     /* igdsp_ec_rec.flags                                       */
#define IGDSP_EC_DOUBLETALK  0x02
#define IGDSP_EC_FAR_ACTIVE  0x04
#define IGDSP_EC_W_SATURATED 0x08     /* igdsp_ec_state.flags as well                             */
#define IGDSP_EC_BYPASSED    0x10
typedef struct igdsp_ec_cfg {
    uint16_t tail;                  /* L: 128 or 256                                            */
    uint8_t  mu_shift;              /* 0..6: the step is 2^-mu_shift                            */
    uint8_t  reserved;
    uint32_t pmin;                  /* adapt only when P >= pmin                                */
    uint16_t hang;                  /* blocks without adaptation after the detector fires       */
    uint16_t dmin;                  /* the detector fires only when dmax >= dmin                */
} igdsp_ec_cfg;                     /* 12 bytes */
typedef struct igdsp_ec_state {
    int32_t  w[IGDSP_EC_MAX_TAIL];    /* Q31: w / 2^31 is the tap                                 */
    int16_t  hist[IGDSP_EC_MAX_TAIL]; /* the last L values far >> 2, oldest first, in hist[0 .. L) */
    uint32_t hang, flags, tag, reserved;
} igdsp_ec_state;                   /* 1552 bytes */
typedef struct igdsp_ec_rec {
    uint32_t near_e, out_e;         /* (sum of squares) >> 8                                    */
    uint8_t  flags, n_adapt, n_dt, reserved;
    uint16_t wmax, reserved2;
} igdsp_ec_rec;                     /* 16 bytes */
void igdsp_ec_cfg_default(uint32_t tail, igdsp_ec_cfg *out);
int igdsp_ec_frame(const igdsp_ec_cfg *cfg, igdsp_ec_state *st, const int16_t *near_pcm, const int16_t *far_pcm, uint32_t samples_per_frame,
                   uint32_t ctl, int16_t *out, igdsp_ec_rec *rec);
int igdsp_echo_cancel(igdsp_ctx *ctx, const uint8_t *d_near_g711 /* [F][C][n] */, const uint8_t *d_codec /* [C] */,
                      const int16_t *d_near_pcm /* [F][C][n] */, const int16_t *d_far_pcm /* [F][P][n] */, uint32_t n_far_rows,
                      const uint32_t *d_far_of /* [C], NULL: row c */, const uint8_t *d_ctl /* [C], NULL: RUN */, const igdsp_ec_cfg *cfg,
                      uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, igdsp_ec_state *d_state /* [C], in and out */,
                      int16_t *d_out /* [F][C][n] */, igdsp_ec_rec *d_rec /* [F][C] */, igdsp_frame_stats *d_stats /* [F][C] */, void *stream);

/* ---- Level control: per channel an automatic gain control with a peak limiter ------------------------------------------------------------
 * Neither pjmedia nor the reference holds one: the only gain there is the static SLOT_VOLUME (igdsp_conf_level_q7).  igdsp_agc_run brings
 * a row (G.711 codes with d_codec, or PCM, [F][C][n]) to a target peak level with a slow gain and keeps every output sample under a
 * ceiling with a fast limiter whose gain ramp starts one block ahead of a loud block, at no added delay.  It stands between
 * igdsp_plc_conceal / igdsp_bss_select and igdsp_conf_mix (the mix takes d_out as d_pcm), and between a port row of igdsp_conf_mix and
 * igdsp_tx_packetize.  Everything is integer.  This is the library's own rule, UNVERIFIED against ITU-T G.169.
 *
 * RULE.  A frame is n samples, n a multiple of 8 in 8..256: B = n / 8 blocks of 8 and B + 1 knots, knot k at sample 8 k (knot B is knot 0
 * of the next frame).  Gains are Q12 in 16 bits, 4096 is unity, CAP = 65535.  "/" is C division, toward zero.  G, env, cap: the state.
 *   1. p_b = max |x| over block b (32768 for -32768);  pk = max p_b.
 *   2. The slow gain.  The frame is ACTIVE when pk >= gate.  Not active, or frozen: Gn = G, env stays.  Active:
 *        env == 0: env = pk;   pk > env: env += (pk - env + (1 << att) - 1) >> att;   else env -= (env - pk) >> rel
 *        Gt = clamp((target << 12) / env, gmin, gmax);  d = Gt - G
 *        d >= 0: Gn = G + ((d + (1 << up) - 1) >> up);   else Gn = G - ((-d + (1 << down) - 1) >> down)
 *      The slow gain at knot k: A_k = G + ((Gn - G) * k) / B.
 *   3. The limiter's cap.  r_b = CAP when p_b == 0, else min(CAP, (ceil << 12) / p_b);  m_k = min(r_(k-1), r_k), a term outside
 *      0..B-1 counting as CAP;  c_0 = min(m_0, cap) (no release step across the frame boundary: it is one instant);
 *      c_k = min(m_k, min(CAP, c_(k-1) + max(1, c_(k-1) >> lrel))) for k >= 1;  cap' = c_B.
 *   4. T_k = min(A_k, c_k);  sample j = 8 b + i takes t_j = T_b + ((T_(b+1) - T_b) * i) / 8;  out_j = (x_j * t_j + 2048) >> 12
 *      (arithmetic shift).
 *   5. G' = Gn.
 * In block b both knots are <= r_b, and t_j lies between them, so |x_j| * t_j <= ceil << 12 < 2^27: the product fits 32 bits, and
 * |out_j| <= ceil on every sample: no clamp exists (csrc/igdsp_agc.h proves both).  A loud onset is met by a ramp that starts one
 * block (1 ms at 8 kHz) before the loud block; an onset in a frame's FIRST block has no block before it, the gain steps down at the
 * frame boundary, and the record carries IGDSP_AGC_ATTACKED.
 *
 * CONFIGURATION.  igdsp_agc_cfg holds for the launch; NULL: the defaults of igdsp_agc_cfg_default: target 8192, ceil 23170 (-3 dBFS),
 * gate 256, gmin 1024, gmax 32768, att 1, rel 5, up 5, down 2, lrel 6.  Valid: 1 <= gate; 1 <= target <= ceil <= 32767;
 * 1 <= gmin <= 4096 <= gmax <= 65535; att, rel, up, down <= 15; 1 <= lrel <= 15.
 *
 * STATE.  igdsp_agc_state, one per channel, read at the start of a launch and written at its end.  A tag other than IGDSP_AGC_TAG
 * (all-zero included) means the RESET state: env 0, gain 4096, cap CAP.  Under the right tag any bytes are a valid state: gain is read
 * clamped to [gmin, gmax], nothing indexes by a field.  flags is written as the last frame's record flags, reserved as 0.  F frames
 * in one launch, F launches of one frame and any split in between write the same bytes; a channel's results are the same at any
 * channel count and position.
 *
 * CONTROL.  d_ctl[c] (NULL: IGDSP_AGC_RUN; a value above 3 counts as RUN) holds for the launch:
 *   IGDSP_AGC_RUN;   IGDSP_AGC_FREEZE: step 2 is skipped (Gn = G, env stays), the limiter runs;   IGDSP_AGC_BYPASS: out = x, the
 *   state's bytes are not touched;   IGDSP_AGC_RESET: the state becomes the RESET state before the first frame, then RUN.
 *
 * OUTPUTS, each optional, at least one required.  d_out[f][c][n].  d_rec[f][c] (igdsp_agc_rec): gain = Gn, tmin = min T_k, in_peak =
 * pk, out_peak = max |out|, env after the frame, n_limited = the knots with c_k < A_k, flags = IGDSP_AGC_ACTIVE (pk >= gate),
 * _LIMITED (n_limited > 0), _AT_MAX / _AT_MIN ((target << 12) / env lay above gmax / below gmin), _ATTACKED (m_0 < cap), _FROZEN,
 * _BYPASSED (then gain = G and env as read, tmin 4096, out_peak = in_peak, nothing else).  d_stats[f][c]: the PCM record of out, as
 * igdsp_conf_mix writes it.  With d_out NULL the stage runs for state and records only.
 *
 * ARGUMENTS.  samples_per_frame not a multiple of 8 in 8..256, an invalid cfg: IGDSP_EINVAL, whether or not there is work.
 * n_channels == 0 or n_frames == 0: nothing to do.  Exactly one of d_g711 (with d_codec) and d_pcm; d_state and one of d_out, d_rec,
 * d_stats required.  n_channels * n_frames < 2^32 - 32 (IGDSP_ERANGE).  d_g711 8-byte, d_pcm, d_out, d_state, d_rec 16-byte, d_stats
 * 8-byte aligned (a block of 8 samples is one load and one store; state and record are 16 bytes: tighter than igdsp_echo_cancel's rows).
 * The state and the outputs may overlap neither an input nor each other.  Enqueued on `stream`, not synchronised.
 *
 * igdsp_agc_frame (host only, no GPU): one frame of one channel from PCM by the same rule; out and rec optional.  IGDSP_EINVAL for
 * what the entry rejects. */
#define IGDSP_AGC_BLOCK   8
#define IGDSP_AGC_UNITY   4096
#define IGDSP_AGC_CAP     65535
#define IGDSP_AGC_TAG     0xA6C10001u /* igdsp_agc_state.tag                                      */
#define IGDSP_AGC_RUN     0           /* d_ctl                                                    */
#define IGDSP_AGC_FREEZE  1
#define IGDSP_AGC_BYPASS  2
#define IGDSP_AGC_RESET   3
#define IGDSP_AGC_ACTIVE   0x01       /* igdsp_agc_rec.flags                                      */
#define IGDSP_AGC_LIMITED  0x02
#define IGDSP_AGC_AT_MAX   0x04
#define IGDSP_AGC_AT_MIN   0x08
#define IGDSP_AGC_ATTACKED 0x10
#define IGDSP_AGC_FROZEN   0x20
#define IGDSP_AGC_BYPASSED 0x40
typedef struct igdsp_agc_cfg {
    uint16_t target;                /* the peak level the slow gain aims at                      */
    uint16_t ceil;                  /* no output sample exceeds it                               */
    uint16_t gate;                  /* a frame with pk below it moves neither env nor gain       */
    uint16_t gmin, gmax;            /* Q12 bounds of the slow gain                               */
    uint8_t  att, rel;              /* env: shifts of the rise and the fall                      */
    uint8_t  up, down;              /* gain: shifts of the rise and the fall per frame           */
    uint8_t  lrel;                  /* the limiter's release: cap += max(1, cap >> lrel) a block */
    uint8_t  reserved;
} igdsp_agc_cfg;                    /* 16 bytes */
typedef struct igdsp_agc_state {
    uint32_t tag;
    uint16_t env, gain, cap, flags;
    uint32_t reserved;
} igdsp_agc_state;                  /* 16 bytes */
typedef struct igdsp_agc_rec {
    uint16_t gain, tmin, in_peak, out_peak, env;
    uint8_t  flags, n_limited;
    uint32_t reserved;
} igdsp_agc_rec;                    /* 16 bytes */
void igdsp_agc_cfg_default(igdsp_agc_cfg *out);
int igdsp_agc_frame(const igdsp_agc_cfg *cfg, igdsp_agc_state *st, const int16_t *pcm, uint32_t samples_per_frame, uint32_t ctl,
                    int16_t *out, igdsp_agc_rec *rec);
int igdsp_agc_run(igdsp_ctx *ctx, const uint8_t *d_g711 /* [F][C][n] */, const uint8_t *d_codec /* [C] */,
                  const int16_t *d_pcm /* [F][C][n] */, const uint8_t *d_ctl /* [C], NULL: RUN */, const igdsp_agc_cfg *cfg,
                  uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, igdsp_agc_state *d_state /* [C], in and out */,
                  int16_t *d_out /* [F][C][n] */, igdsp_agc_rec *d_rec /* [F][C] */, igdsp_frame_stats *d_stats /* [F][C] */, void *stream);

/* ---- Voice activity: the stream's silence detector, DTX and the RFC 3389 comfort-noise payload, per channel and frame ----------------------
 * pjmedia's stream holds a silence detector and the reference switches it off (media_cfg.no_vad = 1, next to ec_tail_len = 0).
 * igdsp_vad_run is that detector for a batch, on the send side in front of igdsp_tx_packetize: it follows igdsp_conf_mix or
 * igdsp_agc_run (their d_out as d_pcm) or sits on a leg's G.711 rows.  It gives a leg without a PTT line its control byte (VOX), tells
 * a SIP leg which frames to send, which to replace by one PT 13 comfort-noise packet and which to skip (DTX), and lists the talkspurt
 * edges.  Everything is integer: the same bits on the host and the device, at any channel count and position and for any split of
 * the frames over launches.  The rule is the library's own; the payload's scale and sign convention are RFC 3389 section 3.2 as
 * recalled.  UNVERIFIED against RFC 3389 and G.711 Appendix II.
 *
 * RULE.  A frame is n samples, n a multiple of 8 in 16..256.  M = 10.  "/" is C division, ">>" on a signed value an arithmetic shift.
 *   0. v_j = x_j >> 2 (G.711 decoded as igdsp_spectrum does; decoded mu-law values are multiples of 4, A-law of 8: nothing is lost.
 *      PCM loses two bits).
 *   1. r[k] = sum over j = k .. n - 1 of v_j * v_(j-k), k = 0..M, exact in 64 bits (r[0] < 2^34), no history across frames.
 *      E = r[0], ms = E / n.
 *   2. The decision.  nf == 0 (the floor is unset): nf = clamp(ms, nf_min, nf_max) first.  ratio = VOICE ? ratio_off_q4 : ratio_on_q4;
 *      raw = ms >= thr_abs && ms * 16 > nf * ratio.
 *   3. The floor (skipped under FREEZE).  QUIET = ms < nf_min: the floor stays (digital silence does not teach it).  Else ms <= nf:
 *      nf -= (nf - ms) >> dn;  else nf = min(ms, nf + max(1, nf >> (raw ? up_v : up))).  Then nf = clamp(nf, nf_min, nf_max).
 *   4. The hangover.  raw: run = min(run + 1, 65535); hang = run >= burst ? hang_long : max(hang, hang_short); VOICE.  Not raw: run = 0;
 *      hang > 0: hang -= 1 and VOICE stays as it was;  else not VOICE.  ONSET: VOICE after not-VOICE; OFFSET: the first not-VOICE
 *      frame after VOICE.  raw, QUIET, VOICE, ONSET and OFFSET are the record's flags IGDSP_VAD_F_RAW, _F_QUIET, _F_VOICE, _F_ONSET and
 *      _F_OFFSET; the kind IGDSP_VAD_VOICE of step 6 is a value of its own.
 *   5. The noise model (skipped under FREEZE).  On every frame that is not raw (hangover and QUIET frames included):
 *      avalid == 0: A[k] = r[k], avalid = 1;  else A[k] += (r[k] - A[k]) >> asm_shift.
 *   6. DTX.  cfg.dtx == 0: kind = VOICE on every frame, no SID (the flags still carry the decision).  Else a VOICE frame has kind =
 *      VOICE; on a non-VOICE frame lvl = level(A[0]) and a SID is due when it is the OFFSET frame, or no SID has been sent since RESET,
 *      or sid_every > 0 && since_sid >= sid_every, or |lvl - last_level| >= sid_delta && since_sid >= sid_gap.  Due: kind = SID,
 *      since_sid = 0, last_level = lvl, sid_sent = 1.  Else kind = NONE, since_sid = min(since_sid + 1, 65535).
 *   7. The SID payload, 1 + order bytes (order 0..10).  Byte 0 = lvl.  level(e) = 127 for e <= 0, else the least d in 0..126 with
 *      (e << 8) >= n * T8[d], 127 if there is none;  T8[d] = floor(2^34 * 10^(-d / 10) + 1/2) (igdsp_vad_table): lvl = ceil(-dBov), a
 *      full-scale square wave reads 0.  Bytes 1..order: N_i = 127 + sign(k_i) * ((|k_i| + 129) / 258), k_i in Q15 from this
 *      recursion on A:  A[0] <= 0: every k = 0.  R0 = A[0] + (A[0] >> 10) + 1;  sh = bitlen(R0) - 30;  R[k] = clamp(A[k], -A[0], A[0])
 *      >> sh (<< -sh when sh < 0), R[0] from R0;  a[] Q15 in 64 bits;  err = R[0].  For i = 1..order:
 *        acc = (R[i] << 15) + sum over 1 <= j < i of a[j] * R[i-j];  k_i = clamp(-acc / err, -32508, 32508);
 *        a'[j] = a[j] + ((k_i * a[i-j] + 16384) >> 15) for j < i, a'[i] = k_i;  err -= (((k_i * k_i) >> 15) * err) >> 15;
 *        err <= 0: stop, the remaining k are 0.
 *      k_i = a_i^(i) of the predictor A(z) = 1 + sum a_j z^-j: positively correlated noise has k_1 < 0.  igdsp_sid_decode is the
 *      inverse map: level = byte 0, k_i = 258 * (N_i - 127), N_i = 255 read as 254; bytes past 1 + 10 are ignored; k past the payload 0.
 *
 * CONFIGURATION.  igdsp_vad_cfg holds for the launch; NULL: the defaults of igdsp_vad_cfg_default.  Levels are in the v domain (ms of
 * v): thr_abs 212 (about -55 dBov), nf_min 8 (just above both G.711 digital silences: 0, and A-law's +8, ms 4), nf_max 1 << 20,
 * ratio_on_q4 80 (about 7 dB), ratio_off_q4 40 (about 4 dB), dn 2, up 5, up_v 7, burst 5, hang_long 10, hang_short 2, order 10,
 * asm_shift 2, dtx 1, sid_every 0, sid_delta 2, sid_gap 2, vox_on 0x81, vox_off 0x80.  Valid: 1 <= nf_min <= nf_max <= 1 << 24;
 * 16 <= ratio_off_q4 <= ratio_on_q4; dn, up, up_v, asm_shift <= 15; order <= 10; hang_short <= hang_long.
 *
 * STATE.  igdsp_vad_state, 128 bytes, one per channel, read at the start of a launch and written at its end.  A tag other than
 * IGDSP_VAD_TAG (all-zero included) means the RESET state: everything 0.  Under the right tag any bytes are a valid state: nf is read
 * clamped to [nf_min, nf_max] (0 stays 0: unset), A[k] clamped to +-2^40, voice, avalid and sid_sent by their bit 0; nothing indexes by
 * a field.  flags is written as the last frame's record flags, reserved as 0.
 *
 * CONTROL.  d_ctl[c] (NULL: IGDSP_VAD_RUN; a value above 3 counts as RUN) holds for the launch: IGDSP_VAD_FREEZE skips steps 3 and 5
 * (the decision still runs; an unset floor is still set);  IGDSP_VAD_BYPASS: kind = VOICE, vox_on, flags = IGDSP_VAD_F_BYPASSED, ms and
 * level of the frame, nf, run and hang as read, no SID, the state's bytes untouched;  IGDSP_VAD_RESET: the state becomes the RESET
 * state before the first frame, then RUN.
 *
 * OUTPUTS, each optional; one of d_kind, d_rec, d_sid, d_txctl or the event list is required.  d_kind[f][c]: IGDSP_VAD_NONE / _VOICE /
 * _SID.  d_rec[f][c] (igdsp_vad_rec): ms, nf after the frame, run, flags (IGDSP_VAD_F_RAW, _F_VOICE, _F_ONSET, _F_OFFSET, _F_SID,
 * _F_QUIET, _F_FROZEN, _F_BYPASSED), kind (IGDSP_VAD_NONE / _VOICE / _SID), level = this frame's own level(E), hang, sid_len.  d_sid[f][c][16]: always written as one 16-byte store,
 * the payload in the first sid_len bytes, zeros behind.  d_txctl[f][c]: vox_on on frames whose flags carry IGDSP_VAD_F_VOICE (or _F_BYPASSED), vox_off otherwise:
 * igdsp_tx_packetize takes it as d_ctl.  The event list has igdsp_link_watch's contract: (f, c) is an event iff flags & event_mask
 * (0 = IGDSP_VAD_EVENT_DEFAULT = IGDSP_VAD_F_ONSET | IGDSP_VAD_F_OFFSET), order frame-major then ascending channel, d_event_count[0] = the number of events,
 * [1] = min(that, event_cap) = the number stored, nothing is written past d_events[event_cap); d_events may be NULL iff event_cap ==
 * 0; d_event_count NULL: no list.  A list needs d_work of igdsp_vad_work_bytes(n_channels, n_frames, d_rec != NULL) bytes.
 *
 * ARGUMENTS.  samples_per_frame not a multiple of 8 in 16..256, an invalid cfg: IGDSP_EINVAL, whether or not there is work.
 * n_channels == 0 or n_frames == 0: nothing to do, the counts of a list are written as 0.  Exactly one of d_g711 (with d_codec) and
 * d_pcm; d_state required.  n_channels * n_frames < 2^32 - 32 (IGDSP_ERANGE).  d_g711 8-byte, d_event_count 4-byte, d_pcm, d_state,
 * d_rec, d_sid, d_events, d_work 16-byte aligned.  The state and the outputs may overlap neither an input nor each other.  Enqueued
 * on `stream`, not synchronised.
 *
 * igdsp_vad_frame (host only, no GPU): one frame of one channel from PCM by the same rule; rec and sid optional; returns the kind
 * (>= 0) or IGDSP_EINVAL for what the entry rejects.  igdsp_vad_table: the 128 values of T8. */
#define IGDSP_VAD_ORDER   10
#define IGDSP_VAD_KMAX    32508       /* 126 * 258: the largest |k| the payload carries               */
#define IGDSP_VAD_TAG     0x7AD10001u /* igdsp_vad_state.tag                                      */
#define IGDSP_VAD_RUN     0           /* d_ctl                                                    */
#define IGDSP_VAD_FREEZE  1
#define IGDSP_VAD_BYPASS  2
#define IGDSP_VAD_RESET   3
#define IGDSP_VAD_NONE    0           /* d_kind, igdsp_vad_rec.kind                               */
#define IGDSP_VAD_VOICE   1
#define IGDSP_VAD_SID     2
#define IGDSP_VAD_F_RAW      0x01     /* igdsp_vad_rec.flags                                      */
#define IGDSP_VAD_F_VOICE    0x02
#define IGDSP_VAD_F_ONSET    0x04
#define IGDSP_VAD_F_OFFSET   0x08
#define IGDSP_VAD_F_SID      0x10
#define IGDSP_VAD_F_QUIET    0x20
#define IGDSP_VAD_F_FROZEN   0x40
#define IGDSP_VAD_F_BYPASSED 0x80
#define IGDSP_VAD_EVENT_DEFAULT 0x0C
typedef struct igdsp_vad_cfg {
    uint32_t thr_abs;               /* ms below it is never raw                                  */
    uint32_t nf_min, nf_max;        /* the floor's bounds                                        */
    uint16_t sid_every;             /* frames between scheduled SIDs, 0: none                    */
    uint8_t  ratio_on_q4, ratio_off_q4;
    uint8_t  dn, up, up_v, asm_shift;
    uint8_t  burst, hang_long, hang_short, order;
    uint8_t  dtx, sid_delta, sid_gap, vox_on;
    uint8_t  vox_off, reserved[3];
} igdsp_vad_cfg;                    /* 32 bytes */
typedef struct igdsp_vad_state {
    uint32_t tag;
    uint32_t nf;                    /* 0: unset                                                  */
    int64_t  A[IGDSP_VAD_ORDER + 1];/* the noise model's autocorrelation                         */
    uint16_t since_sid, run;
    uint8_t  hang, voice, avalid, last_level;
    uint8_t  sid_sent, flags, reserved[22];
} igdsp_vad_state;                  /* 128 bytes */
typedef struct igdsp_vad_rec {
    uint32_t ms, nf;
    uint16_t run;
    uint8_t  flags, kind, level, hang, sid_len, reserved;
} igdsp_vad_rec;                    /* 16 bytes */
typedef struct igdsp_vad_event {
    uint32_t channel;
    uint32_t frame;                 /* f within this launch                                      */
    uint32_t ms;
    uint16_t run;
    uint8_t  flags, level;
} igdsp_vad_event;                  /* 16 bytes */
void igdsp_vad_cfg_default(igdsp_vad_cfg *out);
int igdsp_vad_table(uint64_t out[128]);
int igdsp_vad_frame(const igdsp_vad_cfg *cfg, igdsp_vad_state *st, const int16_t *pcm, uint32_t samples_per_frame, uint32_t ctl,
                    igdsp_vad_rec *rec, uint8_t sid[16]);
int igdsp_sid_decode(const uint8_t *payload, uint32_t len, uint8_t *level_dbov, int16_t k_q15[10]);
size_t igdsp_vad_work_bytes(uint32_t n_channels, uint32_t n_frames, int with_rec);
int igdsp_vad_run(igdsp_ctx *ctx, const uint8_t *d_g711 /* [F][C][n] */, const uint8_t *d_codec /* [C] */,
                  const int16_t *d_pcm /* [F][C][n] */, const uint8_t *d_ctl /* [C], NULL: RUN */, const igdsp_vad_cfg *cfg,
                  uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, uint32_t event_mask,
                  igdsp_vad_state *d_state /* [C], in and out */, uint8_t *d_kind /* [F][C] */, igdsp_vad_rec *d_rec /* [F][C] */,
                  uint8_t *d_sid /* [F][C][16] */, uint8_t *d_txctl /* [F][C] */, igdsp_vad_event *d_events, uint32_t event_cap,
                  uint32_t *d_event_count, void *d_work, void *stream);

/* ---- Comfort noise: RFC 3389 SID payloads back into audio, per channel and frame ---------------------------------------------------------
 * The receive side of igdsp_vad_run's DTX.  A leg under DTX reaches the bridge as one PT 13 packet now and then and nothing in
 * between; igdsp_cng_run turns the frame's kind (as igdsp_vad_run writes d_kind) and, on SID frames, the payload into a row for
 * igdsp_conf_mix / igdsp_bss_select: VOICE frames pass the leg's row through, SID and NONE frames get synthetic noise at the payload's
 * level and spectral shape.  Everything is integer: the same bits on the host and the device, at any channel count and position and
 * for any split of the frames over launches.  The rule is the library's own.  UNVERIFIED against RFC 3389 and G.711 Appendix II.
 *
 * RULE.  A frame is n samples, n a multiple of 8 in 16..256.  ">>" on a signed value is an arithmetic shift, "/" C division,
 * clamp(v) = min(131071, max(-131071, v)).
 *   Tables and helpers.  G[d] = isqrt(T8[d]), d = 0..127 (igdsp_cng_table; T8 is igdsp_vad_table's, isqrt the floor integer square
 *   root): the rms of a -d dBov signal in Q2, G[0] = 131072, 0 from d = 106 on.  mix(x) on uint32: x ^= x >> 16; x *= 0x7feb352d;
 *   x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.  hs = mix(seed).  For the stream's sample index q (mod 2^32): r = mix(q ^ hs), e(q) =
 *   the sum of the four bytes of r, minus 510: -510..510, variance 65535 / 3 (sd 147.80).  Legs differ by their seed (d_seed, for
 *   example the SSRC); nothing depends on the channel's index.
 *   Per frame, unless the channel is under BYPASS:
 *   1. A SID is taken when kind == IGDSP_VAD_SID, the channel is not under FREEZE and len = min(sid_len, 11) > 0.  A SID frame of
 *      length 0 counts as NONE (IGDSP_CNG_F_SID_EMPTY).  Any kind other than SID or NONE is VOICE.
 *   2. A taken SID sets the model: (level, k[10]) = igdsp_sid_decode(payload, len); kq[i] = k[i] / 2 (Q14, |kq| <= 16383, 0 past the
 *      payload); order = len - 1; p = 1 << 30, then for all ten k: p = (p * ((1 << 30) - k * k)) >> 30 in 64 bits; sp = isqrt(p);
 *      g_tgt = (G[min(level, 127)] * sp * 7095) >> 23 (7095 is about 2^20 / 147.80; g_tgt is Q12, at most 3 632 640).  No model was
 *      held: g = g_tgt, have = 1.  since_sid = 0.  A frame that takes no SID: since_sid = min(since_sid + 1, 65535).
 *   3. A VOICE frame: out = the voice row (d_g711 decoded as igdsp_decode_meter decodes, or d_pcm), len_out = n; with neither input
 *      zeros and len_out = 0.  The lattice's state is left alone.
 *   4. A SID or NONE frame with have == 0: zeros, len_out = 0, IGDSP_CNG_F_NO_MODEL.
 *   5. A SID or NONE frame with a model: d = g_tgt - g; g += d - d / 2 (the gain halves its distance per frame and arrives exactly).
 *      For j = 0..n-1:  f = clamp((e(ctr + j) * g + 2048) >> 12);  for i = 10 down to 1:  f = clamp(f - ((kq_i * b[i-1] + 8192) >>
 *      14)) and, if i < 10, b[i] = clamp(b[i-1] + ((kq_i * f + 8192) >> 14)) with the old b[i-1];  then b[0] = f and out[j] =
 *      min(32767, max(-32768, (f + 2) >> 2)).  kq_i is the state's kq[i-1].  All ten stages always run: a stage with kq = 0 is a plain
 *      delay, so a shorter payload leaves no stale state.  Every product fits 32 bits.  len_out = n.
 *   6. ctr += n (mod 2^32) on every frame of any kind.
 *   The sign convention is the voice detector's: k_i = a_i^(i) of A(z) = 1 + sum a_j z^-j, the synthesis is 1 / A(z); positively
 *   correlated noise has k_1 < 0 and comes out low-pass.
 *
 * CONTROL.  d_ctl[c] (NULL: IGDSP_CNG_RUN; a value above 3 counts as RUN) holds for the launch.  IGDSP_CNG_FREEZE: SIDs are not taken,
 * model and gain's target stay, noise goes on (IGDSP_CNG_F_FROZEN).  IGDSP_CNG_BYPASS: out = the voice row on VOICE frames (len_out = n),
 * zeros (len_out = 0) otherwise; the state's bytes are untouched, the record carries the state as read and only the flag
 * IGDSP_CNG_F_BYPASSED.  IGDSP_CNG_RESET: the state becomes the RESET state before the first frame, then RUN.
 *
 * STATE.  igdsp_cng_state, 96 bytes, one per channel, read at the start of a launch and written at its end.  A tag other than
 * IGDSP_CNG_TAG (all-zero included) means the RESET state: everything 0 and seed = d_seed ? d_seed[c] : 0.  d_seed is read only then
 * and on IGDSP_CNG_RESET.  Under the right tag any bytes are a valid state: b is read clamped to +-131071, kq to +-16383, g and g_tgt
 * to at most 3 632 640, have by its bit 0; nothing indexes by a field.  flags is written as the last frame's record flags, reserved
 * as 0.
 *
 * OUTPUTS.  d_out[f][c][n] is required, the others optional.  d_len_out[f][c]: n, or 0 on the zero rows of steps 3 and 4 and of a
 * bypass.  d_rec[f][c] (igdsp_cng_rec): g, g_tgt and since_sid after the frame, the flags, the model's level byte and order.
 * d_stats[f][c]: the PCM record of igdsp_conf_mix over out; rows with len 0 get the len-0 record (IGDSP_FLAG_EMPTY).  (d_out,
 * d_len_out) feed igdsp_conf_mix and igdsp_bss_select through d_pcm / d_len unchanged.
 *
 * ARGUMENTS.  samples_per_frame not a multiple of 8 in 16..256: IGDSP_EINVAL, whether or not there is work.  n_channels == 0 or
 * n_frames == 0: nothing to do.  d_kind, d_sid, d_state and d_out are required; d_sid_len NULL: every payload has 11 bytes; at most
 * one of d_g711 (with d_codec) and d_pcm.  n_channels * n_frames < 2^32 - 32 (IGDSP_ERANGE).  d_g711 8-byte, d_sid, d_pcm, d_state,
 * d_out, d_rec, d_stats 16-byte aligned.  The state and the outputs may overlap neither an input nor each other.  Enqueued on
 * `stream`, not synchronised.
 *
 * Host only, no GPU: igdsp_cng_frame is one frame of one channel by the same rule (sid may be NULL unless a SID is taken; voice may be
 * NULL; rec optional; seed is d_seed[c]); it returns len_out (>= 0) or IGDSP_EINVAL.  igdsp_cng_gain is step 2's g_tgt of a payload of
 * 1..16 bytes (bytes past 11 are ignored).  igdsp_cng_table: the 128 values of G. */
#define IGDSP_CNG_TAG     0xC4610001u /* igdsp_cng_state.tag                                      */
#define IGDSP_CNG_GMAX    3632640u    /* the largest g and g_tgt                                  */
#define IGDSP_CNG_RUN     0           /* d_ctl                                                    */
#define IGDSP_CNG_FREEZE  1
#define IGDSP_CNG_BYPASS  2
#define IGDSP_CNG_RESET   3
#define IGDSP_CNG_F_GENERATED 0x01    /* igdsp_cng_rec.flags: the row is synthetic noise          */
#define IGDSP_CNG_F_SID       0x02    /* a SID was taken on this frame                            */
#define IGDSP_CNG_F_NO_MODEL  0x04    /* a silent frame before any model was held                 */
#define IGDSP_CNG_F_VOICE     0x08    /* the frame was passed through as voice                    */
#define IGDSP_CNG_F_CLIPPED   0x10    /* a generated row holds a sample of magnitude >= 32767     */
#define IGDSP_CNG_F_SID_EMPTY 0x20    /* a SID frame of length 0, counted as NONE                 */
#define IGDSP_CNG_F_FROZEN    0x40
#define IGDSP_CNG_F_BYPASSED  0x80
typedef struct igdsp_cng_state {
    uint32_t tag, seed, ctr, g, g_tgt;
    int32_t  b[10];                 /* the lattice's delays                                      */
    int16_t  kq[10];                /* the model's reflection coefficients, Q14                  */
    uint16_t since_sid;
    uint8_t  level, order, have, flags, reserved[10];
} igdsp_cng_state;                  /* 96 bytes */
typedef struct igdsp_cng_rec {
    uint32_t g, g_tgt;
    uint16_t since_sid;
    uint8_t  flags, level, order, reserved[3];
} igdsp_cng_rec;                    /* 16 bytes */
int igdsp_cng_table(uint32_t out[128]);
int igdsp_cng_gain(const uint8_t *payload, uint32_t len, uint32_t *g_tgt);
int igdsp_cng_frame(igdsp_cng_state *st, uint32_t kind, const uint8_t *sid, uint32_t sid_len, const int16_t *voice /* may be NULL */,
                    uint32_t samples_per_frame, uint32_t ctl, uint32_t seed, int16_t *out, igdsp_cng_rec *rec);
int igdsp_cng_run(igdsp_ctx *ctx, const uint8_t *d_kind /* [F][C] */, const uint8_t *d_sid /* [F][C][16] */,
                  const uint8_t *d_sid_len /* [F][C], NULL: 11 */, const uint8_t *d_g711 /* [F][C][n] */, const uint8_t *d_codec /* [C] */,
                  const int16_t *d_pcm /* [F][C][n] */, const uint8_t *d_ctl /* [C], NULL: RUN */, const uint32_t *d_seed /* [C] */,
                  uint32_t n_channels, uint32_t n_frames, uint32_t samples_per_frame, igdsp_cng_state *d_state /* [C], in and out */,
                  int16_t *d_out /* [F][C][n] */, uint16_t *d_len_out /* [F][C] */, igdsp_cng_rec *d_rec /* [F][C] */,
                  igdsp_frame_stats *d_stats /* [F][C] */, void *stream);

/* ---- Filter: per channel a chain of up to four second-order IIR sections ------------------------------------------------------------------
 * Neither pjmedia nor the reference holds a linear filter: the reference's only per-slot control is the static SLOT_VOLUME, its sidetone
 * levels are further static gains.  igdsp_filt_run runs a row (G.711 codes with d_codec, or PCM, [F][C][n]) through the channel's plan:
 * a high pass under a radio's sub-audible tone, a de- or pre-emphasis, a band limit, a notch, a DC block.  It stands after
 * igdsp_plc_conceal / igdsp_cng_run / igdsp_bss_select and before igdsp_agc_run, on a port row before igdsp_tx_packetize, on
 * igdsp_snd_split's rows before igdsp_vad_run, and behind igdsp_tone_detect for a notch.  Everything is integer.
 * The rule is the library's own, UNVERIFIED against any other filter implementation.
 *
 * RULE.  A section is five Q13 coefficients in int16, b0 b1 b2 a1 a2 (8192 is 1.0, a0 is 1).  A plan is 1..4 sections and the clock
 * rate it was designed for (informational: it plays no part in the arithmetic).  A section is VALID when
 * |b0| + |b1| + |b2| + |a1| + |a2| <= 65535.  Per channel and section the state is x1, x2, y1, y2 (int16) and e (0..8191).  Each sample
 * goes through the sections 0 .. S-1 in order, v the section's input:
 *        acc = b0*v + b1*x1 + b2*x2 - a1*y1 - a2*y2 + e          (int32, exact)
 *        y = acc >> 13 (arithmetic);  e = acc & 8191
 *        y > 32767: y = 32767, e = 0, clipped += 1;   y < -32768: y = -32768, e = 0, clipped += 1
 *        x2 = x1; x1 = v; y2 = y1; y1 = y;   v = y
 * e is first-order error feedback: the 13 bits the shift drops go into the next sample, which holds a 300 Hz pole pair in place with
 * 16-bit states and lets the output of a stable section decay to exact zero on zero input.  Every |state| <= 32768, so with a valid
 * section |acc| and every partial sum of it stay <= 65535 * 32768 + 8191 < 2^31 (csrc/igdsp_filt.h proves it): nothing needs 64 bits.
 * The identity section {8192, 0, 0, 0, 0} returns its input bit for bit and leaves e as it was.
 *
 * PLANS.  d_plans[n_plans] lives in device memory and may hold any bytes; d_plan_of[c] (NULL: plan 0) picks the channel's.
 * n_sections is read as min(n_sections, 4).  A channel whose index is >= n_plans, or whose plan has n_sections 0: out = x, the state's
 * bytes are not touched, IGDSP_FILT_NO_PLAN.  An invalid section is not run (IGDSP_FILT_BAD_PLAN).  A section that is not run -
 * invalid, or at or past n_sections - passes its input on and leaves its history as read.  max_sections is the caller's word for
 * the largest n_sections among the launch's plans (1..4; 0 counts as 4): it picks the kernel, one written for 1, 2 or 4 sections.  A
 * plan with more sections than that is not run at all: out = x, the state untouched, IGDSP_FILT_NO_PLAN | IGDSP_FILT_BAD_PLAN.
 *
 * STATE.  igdsp_filt_state, 48 bytes, one per channel, read at the start of a launch and written at its end.  A tag other than
 * IGDSP_FILT_TAG (all-zero included) means all-zero histories.  Under the right tag any bytes are a valid state: e is read & 8191,
 * nothing indexes by a field.  flags is written as the last frame's record flags, reserved as 0.  F frames in one launch, F launches
 * of one frame and any split in between write the same bytes; a channel's results are the same at any channel count and position.
 * The state carries no plan identity: a caller that changes a channel's plan sends IGDSP_FILT_RESET.
 *
 * CONTROL.  d_ctl[c] (NULL: IGDSP_FILT_RUN; a value above 2 counts as RUN) holds for the launch:
 *   IGDSP_FILT_RUN;   IGDSP_FILT_BYPASS: out = x, the state's bytes are not touched, the record carries IGDSP_FILT_BYPASSED alone;
 *   IGDSP_FILT_RESET: the histories are zeroed before the first frame, then RUN (a channel without a plan stays untouched).
 *
 * OUTPUTS, each optional, at least one required.  d_out[f][c][n].  d_rec[f][c] (igdsp_filt_rec): in_peak = max |x| (32768 for
 * -32768), out_peak = max |out|, n_clipped = the frame's clipped count summed over the sections (saturating at 65535), plan =
 * the channel's plan index, n_sections = min(n_sections, 4) of its plan (0 without one), flags = IGDSP_FILT_CLIPPED (n_clipped > 0),
 * _NO_PLAN, _BAD_PLAN, _BYPASSED, _WAS_RESET (the launch's first frame, when the histories were zeroed by RESET or by another tag).
 * d_stats[f][c]: the PCM record of out, as igdsp_conf_mix writes it.  With d_out NULL the stage runs for state and records only.
 * Rows at a bridge rate above 8 kHz go as the sub-frames igdsp_resample writes: the state chains across frames.
 *
 * ARGUMENTS.  samples_per_frame not a multiple of 8 in 8..256, max_sections > 4: IGDSP_EINVAL, whether or not there is work.
 * n_channels == 0 or n_frames == 0: nothing to do.  Exactly one of d_g711 (with d_codec) and d_pcm; d_plans with n_plans >= 1, d_state
 * and one of d_out, d_rec, d_stats required.  n_channels * n_frames < 2^32 - 32 (IGDSP_ERANGE).  d_g711 8-byte, d_pcm, d_out,
 * d_state, d_rec, d_stats 16-byte, d_plans 4-byte, d_plan_of 2-byte aligned.  The state and the outputs may overlap neither an input
 * nor each other.  Enqueued on `stream`, not synchronised.
 *
 * Host only, no GPU.  igdsp_filt_frame: one frame of one channel from PCM by the same rule (plan NULL: a channel without a plan; out
 * and rec optional; rec.plan is 0).  igdsp_filt_plan_check: IGDSP_EINVAL for a plan the kernel would flag (n_sections 0 or above 4,
 * an invalid section).  igdsp_filt_design: one section of the RBJ cookbook, computed in double and rounded to the nearest Q13:
 * LOWPASS, HIGHPASS, BANDPASS (0 dB peak), NOTCH, PEAK, LOWSHELF, HIGHSHELF (q sets alpha = sin(w0) / (2 q); gain_db is read by the
 * last three), and the first-order LP1 / HP1 (bilinear, b2 = a2 = 0; q and gain_db are not read).  It needs 0 < f0_hz < clock_rate / 2
 * and q > 0, and returns IGDSP_EINVAL, writing nothing, when a coefficient leaves int16, when the section is invalid or when the
 * QUANTISED poles are not strictly inside the unit circle (|a2| < 8192 and |a1| < 8192 + a2).  igdsp_filt_plan_preset, clock rates
 * 8000..48000, IGDSP_EINVAL when a corner is at or above half the clock rate:
 *   VOICE_BAND: Butterworth HIGHPASS 300 Hz then LOWPASS 3400 Hz, q = 1/sqrt(2) each;
 *   CTCSS_HP:   fourth-order Butterworth HIGHPASS 300 Hz as two sections, q = 1/(2 cos(pi/8)) and 1/(2 cos(3 pi/8));
 *   PREEMPH:    6 dB/octave up from 300 Hz, levelling at 3400 Hz: g (1 - a z^-1) / (1 - p z^-1) with a = exp(-2 pi 300 / clock_rate) and
 *               p = exp(-2 pi 3400 / clock_rate) (the corners matched in z, not warped), g for unity gain at 1 kHz;
 *   DEEMPH:     its inverse, 6 dB/octave down from 300 Hz: g' (1 - p z^-1) / (1 - a z^-1), unity gain at 1 kHz;
 *   DC_BLOCK:   HP1 at 20 Hz. */
#define IGDSP_FILT_TAG      0xF1170001u /* igdsp_filt_state.tag                                   */
#define IGDSP_FILT_MAX_SECTIONS 4
#define IGDSP_FILT_UNITY    8192
#define IGDSP_FILT_RUN      0           /* d_ctl                                                    */
#define IGDSP_FILT_BYPASS   1
#define IGDSP_FILT_RESET    2
#define IGDSP_FILT_CLIPPED   0x01       /* igdsp_filt_rec.flags                                     */
#define IGDSP_FILT_NO_PLAN   0x02
#define IGDSP_FILT_BAD_PLAN  0x04
#define IGDSP_FILT_BYPASSED  0x08
#define IGDSP_FILT_WAS_RESET 0x10
#define IGDSP_FILT_LOWPASS   0          /* igdsp_filt_design's kind                                 */
#define IGDSP_FILT_HIGHPASS  1
#define IGDSP_FILT_BANDPASS  2
#define IGDSP_FILT_NOTCH     3
#define IGDSP_FILT_PEAK      4
#define IGDSP_FILT_LOWSHELF  5
#define IGDSP_FILT_HIGHSHELF 6
#define IGDSP_FILT_LP1       7
#define IGDSP_FILT_HP1       8
#define IGDSP_FILT_VOICE_BAND 0         /* igdsp_filt_plan_preset's preset                          */
#define IGDSP_FILT_CTCSS_HP   1
#define IGDSP_FILT_DEEMPH     2
#define IGDSP_FILT_PREEMPH    3
#define IGDSP_FILT_DC_BLOCK   4
typedef struct igdsp_filt_section {
    int16_t b0, b1, b2, a1, a2;     /* Q13                                                       */
} igdsp_filt_section;               /* 10 bytes */
typedef struct igdsp_filt_plan {
    uint16_t n_sections, reserved;
    uint32_t clock_rate;            /* informational                                             */
    igdsp_filt_section s[4];
} igdsp_filt_plan;                  /* 48 bytes */
typedef struct igdsp_filt_hist {
    int16_t  x1, x2, y1, y2;
    uint16_t e;                     /* the error feedback, 0..8191                               */
} igdsp_filt_hist;                  /* 10 bytes */
typedef struct igdsp_filt_state {
    uint32_t tag;
    igdsp_filt_hist s[4];
    uint16_t flags, reserved;
} igdsp_filt_state;                 /* 48 bytes */
typedef struct igdsp_filt_rec {
    uint16_t in_peak, out_peak, n_clipped, plan;
    uint8_t  flags, n_sections, reserved[6];
} igdsp_filt_rec;                   /* 16 bytes */
int igdsp_filt_frame(const igdsp_filt_plan *plan, igdsp_filt_state *st, const int16_t *pcm, uint32_t samples_per_frame, uint32_t ctl,
                     int16_t *out, igdsp_filt_rec *rec);
int igdsp_filt_plan_check(const igdsp_filt_plan *plan);
int igdsp_filt_design(uint32_t kind, uint32_t clock_rate, double f0_hz, double q, double gain_db, int16_t *out /* [5] */);
int igdsp_filt_plan_preset(uint32_t preset, uint32_t clock_rate, igdsp_filt_plan *plan);
int igdsp_filt_run(igdsp_ctx *ctx, const uint8_t *d_g711 /* [F][C][n] */, const uint8_t *d_codec /* [C] */,
                   const int16_t *d_pcm /* [F][C][n] */, const uint8_t *d_ctl /* [C], NULL: RUN */, const igdsp_filt_plan *d_plans,
                   uint32_t n_plans, const uint16_t *d_plan_of /* [C], NULL: plan 0 */, uint32_t max_sections, uint32_t n_channels,
                   uint32_t n_frames, uint32_t samples_per_frame, igdsp_filt_state *d_state /* [C], in and out */,
                   int16_t *d_out /* [F][C][n] */, igdsp_filt_rec *d_rec /* [F][C] */, igdsp_frame_stats *d_stats /* [F][C] */, void *stream);

/* ---- Noise suppression: per channel a spectral gain under and between speech ------------------------------------------------------------
 * What pjmedia's sound port switches on with PJMEDIA_ECHO_USE_NOISE_SUPPRESSOR (speex's preprocessor, `denoise`) and the reference
 * leaves out: stationary noise (a receiver's hiss) is lowered by up to `floor_q15` under and between transmissions.  Stands behind
 * igdsp_plc_conceal / igdsp_cng_run / igdsp_bss_select / igdsp_filt_run and before igdsp_agc_run and igdsp_conf_mix; on igdsp_snd_split's
 * rows before igdsp_vad_run and igdsp_echo_cancel's near end.  The rule is the library's own, UNVERIFIED against speex, WebRTC and
 * ITU-T G.160.  All integer: the host (igdsp_ns_frame) and the device (igdsp_ns_run) give the same bits, and a channel's bits depend on
 * nothing but its own samples, state, cfg and ctl: the same at any channel count and position, from G.711 or its decoded PCM, and for
 * any split of the frames over launches.
 * THE OUTPUT IS THE INPUT DELAYED BY EXACTLY 80 SAMPLES (10 ms), under every control value.
 *
 * 8 kHz rows only (a bridge at a higher rate runs the stage on the narrow side of igdsp_resample).  samples_per_frame is 80, 160, 240
 * or 320: a frame is 1 to 4 hops of 80 samples.  Per hop (csrc/igdsp_ns.h has every rounding step; tests/ns_model.py restates it):
 *   1. window: x[0..159] = the previous hop's samples (state.prev), then this hop's; w[i] = round(32768 sin(pi (i + 0.5) / 160))
 *      (igdsp_ns_tables); xw[i] = (x[i] w[i] + 128) >> 8 (Q7, |xw| < 2^22).
 *   2. forward transform: xw zero-padded to 256 points; 128 packed complex points z[k] = xw[2k] + i xw[2k+1] through seven radix-2
 *      passes, decimation in frequency, spans 128 down to 2: a' = a + b (exact), b' = ((a - b) t + 2^29) >> 30 with t = W^pos of the
 *      span, conjugate for the forward direction; then a split pass over the pairs (k, 128 - k): with A = Z[k], B = conj(Z[128 - k]),
 *      E = A + B, O = A - B and (c, s) = (cos, sin)(2 pi k / 256): X[k] = (E 2^30 + (-s - i c) O + 2^30) >> 31; X[0] = Re Z[0] + Im Z[0],
 *      X[128] = Re Z[0] - Im Z[0].  Bins 0..128, unscaled, int32 pairs in Q7.  The twiddle factors are Q30 (igdsp_ns_tables); every
 *      product with one is formed in 64 bits, a butterfly's sum is kept in 64 bits and each component rounded once.  ">>" is arithmetic.
 *   3. bands: 32 bands of four bins, band b = bins 4b+1 .. 4b+4; E[b] = (sum of re^2 + im^2, exact in 64 bits) >> 14.
 *   4. S[b] = E[b] on the state's hop 0, else S[b] += (E[b] - S[b]) >> 2.
 *   5. unless frozen: hops < init_hops: N += (S - N) >> 2; else S < 4 N: N += (S - N) >> track_shift; else N += (N >> rise_shift) + 1.
 *   6. d = S - ((over_q4 N) >> 4); d <= 0 or S == 0: G = 0; else t = max(0, bitlen(S) - 16), G = min(32768, ((d >> t) << 15) /
 *      max(1, S >> t)) (one exact unsigned 32-bit division); G = max(G, floor_q15).
 *   7. Gs[b] = (G[b-1] + 2 G[b] + G[b+1] + 2) >> 2, the edge bands repeated.
 *   8. Gs[b] >= Gt[b]: Gt[b] = Gs[b]; else Gt[b] += (Gs[b] - Gt[b]) >> 1 (Gt in the state; fresh: 32768).
 *   9. bin 0 takes Gt[0], bins 4b+1..4b+4 take Gt[b]: Y = (X Gt + 16384) >> 15 per component.
 *  10. inverse transform with the 1/256 inside: the split pass backwards, Z[k] = (E 2^30 + (-s + i c) O + 2^30) >> 31 from A = Y[k],
 *      B = conj(Y[128 - k]), Z[0] = ((Y[0] + Y[128] + 1) >> 1, (Y[0] - Y[128] + 1) >> 1); then seven radix-2 passes, decimation in time,
 *      spans 2 up to 128, each halving: a' = (a 2^30 + b t + 2^30) >> 31, b' = (a 2^30 - b t + 2^30) >> 31;
 *      y[i], i = 0..159, Q7, the padded tail dropped; yw[i] = (y[i] w[i] + 16384) >> 15; for i < 80: out[i] = (ola[i] + yw[i] + 64) >> 7
 *      saturated to int16 (each saturation counts as clipped); then ola[i] = yw[i + 80]; then hops += 1 (saturating at 65535).
 * Defaults (igdsp_ns_cfg_default): floor_q15 5827 (-15 dB), over_q4 24, init_hops 16, track_shift 4, rise_shift 9.  Ranges, anything
 * else IGDSP_EINVAL: floor_q15 1..32768, over_q4 16..64, init_hops 1..255, track_shift 1..8, rise_shift 4..12.
 * LIMIT: a steady tone present from hop 0 is learnt as noise and lands at the floor; one that starts later is kept (the third branch
 * of step 5 moves N by under 1 dB in 3 s).  A caller sets IGDSP_NS_FREEZE while a tone port or DTMF plays on the leg.
 *
 * STATE, 1 072 bytes: another tag (all-zero included) is a fresh state: hops 0, prev, ola, S, N zero, Gt 32768.  Under the tag any
 * bytes are valid: S and N are read masked to 56 bits, Gt clamped to 32768, nothing indexes by a field.
 * CONTROL d_ctl[c] (NULL or a value above 3: RUN), held for the launch: RUN; FREEZE (S, N and hops held; the gains still computed, from
 * the S the hop would have had against the held N, smoothed into Gt and applied); BYPASS (out = the input through the same 80-sample delay, bit for bit; prev is
 * kept and ola holds what unity gains would leave, so that a switch between RUN and BYPASS does not click; S, N, Gt, hops untouched;
 * the record carries BYPASSED alone among the flags); RESET (fresh state, then RUN; WAS_RESET on the launch's first frame, as after
 * another tag).
 * RECORD, 16 bytes per frame: in_energy / out_energy = (sum of squares of the frame's input / output) >> 8; min_gain_q15 = the least
 * Gt over the frame's hops and bands (32768 under BYPASS); noise_idx = bitlen(sum of N) after the frame; n_clipped; flags LEARNING (a
 * hop ran with hops < init_hops), SUPPRESSING (min_gain_q15 < 32768), CLIPPED, FROZEN, BYPASSED, WAS_RESET.
 * d_stats[f][c]: the PCM record of out, as igdsp_conf_mix writes it.  With d_out NULL the stage runs for state and records only.
 *
 * ARGUMENTS.  samples_per_frame not 80, 160, 240 or 320, cfg NULL or out of range: IGDSP_EINVAL, whether or not there is work.
 * n_channels == 0 or n_frames == 0: nothing to do.  Exactly one of d_g711 (with d_codec) and d_pcm; d_state and one of d_out, d_rec,
 * d_stats required.  n_channels * n_frames < 2^32 - 32 (IGDSP_ERANGE).  d_g711 8-byte, d_pcm, d_out, d_state, d_rec, d_stats 16-byte
 * aligned.  The state and the outputs may overlap neither an input nor each other.  cfg is host memory, copied.  Enqueued on `stream`,
 * not synchronised.
 * Host only, no GPU: igdsp_ns_cfg_default; igdsp_ns_tables (the window's 160 int16 and the 128 twiddle pairs, either may be NULL);
 * igdsp_ns_frame: one frame of one channel from PCM by the same rule (out and rec optional). */
#define IGDSP_NS_TAG        0x4E530001u /* igdsp_ns_state.tag                                      */
#define IGDSP_NS_HOP        80
#define IGDSP_NS_BANDS      32
#define IGDSP_NS_UNITY      32768
#define IGDSP_NS_RUN        0           /* d_ctl                                                    */
#define IGDSP_NS_FREEZE     1
#define IGDSP_NS_BYPASS     2
#define IGDSP_NS_RESET      3
#define IGDSP_NS_LEARNING    0x01       /* igdsp_ns_rec.flags                                       */
#define IGDSP_NS_SUPPRESSING 0x02
#define IGDSP_NS_CLIPPED     0x04
#define IGDSP_NS_FROZEN      0x08
#define IGDSP_NS_BYPASSED    0x10
#define IGDSP_NS_WAS_RESET   0x20
typedef struct igdsp_ns_cfg {
    uint32_t floor_q15;             /* the least gain, Q15: 1..32768                             */
    uint16_t over_q4;               /* the noise estimate's weight in the gain, Q4: 16..64       */
    uint16_t init_hops;             /* hops that learn the floor at the start of a leg: 1..255   */
    uint16_t track_shift;           /* 1..8                                                      */
    uint16_t rise_shift;            /* 4..12                                                     */
    uint32_t reserved;
} igdsp_ns_cfg;                     /* 16 bytes */
typedef struct igdsp_ns_state {
    uint32_t tag;
    uint16_t hops, flags;           /* hops saturates at 65535; flags: the last frame's record flags */
    uint32_t reserved[2];
    int16_t  prev[80];              /* the previous hop's input                                  */
    int32_t  ola[80];               /* the synthesis overlap, Q7                                 */
    uint64_t S[32], N[32];          /* smoothed band energy, noise estimate                      */
    uint16_t Gt[32];                /* the band gains, Q15                                       */
} igdsp_ns_state;                   /* 1 072 bytes */
typedef struct igdsp_ns_rec {
    uint32_t in_energy, out_energy;
    uint16_t min_gain_q15, n_clipped;
    uint8_t  noise_idx, flags, reserved[2];
} igdsp_ns_rec;                     /* 16 bytes */
void igdsp_ns_cfg_default(igdsp_ns_cfg *out);
int  igdsp_ns_tables(const int16_t **window /* [160] */, const int32_t **twiddle /* [128][2] */);
int  igdsp_ns_frame(const igdsp_ns_cfg *cfg, igdsp_ns_state *st, const int16_t *pcm, uint32_t samples_per_frame, uint32_t ctl,
                    int16_t *out, igdsp_ns_rec *rec);
int  igdsp_ns_run(igdsp_ctx *ctx, const uint8_t *d_g711 /* [F][C][n] */, const uint8_t *d_codec /* [C] */, const int16_t *d_pcm /* [F][C][n] */,
                  const uint8_t *d_ctl /* [C], NULL: RUN */, const igdsp_ns_cfg *cfg /* host, copied */, uint32_t n_channels, uint32_t n_frames,
                  uint32_t samples_per_frame, igdsp_ns_state *d_state /* [C], in and out */, int16_t *d_out /* [F][C][n] */,
                  igdsp_ns_rec *d_rec /* [F][C] */, igdsp_frame_stats *d_stats /* [F][C] */, void *stream);

/* ---- SRTP: RFC 3711 protection of the RTP packets, per leg and direction -------------------------------------------------------------------
 * What pjmedia's transport_srtp does between the adapter and the socket when `use_srtp` is on: igdsp_srtp_protect stands behind
 * igdsp_tx_packetize (in front of transport_send_rtp), igdsp_srtp_unprotect in front of igdsp_jb_receive / igdsp_depayload /
 * igdsp_decode_meter_packets* (behind transport_rtp_cb).  The rule is pinned bit for bit by RFC 3711, FIPS-197 and FIPS 180 / RFC 2104;
 * tests/golden/srtp_kat.json holds the standards' known answers.  The host entries (igdsp_srtp_*_packet) and the device entries run
 * the same code (csrc/igdsp_srtp.h; independent restatement: tests/srtp_model.py) and give the same bytes, records and states for any
 * split of the frames over launches and at any channel count and position.
 * SCOPE: AES_CM_128_HMAC_SHA1_80 and its _32 tag length, for RTP (SRTCP: the section "RTCP / SRTCP" below).  NOT built: MKI, a non-zero
 * key derivation rate, AES-256 in counter mode (RFC 6188; AES-GCM with either key size: the section "SRTP with AES-GCM" below),
 * F8, the NULL cipher, and SDES / DTLS key exchange: the caller brings the 30 bytes of master key and salt that pjmedia keeps in
 * pjmedia_srtp_crypto.key.
 *
 * HEADER LENGTH.  h = 12 + 4 CC; with X set h += 4 + 4 ext_len, ext_len the big-endian u16 at h + 2.  Every read is bounded by the
 * packet's size.  MALFORMED: version not 2, size < 12, the header passing size at any step, size > 2048, size above the input slot,
 * size_out above the output slot or capacity, and on unprotect size < h + tag_len.  The header, an ED-137 extension included, stays
 * in the clear and under the tag.
 * INDEX.  The state holds roc, s_l and have_s_l.  First packet: s_l := seq.  v as RFC 3711 Appendix A: s_l < 32768: v = (seq - s_l >
 * 32768) ? roc - 1 : roc; else v = (s_l - 32768 > seq) ? roc + 1 : roc (integer comparisons, v mod 2^32).  index = v 2^16 + seq, a
 * 48-bit number, compared against top = roc 2^16 + s_l.
 * KEYSTREAM.  IV = (k_s 2^16) xor (SSRC 2^64) xor (index 2^16), 128 bits big-endian, the packet's own SSRC; block j = AES_k_e(IV + j),
 * XORed onto the bytes from h on.  An empty payload is legal.
 * TAG.  The first tag_len bytes of HMAC-SHA1(k_a, header || encrypted payload || v as 4 big-endian bytes).
 * PROTECT.  The estimate, no replay test; writes header || ciphertext || tag, size_out = size + tag_len; roc = v, s_l = seq when index
 * > top or on the first packet; ROLLED when roc changed.  size == 0 (igdsp_tx_packetize's unsent frames): EMPTY, size_out 0.
 * UNPROTECT.  size includes the tag.  Estimate; against a 64-packet window top - index >= 64 is OLD, a set bit REPLAY; the tag is
 * computed with v and compared, a mismatch is AUTH_FAIL; decrypt, size_out = size - tag_len; the window moves (an index ahead shifts
 * it by the distance, >= 64 clears it, sets bit 0 and takes roc / s_l; otherwise the index's bit is set).  Any failure leaves the
 * state as it was except its counter, gives size_out 0 and writes nothing into the output slot.
 * FAIL CLOSED.  A state whose tag word is not IGDSP_SRTP_TAG | 4 or | 10 gives NO_KEY (the record's flags are 0) and size_out 0 in both
 * directions, whatever its other bytes; protect never emits a clear packet.
 * CONTROL d_ctl[f][c] (NULL or another value: RUN): BYPASS copies the packet through unchanged, the state untouched, with or without a
 * key; RESET sets roc = 0, have_s_l = 0 and clears the window before the frame, the keys kept.
 * RECORD, 8 bytes: roc_used = v (0 where no index was estimated), size_out, flags.  The outcomes OK, AUTH_FAIL, REPLAY, OLD, MALFORMED,
 * EMPTY, BYPASSED exclude each other; ROLLED comes with OK; NO_KEY is the value 0.
 * STATE, 288 bytes, one per leg and direction, from igdsp_srtp_derive: the tag word, roc, s_l, have_s_l, the replay window, four
 * counters (ok, auth failures, replays and old, malformed), the 44 words of k_e's key schedule, k_s, and the two SHA-1 states after
 * k_a xor ipad and k_a xor opad.
 *
 * ARGUMENTS of the two batched entries.  packets[f][c][pkt_stride] + sizes[f][c] is what igdsp_tx_packetize writes and igdsp_depayload
 * / igdsp_jb_receive read.  Both strides multiples of 4, 12..2048.  d_sizes is required (a protected packet never fills its slot).
 * n_channels * n_frames < 2^32 - 32 (IGDSP_ERANGE).  d_packets, d_out 4-byte, d_sizes, d_sizes_out 2-byte, d_rec 8-byte, d_state 16-byte
 * aligned.  In place is allowed: d_out == d_packets with equal strides, d_sizes_out == d_sizes; any other overlap of an output with an
 * input, the state or another output is IGDSP_EINVAL.  Bytes of an output slot past size_out are never written.  Enqueued on `stream`.
 * Host only, no GPU: igdsp_srtp_derive (RFC 3711 4.3.1, labels 0, 1, 2; tag_len 4 or 10, anything else IGDSP_EINVAL);
 * igdsp_srtp_protect_packet / igdsp_srtp_unprotect_packet: one packet by the same rule, in == out allowed. */
#define IGDSP_SRTP_TAG        0x53525000u /* igdsp_srtp_state.tag, | tag_len (4 or 10)                */
#define IGDSP_SRTP_MAX_PACKET 2048
#define IGDSP_SRTP_RUN        0           /* d_ctl                                                    */
#define IGDSP_SRTP_BYPASS     1
#define IGDSP_SRTP_RESET      2
#define IGDSP_SRTP_NO_KEY     0x00        /* igdsp_srtp_rec.flags: no flag at all                     */
#define IGDSP_SRTP_OK         0x01
#define IGDSP_SRTP_AUTH_FAIL  0x02
#define IGDSP_SRTP_REPLAY     0x04
#define IGDSP_SRTP_OLD        0x08
#define IGDSP_SRTP_MALFORMED  0x10
#define IGDSP_SRTP_EMPTY      0x20
#define IGDSP_SRTP_ROLLED     0x40
#define IGDSP_SRTP_BYPASSED   0x80
typedef struct igdsp_srtp_state {
    uint32_t tag;                   /* IGDSP_SRTP_TAG | tag_len                                  */
    uint32_t roc;
    uint16_t s_l, have_s_l;
    uint32_t reserved;
    uint64_t window;                /* bit i: index top - i was accepted (unprotect)             */
    uint32_t n_ok, n_auth_fail, n_replay, n_malformed;
    uint32_t rk[44];                /* AES-128 encryption key schedule of k_e                    */
    uint8_t  ks[16];                /* k_s, 14 bytes, then two zero bytes: k_s 2^16, big-endian  */
    uint32_t mid_i[5], mid_o[5];    /* SHA-1 after the block k_a xor ipad / k_a xor opad         */
    uint32_t reserved2[4];
} igdsp_srtp_state;                 /* 288 bytes */
typedef struct igdsp_srtp_rec {
    uint32_t roc_used;
    uint16_t size_out;
    uint8_t  flags, reserved;
} igdsp_srtp_rec;                   /* 8 bytes */
int  igdsp_srtp_derive(const uint8_t key_salt[30], uint32_t tag_len, uint32_t roc0, igdsp_srtp_state *out);
int  igdsp_srtp_protect_packet(igdsp_srtp_state *st, uint32_t ctl, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity,
                               uint32_t *size_out, igdsp_srtp_rec *rec);
int  igdsp_srtp_unprotect_packet(igdsp_srtp_state *st, uint32_t ctl, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity,
                                 uint32_t *size_out, igdsp_srtp_rec *rec);
int  igdsp_srtp_protect(igdsp_ctx *ctx, const uint8_t *d_ctl /* [F][C], NULL: RUN */, const uint8_t *d_packets /* [F][C][pkt_stride] */,
                        const uint16_t *d_sizes /* [F][C] */, uint32_t n_channels, uint32_t n_frames, uint32_t pkt_stride,
                        igdsp_srtp_state *d_state /* [C], in and out */, uint8_t *d_out /* [F][C][out_stride] */, uint32_t out_stride,
                        uint16_t *d_sizes_out /* [F][C] */, igdsp_srtp_rec *d_rec /* [F][C] */, void *stream);
int  igdsp_srtp_unprotect(igdsp_ctx *ctx, const uint8_t *d_ctl /* [F][C], NULL: RUN */, const uint8_t *d_packets /* [F][C][pkt_stride] */,
                          const uint16_t *d_sizes /* [F][C] */, uint32_t n_channels, uint32_t n_frames, uint32_t pkt_stride,
                          igdsp_srtp_state *d_state /* [C], in and out */, uint8_t *d_out /* [F][C][out_stride] */, uint32_t out_stride,
                          uint16_t *d_sizes_out /* [F][C] */, igdsp_srtp_rec *d_rec /* [F][C] */, void *stream);

/* ---- RTCP / SRTCP: the reports of RFC 3550 per leg, clear and protected (RFC 3711 3.4) ------------------------------------------------------
 * The other two per-packet slots of the pjmedia adapter: igdsp_rtcp_build -> igdsp_srtcp_protect stand in front of transport_send_rtcp /
 * transport_send_rtcp2, igdsp_srtcp_unprotect -> igdsp_rtcp_parse behind transport_rtcp_cb.  The caller decides the ticks (the report
 * interval's timing is not built).  The host entries (igdsp_rtcp_*_packet, igdsp_srtcp_*_packet) and the device entries run the same
 * code (csrc/igdsp_rtcp.h; independent restatement: tests/rtcp_model.py) and give the same bytes, records and states for any split of
 * the ticks over launches and at any leg count and position.
 * Fidelity.  PINNED to RFC 3550 6.4, 6.5, 6.6, A.2, A.3 and RFC 3711 3.4, 4.3.1.  UNVERIFIED against pjmedia's rtcp.c and against libsrtp
 * (neither is in this tree).  NOT built: XR, APP, feedback packets, reason text in BYE, more than one report block, the report
 * interval's timing, MKI.
 *
 * BUILD, per leg, ticks in order.  d_ctl[f][c]: NONE (or any other value) builds nothing: size 0, the slot, the state untouched, the
 * record's flags 0.  REPORT builds a compound packet, BYE the same with a BYE appended.
 *   Packet type: SR (200) when src.packets != state.sent_prior, else RR (201) (RFC 3550 6.4).  Report count 1 when d_jb[c] has
 *   IGDSP_JB_HEARD, else 0 (d_jb NULL: 0).  The block: the source's SSRC; fraction lost, 24-bit cumulative lost, extended highest seq
 *   and jitter exactly what igdsp_jb_report returns for that state and state.prior (A.3, the epoch rule included); LSR = state.lsr and
 *   DLSR = mid - state.lsr_arrival mod 2^32, mid = (d_now[f] >> 16) & 0xFFFFFFFF, both 0 without HAVE_SR.  state.prior advances only
 *   when a block is written.  SR sender info: NTP msw, NTP lsw of d_now[f], src.rtp_ts, src.packets, src.octets.
 *   SDES (202), one chunk: SSRC, item 1 (CNAME) of length L = min(d_cname_len[c], 64) and the text, then at least one null octet up to
 *   a 4-byte boundary: 4 * ceil((7 + L) / 4) bytes.  d_cname and d_cname_len both NULL: L = 0.  With BYE: 0x81, 203, length 1, SSRC.
 *   Byte 0 of every header is 0x80 | count, lengths are words minus one, every field big-endian, every SSRC of ours src.ssrc.  The
 *   largest packet is 52 + 76 + 8 = IGDSP_RTCP_MAX_BUILT bytes.  After the packet: sent_prior = src.packets, n_built += 1.
 *   Record, 8 bytes: size, flags (SR or RR, HAS_BLOCK, BYE_SENT).  Bytes of the slot past the size are never written.
 * PARSE.  size 0: EMPTY.  d_arrival[f][c]: the arrival time's middle 32 NTP bits.  Every read is bounded by the packet's size and slot.
 *   MALFORMED (RFC 3550 A.2, integer comparisons; the state unchanged except n_malformed): size < 8, size % 4 != 0, size > pkt_stride;
 *   the first sub-packet without V = 2, P = 0 and PT 200 or 201; a sub-packet without V = 2 or whose 4 * (length + 1) bytes pass the
 *   packet's end (the walk ends exactly at size); P on another sub-packet than the last; an SR shorter than 28 + 24 RC, an RR shorter
 *   than 8 + 24 RC, a BYE shorter than 4 + 4 SC.
 *   A valid packet: the record's sender SSRC is the first sub-packet's.  An SR gives lsr = (msw << 16) | (lsw >> 16), lsr_arrival =
 *   arrival, HAVE_SR, and its counts go into the record (of several SRs the last).  In SR and RR the first block of the packet whose
 *   source SSRC equals d_local_ssrc[c] gives peer_fraction_lost, peer_cum_lost (24 bits, sign-extended), peer_ext_seq, peer_jitter:
 *   kept in the state (PEER_VALID) and the record.  With a non-zero LSR in that block rtt = arrival - LSR - DLSR mod 2^32, in units of
 *   1 / 65536 s: below 2^31 it is stored as rtt_last, rtt_count += 1, RTT_VALID; otherwise the record gets RTT_NEGATIVE and nothing is
 *   stored.  BYE sets BYE_SEEN.  SDES and every other type are stepped over by their length.  n_parsed += 1.
 * igdsp_rtcp_state: 80 bytes per leg, shared by build and parse; all-zero is the reset state; nothing in it is used as an index.
 *
 * SRTCP (RFC 3711 3.4), AES_CM_128_HMAC_SHA1_80 and _32 (the RTCP tag is 10 bytes in both: RFC 3711 / RFC 4568).  The state is an
 * igdsp_srtp_state from igdsp_srtcp_derive: key derivation labels 3 (k_e), 4 (k_a), 5 (k_s), the tag word IGDSP_SRTCP_TAG | 10.  A state
 * of igdsp_srtp_derive handed to an SRTCP entry is NO_KEY, and the other way round: both fail closed.  `roc` holds the 31-bit SRTCP index:
 * on protect the index the next packet carries (the packet takes it, then roc = (roc + 1) mod 2^31; index0 lets the caller start at 0,
 * as the RFC says, or at 1, libsrtp's habit: UNVERIFIED); on unprotect the highest index accepted, with have_s_l and the 64-bit window
 * as in SRTP.  s_l stays 0.
 *   Packet: header (8) || AES-CM(bytes 8 .. size) || (E << 31 | index) || tag (10).  IV as in SRTP with the packet's SSRC (bytes 4..7)
 *   and the index as the 48-bit index.  Tag: the first 10 bytes of HMAC-SHA1 over the packet and the index word.
 *   PROTECT: V = 2, size >= 8, size % 4 == 0 and size + 14 <= the output slot, else MALFORMED; E = 1 always; size_out = size + 14;
 *   size 0: EMPTY.  UNPROTECT: size >= 22 and (size - 14) % 4 == 0, else MALFORMED; then OLD / REPLAY against the window, then
 *   AUTH_FAIL.  E = 0: authenticated and copied without decryption (IGDSP_SRTCP_CLEAR beside OK).  Indices are compared as plain 31-bit
 *   numbers: a wrap of the received index is not handled (2^31 reports).
 *   Records are igdsp_srtp_rec with roc_used = the index word; flags, RUN / BYPASS / RESET, in place, a refused packet's slot never
 *   written, the counters and the argument rules are SRTP's (strides multiples of 4, 12..2048).
 *
 * ARGUMENTS of igdsp_rtcp_build: d_ctl, d_src, d_now, d_state, d_packets, d_sizes required; d_jb, d_rec optional; d_cname and
 * d_cname_len both or neither.  pkt_stride a multiple of 4, IGDSP_RTCP_MAX_BUILT..2048.  d_packets 4-byte, d_sizes 2-byte, d_now, d_rec 8-byte, d_jb, d_src,
 * d_cname (rows of 64 bytes), d_state 16-byte aligned.  Of igdsp_rtcp_parse: d_packets, d_sizes, d_arrival,
 * d_local_ssrc, d_state required, d_rec optional (32-byte records, 16-byte aligned); pkt_stride a multiple of 4, 8..2048.  No output may
 * overlap an input or another output.  n_channels * n_frames < 2^32 - 32 (IGDSP_ERANGE).  Enqueued on `stream`.
 * Host only, no GPU: igdsp_srtcp_derive, igdsp_srtcp_protect_packet / igdsp_srtcp_unprotect_packet (in == out allowed),
 * igdsp_rtcp_build_packet (out_capacity >= IGDSP_RTCP_MAX_BUILT, else IGDSP_EINVAL) / igdsp_rtcp_parse_packet: one packet by the same rule. */
#define IGDSP_RTCP_MAX_BUILT  136
#define IGDSP_RTCP_CNAME_MAX  64
#define IGDSP_RTCP_NONE       0           /* d_ctl of igdsp_rtcp_build                                */
#define IGDSP_RTCP_REPORT     1
#define IGDSP_RTCP_BYE        2
#define IGDSP_RTCP_SR         0x01        /* igdsp_rtcp_built.flags                                   */
#define IGDSP_RTCP_RR         0x02
#define IGDSP_RTCP_HAS_BLOCK  0x04
#define IGDSP_RTCP_BYE_SENT   0x08
#define IGDSP_RTCP_HAVE_SR    0x01        /* igdsp_rtcp_state.flags                                   */
#define IGDSP_RTCP_PEER_VALID 0x02
#define IGDSP_RTCP_RTT_VALID  0x04
#define IGDSP_RTCP_BYE_SEEN   0x08
#define IGDSP_RTCP_PARSED       0x01      /* igdsp_rtcp_seen.flags: PARSED, MALFORMED, EMPTY exclude each other; the rest come with PARSED */
#define IGDSP_RTCP_MALFORMED    0x02
#define IGDSP_RTCP_EMPTY        0x04
#define IGDSP_RTCP_GOT_SR       0x08
#define IGDSP_RTCP_GOT_BLOCK    0x10
#define IGDSP_RTCP_GOT_RTT      0x20
#define IGDSP_RTCP_RTT_NEGATIVE 0x40
#define IGDSP_RTCP_GOT_BYE      0x80
typedef struct igdsp_rtcp_src {     /* the local sender as of a tick */
    uint32_t ssrc, rtp_ts, packets, octets;
} igdsp_rtcp_src;                   /* 16 bytes */
typedef struct igdsp_rtcp_state {   /* per leg, ALL-ZERO = reset */
    igdsp_jb_prior prior;           /* what igdsp_jb_report keeps between two reports: advances when a block is written */
    uint32_t sent_prior;            /* src.packets at the last packet built                      */
    uint32_t n_built;
    uint32_t lsr, lsr_arrival;      /* the last SR heard: its NTP time's middle 32 bits, and ours when it came */
    uint32_t flags;                 /* IGDSP_RTCP_HAVE_SR | PEER_VALID | RTT_VALID | BYE_SEEN     */
    uint32_t n_parsed, n_malformed;
    uint32_t rtt_last, rtt_count;   /* 1 / 65536 s                                               */
    uint32_t peer_fraction_lost;    /* what the far end reports about our stream                 */
    int32_t  peer_cum_lost;
    uint32_t peer_ext_seq, peer_jitter;
    uint32_t reserved[3];
} igdsp_rtcp_state;                 /* 80 bytes */
typedef struct igdsp_rtcp_built {
    uint16_t size;
    uint8_t  flags, reserved;
    uint32_t reserved2;
} igdsp_rtcp_built;                 /* 8 bytes */
typedef struct igdsp_rtcp_seen {
    uint8_t  flags, n_sub, peer_fraction_lost, reserved;
    uint32_t sender_ssrc;
    uint32_t rtt;                   /* as computed, with GOT_RTT or RTT_NEGATIVE; else 0         */
    int32_t  peer_cum_lost;
    uint32_t peer_ext_seq, peer_jitter;
    uint32_t sr_packets, sr_octets; /* with GOT_SR                                               */
} igdsp_rtcp_seen;                  /* 32 bytes */
#define IGDSP_SRTCP_TAG       0x53524300u /* igdsp_srtp_state.tag of an SRTCP state, | 10             */
#define IGDSP_SRTCP_TRAILER   14          /* the index word and the tag                               */
#define IGDSP_SRTCP_CLEAR     IGDSP_SRTP_ROLLED /* igdsp_srtp_rec.flags, with OK: E was 0, nothing decrypted */
int  igdsp_rtcp_build_packet(igdsp_rtcp_state *st, uint32_t ctl, const igdsp_jb_state *jb /* or NULL */, const igdsp_rtcp_src *src, uint64_t now,
                             const uint8_t *cname /* or NULL */, uint32_t cname_len, uint8_t *out, uint32_t out_capacity, uint32_t *size_out,
                             igdsp_rtcp_built *rec /* or NULL */);
int  igdsp_rtcp_parse_packet(igdsp_rtcp_state *st, const uint8_t *in, uint32_t size, uint32_t arrival, uint32_t local_ssrc, igdsp_rtcp_seen *rec /* or NULL */);
int  igdsp_srtcp_derive(const uint8_t key_salt[30], uint32_t index0, igdsp_srtp_state *out);
int  igdsp_srtcp_protect_packet(igdsp_srtp_state *st, uint32_t ctl, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity,
                                uint32_t *size_out, igdsp_srtp_rec *rec);
int  igdsp_srtcp_unprotect_packet(igdsp_srtp_state *st, uint32_t ctl, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity,
                                  uint32_t *size_out, igdsp_srtp_rec *rec);
int  igdsp_rtcp_build(igdsp_ctx *ctx, const uint8_t *d_ctl /* [F][C] */, const igdsp_jb_state *d_jb /* [C], read only, or NULL */,
                      const igdsp_rtcp_src *d_src /* [F][C] */, const uint64_t *d_now /* [F] */, const uint8_t *d_cname /* [C][64] or NULL */,
                      const uint8_t *d_cname_len /* [C] or NULL */, uint32_t n_channels, uint32_t n_frames, igdsp_rtcp_state *d_state /* [C], in and out */,
                      uint8_t *d_packets /* [F][C][pkt_stride] */, uint32_t pkt_stride, uint16_t *d_sizes /* [F][C] */, igdsp_rtcp_built *d_rec /* [F][C] or NULL */,
                      void *stream);
int  igdsp_rtcp_parse(igdsp_ctx *ctx, const uint8_t *d_packets /* [F][C][pkt_stride] */, const uint16_t *d_sizes /* [F][C] */,
                      const uint32_t *d_arrival /* [F][C] */, const uint32_t *d_local_ssrc /* [C] */, uint32_t n_channels, uint32_t n_frames,
                      uint32_t pkt_stride, igdsp_rtcp_state *d_state /* [C], in and out */, igdsp_rtcp_seen *d_rec /* [F][C] or NULL */, void *stream);
int  igdsp_srtcp_protect(igdsp_ctx *ctx, const uint8_t *d_ctl /* [F][C], NULL: RUN */, const uint8_t *d_packets /* [F][C][pkt_stride] */,
                         const uint16_t *d_sizes /* [F][C] */, uint32_t n_channels, uint32_t n_frames, uint32_t pkt_stride,
                         igdsp_srtp_state *d_state /* [C], in and out */, uint8_t *d_out /* [F][C][out_stride] */, uint32_t out_stride,
                         uint16_t *d_sizes_out /* [F][C] */, igdsp_srtp_rec *d_rec /* [F][C] */, void *stream);
int  igdsp_srtcp_unprotect(igdsp_ctx *ctx, const uint8_t *d_ctl /* [F][C], NULL: RUN */, const uint8_t *d_packets /* [F][C][pkt_stride] */,
                           const uint16_t *d_sizes /* [F][C] */, uint32_t n_channels, uint32_t n_frames, uint32_t pkt_stride,
                           igdsp_srtp_state *d_state /* [C], in and out */, uint8_t *d_out /* [F][C][out_stride] */, uint32_t out_stride,
                           uint16_t *d_sizes_out /* [F][C] */, igdsp_srtp_rec *d_rec /* [F][C] */, void *stream);

/* ---- SRTP with AES-GCM: RFC 7714 protection of the RTP packets, per leg and direction ---------------------------------------------------------
 * The suites a peer with AEAD support offers ahead of the SHA-1 ones: AEAD_AES_128_GCM (16-byte key, 12-byte salt) and AEAD_AES_256_GCM
 * (32-byte key, 12-byte salt), both with the 16-byte tag.  igdsp_srtp_gcm_protect / igdsp_srtp_gcm_unprotect stand where
 * igdsp_srtp_protect / igdsp_srtp_unprotect stand.  Everything not named here is the section "SRTP"'s, word for word: HEADER LENGTH and
 * its MALFORMED cases, the INDEX estimate, the 64-packet window, OLD / REPLAY, the CONTROL values RUN / BYPASS / RESET, EMPTY, the
 * counters, the RECORD igdsp_srtp_rec and its flags, in place, "a refused packet gets size 0 and its slot is never written", and the
 * ARGUMENTS clauses (strides, alignment, range, overlap).  The rule is pinned bit for bit by FIPS-197 and the GCM specification
 * (tests/golden/srtp_gcm_kat.json holds their known answers and whole packets recorded from OpenSSL); the host entries and the device
 * entries run the same code (csrc/igdsp_srtp_gcm.h; independent restatement: tests/srtp_gcm_model.py).
 * SCOPE: RTP only.  NOT built: SRTCP under GCM (RFC 7714 9, 10: a GCM call's RTCP stays on the host), AES_256_CM_HMAC_SHA1_* (RFC 6188),
 * 8-byte GCM tags, MKI, a key derivation rate, SDES / DTLS key exchange.
 *
 * SESSION KEYS.  RFC 3711 4.3.1's AES-CM key derivation with AES of the suite's own key size: label 0 gives the 16 / 32 bytes of k_e,
 * label 2 the 12 bytes of k_s; there is no k_a.  The 12-byte master salt is used as a 112-bit salt by appending 16 zero bits (RFC 7714
 * 11).  This clause is UNVERIFIED against RFC 7714's vectors (section 16), which were not at hand; the AES-CM keystream under it is
 * held against OpenSSL's EVP_aes_128_ctr / EVP_aes_256_ctr.  H = AES_k_e(0^128) is computed at derive time.
 * IV, 12 bytes: k_s xor (00 00 || SSRC || v || SEQ), big-endian, the packet's own SSRC, v the estimated rollover counter.
 * COUNTER BLOCKS.  J0 = IV || 00 00 00 01; payload block j (from 0) is XORed with AES_k_e(IV || be32(j + 2)), from byte h on.  An empty
 * payload is legal.
 * TAG, 16 bytes, appended: GHASH_H(A, C) xor AES_k_e(J0).  A is the header bytes [0, h), an ED-137 extension included, zero-padded to 16;
 * C the encrypted payload [h, end), zero-padded; the last block the two 64-bit bit lengths.  GHASH in GCM's convention: a block is a
 * 128-bit big-endian number, bit 0 the most significant, reduction by 0xE1 || 0^120.
 * PROTECT.  size_out = size + 16, MALFORMED when that passes the output slot or capacity.  No replay test.
 * UNPROTECT.  MALFORMED when size < h + 16.  The tag is computed over the ciphertext and all 16 bytes are compared before anything is
 * decrypted or stored; a mismatch is AUTH_FAIL (a flipped header bit too: the header is the AAD).  size_out = size - 16.
 * FAIL CLOSED, both ways.  The GCM entries accept a state only when its first word is IGDSP_SRTP_GCM_TAG | 16 or | 32; an
 * igdsp_srtp_state, an SRTCP state or random bytes give NO_KEY.  A GCM state handed to the SRTP / SRTCP entries is NO_KEY by their rule.
 * STATE, 320 bytes, 16-byte aligned, from igdsp_srtp_gcm_derive: the first ten words are igdsp_srtp_state's (tag, roc, s_l / have_s_l,
 * reserved, window, four counters), then the key schedule of k_e (AES-128 uses 44 of the 60 words), k_s and H.  Legs of both key sizes
 * may stand side by side in one launch.
 * Host only, no GPU: igdsp_srtp_gcm_derive (key_salt: key_bytes + 12 bytes; key_bytes 16 or 32, anything else IGDSP_EINVAL);
 * igdsp_srtp_gcm_protect_packet / igdsp_srtp_gcm_unprotect_packet: one packet by the same rule, in == out allowed. */
#define IGDSP_SRTP_GCM_TAG    0x53524700u /* igdsp_srtp_gcm_state.tag, | key_bytes (16 or 32)         */
#define IGDSP_SRTP_GCM_TAG_LEN 16
typedef struct igdsp_srtp_gcm_state {
    uint32_t tag;                   /* IGDSP_SRTP_GCM_TAG | key_bytes                            */
    uint32_t roc;
    uint16_t s_l, have_s_l;
    uint32_t reserved;
    uint64_t window;                /* bit i: index top - i was accepted (unprotect)             */
    uint32_t n_ok, n_auth_fail, n_replay, n_malformed;
    uint32_t rk[60];                /* AES encryption key schedule of k_e: 44 words (128), 60 (256) */
    uint8_t  salt[12];              /* k_s                                                       */
    uint32_t pad;
    uint8_t  h[16];                 /* H = AES_k_e(0^128)                                        */
    uint32_t reserved2[2];
} igdsp_srtp_gcm_state;             /* 320 bytes */
int  igdsp_srtp_gcm_derive(const uint8_t *key_salt /* [key_bytes + 12] */, uint32_t key_bytes /* 16 | 32 */, uint32_t roc0, igdsp_srtp_gcm_state *out);
int  igdsp_srtp_gcm_protect_packet(igdsp_srtp_gcm_state *st, uint32_t ctl, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity,
                                   uint32_t *size_out, igdsp_srtp_rec *rec);
int  igdsp_srtp_gcm_unprotect_packet(igdsp_srtp_gcm_state *st, uint32_t ctl, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity,
                                     uint32_t *size_out, igdsp_srtp_rec *rec);
int  igdsp_srtp_gcm_protect(igdsp_ctx *ctx, const uint8_t *d_ctl /* [F][C], NULL: RUN */, const uint8_t *d_packets /* [F][C][pkt_stride] */,
                            const uint16_t *d_sizes /* [F][C] */, uint32_t n_channels, uint32_t n_frames, uint32_t pkt_stride,
                            igdsp_srtp_gcm_state *d_state /* [C], in and out */, uint8_t *d_out /* [F][C][out_stride] */, uint32_t out_stride,
                            uint16_t *d_sizes_out /* [F][C] */, igdsp_srtp_rec *d_rec /* [F][C] */, void *stream);
int  igdsp_srtp_gcm_unprotect(igdsp_ctx *ctx, const uint8_t *d_ctl /* [F][C], NULL: RUN */, const uint8_t *d_packets /* [F][C][pkt_stride] */,
                              const uint16_t *d_sizes /* [F][C] */, uint32_t n_channels, uint32_t n_frames, uint32_t pkt_stride,
                              igdsp_srtp_gcm_state *d_state /* [C], in and out */, uint8_t *d_out /* [F][C][out_stride] */, uint32_t out_stride,
                              uint16_t *d_sizes_out /* [F][C] */, igdsp_srtp_rec *d_rec /* [F][C] */, void *stream);

/* ---- synthetic input generators (device side; SURVEY 8(d) definitions) ---------
 * D-uniform: byte k of global byte index g is
 *   (splitmix64(seed + (g>>3)) >> (8*(g&7))) & 0xFF,  g = first_byte + k
 * so any shard of the [F][C][n] array is reproducible on any GPU count. */
int igdsp_gen_uniform(igdsp_ctx *ctx, uint8_t *d_out, uint64_t n_bytes,
                      uint64_t seed, uint64_t first_byte, void *stream);

/* ---- small device-memory helpers for hosts that do not carry a HIP runtime
 * of their own (the Qt/C++ softphone).  Thin wrappers; all synchronous except
 * where a stream is given. */
int igdsp_dev_alloc(igdsp_ctx *ctx, void **d_ptr, size_t bytes);
int igdsp_dev_free(igdsp_ctx *ctx, void *d_ptr);
/* (Round-1 helper, superseded by igdsp_io_alloc below which places a whole buffer set and also finds the third class.)
 * Allocate an OUTPUT buffer in another class of device memory than the input it will be written from (see
 * igdsp_probe_placement): tries up to max_tries positions, each a further spacer_bytes (0 = 12 GiB) of temporary
 * allocation away, times the bare read(d_in) + write(candidate) stream for each, keeps the fastest candidate, frees the
 * rest and the spacers.  Stops early once a candidate is >= 8 % faster than the first.  ms_first / ms_kept (optional)
 * return the probe times of the plain first allocation and of the one kept.  Synchronous; start-up use only. */
int igdsp_dev_alloc_far(igdsp_ctx *ctx, void **d_ptr, size_t bytes, const void *d_in, size_t in_bytes,
                        uint32_t max_tries, size_t spacer_bytes, float *ms_first, float *ms_kept);
/* ---- placement-aware allocation of a whole input / output buffer set ---------------------------------------------------
 * On MI355X a launch that reads one class of device memory and writes another is ~13 % faster than one that reads and
 * writes the same class, and a bulk write stream spread over the two classes the inputs are NOT in gains another 5-8 %
 * (igdsp_probe_placement below).  Which class an allocation lands in cannot be queried and differs per
 * process; consecutive plain allocations normally share one.  igdsp_io_alloc therefore takes the whole buffer set of a
 * pipeline stage at once, classifies 128 MiB chunks of physical device memory by timing the bare read + record-store
 * stream against the INPUT buffers, and maps chunks of the right class behind each buffer's (contiguous) address range:
 *   IGDSP_IO_INPUT   buffers the kernels read (payload ring, packet ring, PCM to encode): consecutive chunks, class "A";
 *   IGDSP_IO_RECORD  small written outputs (igdsp_frame_stats, igdsp_rtp_info, len, hold): a class other than A;
 *   IGDSP_IO_BULK    large written outputs (PCM, re-encoded / dense payload): first half in one non-A class, second half
 *                    in the other (the kernels visit the two halves of a bulk output alternately).
 * Start-up use: synchronous, the first call takes 0.2-10 s (the search, then report->settle_ms of waiting until the driver has finished
 * clearing the memory the search gave back: launches run 1-5 % slow while it does); temporarily holds up to
 * explore_limit_bytes (0 = 50 % of the free device memory, 85 % when BULK buffers want a third class) of chunks while it searches and releases everything it does not
 * hand out — except up to 16 spare chunks (2 GiB) per memory class, which stay with the context (as do the chunks of a set given back with igdsp_io_free): a later
 * call that the spares cover is placed in < 100 ms without probing or waiting; igdsp_destroy gives them back (IGDSP_IO_SPARE_CHUNKS=0: keep none).  The pointers stay valid until igdsp_io_free.  If the virtual-memory API is missing, the largest input is < 512 MiB (the probe then measures the
 * Infinity Cache, and placement does not matter) or no second class is found, the buffers are still allocated and
 * report->placed is 0.  Buffer sizes are rounded up to whole chunks internally. */
#define IGDSP_IO_INPUT   0u
#define IGDSP_IO_RECORD  1u
#define IGDSP_IO_BULK    2u
typedef struct igdsp_io_buf {
    size_t   bytes;      /* in  */
    uint32_t role;       /* in: IGDSP_IO_* */
    uint32_t reserved;
    void    *ptr;        /* out: device pointer (chunk aligned) */
} igdsp_io_buf;
typedef struct igdsp_io_report {
    uint32_t placed;           /* 1: every RECORD / BULK buffer sits in another class than the inputs                  */
    uint32_t bulk_spread;      /* 1: BULK buffers have their halves in two different non-input classes                 */
    uint32_t classes_found;    /* 0 (no probing done), 1, 2 or 3                                                       */
    uint32_t chunks_explored;  /* chunks created while searching (most are released again)                            */
    uint32_t probes;           /* timed probe rounds                                                                   */
    uint32_t reseeds;          /* times the probe source was re-seeded because it straddled a class boundary          */
    uint64_t chunk_bytes;
    uint64_t explored_bytes;
    float    probe_ms_same;    /* bare probe stream (1.25 GiB read + 1/10 written) writing into the class it reads     */
    float    probe_ms_other;   /* ... writing into another class                                                       */
    float    setup_ms;         /* host wall time of the call                                                           */
    float    settle_ms;        /* of setup_ms: waiting for the memory system to go quiet after the search released its chunks */
} igdsp_io_report;
typedef struct igdsp_io_set igdsp_io_set;
int igdsp_io_alloc(igdsp_ctx *ctx, igdsp_io_buf *bufs, uint32_t n_bufs, size_t explore_limit_bytes,
                   igdsp_io_set **set, igdsp_io_report *report);
int igdsp_io_free(igdsp_ctx *ctx, igdsp_io_set *set);

int igdsp_copy_h2d(igdsp_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int igdsp_copy_d2h(igdsp_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int igdsp_dev_memset(igdsp_ctx *ctx, void *d_ptr, int value, size_t bytes);
int igdsp_sync(igdsp_ctx *ctx, void *stream);

/* ---- measurement helpers (HIP events on the launch stream; bench.py uses these
 * so timing does not depend on which stream torch considers current) ------------ */
int igdsp_timer_create(igdsp_ctx *ctx, void **timer);
int igdsp_timer_destroy(igdsp_ctx *ctx, void *timer);
int igdsp_timer_start(igdsp_ctx *ctx, void *timer, void *stream);
int igdsp_timer_stop(igdsp_ctx *ctx, void *timer, void *stream);
int igdsp_timer_elapsed_ms(igdsp_ctx *ctx, void *timer, float *ms); /* syncs on stop */

/* Read-only streaming-read calibration kernel (16 B/lane loads, xor-folded into
 * one word per workgroup): the "measured read-stream" the roofline is quoted
 * against besides the 8 TB/s nominal. */
int igdsp_stream_read(igdsp_ctx *ctx, const void *d_src, size_t bytes, uint64_t *d_sink, void *stream);

/* Placement probe.  On MI355X a stream that READS one large region of device memory and WRITES another runs ~13 %
 * faster than one that reads and writes the same region (regions are tens of GiB; inside one 80 GiB allocation the
 * bare read + record stream takes 0.218 ms across a region boundary and 0.252 ms within a region; the pure read rate
 * is the same everywhere; tools/placement_map.py grid).  This call times the bare read + record-store stream
 * (the meter kernel's traffic, no compute) reading d_in and writing d_out (bytes / 10 are written; NULL = a scratch
 * buffer allocated for the call), so a host can place its output buffers (records, PCM, re-encoded payload) a few
 * candidate distances away from its payload ring at start-up and keep the fastest.  Synchronous: 3 + reps launches
 * on `stream`, then waits. */
int igdsp_probe_placement(igdsp_ctx *ctx, const void *d_in, size_t bytes, void *d_out, uint32_t reps,
                          float *ms_per_launch, void *stream);

/* Kernel variant selection for experiments (0 = default tuned path).
 *   1 = one wavefront per channel-frame (40 lanes x dword), the literal north_star mapping
 *   2 = chunk64: one wavefront per 64 consecutive frames, 16 B/lane loads, 16 waves/CU (default for n == 160)
 *   3 = chunk64 with four super-chunks of lookahead per wave, 8 waves/CU (meter-only; experiment)
 *   4 = igdsp_roundtrip_peakhold through the compressor cell table (k_roundtrip_chunk64, the round-1 form) instead of
 *       the compressor folded into the expansion LUT; decode_meter as variant 0 */
int igdsp_set_variant(igdsp_ctx *ctx, int variant);

#ifdef __cplusplus
}
#endif
#endif /* IGDSP_H */
