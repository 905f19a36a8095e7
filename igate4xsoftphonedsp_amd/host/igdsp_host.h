// igdsp_host.h — C++11 host side above the C ABI: the reference's per-frame plugin interface,
// re-created so the softphone's RTP depayloader drops onto the MI355X path unchanged.
//
// Names, argument meaning and error behaviour mirror (own implementation, nothing copied):
//   struct tp_adapter                      TransportAdapter.h:40-93   (only the fields the hooks touch)
//   transport_rtp_cb(user_data,pkt,size)   TransportAdapter.cpp:240-316
//   transport_send_rtp(tp,pkt,size)        TransportAdapter.cpp:635-874 (level/probe part only)
//   RoIP_ED137::setIncomingRTP / setOutgoingRTP / setIncomingED137Value   roip_ed137.cpp:6500-6587
//   trx::IncomingRTP / OutgoingRTP slots   roip_ed137.h:741-750
//   updateInputLevel(int percent)          roip_ed137.cpp:584-592 ; AudioMeter::onValueChanged audiometer.h:14
// PJSIP types are replaced by plain ones (pj_status_t -> int, PJ_SUCCESS == 0, pj_ssize_t -> long).
// No Qt is needed to build this file; a Qt build can forward `onValueChanged(int)` to its own signal.
#ifndef IGDSP_HOST_H
#define IGDSP_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "igdsp.h"

#define SERVER 1      /* roip_ed137.h:107 — hooks only meter when inviteMode == SERVER */
#define CLIENT 2

// 20-byte ED-137 RTP header as the reference lays it out for little-endian targets
// (ed137_rtp.h:22-48 with PJ_IS_LITTLE_ENDIAN, iGate4xSoftphoneDSP.pro:88): 12 B RTP, 4 B
// extension header (profile 0x0167, length 1), 4 B ED-137 word (network order).
#pragma pack(push, 1)
struct custom_rtp_hdr {
    uint8_t  cc : 4, x : 1, p : 1, v : 2;
    uint8_t  pt : 7, m : 1;
    uint16_t seq;
    uint32_t ts;
    uint32_t ssrc;
    uint16_t profile_data;
    uint16_t length;
    uint32_t ed137;
};
#pragma pack(pop)
static_assert(sizeof(custom_rtp_hdr) == 20, "ED-137 RTP header is 20 bytes");
enum { IGDSP_RTP_HDR = 12 };                 /* sizeof(pjmedia_rtp_hdr), TransportAdapter.cpp:270 */

struct tp_adapter {
    void *stream_user_data;
    void (*stream_rtp_cb)(void *user_data, void *pkt, long size);   // pjmedia stream callback (G.711 decode happened behind it)
    int      radiostatus;                    // radio call => 20-byte header, else plain 12-byte RTP
    int16_t  rtpFalse;                       // consecutive TX silence-probe hits (TransportAdapter.cpp:661-672)
    int      callID;
    uint32_t ed137_value;
    uint32_t payloadsize;
    uint8_t  pkt_buff[256];
    size_t   bufSize;
    uint8_t  payload_buff[256];
    size_t   payload_bufSize;
    uint8_t  send_pkt_buff[256];
    uint8_t  tmp_payload_buf[256];
    size_t   send_bufSize;
    uint8_t  send_payload_buff[256];
    size_t   send_payload_bufSize;
    long long r2sPacket;                     // ms timestamp of the last packet (R2S watchdog input)
    int      rtpAudio;
    uint8_t  last_rx_pt, last_tx_pt;         // (ours) PT seen by the callback, handed to the shim
};

struct trx {                                 // roip_ed137.h:741-750 (level slots only)
    int     call_id;
    uint8_t OutgoingRTP, IncomingRTP;
    // decoded-domain meter of the same frames (new; filled from igdsp_poll)
    float    in_rms, out_rms;
    uint16_t in_peak, out_peak, in_peak_hold, out_peak_hold;
    int      in_percent, out_percent;        // AudioMeter scale: int(float(v*100.0/30000.0))
    uint8_t  in_flags, out_flags;
};

// PTT-window level logger state, field for field after trx (roip_ed137.h:719-745)
struct ptt_window {
    bool     eventPttSQL_In_LoggingOn;
    int      level_in_count;
    double   level_in, level_in_av, level_in_max, level_in_min;
    uint16_t OutgoingRTPSum;                 // uint16_t in the reference too: wraps after >= 257 frames of 255
    uint8_t  OutgoingRTPav, OutgoingRTPmax, OutgoingRTPmin;
};

// Receive levels of the calls on the conference bridge (setSlotVolume roip_ed137.cpp:5190-5233, setvolumeSiteTone :6869-6878): the
// reference's one float SLOT_VOLUME, stepped by 0.1f in [MIN_SLOT_VOLUME, MAX_SLOT_VOLUME] (roip_ed137.h:246-247), applied to a call's
// conference slot as pjsua_conf_adjust_rx_level does — here a per-channel Q7 gain (igdsp_conf_level_q7) for igdsp_conf_mix.  Needs no
// device: a call's channel is its conference slot (mapCall), an unmapped call fails as pjsua_call_get_info does.
class ConfLevels {
public:
    static constexpr float MIN_SLOT_VOLUME = 0.0f, MAX_SLOT_VOLUME = 2.0f;
    explicit ConfLevels(uint32_t n_channels);
    ~ConfLevels();
    float SLOT_VOLUME;                       // 2.0f at start (roip_ed137.cpp:210)
    float sidetone;                          // 0.1f (roip_ed137.h:779), set by initSoftPhone
    int radio_call[4];                       // trx1->radio1, trx1->radio2, trx2->radio1, trx2->radio2 (-1 = none)
    int mapCall(int callId, uint32_t channel);   // the call's conference slot; channel >= n_channels unmaps
    // false where the reference's returns false: no such call, or a level pjsua_conf_adjust_rx_level rejects (nothing applied)
    bool setSlotVolume(int callId, bool increase, bool current);
    void setvolumeSiteTone(int callId);
    const uint16_t *gains() const { return gain_; }   // [n_channels] Q7, 256 (the start level 2.0) until set
    uint32_t channels() const { return n_; }
private:
    int channelOf(int callId) const;
    uint32_t n_;
    uint16_t *gain_;
    int *call_of_;                           // [n_channels] call id of each channel, -1 = none
};

// Best signal selection, the SERVER-mode block of RoIP_ED137::checkEvents (roip_ed137.cpp:5609-5669, 5985-6119) over the reference's
// four radios, restated literally and without a context: the per-radio squelch / BSS read and the vote on lastRx, rssi, audioSQLOn,
// sqlStatusCount and sqlStatusOn, in the fixed order trx1.radio1, trx1.radio2, trx2.radio1, trx2.radio2.  A host that keeps the vote
// on the CPU calls tick() where checkEvents runs it; igdsp_bss_select is the same vote on the device, one tick per frame.
class BssVoter {
public:
    struct Radio {
        bool callState;                      // the call is up (the per-radio block runs)
        int lastRx;                          // the squelch as checkEvents last read it
        int rssi;                            // BSS index, -1 while closed
        bool audioSQLOn;                     // the voted radio
    };
    BssVoter();
    Radio radio[4];                          // trx1->radio1, trx1->radio2, trx2->radio1, trx2->radio2
    int sqlStatusCount;
    bool sqlStatusOn;
    int voteTicks;                           // 5 in the reference (sqlStatusCount >= 5)
    unsigned votes;                          // votes taken (telemetry)
    // The reference keeps a dropped call's last lastRx (its per-radio block does not run); igdsp_bss_select counts the call as
    // closed.  false (default): as igdsp_bss_select; true: the reference's stale lastRx.
    bool staleLastRx;
    // One tick: words[i] = the radio's stored ED-137 word (get_ed137_value), call_up[i] = its callState, force_mute = forceMuteSqlOn /
    // group PTT under MUTEALL.  Returns the voted radio (0..3), or -1.
    int tick(const uint32_t words[4], const bool call_up[4], bool force_mute);
    int voted() const;
};

// PTT priority arbitration, the CLIENT-mode block of RoIP_ED137::checkEvents (roip_ed137.cpp:6124-6231) over the call-in legs of one
// frequency (trx_incall order), restated literally and without a context: per leg lastTx, lastTxmsec, m_PttPressed and a slot volume
// (unmuted or not), one ptt_level.  A host that keeps the arbitration on the CPU calls tick() where checkEvents runs it;
// igdsp_ptt_arbitrate is the same loop on the device, one tick per frame, with one holder in place of the volumes.
class PttArbiter {
public:
    enum { kMaxLegs = 64 };
    struct Leg {
        bool callState;                      // the call is up (the per-leg block runs)
        bool rxOnly;                         // TRXMODE_RX: never keys
        int lastTx;                          // the (substituted) PTT type of the last tick
        int lastTxmsec;                      // ticks of the release being debounced, saturating at 255
        bool m_PttPressed;
        bool unmuted;                        // the slot volume: UNMUTE (true) or MUTE
    };
    explicit PttArbiter(int n_legs);
    Leg leg[kMaxLegs];
    int nLegs;
    int ptt_level;
    int releaseTicks;                        // ticks a release is bridged for (IGDSP_PTT_RELEASE_FRAMES at one tick per frame)
    unsigned takeovers;                      // takeovers so far (telemetry)
    int lastFlags;                           // IGDSP_PTT_* of the last tick
    // One tick: words[i] = the leg's stored ED-137 word (get_ed137_value), call_up[i] = its callState.  Returns the unmuted leg, or -1.
    int tick(const uint32_t *words, const bool *call_up);
    int unmutedLeg() const;
};

// R2S link supervision, the timer body of RoIP_ED137::detectR2SPacketAndReconn (roip_ed137.cpp:1764-1780, :2009-2040) and the tail of
// transport_rtp_cb that feeds it (TransportAdapter.cpp:286-315), restated literally and without a context over tp_adapter-shaped legs:
// r2sPacket, rtpAudio, r2sCount, r2sPeriod and callState.  A host that keeps the supervision on the CPU calls beginTick() where the
// timer fires, packet() where transport_rtp_cb runs and endTick() where the timer checks; igdsp_link_watch is the same steps on the
// device, one tick per frame, every packet stamped with its tick's time.
class LinkWatch {
public:
    struct Leg {
        bool callState;                      // the call is up (the per-leg block runs)
        unsigned long long r2sPacket;        // ms of the last packet of any kind
        bool rtpAudio;
        int r2sCount;                        // saturating at 65535
        int r2sPeriod;                       // ms, 200 in the reference
        bool alarmed;                        // the hang-up condition fired in this outage
        unsigned alarms;                     // times it fired (telemetry)
        int kind;                            // IGDSP_LINK_* of the tick so far
        uint32_t word;                       // ed137 of the tick's last edge packet, else 0
    };
    explicit LinkWatch(int n_legs);
    ~LinkWatch();
    int nLegs;
    int missTicks;                           // 6 in the reference (r2sCount == 5); IGDSP_LINK_MISS_TICKS at one tick per frame
    unsigned long long now;                  // the tick's time
    Leg *leg;
    // The tick begins: call_up[i] = the leg's callState (NULL: all up).  A leg that comes up is stamped and reset.
    void beginTick(unsigned long long now_ms, const bool *call_up);
    // One received packet (transport_rtp_cb): returns the edge it made, IGDSP_LINK_AUDIO_ON / _OFF or 0.
    int packet(int i, int pt, unsigned payload_len, bool runt, uint32_t ed137);
    // The timer's check: returns the number of legs whose hang-up condition fired; leg[i].kind holds every leg's kind byte.
    int endTick();
private:
    LinkWatch(const LinkWatch &);
    LinkWatch &operator=(const LinkWatch &);
};

// The sound-card splitter / combiner, pjmedia_splitcomb as initSlaveSoundCard drives it (roip_ed137.cpp:3314-3435), without a context:
// K mono rows of n samples <-> one card frame of n x K interleaved samples, and the per-channel VU of either side in plain loops.  A
// gateway of the reference's size (one card) keeps the step on the CPU with this; igdsp_snd_combine / igdsp_snd_split are the same
// steps on the device for thousands of cards.  It buffers nothing, one call is one frame; the card's other clock is DelayBuf's business.
class SplitComb {
public:
    SplitComb(int channels, int samples_per_frame);   // clamped to 1 .. IGDSP_SND_MAX_CHANNELS and 1 .. IGDSP_MAX_PAYLOAD
    int K, n;
    // playback: frame[s * K + k] = rows[k][s] (the splitcomb's get_frame over its reverse channels' put_frame)
    void combine(const int16_t *const *rows, int16_t *frame) const;
    // capture: rows[k][s] = frame[s * K + k] (the splitcomb's put_frame, the reverse channels' get_frame)
    void split(const int16_t *frame, int16_t *const *rows) const;
    // the record of card channel k of a frame, as igdsp_snd_combine / igdsp_snd_split write it
    igdsp_frame_stats vu(const int16_t *frame, int k) const;
};

// The ring tone, RoIP_ED137::init_ringTone / playRing / stopRing (Functions.cpp:523-571), without a context: the tonegen port's plan and
// state, and whether the port is connected to port 0 of the bridge.  The reference fills three descriptors (440 + 480 Hz, 2 s on, then
// 1 s / 4 s / 3 s off) and plays count = 1 with PJMEDIA_TONEGEN_LOOP: the cadence is 2 s on / 1 s off, and so it is here.  The bridge
// pulls a port only while something listens to it, so a ring that is not connected is held (IGDSP_TONE_CMD_HOLD) and stays where
// stopRing's rewind left it.  A gateway of the reference's size calls frame() once per tick; igdsp_tone_generate takes plan, cmd() and
// the state for thousands of consoles.
class RingTone {
public:
    explicit RingTone(uint32_t clock_rate = 8000, uint32_t samples_per_frame = IGDSP_SAMPLES_PER_FRAME);   // init_ringTone
    igdsp_tone_desc tone[3];                 // as the reference fills them; tone[1] and tone[2] are never played
    igdsp_tone_plan plan;                    // igdsp_tone_plan_build(tone, 1, clock_rate, IGDSP_TONE_LOOP)
    igdsp_tone_state state;                  // pjmedia_tonegen_play at init: PLAYING from position 0
    uint32_t n;
    bool ok;                                 // the plan was built (a clock rate igdsp_tone_plan_build takes)
    void playRing();                         // pjsua_conf_connect(in_ring_slot_, 0)
    void stopRing();                         // pjsua_conf_disconnect(in_ring_slot_, 0), pjmedia_tonegen_rewind
    bool connected() const { return connected_; }
    // the (tone row -> port 0) connection for igdsp_conf_build: writes channel[0] = tone_channel, port[0] = 0 and returns 1 while
    // connected, else returns 0
    uint32_t connections(uint32_t tone_channel, uint32_t *channel, uint32_t *port) const;
    uint32_t cmd();                          // the d_cmd byte of the next launch: REWIND once after stopRing, HOLD while not connected
    int frame(int16_t *out, uint16_t *len);  // one tick on the CPU: igdsp_tone_frame with cmd()
private:
    bool connected_, rewind_;
};

// A call port's rate conversion, as pjmedia's bridge does it when media_cfg.clock_rate (roip_ed137.cpp:3031) is not the streams' 8 kHz,
// without a context: one channel's two converters, towards the bridge (up) and back (down), each with its own history.  A gateway of
// the reference's size calls up() / down() once per tick and call; igdsp_resample takes the same states for thousands of calls.
class Resampler {
public:
    explicit Resampler(uint32_t bridge_rate = 16000, uint32_t samples_per_frame = IGDSP_SAMPLES_PER_FRAME);   // the narrow side: 8 kHz, n samples
    uint32_t factor, n;                      // bridge_rate / 8000
    bool ok;                                 // a factor igdsp_resample takes (2, 3, 4, 6) and n in 1 .. 256
    igdsp_rs_state to_bridge, from_bridge;
    int up(const int16_t *narrow, int16_t *wide);      // n samples -> n * factor (igdsp_rs_frame, IGDSP_RS_UP)
    int down(const int16_t *wide, int16_t *narrow);    // n * factor samples -> n (IGDSP_RS_DOWN)
};

// A reverse channel's delay buffer, as pjmedia_splitcomb_create_rev_channel puts one between the bridge's tick and the card's clock
// (initSlaveSoundCard, roip_ed137.cpp:3314-3435), without a context: one channel, one direction.  put() is the producer's frame, get() the
// consumer's: they are called as the two clocks deliver, in any order.  A gateway of the reference's size keeps one per card channel and
// direction; igdsp_dbuf_run takes the same states for thousands of card channels.
class DelayBuf {
public:
    explicit DelayBuf(uint32_t samples_per_frame = IGDSP_SAMPLES_PER_FRAME, uint32_t max_samples = 6 * IGDSP_SAMPLES_PER_FRAME);
    uint32_t n, max_samples;
    bool ok;                                 // n in 1 .. 256 and 2 n <= max_samples <= IGDSP_DBUF_CAP
    igdsp_dbuf_state state;
    int put(const int16_t *frame);           // n samples in (igdsp_dbuf_step, IGDSP_DBUF_PUT)
    int get(int16_t *frame);                 // n samples out; IGDSP_JB_PLAYED, or IGDSP_JB_LOST with a frame of zeros on underrun; negative: an error
    uint32_t fill() const { return state.len; }   // the delay, samples
};

// The spectrum graph the reference declares (roip_ed137.h:510-522: fftSize, d_realFftData, d_iirFftData, d_fftAvg, spectValueChanged,
// spectClear) and initialises (initSpectrumGraph, roip_ed137.cpp:6350-6365) without ever computing a transform, without a context: one
// channel through igdsp_spec_frame.  d_fftAvg keeps the reference's value 1.0 - 1.0e-2 * 75; the average's gain is 1 - d_fftAvg = 0.25
// unless the constructor is given another.  A gateway of the reference's size keeps one per displayed leg; igdsp_spectrum takes the same
// states for thousands of channels.
class SpectrumGraph {
public:
    explicit SpectrumGraph(uint32_t samples_per_frame = IGDSP_SAMPLES_PER_FRAME, uint32_t hop_frames = 1, float alpha = 0.25f);
    uint32_t n;
    igdsp_spec_cfg cfg;
    bool ok;                                 // n in 1 .. 256, hop_frames >= 1, alpha in (0, 1]
    int fftSize;                             // IGDSP_SPEC_N
    float d_fftAvg;                          // 1.0 - 1.0e-2 * 75, as the reference sets it
    float d_realFftData[IGDSP_SPEC_BINS];    // the last raw spectrum, dBFS
    float d_iirFftData[IGDSP_SPEC_BINS];     // the averaged spectrum, dBFS
    igdsp_spec_state state;
    igdsp_spec_rec last;                     // the record of the last frame that computed a spectrum
    void initSpectrumGraph();                // both arrays -70 dBFS, d_fftAvg, the state reset
    void spectClear();                       // the state reset: history silent, both arrays -70 dBFS
    int feed(const int16_t *frame);          // n samples in; 1 when the frame computed a spectrum (the reference's spectValueChanged), 0 when not; negative: an error
};

// In-band DTMF on one leg, without a context: one channel through igdsp_tdet_frame with the DTMF plan.  pjsua reports digits through
// on_dtmf_digit only when the far end sends telephone-event packets; this hears the digits inside the audio.  feed() returns the digit
// a frame's ON raised (its character), 0 when none; digits() is the string dialled so far in this call.  A gateway of the reference's
// size keeps one per SIP leg; igdsp_tone_detect takes the same states for thousands of channels.
class DtmfReceiver {
public:
    explicit DtmfReceiver(uint32_t samples_per_frame = IGDSP_SAMPLES_PER_FRAME, uint32_t clock_rate = IGDSP_CLOCK_RATE);
    uint32_t n;
    bool ok;                                 // n even in 2 .. 256 and a clock rate igdsp_tdet_plan_dtmf takes
    igdsp_tdet_plan plan;
    igdsp_tdet_state state;
    igdsp_tdet_rec last;                     // the record of the last frame fed
    int feed(const int16_t *frame);          // n samples in; the digit's character when the frame raised ON, 0 when not; negative: an error
    const char *digits() const { return dialled; }   // the digits of this call, oldest first (the last 63 of them)
    void newCall();                          // the state reset, the string emptied
private:
    char dialled[64];
    uint32_t count;
};

// The sound port's echo canceller on one leg, without a context: one channel through igdsp_ec_frame.  pjmedia creates one on the
// pjmedia_snd_port when media_cfg.ec_tail_len is not 0; the reference sets it to 0 and mutes a group's receivers during transmit
// instead.  cancel() takes the frame the card captured (near) and the frame that was played (far) and returns what is left; the
// record of the frame tells the echo return loss enhancement and whether the filter adapted.  A gateway of the reference's size keeps
// one per sound-card channel; igdsp_echo_cancel takes the same states for thousands of channels.
class EchoCanceller {
public:
    explicit EchoCanceller(uint32_t samples_per_frame = IGDSP_SAMPLES_PER_FRAME, uint32_t tail = 128);
    uint32_t n;
    bool ok;                                 // n even in 2 .. 256 and a tail of 128 or 256
    igdsp_ec_cfg cfg;                        // the defaults at this tail; a caller may change mu_shift, pmin, hang, dmin
    igdsp_ec_state state;
    igdsp_ec_rec last;                       // the record of the last frame
    int cancel(const int16_t *near_frame, const int16_t *far_frame, int16_t *out, uint32_t ctl = IGDSP_EC_RUN);   // far NULL: nothing was played
    float erleDb() const;                    // of the last frame: 10 log10(near_e / out_e), 0 when either is 0
    void reset();                            // the filter, the history and the hold forgotten
};

// The level control on one leg, without a context: one channel through igdsp_agc_frame.  Neither pjmedia nor the reference holds one (the
// only gain there is SLOT_VOLUME); process() brings a frame to the target level and keeps every sample under the ceiling, the record of
// the frame tells the gain and whether the limiter worked.  igdsp_agc_run takes the same states for thousands of channels.
class LevelControl {
public:
    explicit LevelControl(uint32_t samples_per_frame = IGDSP_SAMPLES_PER_FRAME);
    uint32_t n;
    bool ok;                                 // n a multiple of 8 in 8 .. 256
    igdsp_agc_cfg cfg;                       // the defaults; a caller may change any field (an invalid cfg: process() gives IGDSP_EINVAL)
    igdsp_agc_state state;
    igdsp_agc_rec last;                      // the record of the last frame
    int process(const int16_t *frame, int16_t *out, uint32_t ctl = IGDSP_AGC_RUN);
    float gainDb() const;                    // of the last frame: 20 log10(gain / 4096)
    void reset();                            // envelope, gain and cap forgotten
};

// The stream's silence detector on one leg, without a context: one channel through igdsp_vad_frame.  pjmedia's stream holds one and the
// reference switches it off (media_cfg.no_vad = 1); process() tells per frame whether to send it (IGDSP_VAD_VOICE), to send the
// comfort-noise payload instead (IGDSP_VAD_SID: sid, sidLen bytes, RTP payload type 13) or nothing (IGDSP_VAD_NONE), and the record
// carries the talkspurt's edges.  igdsp_vad_run takes the same states for thousands of channels.  UNVERIFIED against RFC 3389.
class VoiceDetector {
public:
    explicit VoiceDetector(uint32_t samples_per_frame = IGDSP_SAMPLES_PER_FRAME);
    uint32_t n;
    bool ok;                                 // n a multiple of 8 in 16 .. 256
    igdsp_vad_cfg cfg;                       // the defaults; a caller may change any field (an invalid cfg: process() gives IGDSP_EINVAL)
    igdsp_vad_state state;
    igdsp_vad_rec last;                      // the record of the last frame
    uint8_t sid[16];                         // the last frame's payload (zeros unless it was a SID frame)
    int process(const int16_t *frame, uint32_t ctl = IGDSP_VAD_RUN);   // the frame's kind, or IGDSP_EINVAL
    uint32_t sidLen() const { return last.sid_len; }
    bool onset() const { return (last.flags & IGDSP_VAD_F_ONSET) != 0; }      // the RTP marker bit belongs on this frame
    bool offset() const { return (last.flags & IGDSP_VAD_F_OFFSET) != 0; }
    bool voice() const { return (last.flags & IGDSP_VAD_F_VOICE) != 0; }
    void reset();                            // the floor, the hangover and the noise model forgotten
};

// Comfort noise on one leg, without a context: one channel through igdsp_cng_frame, the receive side of VoiceDetector's DTX.  A PT 13
// packet's payload goes in as a SID frame, the ticks without a packet as IGDSP_VAD_NONE, a decoded voice frame as IGDSP_VAD_VOICE;
// process() writes the row the bridge plays and returns its length (n, or 0 for a row that does not exist: no model yet, or a voice
// frame without a row).  igdsp_cng_run takes the same states for thousands of channels.  UNVERIFIED against RFC 3389.
class ComfortNoise {
public:
    explicit ComfortNoise(uint32_t samples_per_frame = IGDSP_SAMPLES_PER_FRAME, uint32_t seed = 0);
    uint32_t n;
    bool ok;                                 // n a multiple of 8 in 16 .. 256
    uint32_t seed;                           // the excitation's seed, for example the leg's SSRC; taken at construction and reset()
    igdsp_cng_state state;
    igdsp_cng_rec last;                      // the record of the last frame
    int process(uint32_t kind, const uint8_t *sid, uint32_t sid_len, const int16_t *voice, int16_t *out, uint32_t ctl = IGDSP_CNG_RUN);
    bool generated() const { return (last.flags & IGDSP_CNG_F_GENERATED) != 0; }
    bool hasModel() const { return state.have != 0; }
    void reset();                            // model, gain and the lattice's delays forgotten
};

// A filter on one leg, without a context: one channel through igdsp_filt_frame with one plan and one state: a high pass under a radio's
// sub-audible tone, a de- or pre-emphasis, a band limit, a notch.  setPlan() / setPreset() take a new plan and forget the histories (the
// state carries no plan identity).  igdsp_filt_run takes the same states for thousands of channels.  The rule is the library's own,
// UNVERIFIED against any other filter implementation.
class LegFilter {
public:
    explicit LegFilter(uint32_t samples_per_frame = IGDSP_SAMPLES_PER_FRAME);
    uint32_t n;
    bool ok;                                 // n a multiple of 8 in 8 .. 256
    bool planned;                            // a plan was taken: without one process() passes the row through (IGDSP_FILT_NO_PLAN)
    igdsp_filt_plan plan;
    igdsp_filt_state state;
    igdsp_filt_rec last;                     // the record of the last frame
    int setPlan(const igdsp_filt_plan *p);   // IGDSP_EINVAL (and the old plan stays) for a plan igdsp_filt_plan_check rejects
    int setPreset(uint32_t preset, uint32_t clock_rate);
    int process(const int16_t *pcm, int16_t *out, uint32_t ctl = IGDSP_FILT_RUN);
    bool clipped() const { return (last.flags & IGDSP_FILT_CLIPPED) != 0; }
    void reset();                            // the histories forgotten, the plan stays
};

// A noise suppressor on one leg, without a context: one channel through igdsp_ns_frame with one cfg and one state: a receiver's hiss
// lowered under and between transmissions.  The output is the input delayed by 80 samples (10 ms).  freeze(true) holds the noise
// estimate while a tone port or DTMF plays on the leg; bypass(true) passes the input through the same delay.  igdsp_ns_run takes the
// same states for thousands of channels.  The rule is the library's own, UNVERIFIED against speex, WebRTC and ITU-T G.160.
class LegDenoiser {
public:
    explicit LegDenoiser(uint32_t samples_per_frame = IGDSP_SAMPLES_PER_FRAME);
    uint32_t n;
    bool ok;                                 // n is 80, 160, 240 or 320
    igdsp_ns_cfg cfg;
    igdsp_ns_state state;
    igdsp_ns_rec last;                       // the record of the last frame
    uint32_t ctl;                            // IGDSP_NS_RUN, _FREEZE or _BYPASS: what process() passes
    int setConfig(const igdsp_ns_cfg *c);    // IGDSP_EINVAL (and the old cfg stays) for one out of range; the state stays
    void freeze(bool on) { ctl = on ? (uint32_t)IGDSP_NS_FREEZE : (uint32_t)IGDSP_NS_RUN; }
    void bypass(bool on) { ctl = on ? (uint32_t)IGDSP_NS_BYPASS : (uint32_t)IGDSP_NS_RUN; }
    int process(const int16_t *pcm, int16_t *out);
    bool suppressing() const { return (last.flags & IGDSP_NS_SUPPRESSING) != 0; }
    void reset();                            // the estimate, the gains and the overlap forgotten, the cfg stays
};

// SRTP on one leg and direction, without a context: one igdsp_srtp_state through igdsp_srtp_protect_packet / igdsp_srtp_unprotect_packet,
// what pjmedia's transport_srtp keeps per stream and direction.  A sender and a receiver are two objects from the same 30 bytes of
// pjmedia_srtp_crypto.key.  RFC 3711, AES_CM_128_HMAC_SHA1_80 or _32, RTP only; igdsp_srtp_protect / igdsp_srtp_unprotect take the same
// states for thousands of legs.
class LegSrtp {
public:
    LegSrtp(const uint8_t key_salt[30], uint32_t tag_len = 10, uint32_t roc0 = 0);
    bool ok;                                 // tag_len is 4 or 10 and a key was given
    igdsp_srtp_state state;
    igdsp_srtp_rec last;                     // the record of the last packet
    uint32_t ctl;                            // IGDSP_SRTP_RUN or _BYPASS: what protect() / unprotect() pass
    void bypass(bool on) { ctl = on ? (uint32_t)IGDSP_SRTP_BYPASS : (uint32_t)IGDSP_SRTP_RUN; }
    // the output's size, 0 for a packet that is refused (it did not arrive / is not sent), IGDSP_EINVAL for a NULL argument; in == out is allowed
    int protect(const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity);
    int unprotect(const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity);
    bool authFailed() const { return (last.flags & IGDSP_SRTP_AUTH_FAIL) != 0; }
    void reset();                            // roc, s_l and the replay window start over with the next packet; the keys stay
private:
    bool resetNext;
};

// LegSrtp for the AEAD suites: one igdsp_srtp_gcm_state through igdsp_srtp_gcm_protect_packet / igdsp_srtp_gcm_unprotect_packet.  RFC 7714,
// AEAD_AES_128_GCM (key_bytes 16) or AEAD_AES_256_GCM (32), 16-byte tags, RTP only; key_salt is the key_bytes + 12 bytes of
// pjmedia_srtp_crypto.key.  igdsp_srtp_gcm_protect / igdsp_srtp_gcm_unprotect take the same states for thousands of legs.
class LegSrtpGcm {
public:
    LegSrtpGcm(const uint8_t *key_salt, uint32_t key_bytes, uint32_t roc0 = 0);
    bool ok;                                 // key_bytes is 16 or 32 and a key was given
    igdsp_srtp_gcm_state state;
    igdsp_srtp_rec last;                     // the record of the last packet
    uint32_t ctl;                            // IGDSP_SRTP_RUN or _BYPASS: what protect() / unprotect() pass
    void bypass(bool on) { ctl = on ? (uint32_t)IGDSP_SRTP_BYPASS : (uint32_t)IGDSP_SRTP_RUN; }
    // the output's size, 0 for a packet that is refused (it did not arrive / is not sent), IGDSP_EINVAL for a NULL argument; in == out is allowed
    int protect(const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity);
    int unprotect(const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity);
    bool authFailed() const { return (last.flags & IGDSP_SRTP_AUTH_FAIL) != 0; }
    void reset();                            // roc, s_l and the replay window start over with the next packet; the keys stay
private:
    bool resetNext;
};

// RTCP on one leg, without a context: one igdsp_rtcp_state through igdsp_rtcp_build_packet / igdsp_rtcp_parse_packet and, when a key is
// given, two SRTCP states (ours to send, the peer's to receive) through igdsp_srtcp_protect_packet / igdsp_srtcp_unprotect_packet: what
// pjmedia's rtcp session and transport_srtp keep per stream for transport_send_rtcp and transport_rtcp_cb.  igdsp_rtcp_build /
// igdsp_rtcp_parse / igdsp_srtcp_protect / igdsp_srtcp_unprotect take the same states for thousands of legs.
class LegRtcp {
public:
    // key_salt: our 30 bytes of master key and salt, peer_key_salt the far end's; both NULL: RTCP in the clear
    LegRtcp(uint32_t ssrc, const char *cname, const uint8_t *key_salt = 0, const uint8_t *peer_key_salt = 0, uint32_t index0 = 0);
    bool secure;
    uint32_t ssrc;
    uint8_t cname[IGDSP_RTCP_CNAME_MAX];
    uint32_t cnameLen;
    igdsp_rtcp_state state;
    igdsp_srtp_state tx, rx;
    igdsp_rtcp_built lastBuilt;              // the records of the last report sent and the last packet received
    igdsp_rtcp_seen lastSeen;
    igdsp_srtp_rec lastSrtcp;
    // one report (SR when `packets` moved since the last one, else RR; with a BYE when bye) from the leg's jitter buffer state (or NULL)
    // into out (at least IGDSP_RTCP_MAX_BUILT, secure: + IGDSP_SRTCP_TRAILER bytes): its size, or IGDSP_EINVAL
    int report(const igdsp_jb_state *jb, uint32_t rtp_ts, uint32_t packets, uint32_t octets, uint64_t now_ntp, bool bye, uint8_t *out, uint32_t out_capacity);
    // one packet from the RTCP port, arrival its time's middle 32 NTP bits: 1 parsed, 0 refused (lastSrtcp / lastSeen say why), IGDSP_EINVAL
    int received(const uint8_t *in, uint32_t size, uint32_t arrival);
    bool rttValid() const { return (state.flags & IGDSP_RTCP_RTT_VALID) != 0; }
    uint32_t rtt() const { return state.rtt_last; }   // 1 / 65536 s
};

class RoIP_ED137 {
public:
    // Unlike the reference singleton (roip_ed137.cpp:192) the instance owns an igdsp context; device < 0
    // is rejected — there is no CPU metering path.
    static RoIP_ED137 *create(int device, uint32_t max_calls);
    static RoIP_ED137 *instance();           // the last created instance (the hooks' entry point)
    ~RoIP_ED137();

    int inviteMode;
    bool referenceTxQuirk;                   // true: TX level over the first n bytes of the WHOLE packet, as
                                             // setOutgoingRTP does (tmp_payload_buf = header+payload, roip_ed137.cpp:6505)
    trx *radio[4];                           // trx1->radio1, trx1->radio2, trx2->radio1, trx2->radio2

    void setIncomingRTP(tp_adapter *adapter);
    void setOutgoingRTP(tp_adapter *adapter);
    void setIncomingED137Value(uint32_t ed137_value, int acc_id);
    uint32_t ed137Events;                    // times checkEvents() would have been entered (roip_ed137.cpp:6537-6540)

    // Owner-thread tick (the reference polls on a 40 ms QTimer, roip_ed137.cpp:1756): flush staged frames to
    // the GPU, then fill trx slots exactly where the reference's if-chain would (roip_ed137.cpp:6519-6534, 6570-6585).
    int tick(uint32_t *frames_done);
    void (*onValueChanged)(int call_id, int is_tx, int percent);   // AudioMeter::onValueChanged stand-in
    igdsp_ctx *ctx() { return ctx_; }
    int bindRadio(int slot, int call_id);    // slot 0..3; maps RX to channel 2*slot, TX to 2*slot+1
    // conference receive levels of the four radios' RX channels 0, 2, 4, 6 (conf.radio_call and the call -> channel map follow
    // bindRadio); the bridge's gain array is conf.gains()
    ConfLevels conf;
    bool setSlotVolume(int callId, bool increase, bool current) { return conf.setSlotVolume(callId, increase, current); }
    void setvolumeSiteTone(int callId) { conf.setvolumeSiteTone(callId); }

    // SURVEY 8(f) rank 3 — PTT-window level logger (Functions.cpp:2126-2230), sampled per tick like the reference.
    // audioInLevel is the linear input level (the reference receives it over the WebSocket VU broadcast,
    // roip_ed137.cpp:7686-7716; here callers usually pass radio[slot]->in_rms).  createPTTEventDataLogger writes
    // the reference's "PTTEventDataLogger" JSON text into `json` and returns its length (0 = no message emitted).
    ptt_window window[4];
    int m_softPhoneID;
    void keeplogAudioLevel(int slot, double audioInLevel);
    int  createPTTEventDataLogger(int slot, const char *strEvent, const char *url, double audioInLevel, char *json, size_t cap);

private:
    RoIP_ED137();
    igdsp_ctx *ctx_;
};

extern "C" {
// pjmedia-facing callbacks with the reference's signatures
void transport_rtp_cb(void *user_data, void *pkt, long size);
int  transport_send_rtp(tp_adapter *tp, const void *pkt, size_t size);
int  decodeRtp(void *pkt, custom_rtp_hdr **hdr);

// flat C handles for tests / non-C++ hosts
void       *igdsp_host_create(int device, uint32_t max_calls);
void        igdsp_host_destroy(void *h);
tp_adapter *igdsp_host_adapter_new(int call_id, int radiostatus);
void        igdsp_host_adapter_free(tp_adapter *a);
int         igdsp_host_bind_radio(void *h, int slot, int call_id);
int         igdsp_host_set_mode(void *h, int invite_mode, int reference_tx_quirk);
int         igdsp_host_tick(void *h, uint32_t *frames_done);
int         igdsp_host_get_trx(void *h, int slot, trx *out);
uint32_t    igdsp_host_ed137_events(void *h);
igdsp_ctx  *igdsp_host_ctx(void *h);
int         igdsp_host_keeplog(void *h, int slot, double audioInLevel);
int         igdsp_host_ptt_event(void *h, int slot, const char *strEvent, const char *url, double audioInLevel, char *json, size_t cap);
int         igdsp_host_get_window(void *h, int slot, ptt_window *out);
// conference receive levels without a context (ConfLevels): the bool results as 1 / 0
void           *igdsp_host_levels_new(uint32_t n_channels);
void            igdsp_host_levels_free(void *l);
int             igdsp_host_levels_map_call(void *l, int call_id, uint32_t channel);
int             igdsp_host_levels_bind_radio(void *l, int slot, int call_id);
int             igdsp_host_levels_set(void *l, float slot_volume, float sidetone);   /* SLOT_VOLUME / sidetone as the reference assigns them */
float           igdsp_host_levels_slot_volume(void *l);
int             igdsp_host_set_slot_volume(void *l, int call_id, int increase, int current);
int             igdsp_host_set_volume_sidetone(void *l, int call_id);
const uint16_t *igdsp_host_levels_gains(void *l);   /* [n_channels] Q7 */
// best signal selection without a context (BssVoter): tick returns the voted radio, -1 for none (IGDSP_EINVAL for a NULL handle)
void *igdsp_host_bss_new(int vote_ticks, int stale_last_rx);
void  igdsp_host_bss_free(void *v);
int   igdsp_host_bss_tick(void *v, const uint32_t *words4, const int *call_up4, int force_mute);
int   igdsp_host_bss_state(void *v, int *count, int *on, unsigned *votes);
// PTT priority arbitration without a context (PttArbiter, 1 .. 64 legs): tick returns the unmuted leg, -1 for none (IGDSP_EINVAL for a
// NULL handle); rx_only may be NULL
void *igdsp_host_ptt_new(int n_legs, int release_ticks);
void  igdsp_host_ptt_free(void *v);
int   igdsp_host_ptt_tick(void *v, const uint32_t *words, const int *call_up, const int *rx_only);
int   igdsp_host_ptt_state(void *v, int *level, unsigned *takeovers, int *flags);
int   igdsp_host_ptt_leg(void *v, int leg, int *last_tx, int *release_cnt, int *pressed, int *unmuted);
// R2S link supervision without a context (LinkWatch, 1 .. 65 536 legs): begin / packet / end as the class; miss_ticks 0 = the default,
// call_up and the outputs of _end may be NULL; _end returns the number of MISSING legs (IGDSP_EINVAL for a NULL handle or a bad leg)
void *igdsp_host_link_new(int n_legs, int miss_ticks);
void  igdsp_host_link_free(void *v);
int   igdsp_host_link_set_period(void *v, int leg, int period_ms);
int   igdsp_host_link_begin(void *v, unsigned long long now_ms, const int *call_up);
int   igdsp_host_link_packet(void *v, int leg, int pt, unsigned payload_len, int runt, uint32_t ed137);
int   igdsp_host_link_end(void *v, uint8_t *kinds, uint32_t *words);
int   igdsp_host_link_leg(void *v, int leg, unsigned long long *last_ms, int *count, int *flags, unsigned *alarms);
// the sound-card splitter / combiner without a context (SplitComb, 1 .. 8 channels of 1 .. 256 samples): rows = K pointers to n samples;
// _vu writes the K records of a card frame (IGDSP_EINVAL for a NULL argument, NULL from _new for a bad shape)
void *igdsp_host_sc_new(int channels, int samples_per_frame);
void  igdsp_host_sc_free(void *v);
int   igdsp_host_sc_combine(void *v, const int16_t *const *rows, int16_t *frame);
int   igdsp_host_sc_split(void *v, const int16_t *frame, int16_t *const *rows);
int   igdsp_host_sc_vu(void *v, const int16_t *frame, igdsp_frame_stats *out);
// the ring tone without a context (RingTone): NULL from _new for a clock rate igdsp_tone_plan_build rejects or samples_per_frame outside
// 1 .. 256; _connections as RingTone::connections; _cmd as RingTone::cmd; _frame one tick (IGDSP_EINVAL for a NULL argument)
void *igdsp_host_ring_new(uint32_t clock_rate, uint32_t samples_per_frame);
void  igdsp_host_ring_free(void *v);
int   igdsp_host_ring_play(void *v);
int   igdsp_host_ring_stop(void *v);
int   igdsp_host_ring_connections(void *v, uint32_t tone_channel, uint32_t *channel, uint32_t *port);
int   igdsp_host_ring_cmd(void *v);
int   igdsp_host_ring_frame(void *v, int16_t *out, uint16_t *len);
int   igdsp_host_ring_get(void *v, igdsp_tone_plan *plan, igdsp_tone_state *state);
// a call port's rate converters without a context (Resampler): NULL from _new for a bridge rate other than 16 000, 24 000, 32 000,
// 48 000 or samples_per_frame outside 1 .. 256; _up / _down one tick (IGDSP_EINVAL for a NULL argument)
void *igdsp_host_rs_new(uint32_t bridge_rate, uint32_t samples_per_frame);
void  igdsp_host_rs_free(void *v);
int   igdsp_host_rs_up(void *v, const int16_t *narrow, int16_t *wide);
int   igdsp_host_rs_down(void *v, const int16_t *wide, int16_t *narrow);
// a reverse channel's delay buffer without a context (DelayBuf): NULL from _new for sizes igdsp_dbuf_step rejects; _put one frame in, _get
// one frame out (returns IGDSP_JB_PLAYED or IGDSP_JB_LOST; IGDSP_EINVAL for a NULL argument); _fill the delay in samples; _state a copy
void *igdsp_host_dbuf_new(uint32_t samples_per_frame, uint32_t max_samples);
void  igdsp_host_dbuf_free(void *v);
int   igdsp_host_dbuf_put(void *v, const int16_t *frame);
int   igdsp_host_dbuf_get(void *v, int16_t *frame);
int   igdsp_host_dbuf_fill(void *v);
int   igdsp_host_dbuf_state(void *v, igdsp_dbuf_state *out);
// in-band DTMF on one leg without a context (DtmfReceiver): NULL from _new for a frame length or clock rate igdsp_tdet_frame /
// igdsp_tdet_plan_dtmf reject; _feed one frame in (the digit's character when the frame raised ON, 0 when not, IGDSP_EINVAL for a NULL
// argument); _digits the string dialled in this call, owned by the handle; _new_call resets the state and empties the string
void *igdsp_host_dtmf_new(uint32_t samples_per_frame, uint32_t clock_rate);
void  igdsp_host_dtmf_free(void *v);
int   igdsp_host_dtmf_feed(void *v, const int16_t *frame);
const char *igdsp_host_dtmf_digits(void *v);
void  igdsp_host_dtmf_new_call(void *v);
// the echo canceller on one leg without a context (EchoCanceller): NULL from _new for a frame length or tail igdsp_ec_frame rejects;
// _cancel one frame (far NULL: nothing was played; IGDSP_EINVAL for a NULL handle, near or out); _rec a copy of the last frame's record;
// _erle_db of the last frame; _reset forgets the filter
void *igdsp_host_ec_new(uint32_t samples_per_frame, uint32_t tail);
void  igdsp_host_ec_free(void *v);
int   igdsp_host_ec_cancel(void *v, const int16_t *near_frame, const int16_t *far_frame, int16_t *out, uint32_t ctl);
int   igdsp_host_ec_rec(void *v, igdsp_ec_rec *out);
float igdsp_host_ec_erle_db(void *v);
void  igdsp_host_ec_reset(void *v);
// the level control on one leg without a context (LevelControl): NULL from _new for a frame length igdsp_agc_frame rejects; _process
// one frame (IGDSP_EINVAL for a NULL handle, frame or out); _rec a copy of the last frame's record; _gain_db of the last frame;
// _reset forgets envelope, gain and cap
void *igdsp_host_agc_new(uint32_t samples_per_frame);
void  igdsp_host_agc_free(void *v);
int   igdsp_host_agc_process(void *v, const int16_t *frame, int16_t *out, uint32_t ctl);
int   igdsp_host_agc_rec(void *v, igdsp_agc_rec *out);
float igdsp_host_agc_gain_db(void *v);
void  igdsp_host_agc_reset(void *v);
// the silence detector on one leg without a context (VoiceDetector): NULL from _new for a frame length igdsp_vad_frame rejects;
// _process one frame: its kind (IGDSP_EINVAL for a NULL handle or frame); _rec a copy of the last frame's record; _sid its payload's 16
// bytes, returns the length; _cfg replaces the cfg (IGDSP_EINVAL for NULL); _reset forgets the state
void *igdsp_host_vad_new(uint32_t samples_per_frame);
void  igdsp_host_vad_free(void *v);
int   igdsp_host_vad_process(void *v, const int16_t *frame, uint32_t ctl);
int   igdsp_host_vad_rec(void *v, igdsp_vad_rec *out);
int   igdsp_host_vad_sid(void *v, uint8_t out[16]);
int   igdsp_host_vad_cfg(void *v, const igdsp_vad_cfg *cfg);
void  igdsp_host_vad_reset(void *v);
// comfort noise on one leg without a context (ComfortNoise): NULL from _new for a frame length igdsp_cng_frame rejects; _process one
// frame: the row's length (IGDSP_EINVAL for a NULL handle or out, or a SID without its payload); _rec a copy of the last frame's
// record; _reset forgets the state
void *igdsp_host_cng_new(uint32_t samples_per_frame, uint32_t seed);
void  igdsp_host_cng_free(void *v);
int   igdsp_host_cng_process(void *v, uint32_t kind, const uint8_t *sid, uint32_t sid_len, const int16_t *voice, int16_t *out, uint32_t ctl);
int   igdsp_host_cng_rec(void *v, igdsp_cng_rec *out);
void  igdsp_host_cng_reset(void *v);
// a filter on one leg without a context (LegFilter): NULL from _new for a frame length igdsp_filt_frame rejects; _plan / _preset take a
// plan (IGDSP_EINVAL for one igdsp_filt_plan_check / igdsp_filt_plan_preset rejects) and forget the histories; _process one frame
// (IGDSP_EINVAL for a NULL argument); _rec a copy of the last frame's record; _reset forgets the histories
void *igdsp_host_filt_new(uint32_t samples_per_frame);
void  igdsp_host_filt_free(void *v);
int   igdsp_host_filt_plan(void *v, const igdsp_filt_plan *plan);
int   igdsp_host_filt_preset(void *v, uint32_t preset, uint32_t clock_rate);
int   igdsp_host_filt_process(void *v, const int16_t *pcm, int16_t *out, uint32_t ctl);
int   igdsp_host_filt_rec(void *v, igdsp_filt_rec *out);
void  igdsp_host_filt_reset(void *v);
// a noise suppressor on one leg without a context (LegDenoiser): NULL from _new for a frame length igdsp_ns_frame rejects; _config
// takes a cfg (IGDSP_EINVAL for one out of range); _control sets what _process passes as ctl (IGDSP_NS_RUN, _FREEZE, _BYPASS; anything
// else IGDSP_EINVAL); _process one frame (IGDSP_EINVAL for a NULL argument); _rec a copy of the last frame's record; _reset forgets
void *igdsp_host_ns_new(uint32_t samples_per_frame);
void  igdsp_host_ns_free(void *v);
int   igdsp_host_ns_config(void *v, const igdsp_ns_cfg *cfg);
int   igdsp_host_ns_control(void *v, uint32_t ctl);
int   igdsp_host_ns_process(void *v, const int16_t *pcm, int16_t *out);
int   igdsp_host_ns_rec(void *v, igdsp_ns_rec *out);
void  igdsp_host_ns_reset(void *v);
// SRTP on one leg and direction without a context (LegSrtp): NULL from _new for a NULL key or a tag_len that is not 4 or 10; _protect /
// _unprotect one packet: the output's size, 0 for a refused packet, IGDSP_EINVAL for a NULL argument; _control sets IGDSP_SRTP_RUN or
// _BYPASS (anything else IGDSP_EINVAL); _rec a copy of the last packet's record; _reset starts index and window over, the keys stay
// RTCP on one leg without a context (LegRtcp): key_salt and peer_key_salt both NULL for RTCP in the clear (NULL from _new for one
// alone); _report / _received as the class's; _state copies the igdsp_rtcp_state out
void *igdsp_host_rtcp_new(uint32_t ssrc, const char *cname, const uint8_t *key_salt, const uint8_t *peer_key_salt, uint32_t index0);
void  igdsp_host_rtcp_free(void *v);
int   igdsp_host_rtcp_report(void *v, const igdsp_jb_state *jb, uint32_t rtp_ts, uint32_t packets, uint32_t octets, uint64_t now_ntp, int bye, uint8_t *out,
                             uint32_t out_capacity);
int   igdsp_host_rtcp_received(void *v, const uint8_t *in, uint32_t size, uint32_t arrival);
int   igdsp_host_rtcp_state(void *v, igdsp_rtcp_state *out);
void *igdsp_host_srtp_new(const uint8_t *key_salt, uint32_t tag_len, uint32_t roc0);
void  igdsp_host_srtp_free(void *v);
int   igdsp_host_srtp_control(void *v, uint32_t ctl);
int   igdsp_host_srtp_protect(void *v, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity);
int   igdsp_host_srtp_unprotect(void *v, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity);
int   igdsp_host_srtp_rec(void *v, igdsp_srtp_rec *out);
void  igdsp_host_srtp_reset(void *v);
// SRTP with AES-GCM on one leg and direction (LegSrtpGcm): igdsp_host_srtp_*'s faces; NULL from _new for a NULL key or a key_bytes that is
// not 16 or 32
void *igdsp_host_srtp_gcm_new(const uint8_t *key_salt, uint32_t key_bytes, uint32_t roc0);
void  igdsp_host_srtp_gcm_free(void *v);
int   igdsp_host_srtp_gcm_control(void *v, uint32_t ctl);
int   igdsp_host_srtp_gcm_protect(void *v, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity);
int   igdsp_host_srtp_gcm_unprotect(void *v, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity);
int   igdsp_host_srtp_gcm_rec(void *v, igdsp_srtp_rec *out);
void  igdsp_host_srtp_gcm_reset(void *v);
// the spectrum graph without a context (SpectrumGraph): NULL from _new for sizes igdsp_spec_frame rejects; _feed one frame in (1: it
// computed a spectrum, 0: not, IGDSP_EINVAL for a NULL argument); _real / _iir the two arrays of 512 floats, owned by the handle; _clear
// is spectClear; _fft_avg is d_fftAvg
void *igdsp_host_spect_new(uint32_t samples_per_frame, uint32_t hop_frames, float alpha);
void  igdsp_host_spect_free(void *v);
int   igdsp_host_spect_feed(void *v, const int16_t *frame);
void  igdsp_host_spect_clear(void *v);
const float *igdsp_host_spect_real(void *v);
const float *igdsp_host_spect_iir(void *v);
float igdsp_host_spect_fft_avg(void *v);
// Meter output on the reference's other channel: AudioMeter (audiometer.cpp:11-34) reads ASCII decimal levels from the
// FIFO /tmp/capturefifo<card>, 32 bytes per read, and emits onValueChanged(int(float(v*100.0/30000.0))).  These write
// such records, so the reference's own meter consumer can be fed from igdsp_poll().rms.  open() waits up to
// `timeout_ms` for a reader (the reference creates the FIFO itself); returns an fd or a negative IGDSP_E*.
int igdsp_meter_fifo_open(const char *card, int timeout_ms);
int igdsp_meter_fifo_write(int fd, int level);
int igdsp_meter_fifo_close(int fd);
// WavWriter-compatible recorder (WavWriter.cpp:41-156): writeRTPWav signature, same bytes on disk
void *igdsp_wav_start(const char *path, int rate);
int   igdsp_wav_writeRTPWav(void *w, const char *pktbuf, const char *payloadbuf, unsigned pktlen, unsigned payloadlen);
int   igdsp_wav_stop(void *w);
}
#endif
