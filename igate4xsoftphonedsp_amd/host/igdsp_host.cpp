// igdsp_host.cpp — host mirror of the reference's per-frame adapter/hook interface over the C ABI.
// See igdsp_host.h for the reference lines each piece stands for.  Own implementation throughout.
#include "igdsp_host.h"

#include <arpa/inet.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

static RoIP_ED137 *theInstance_ = nullptr;

static long long now_ms()
{
    using namespace std::chrono;
    return duration_cast<milliseconds>(system_clock::now().time_since_epoch()).count();
}

// ---------------------------------------------------------------------------------------------
ConfLevels::ConfLevels(uint32_t n_channels) : SLOT_VOLUME(2.0f), sidetone(0.1f), n_(n_channels), gain_(nullptr), call_of_(nullptr)
{
    for (int i = 0; i < 4; ++i) radio_call[i] = -1;
    gain_ = new (std::nothrow) uint16_t[n_ ? n_ : 1];
    call_of_ = new (std::nothrow) int[n_ ? n_ : 1];
    if (!gain_ || !call_of_) n_ = 0;
    for (uint32_t c = 0; c < n_; ++c) { gain_[c] = (uint16_t)igdsp_conf_level_q7(2.0f); call_of_[c] = -1; }
}

ConfLevels::~ConfLevels()
{
    delete[] gain_;
    delete[] call_of_;
}

int ConfLevels::mapCall(int callId, uint32_t channel)
{
    for (uint32_t c = 0; c < n_; ++c) if (call_of_[c] == callId) call_of_[c] = -1;
    if (channel >= n_) return IGDSP_OK;
    call_of_[channel] = callId;
    return IGDSP_OK;
}

int ConfLevels::channelOf(int callId) const
{
    if (callId < 0) return -1;
    for (uint32_t c = 0; c < n_; ++c) if (call_of_[c] == callId) return (int)c;
    return -1;
}

// roip_ed137.cpp:5190-5233: the float steps and clamps as written, then the level to the call's slot
bool ConfLevels::setSlotVolume(int callId, bool increase, bool current)
{
    const int c = channelOf(callId);
    if (c < 0) return false;                                      // pjsua_call_get_info failed
    if (!current) {
        if (increase) {
            SLOT_VOLUME += 0.1f;
            if (SLOT_VOLUME >= MAX_SLOT_VOLUME) SLOT_VOLUME = MAX_SLOT_VOLUME;
        } else {
            SLOT_VOLUME -= 0.1f;
            if (SLOT_VOLUME <= MIN_SLOT_VOLUME) SLOT_VOLUME = MIN_SLOT_VOLUME;
        }
    }
    const int q = igdsp_conf_level_q7(SLOT_VOLUME);               // pjsua_conf_adjust_rx_level
    if (q < 0) return false;
    gain_[c] = (uint16_t)q;
    return true;
}

// roip_ed137.cpp:6869-6878
void ConfLevels::setvolumeSiteTone(int callId)
{
    bool bound = false;
    for (int i = 0; i < 4; ++i) bound = bound || (callId == radio_call[i]);
    SLOT_VOLUME = bound ? sidetone : 0.5f;
    setSlotVolume(callId, false, true);
}

// ---------------------------------------------------------------------------------------------
RoIP_ED137::RoIP_ED137() : inviteMode(SERVER), referenceTxQuirk(false), ed137Events(0), onValueChanged(nullptr), conf(8u), m_softPhoneID(1), ctx_(nullptr)
{
    std::memset(window, 0, sizeof window);
    for (int i = 0; i < 4; ++i) window[i].OutgoingRTPmin = 255;          // roip_ed137.h:745
    for (int i = 0; i < 4; ++i) {
        radio[i] = new trx();
        std::memset(radio[i], 0, sizeof(trx));
        radio[i]->call_id = -1;
    }
}

RoIP_ED137 *RoIP_ED137::create(int device, uint32_t max_calls)
{
    RoIP_ED137 *r = new (std::nothrow) RoIP_ED137();
    if (!r) return nullptr;
    // two metering channels per call: RX (IncomingRTP) and TX (OutgoingRTP)
    if (igdsp_create(&r->ctx_, device, max_calls * 2u) != IGDSP_OK) {
        delete r;
        return nullptr;
    }
    theInstance_ = r;
    return r;
}

RoIP_ED137 *RoIP_ED137::instance() { return theInstance_; }

RoIP_ED137::~RoIP_ED137()
{
    if (theInstance_ == this) theInstance_ = nullptr;
    igdsp_destroy(ctx_);
    for (int i = 0; i < 4; ++i) delete radio[i];
}

// call ids are mapped to metering channels through the C ABI's routing table; RX and TX of one
// call get distinct ids in that table: rx = call_id * 2, tx = call_id * 2 + 1.
static inline int32_t rx_key(int call_id) { return call_id * 2; }
static inline int32_t tx_key(int call_id) { return call_id * 2 + 1; }

int RoIP_ED137::bindRadio(int slot, int call_id)
{
    if (slot < 0 || slot > 3) return IGDSP_EINVAL;
    if (radio[slot]->call_id >= 0) {
        igdsp_unmap_call(ctx_, rx_key(radio[slot]->call_id));
        igdsp_unmap_call(ctx_, tx_key(radio[slot]->call_id));
    }
    radio[slot]->call_id = call_id;
    conf.radio_call[slot] = call_id;
    conf.mapCall(call_id, (uint32_t)(2 * slot));                  // its conference slot: the RX channel (call_id < 0: nothing)
    if (call_id < 0) return IGDSP_OK;
    int rc = igdsp_map_call(ctx_, rx_key(call_id), (uint32_t)(2 * slot));
    if (rc == IGDSP_OK) rc = igdsp_map_call(ctx_, tx_key(call_id), (uint32_t)(2 * slot + 1));
    return rc;
}

// setIncomingRTP reads callID, payload_buff and payload_bufSize from the adapter (roip_ed137.cpp:6549-6552)
// and only meters in SERVER mode (:6555).  The arithmetic itself now runs on the GPU at the next tick.
void RoIP_ED137::setIncomingRTP(tp_adapter *adapter)
{
    if (!adapter || inviteMode != SERVER) return;
    // the frame is staged under the adapter's current ED-137 word — what get_ed137_value(tp) would return at this moment
    // (ntohl(adapter->ed137_value), TransportAdapter.cpp:337-346): the flush gates the frame's fold into the call's window with it
    // when a gate mode is set (igdsp_set_gate_mode; PTT / SQU masks Functions.cpp:1136, 1160)
    (void)igdsp_set_ed137(ctx_, rx_key(adapter->callID), ntohl(adapter->ed137_value));
    (void)igdsp_on_rtp_frame(ctx_, rx_key(adapter->callID), adapter->last_rx_pt, adapter->payload_buff,
                             (uint32_t)adapter->payload_bufSize);
}

void RoIP_ED137::setOutgoingRTP(tp_adapter *adapter)
{
    if (!adapter || inviteMode != SERVER) return;
    const uint32_t n = (uint32_t)adapter->send_payload_bufSize;
    // reference: payloadbuf = tmp_payload_buf (the WHOLE packet) and the loop runs over its first n bytes
    // (roip_ed137.cpp:6505-6517).  Default here: meter the payload proper, 12 bytes in.
    const uint8_t *p = referenceTxQuirk ? adapter->tmp_payload_buf : adapter->tmp_payload_buf + IGDSP_RTP_HDR;
    (void)igdsp_on_rtp_frame(ctx_, tx_key(adapter->callID), adapter->last_tx_pt, p, n);
}

void RoIP_ED137::setIncomingED137Value(uint32_t, int) { ++ed137Events; }

int RoIP_ED137::tick(uint32_t *frames_done)
{
    int rc = igdsp_flush(ctx_, frames_done);
    if (rc != IGDSP_OK) return rc;
    for (int s = 0; s < 4; ++s) {
        trx *t = radio[s];
        if (t->call_id < 0) continue;
        igdsp_level lv;
        if (igdsp_poll(ctx_, (uint32_t)(2 * s), &lv) == IGDSP_OK && lv.frames) {
            t->IncomingRTP = lv.byte_mean; t->in_rms = lv.rms; t->in_peak = lv.peak; t->in_peak_hold = lv.peak_hold;
            t->in_percent = lv.percent; t->in_flags = lv.flags;
            if (onValueChanged) onValueChanged(t->call_id, 0, lv.percent);
        }
        if (igdsp_poll(ctx_, (uint32_t)(2 * s + 1), &lv) == IGDSP_OK && lv.frames) {
            t->OutgoingRTP = lv.byte_mean; t->out_rms = lv.rms; t->out_peak = lv.peak; t->out_peak_hold = lv.peak_hold;
            t->out_percent = lv.percent; t->out_flags = lv.flags;
            if (onValueChanged) onValueChanged(t->call_id, 1, lv.percent);
        }
    }
    return IGDSP_OK;
}

// ---------------------------------------------------------------------------------------------
// PTT-window logger.  keeplogAudioLevel: Functions.cpp:2126-2145.  createPTTEventDataLogger: reset on
// "pptTest_pressed" (:2155-2167), close + 10*log10 on "pptTest_released" (:2192-2222); message text :2169-2187, :2202-2215.
void RoIP_ED137::keeplogAudioLevel(int slot, double audioInLevel)
{
    if (slot < 0 || slot > 3) return;
    ptt_window &w = window[slot];
    if (!w.eventPttSQL_In_LoggingOn) return;
    const uint8_t out = radio[slot]->OutgoingRTP;
    w.level_in_count += 1;
    w.level_in = audioInLevel;
    w.level_in_av += audioInLevel;
    w.OutgoingRTPSum = (uint16_t)(w.OutgoingRTPSum + out);
    if (audioInLevel > w.level_in_max) w.level_in_max = audioInLevel;
    if (audioInLevel < w.level_in_min) w.level_in_min = audioInLevel;
    if (out > w.OutgoingRTPmax) w.OutgoingRTPmax = out;
    if (out < w.OutgoingRTPmin) w.OutgoingRTPmin = out;
}

static int ptt_json(char *json, size_t cap, int id, const char *ev, double a, double b, double c, const char *url, int x, int y, int z)
{
    // QString::arg(double) prints like %g (6 significant digits); uint8_t arguments promote to int.
    // The key "radioUrl " carries the reference's trailing blank.
    int n = std::snprintf(json, cap,
        "{\"menuID\"                       :\"PTTEventDataLogger\", \"softPhoneID\"                  :%d, "
        "\"Ptt\"                          :\"%s\", \"level_in_av\"                  :%g, "
        "\"level_in_max\"                 :%g, \"level_in_min\"                 :%g, "
        "\"radioUrl \"                    :\"%s\",\"OutgoingRTPAv\"                :%d, "
        "\"OutgoingRTPmax\"               :%d, \"OutgoingRTPmin\"               :%d }",
        id, ev, a, b, c, url ? url : "", x, y, z);
    return (n < 0 || (size_t)n >= cap) ? 0 : n;
}

int RoIP_ED137::createPTTEventDataLogger(int slot, const char *strEvent, const char *url, double audioInLevel, char *json, size_t cap)
{
    if (slot < 0 || slot > 3 || !strEvent || !json || cap == 0 || inviteMode != SERVER) return 0;
    ptt_window &w = window[slot];
    trx *r = radio[slot];
    json[0] = 0;
    if (std::strcmp(strEvent, "pptTest_pressed") == 0) {
        if (w.eventPttSQL_In_LoggingOn) return 0;
        w.eventPttSQL_In_LoggingOn = true;
        w.level_in_count = 0;
        w.level_in = 10 * std::log10(audioInLevel);
        w.level_in_av = 0; w.level_in_max = 0; w.level_in_min = 255;
        w.OutgoingRTPSum = 0; w.OutgoingRTPmax = 0; w.OutgoingRTPmin = 255;
        igdsp_reset_hold(ctx_, (uint32_t)(2 * slot));            // the per-frame device window opens with it
        igdsp_reset_hold(ctx_, (uint32_t)(2 * slot + 1));
        return ptt_json(json, cap, m_softPhoneID, strEvent, w.level_in, w.level_in, w.level_in, url, r->OutgoingRTP, r->OutgoingRTP, r->OutgoingRTP);
    }
    if (std::strcmp(strEvent, "pptTest_released") == 0) {
        if (!w.eventPttSQL_In_LoggingOn) return 0;
        w.eventPttSQL_In_LoggingOn = false;
        w.level_in_av = 10 * std::log10(w.level_in_av / w.level_in_count);
        w.level_in_max = 10 * std::log10(w.level_in_max);
        w.level_in_min = 10 * std::log10(w.level_in_min);
        w.OutgoingRTPav = w.level_in_count ? (uint8_t)(w.OutgoingRTPSum / w.level_in_count) : 0;   // the reference divides unguarded
        const int n = ptt_json(json, cap, m_softPhoneID, strEvent, w.level_in_av, w.level_in_max, w.level_in_min, url,
                               w.OutgoingRTPav, w.OutgoingRTPmax, w.OutgoingRTPmin);
        w.level_in_count = 0; w.level_in = 0; w.level_in_av = 0; w.level_in_max = 0; w.level_in_min = 255;
        return n;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
extern "C" {

int igdsp_host_keeplog(void *h, int slot, double audioInLevel)
{
    if (!h) return IGDSP_EINVAL;
    static_cast<RoIP_ED137 *>(h)->keeplogAudioLevel(slot, audioInLevel);
    return IGDSP_OK;
}

int igdsp_host_ptt_event(void *h, int slot, const char *strEvent, const char *url, double audioInLevel, char *json, size_t cap)
{
    return h ? static_cast<RoIP_ED137 *>(h)->createPTTEventDataLogger(slot, strEvent, url, audioInLevel, json, cap) : 0;
}

int igdsp_host_get_window(void *h, int slot, ptt_window *out)
{
    if (!h || !out || slot < 0 || slot > 3) return IGDSP_EINVAL;
    *out = static_cast<RoIP_ED137 *>(h)->window[slot];
    return IGDSP_OK;
}

int decodeRtp(void *pkt, custom_rtp_hdr **hdr)
{
    *hdr = reinterpret_cast<custom_rtp_hdr *>(pkt);     // a cast, like TransportAdapter.cpp:408-415
    return 0;
}

// RX: header parse, PT gate, payload copy, keep-alive bookkeeping, then the hooks.
void transport_rtp_cb(void *user_data, void *pkt, long size)
{
    tp_adapter *adapter = static_cast<tp_adapter *>(user_data);
    if (!adapter || !pkt || size < (long)IGDSP_RTP_HDR) return;
    custom_rtp_hdr *rtphdr = nullptr;
    decodeRtp(pkt, &rtphdr);
    const unsigned pt = rtphdr->pt;
    const long hdr = adapter->radiostatus ? (long)sizeof(custom_rtp_hdr) : (long)IGDSP_RTP_HDR;
    if (adapter->radiostatus && size >= (long)sizeof(custom_rtp_hdr) && (pt == 8 || pt == 0 || pt == 18 || pt == 123)) {
        adapter->ed137_value = rtphdr->ed137;                  // TransportAdapter.cpp:252-256
        adapter->payloadsize = rtphdr->length;
    }
    long payloadlen = size - hdr;
    // runt (shorter than its header): the reference's unsigned subtraction wraps, fails its `< 1024` guard and
    // returns (TransportAdapter.cpp:279-291); oversize: it guards with `< 1024` into a 256-byte buffer (:286) —
    // both are dropped here without touching the buffers
    if (payloadlen < 0 || payloadlen > (long)sizeof(adapter->payload_buff)) {
        adapter->r2sPacket = now_ms();
        return;
    }
    adapter->payload_bufSize = (size_t)payloadlen;
    std::memcpy(adapter->payload_buff, static_cast<const uint8_t *>(pkt) + hdr, (size_t)payloadlen);
    adapter->last_rx_pt = (uint8_t)pt;
    adapter->r2sPacket = now_ms();
    RoIP_ED137 *app = RoIP_ED137::instance();
    if (pt != 123) {
        if (adapter->stream_rtp_cb) adapter->stream_rtp_cb(adapter->stream_user_data, pkt, size);
        if (app) {
            app->setIncomingRTP(adapter);
            if (!adapter->rtpAudio) app->setIncomingED137Value(ntohl(adapter->ed137_value), adapter->callID);
        }
        adapter->rtpAudio = 1;
    } else {
        if (adapter->rtpAudio && app) app->setIncomingED137Value(ntohl(adapter->ed137_value), adapter->callID);
        adapter->rtpAudio = 0;
    }
}

// TX: the level / silence-probe part of transport_send_rtp (the ED-137 word assembly and the socket
// send stay with the softphone).  `pkt` is the pjmedia stream's 12-byte-header RTP packet.
int transport_send_rtp(tp_adapter *adapter, const void *pkt, size_t size)
{
    if (!adapter || !pkt || size < (size_t)IGDSP_RTP_HDR || size > sizeof(adapter->tmp_payload_buf)) return IGDSP_EINVAL;
    std::memcpy(adapter->tmp_payload_buf, pkt, size);          // whole packet, as TransportAdapter.cpp:654
    const uint8_t *b = adapter->tmp_payload_buf;
    if (size > 60) {                                           // TransportAdapter.cpp:657-673
        if (b[40] == b[50] && b[40] == b[60] && b[40] == 0xD5) { if (adapter->rtpFalse < 32767) adapter->rtpFalse++; }
        else adapter->rtpFalse = 0;
    }
    const unsigned pt = b[1] & 0x7F;
    adapter->last_tx_pt = (uint8_t)pt;
    if (pt != 123) {
        adapter->send_payload_bufSize = size - IGDSP_RTP_HDR;
        RoIP_ED137 *app = RoIP_ED137::instance();
        if (app) app->setOutgoingRTP(adapter);
    }
    return 0;
}

void *igdsp_host_create(int device, uint32_t max_calls) { return RoIP_ED137::create(device, max_calls); }
void igdsp_host_destroy(void *h) { delete static_cast<RoIP_ED137 *>(h); }

tp_adapter *igdsp_host_adapter_new(int call_id, int radiostatus)
{
    tp_adapter *a = new (std::nothrow) tp_adapter();
    if (!a) return nullptr;
    std::memset(a, 0, sizeof *a);
    a->callID = call_id;
    a->radiostatus = radiostatus;
    a->r2sPacket = now_ms();
    return a;
}

void igdsp_host_adapter_free(tp_adapter *a) { delete a; }
int igdsp_host_bind_radio(void *h, int slot, int call_id) { return h ? static_cast<RoIP_ED137 *>(h)->bindRadio(slot, call_id) : IGDSP_EINVAL; }

int igdsp_host_set_mode(void *h, int invite_mode, int reference_tx_quirk)
{
    if (!h) return IGDSP_EINVAL;
    static_cast<RoIP_ED137 *>(h)->inviteMode = invite_mode;
    static_cast<RoIP_ED137 *>(h)->referenceTxQuirk = reference_tx_quirk != 0;
    return IGDSP_OK;
}

int igdsp_host_tick(void *h, uint32_t *frames_done) { return h ? static_cast<RoIP_ED137 *>(h)->tick(frames_done) : IGDSP_EINVAL; }

int igdsp_host_get_trx(void *h, int slot, trx *out)
{
    if (!h || !out || slot < 0 || slot > 3) return IGDSP_EINVAL;
    *out = *static_cast<RoIP_ED137 *>(h)->radio[slot];
    return IGDSP_OK;
}

igdsp_ctx *igdsp_host_ctx(void *h) { return h ? static_cast<RoIP_ED137 *>(h)->ctx() : nullptr; }
uint32_t igdsp_host_ed137_events(void *h) { return h ? static_cast<RoIP_ED137 *>(h)->ed137Events : 0; }

// ---------------------------------------------------------------------------------------------
// FIFO producer for the reference's AudioMeter consumer (audiometer.cpp:11-34)
int igdsp_meter_fifo_open(const char *card, int timeout_ms)
{
    if (!card) return IGDSP_EINVAL;
    char path[256];
    if (std::snprintf(path, sizeof path, "/tmp/capturefifo%s", card) >= (int)sizeof path) return IGDSP_EINVAL;
    for (int waited = 0;; ++waited) {
        const int fd = ::open(path, O_WRONLY | O_NONBLOCK);          // fails with ENXIO until the reader has opened it
        if (fd >= 0) {
            ::fcntl(fd, F_SETFL, ::fcntl(fd, F_GETFL) & ~O_NONBLOCK);
            return fd;
        }
        if (waited >= timeout_ms) return IGDSP_ENOENT;
        ::usleep(1000);
    }
}

int igdsp_meter_fifo_write(int fd, int level)
{
    if (fd < 0) return IGDSP_EINVAL;
    char rec[32];                                                   // one record per read(in_fd, in, 32), NUL padded
    std::memset(rec, 0, sizeof rec);
    std::snprintf(rec, sizeof rec, "%d", level);
    return ::write(fd, rec, sizeof rec) == (ssize_t)sizeof rec ? IGDSP_OK : IGDSP_EDEVICE;
}

int igdsp_meter_fifo_close(int fd) { return (fd >= 0 && ::close(fd) == 0) ? IGDSP_OK : IGDSP_EINVAL; }

// ---------------------------------------------------------------------------------------------
// Recorder with the reference's writeRTPWav signature and byte-for-byte the same file:
// 44-byte header (tag 7, 2 "channels", 16 bit, sizes patched on stop) and every payload byte b
// written as the two bytes [b, 0x00] (WavWriter.cpp:63-156).  Buffered: one fwrite per frame
// instead of the reference's two per sample.
struct igdsp_wav { FILE *f; uint32_t data; };

static void le(uint8_t *p, uint32_t v, int n) { for (int i = 0; i < n; ++i) { p[i] = (uint8_t)v; v >>= 8; } }

void *igdsp_wav_start(const char *path, int rate)
{
    igdsp_wav *w = new (std::nothrow) igdsp_wav();
    if (!w) return nullptr;
    w->f = std::fopen(path, "wb");
    w->data = 0;
    if (!w->f) { delete w; return nullptr; }
    uint8_t h[44];
    std::memcpy(h, "RIFF", 4); le(h + 4, 0, 4); std::memcpy(h + 8, "WAVEfmt ", 8); le(h + 16, 16, 4);
    le(h + 20, 0x0007, 2); le(h + 22, 2, 2); le(h + 24, (uint32_t)rate, 4); le(h + 28, (uint32_t)rate * 4u, 4);
    le(h + 32, 4, 2); le(h + 34, 16, 2); std::memcpy(h + 36, "data", 4); le(h + 40, 0, 4);
    std::fwrite(h, 1, 44, w->f);
    return w;
}

int igdsp_wav_writeRTPWav(void *wv, const char *pktbuf, const char *payloadbuf, unsigned pktlen, unsigned payloadlen)
{
    (void)pktbuf; (void)pktlen;
    igdsp_wav *w = static_cast<igdsp_wav *>(wv);
    if (!w || !w->f || (!payloadbuf && payloadlen)) return IGDSP_EINVAL;
    uint8_t buf[2 * IGDSP_MAX_PAYLOAD];
    while (payloadlen) {
        unsigned n = payloadlen > IGDSP_MAX_PAYLOAD ? IGDSP_MAX_PAYLOAD : payloadlen;
        for (unsigned i = 0; i < n; ++i) { buf[2 * i] = (uint8_t)payloadbuf[i]; buf[2 * i + 1] = 0; }
        if (std::fwrite(buf, 1, 2 * n, w->f) != 2 * n) return IGDSP_EDEVICE;
        w->data += 2 * n; payloadbuf += n; payloadlen -= n;
    }
    return IGDSP_OK;
}

int igdsp_wav_stop(void *wv)
{
    igdsp_wav *w = static_cast<igdsp_wav *>(wv);
    if (!w) return IGDSP_EINVAL;
    uint8_t s[4];
    std::fseek(w->f, 4, SEEK_SET); le(s, 36 + w->data, 4); std::fwrite(s, 1, 4, w->f);
    std::fseek(w->f, 40, SEEK_SET); le(s, w->data, 4); std::fwrite(s, 1, 4, w->f);
    std::fclose(w->f);
    delete w;
    return IGDSP_OK;
}

}  // extern "C"

// ---- best signal selection (roip_ed137.cpp:5609-5669, 5985-6119), no context needed
BssVoter::BssVoter() : sqlStatusCount(0), sqlStatusOn(false), voteTicks(5), votes(0), staleLastRx(false)
{
    for (int i = 0; i < 4; ++i) { radio[i].callState = false; radio[i].lastRx = 0; radio[i].rssi = -1; radio[i].audioSQLOn = false; }
}

int BssVoter::voted() const
{
    for (int i = 0; i < 4; ++i)
        if (radio[i].audioSQLOn) return i;
    return -1;
}

int BssVoter::tick(const uint32_t words[4], const bool call_up[4], bool force_mute)
{
    // the per-radio block (:5614-5669): runs only for a call that is up
    for (int i = 0; i < 4; ++i) {
        Radio &r = radio[i];
        r.callState = call_up[i];
        if (!r.callState) {
            if (!staleLastRx) r.lastRx = 0;
            continue;
        }
        int sqlon = (int)IGDSP_ED137_SQU(words[i]);          // get_IPRadioSquelch
        if (force_mute) sqlon = false;
        r.rssi = (int)IGDSP_ED137_BSS(words[i]);             // get_IPRadioBss
        r.lastRx = sqlon;                                    // (the lastRxmsec hold at :5658-5669 never fires)
    }
    Radio *r1 = &radio[0], *r2 = &radio[1], *r3 = &radio[2], *r4 = &radio[3];
    // :5987-6026 — a closed radio loses its vote, and the count with it
    for (int i = 0; i < 4; ++i) {
        Radio &r = radio[i];
        if ((r.callState == false) || (r.lastRx == 0)) {
            if (r.audioSQLOn == true) {
                sqlStatusCount = 0;
                sqlStatusOn = false;
            }
            r.audioSQLOn = false;
            r.rssi = -1;
        }
    }
    // :6027-6117
    if ((r1->lastRx > 0) || (r2->lastRx > 0) || (r3->lastRx > 0) || (r4->lastRx > 0)) {
        sqlStatusCount++;
        if ((sqlStatusCount >= voteTicks) & (sqlStatusOn == false)) {
            sqlStatusOn = true;                              // (every open radio is set to MUTE here)
            int pick = -1;
            if ((r1->rssi >= r2->rssi) & (r1->rssi >= r3->rssi) & (r1->rssi >= r4->rssi) & (r1->lastRx != 0)) pick = 0;
            else if ((r2->rssi >= r1->rssi) & (r2->rssi >= r3->rssi) & (r2->rssi >= r4->rssi) & (r2->lastRx != 0)) pick = 1;
            else if ((r3->rssi >= r1->rssi) & (r3->rssi >= r2->rssi) & (r3->rssi >= r4->rssi) & (r3->lastRx != 0)) pick = 2;
            else if ((r4->rssi >= r1->rssi) & (r4->rssi >= r2->rssi) & (r4->rssi >= r3->rssi) & (r4->lastRx != 0)) pick = 3;
            if (pick >= 0) {
                for (int i = 0; i < 4; ++i) radio[i].audioSQLOn = i == pick;   // (the voted one UNMUTE)
                ++votes;
            }
        }
    } else {
        sqlStatusCount = 0;
        sqlStatusOn = false;
        for (int i = 0; i < 4; ++i) radio[i].audioSQLOn = false;
    }
    return voted();
}

void *igdsp_host_bss_new(int vote_ticks, int stale_last_rx)
{
    BssVoter *v = new (std::nothrow) BssVoter();
    if (v) { v->voteTicks = vote_ticks; v->staleLastRx = stale_last_rx != 0; }
    return v;
}
void igdsp_host_bss_free(void *v) { delete static_cast<BssVoter *>(v); }
int igdsp_host_bss_tick(void *v, const uint32_t *words4, const int *call_up4, int force_mute)
{
    if (!v || !words4 || !call_up4) return IGDSP_EINVAL;
    const bool up[4] = {call_up4[0] != 0, call_up4[1] != 0, call_up4[2] != 0, call_up4[3] != 0};
    return static_cast<BssVoter *>(v)->tick(words4, up, force_mute != 0);
}
int igdsp_host_bss_state(void *v, int *count, int *on, unsigned *votes)
{
    if (!v) return IGDSP_EINVAL;
    const BssVoter *b = static_cast<const BssVoter *>(v);
    if (count) *count = b->sqlStatusCount;
    if (on) *on = b->sqlStatusOn ? 1 : 0;
    if (votes) *votes = b->votes;
    return IGDSP_OK;
}

// ---- PTT priority arbitration (roip_ed137.cpp:6124-6231), no context needed
PttArbiter::PttArbiter(int n_legs)
    : nLegs(n_legs < 1 ? 1 : (n_legs > kMaxLegs ? (int)kMaxLegs : n_legs)), ptt_level(0), releaseTicks(IGDSP_PTT_RELEASE_FRAMES), takeovers(0),
      lastFlags(0)
{
    for (int i = 0; i < kMaxLegs; ++i) {
        leg[i].callState = false; leg[i].rxOnly = false; leg[i].lastTx = 0; leg[i].lastTxmsec = 0; leg[i].m_PttPressed = false;
        leg[i].unmuted = false;
    }
}

int PttArbiter::unmutedLeg() const
{
    for (int i = 0; i < nLegs; ++i)
        if (leg[i].unmuted) return i;
    return -1;
}

int PttArbiter::tick(const uint32_t *words, const bool *call_up)
{
    int flags = 0;
    for (int i = 0; i < nLegs; ++i) {
        Leg &l = leg[i];
        l.callState = call_up[i];
        if (l.callState == false) continue;                  // :6131
        int ptt = l.rxOnly ? 0 : (int)IGDSP_ED137_PTT_TYPE(words[i]);   // :6134 get_IPRadioPttStatus, TRXMODE_RX
        if (ptt != l.lastTx) {                               // :6139-6154 — a release is bridged, with type 1
            if (ptt == 0) {
                if (l.lastTxmsec < 255) l.lastTxmsec++;
                if (l.lastTxmsec < releaseTicks) ptt = 1;
            }
        } else {
            l.lastTxmsec = 0;
        }
        l.lastTx = ptt;
        if (ptt > ptt_level) {                               // :6157-6177 — the highest type takes the transmitter
            ptt_level = ptt;
            for (int j = 0; j < nLegs; ++j) leg[j].unmuted = j == i;   // (every other leg MUTE, this one UNMUTE)
            ++takeovers;
            flags |= IGDSP_PTT_TAKEOVER;
        }
        if ((ptt > 0) && (l.m_PttPressed == false)) {        // :6191-6222
            l.m_PttPressed = true;
            flags |= IGDSP_PTT_PRESS;
        } else if ((ptt == 0) && (l.m_PttPressed == true)) {
            l.m_PttPressed = false;
            l.unmuted = false;
            ptt_level = 0;                                   // (on any pressed leg's release, not only the holder's)
            flags |= IGDSP_PTT_RELEASE;
        }
    }
    for (int i = 0; i < nLegs; ++i)
        if (leg[i].callState && leg[i].m_PttPressed) flags |= IGDSP_PTT_ON;
    lastFlags = flags;
    return unmutedLeg();
}

void *igdsp_host_ptt_new(int n_legs, int release_ticks)
{
    if (n_legs < 1 || n_legs > PttArbiter::kMaxLegs || release_ticks < 0 || release_ticks > 255) return nullptr;
    PttArbiter *v = new (std::nothrow) PttArbiter(n_legs);
    if (v && release_ticks) v->releaseTicks = release_ticks;
    return v;
}
void igdsp_host_ptt_free(void *v) { delete static_cast<PttArbiter *>(v); }
int igdsp_host_ptt_tick(void *v, const uint32_t *words, const int *call_up, const int *rx_only)
{
    if (!v || !words || !call_up) return IGDSP_EINVAL;
    PttArbiter *a = static_cast<PttArbiter *>(v);
    bool up[PttArbiter::kMaxLegs];
    for (int i = 0; i < a->nLegs; ++i) { up[i] = call_up[i] != 0; a->leg[i].rxOnly = rx_only && rx_only[i] != 0; }
    return a->tick(words, up);
}
int igdsp_host_ptt_state(void *v, int *level, unsigned *takeovers, int *flags)
{
    if (!v) return IGDSP_EINVAL;
    const PttArbiter *a = static_cast<const PttArbiter *>(v);
    if (level) *level = a->ptt_level;
    if (takeovers) *takeovers = a->takeovers;
    if (flags) *flags = a->lastFlags;
    return IGDSP_OK;
}
int igdsp_host_ptt_leg(void *v, int leg, int *last_tx, int *release_cnt, int *pressed, int *unmuted)
{
    if (!v) return IGDSP_EINVAL;
    const PttArbiter *a = static_cast<const PttArbiter *>(v);
    if (leg < 0 || leg >= a->nLegs) return IGDSP_EINVAL;
    if (last_tx) *last_tx = a->leg[leg].lastTx;
    if (release_cnt) *release_cnt = a->leg[leg].lastTxmsec;
    if (pressed) *pressed = a->leg[leg].m_PttPressed ? 1 : 0;
    if (unmuted) *unmuted = a->leg[leg].unmuted ? 1 : 0;
    return IGDSP_OK;
}

// ---- R2S link supervision (roip_ed137.cpp:1764-1780, :2009-2040; TransportAdapter.cpp:286-315), no context needed
LinkWatch::LinkWatch(int n_legs) : nLegs(n_legs < 1 ? 1 : n_legs), missTicks(IGDSP_LINK_MISS_TICKS), now(0), leg(new Leg[n_legs < 1 ? 1 : n_legs])
{
    for (int i = 0; i < nLegs; ++i) {
        Leg &l = leg[i];
        l.callState = false; l.r2sPacket = 0; l.rtpAudio = false; l.r2sCount = 0; l.r2sPeriod = IGDSP_LINK_R2S_PERIOD_MS; l.alarmed = false;
        l.alarms = 0; l.kind = 0; l.word = 0;
    }
}

LinkWatch::~LinkWatch() { delete[] leg; }

void LinkWatch::beginTick(unsigned long long now_ms, const bool *call_up)
{
    now = now_ms;
    for (int i = 0; i < nLegs; ++i) {
        Leg &l = leg[i];
        const bool up = call_up ? call_up[i] : true;
        l.kind = 0; l.word = 0;
        if (up && !l.callState) {                            // transport_adapter_create (TransportAdapter.cpp:122, TransportAdapter.h:91)
            l.r2sPacket = now; l.r2sCount = 0; l.rtpAudio = false; l.alarmed = false;
            l.kind |= IGDSP_LINK_CAME_UP;
        }
        l.callState = up;
    }
}

int LinkWatch::packet(int i, int pt, unsigned payload_len, bool runt, uint32_t ed137)
{
    if (i < 0 || i >= nLegs || !leg[i].callState) return 0;
    Leg &l = leg[i];
    l.r2sPacket = now;                                       // every return path of transport_rtp_cb
    if (runt || (pt != 123 && payload_len >= 1024)) return 0;   // :286-291
    if (pt != 123) {                                         // :298-307
        if (l.rtpAudio == false) { l.rtpAudio = true; l.kind |= IGDSP_LINK_AUDIO_ON; l.word = ed137; return IGDSP_LINK_AUDIO_ON; }
        l.rtpAudio = true;
    } else {                                                 // :308-315
        if (l.rtpAudio == true) { l.rtpAudio = false; l.kind |= IGDSP_LINK_AUDIO_OFF; l.word = ed137; return IGDSP_LINK_AUDIO_OFF; }
        l.rtpAudio = false;
    }
    return 0;
}

int LinkWatch::endTick()
{
    int missing = 0;
    for (int i = 0; i < nLegs; ++i) {
        Leg &l = leg[i];
        if (!l.callState) continue;
        const long long secDiff = (long long)(now - l.r2sPacket);   // qint64, :1768
        if (secDiff > (long long)l.r2sPeriod * 3) {          // :1769
            l.kind |= IGDSP_LINK_LATE;
            if (l.r2sCount == missTicks - 1) {               // :1771 r2sCount == 5
                l.kind |= IGDSP_LINK_MISSING; l.alarmed = true; ++l.alarms; ++missing;
            }
            if (l.r2sCount < 65535) l.r2sCount++;
        } else {
            if (l.r2sCount > 0) l.kind |= IGDSP_LINK_RECOVERED;
            l.r2sCount = 0;
            l.alarmed = false;
        }
    }
    return missing;
}

void *igdsp_host_link_new(int n_legs, int miss_ticks)
{
    if (n_legs < 1 || n_legs > 65536 || miss_ticks < 0 || miss_ticks > 65535) return nullptr;
    LinkWatch *v = nullptr;
    try { v = new LinkWatch(n_legs); } catch (...) { return nullptr; }
    if (miss_ticks) v->missTicks = miss_ticks;
    return v;
}
void igdsp_host_link_free(void *v) { delete static_cast<LinkWatch *>(v); }
int igdsp_host_link_set_period(void *v, int leg, int period_ms)
{
    LinkWatch *a = static_cast<LinkWatch *>(v);
    if (!a || leg < 0 || leg >= a->nLegs || period_ms < 0 || period_ms > 65535) return IGDSP_EINVAL;
    a->leg[leg].r2sPeriod = period_ms;
    return IGDSP_OK;
}
int igdsp_host_link_begin(void *v, unsigned long long now_ms, const int *call_up)
{
    LinkWatch *a = static_cast<LinkWatch *>(v);
    if (!a) return IGDSP_EINVAL;
    if (!call_up) { a->beginTick(now_ms, nullptr); return IGDSP_OK; }
    bool *up = new (std::nothrow) bool[a->nLegs];
    if (!up) return IGDSP_ENOMEM;
    for (int i = 0; i < a->nLegs; ++i) up[i] = call_up[i] != 0;
    a->beginTick(now_ms, up);
    delete[] up;
    return IGDSP_OK;
}
int igdsp_host_link_packet(void *v, int leg, int pt, unsigned payload_len, int runt, uint32_t ed137)
{
    LinkWatch *a = static_cast<LinkWatch *>(v);
    if (!a || leg < 0 || leg >= a->nLegs) return IGDSP_EINVAL;
    return a->packet(leg, pt, payload_len, runt != 0, ed137);
}
int igdsp_host_link_end(void *v, uint8_t *kinds, uint32_t *words)
{
    LinkWatch *a = static_cast<LinkWatch *>(v);
    if (!a) return IGDSP_EINVAL;
    const int missing = a->endTick();
    for (int i = 0; i < a->nLegs; ++i) {
        if (kinds) kinds[i] = (uint8_t)a->leg[i].kind;
        if (words) words[i] = a->leg[i].word;
    }
    return missing;
}
int igdsp_host_link_leg(void *v, int leg, unsigned long long *last_ms, int *count, int *flags, unsigned *alarms)
{
    const LinkWatch *a = static_cast<const LinkWatch *>(v);
    if (!a || leg < 0 || leg >= a->nLegs) return IGDSP_EINVAL;
    const LinkWatch::Leg &l = a->leg[leg];
    if (last_ms) *last_ms = l.r2sPacket;
    if (count) *count = l.r2sCount;
    if (flags) *flags = (l.callState ? IGDSP_LINK_UP : 0) | (l.rtpAudio ? IGDSP_LINK_AUDIO : 0) | (l.alarmed ? IGDSP_LINK_ALARMED : 0);
    if (alarms) *alarms = l.alarms;
    return IGDSP_OK;
}

// ---- the sound-card splitter / combiner, no context needed
SplitComb::SplitComb(int channels, int samples_per_frame)
    : K(channels < 1 ? 1 : (channels > IGDSP_SND_MAX_CHANNELS ? IGDSP_SND_MAX_CHANNELS : channels)),
      n(samples_per_frame < 1 ? 1 : (samples_per_frame > IGDSP_MAX_PAYLOAD ? IGDSP_MAX_PAYLOAD : samples_per_frame))
{
}

void SplitComb::combine(const int16_t *const *rows, int16_t *frame) const
{
    for (int s = 0; s < n; ++s)
        for (int k = 0; k < K; ++k) frame[s * K + k] = rows[k][s];
}

void SplitComb::split(const int16_t *frame, int16_t *const *rows) const
{
    for (int s = 0; s < n; ++s)
        for (int k = 0; k < K; ++k) rows[k][s] = frame[s * K + k];
}

igdsp_frame_stats SplitComb::vu(const int16_t *frame, int k) const
{
    igdsp_frame_stats st;
    uint64_t sumsq = 0;
    uint32_t peak = 0;
    for (int s = 0; s < n; ++s) {
        const int32_t x = frame[s * K + k];
        const uint32_t ax = (uint32_t)(x < 0 ? -x : x);
        sumsq += (uint64_t)ax * ax;
        if (ax > peak) peak = ax;
    }
    st.sumsq = sumsq;
    st.rms = std::sqrt((float)sumsq / (float)n);
    st.peak = (uint16_t)peak;
    st.byte_mean = 0;
    st.flags = (uint8_t)(peak <= 8u ? IGDSP_FLAG_SILENT : 0);
    return st;
}

void *igdsp_host_sc_new(int channels, int samples_per_frame)
{
    if (channels < 1 || channels > IGDSP_SND_MAX_CHANNELS || samples_per_frame < 1 || samples_per_frame > IGDSP_MAX_PAYLOAD) return nullptr;
    return new (std::nothrow) SplitComb(channels, samples_per_frame);
}
void igdsp_host_sc_free(void *v) { delete static_cast<SplitComb *>(v); }
int igdsp_host_sc_combine(void *v, const int16_t *const *rows, int16_t *frame)
{
    if (!v || !rows || !frame) return IGDSP_EINVAL;
    static_cast<const SplitComb *>(v)->combine(rows, frame);
    return IGDSP_OK;
}
int igdsp_host_sc_split(void *v, const int16_t *frame, int16_t *const *rows)
{
    if (!v || !rows || !frame) return IGDSP_EINVAL;
    static_cast<const SplitComb *>(v)->split(frame, rows);
    return IGDSP_OK;
}
int igdsp_host_sc_vu(void *v, const int16_t *frame, igdsp_frame_stats *out)
{
    const SplitComb *a = static_cast<const SplitComb *>(v);
    if (!a || !frame || !out) return IGDSP_EINVAL;
    for (int k = 0; k < a->K; ++k) out[k] = a->vu(frame, k);
    return IGDSP_OK;
}

// ---- the ring tone, no context needed
RingTone::RingTone(uint32_t clock_rate, uint32_t samples_per_frame)
    : n(samples_per_frame < 1 ? 1 : (samples_per_frame > IGDSP_MAX_PAYLOAD ? IGDSP_MAX_PAYLOAD : samples_per_frame)), connected_(false), rewind_(false)
{
    static const uint16_t off_msec[3] = {1000, 4000, 3000};                       // Functions.cpp:542-553
    for (int i = 0; i < 3; ++i) {
        tone[i].freq1 = 440; tone[i].freq2 = 480; tone[i].on_msec = 2000; tone[i].off_msec = off_msec[i];
        tone[i].volume = 0; tone[i].reserved = 0;
    }
    std::memset(&plan, 0, sizeof(plan));
    ok = igdsp_tone_plan_build(tone, 1, clock_rate, IGDSP_TONE_LOOP, &plan) == IGDSP_OK;   // count = 1, as pjmedia_tonegen_play(.., 1, tone, ..)
    state.pos = 0;
    state.flags = IGDSP_TONE_PLAYING;
}

void RingTone::playRing() { connected_ = true; }

void RingTone::stopRing()
{
    connected_ = false;
    rewind_ = true;
}

uint32_t RingTone::connections(uint32_t tone_channel, uint32_t *channel, uint32_t *port) const
{
    if (!connected_ || !channel || !port) return 0;
    channel[0] = tone_channel;
    port[0] = 0;
    return 1;
}

uint32_t RingTone::cmd()
{
    const uint32_t c = (rewind_ ? IGDSP_TONE_CMD_REWIND : 0u) | (connected_ ? 0u : IGDSP_TONE_CMD_HOLD);
    rewind_ = false;
    return c;
}

int RingTone::frame(int16_t *out, uint16_t *len)
{
    if (!ok) return IGDSP_EINVAL;
    return igdsp_tone_frame(&plan, &state, cmd(), n, out, len);
}

void *igdsp_host_ring_new(uint32_t clock_rate, uint32_t samples_per_frame)
{
    if (samples_per_frame < 1 || samples_per_frame > IGDSP_MAX_PAYLOAD) return nullptr;
    RingTone *r = new (std::nothrow) RingTone(clock_rate, samples_per_frame);
    if (r && !r->ok) { delete r; r = nullptr; }
    return r;
}
void igdsp_host_ring_free(void *v) { delete static_cast<RingTone *>(v); }
int igdsp_host_ring_play(void *v)
{
    if (!v) return IGDSP_EINVAL;
    static_cast<RingTone *>(v)->playRing();
    return IGDSP_OK;
}
int igdsp_host_ring_stop(void *v)
{
    if (!v) return IGDSP_EINVAL;
    static_cast<RingTone *>(v)->stopRing();
    return IGDSP_OK;
}
int igdsp_host_ring_connections(void *v, uint32_t tone_channel, uint32_t *channel, uint32_t *port)
{
    if (!v || !channel || !port) return IGDSP_EINVAL;
    return (int)static_cast<const RingTone *>(v)->connections(tone_channel, channel, port);
}
int igdsp_host_ring_cmd(void *v) { return v ? (int)static_cast<RingTone *>(v)->cmd() : IGDSP_EINVAL; }
int igdsp_host_ring_frame(void *v, int16_t *out, uint16_t *len)
{
    if (!v || !out || !len) return IGDSP_EINVAL;
    return static_cast<RingTone *>(v)->frame(out, len);
}
int igdsp_host_ring_get(void *v, igdsp_tone_plan *plan, igdsp_tone_state *state)
{
    const RingTone *r = static_cast<const RingTone *>(v);
    if (!r || !plan || !state) return IGDSP_EINVAL;
    *plan = r->plan;
    *state = r->state;
    return IGDSP_OK;
}

// ---- a call port's rate converters, no context needed
Resampler::Resampler(uint32_t bridge_rate, uint32_t samples_per_frame) : factor(bridge_rate / 8000u), n(samples_per_frame)
{
    ok = bridge_rate % 8000u == 0 && (factor == 2 || factor == 3 || factor == 4 || factor == 6) && n >= 1 && n <= IGDSP_MAX_PAYLOAD;
    std::memset(&to_bridge, 0, sizeof(to_bridge));
    std::memset(&from_bridge, 0, sizeof(from_bridge));
}

int Resampler::up(const int16_t *narrow, int16_t *wide)
{
    return ok ? igdsp_rs_frame(&to_bridge, IGDSP_RS_UP, factor, narrow, n, wide) : IGDSP_EINVAL;
}

int Resampler::down(const int16_t *wide, int16_t *narrow)
{
    return ok ? igdsp_rs_frame(&from_bridge, IGDSP_RS_DOWN, factor, wide, n * factor, narrow) : IGDSP_EINVAL;
}

void *igdsp_host_rs_new(uint32_t bridge_rate, uint32_t samples_per_frame)
{
    Resampler *r = new (std::nothrow) Resampler(bridge_rate, samples_per_frame);
    if (r && !r->ok) { delete r; r = nullptr; }
    return r;
}
void igdsp_host_rs_free(void *v) { delete static_cast<Resampler *>(v); }
int igdsp_host_rs_up(void *v, const int16_t *narrow, int16_t *wide)
{
    if (!v || !narrow || !wide) return IGDSP_EINVAL;
    return static_cast<Resampler *>(v)->up(narrow, wide);
}
int igdsp_host_rs_down(void *v, const int16_t *wide, int16_t *narrow)
{
    if (!v || !wide || !narrow) return IGDSP_EINVAL;
    return static_cast<Resampler *>(v)->down(wide, narrow);
}

// ---- a reverse channel's delay buffer, no context needed
DelayBuf::DelayBuf(uint32_t samples_per_frame, uint32_t max_samples_) : n(samples_per_frame), max_samples(max_samples_)
{
    ok = n >= 1 && n <= IGDSP_MAX_PAYLOAD && max_samples >= 2 * n && max_samples <= IGDSP_DBUF_CAP;
    std::memset(&state, 0, sizeof(state));
}

int DelayBuf::put(const int16_t *frame)
{
    return ok ? igdsp_dbuf_step(&state, IGDSP_DBUF_PUT, frame, n, max_samples, nullptr, nullptr) : IGDSP_EINVAL;
}

int DelayBuf::get(int16_t *frame)
{
    uint32_t flag = 0;
    const int rc = ok ? igdsp_dbuf_step(&state, IGDSP_DBUF_GET, nullptr, n, max_samples, frame, &flag) : IGDSP_EINVAL;
    return rc == IGDSP_OK ? (int)flag : rc;
}

void *igdsp_host_dbuf_new(uint32_t samples_per_frame, uint32_t max_samples)
{
    DelayBuf *d = new (std::nothrow) DelayBuf(samples_per_frame, max_samples);
    if (d && !d->ok) { delete d; d = nullptr; }
    return d;
}
void igdsp_host_dbuf_free(void *v) { delete static_cast<DelayBuf *>(v); }
int igdsp_host_dbuf_put(void *v, const int16_t *frame)
{
    if (!v || !frame) return IGDSP_EINVAL;
    return static_cast<DelayBuf *>(v)->put(frame);
}
int igdsp_host_dbuf_get(void *v, int16_t *frame)
{
    if (!v || !frame) return IGDSP_EINVAL;
    return static_cast<DelayBuf *>(v)->get(frame);
}
int igdsp_host_dbuf_fill(void *v) { return v ? (int)static_cast<DelayBuf *>(v)->fill() : IGDSP_EINVAL; }
int igdsp_host_dbuf_state(void *v, igdsp_dbuf_state *out)
{
    if (!v || !out) return IGDSP_EINVAL;
    *out = static_cast<DelayBuf *>(v)->state;
    return IGDSP_OK;
}

// ---- the spectrum graph, no context needed
SpectrumGraph::SpectrumGraph(uint32_t samples_per_frame, uint32_t hop_frames, float alpha) : n(samples_per_frame), fftSize(IGDSP_SPEC_N)
{
    cfg.hop_frames = hop_frames;
    cfg.alpha = alpha;
    ok = n >= 1 && n <= IGDSP_MAX_PAYLOAD && hop_frames >= 1 && alpha > 0.0f && alpha <= 1.0f;
    initSpectrumGraph();
}

void SpectrumGraph::initSpectrumGraph()
{
    d_fftAvg = (float)(1.0 - 1.0e-2 * 75);
    spectClear();
}

void SpectrumGraph::spectClear()
{
    std::memset(&state, 0, sizeof(state));
    std::memset(&last, 0, sizeof(last));
    for (int k = 0; k < IGDSP_SPEC_BINS; ++k) d_realFftData[k] = d_iirFftData[k] = IGDSP_SPEC_FLOOR_DB;
}

int SpectrumGraph::feed(const int16_t *frame)
{
    if (!ok || !frame) return IGDSP_EINVAL;
    igdsp_spec_rec rec;
    const int rc = igdsp_spec_frame(&state, frame, n, &cfg, &rec, d_realFftData);
    if (rc != IGDSP_OK) return rc;
    if (!(rec.flags & IGDSP_SPEC_HOP)) return 0;
    std::memcpy(d_iirFftData, state.avg, sizeof(d_iirFftData));
    last = rec;
    return 1;
}

void *igdsp_host_spect_new(uint32_t samples_per_frame, uint32_t hop_frames, float alpha)
{
    SpectrumGraph *g = new (std::nothrow) SpectrumGraph(samples_per_frame, hop_frames, alpha);
    if (g && !g->ok) { delete g; g = nullptr; }
    return g;
}
void igdsp_host_spect_free(void *v) { delete static_cast<SpectrumGraph *>(v); }
int igdsp_host_spect_feed(void *v, const int16_t *frame)
{
    if (!v || !frame) return IGDSP_EINVAL;
    return static_cast<SpectrumGraph *>(v)->feed(frame);
}
void igdsp_host_spect_clear(void *v) { if (v) static_cast<SpectrumGraph *>(v)->spectClear(); }
const float *igdsp_host_spect_real(void *v) { return v ? static_cast<SpectrumGraph *>(v)->d_realFftData : nullptr; }
const float *igdsp_host_spect_iir(void *v) { return v ? static_cast<SpectrumGraph *>(v)->d_iirFftData : nullptr; }
float igdsp_host_spect_fft_avg(void *v) { return v ? static_cast<SpectrumGraph *>(v)->d_fftAvg : 0.0f; }

// ---- in-band DTMF on one leg, no context needed
DtmfReceiver::DtmfReceiver(uint32_t samples_per_frame, uint32_t clock_rate) : n(samples_per_frame)
{
    ok = igdsp_tdet_plan_dtmf(clock_rate, &plan) == IGDSP_OK && n >= 2 && n <= IGDSP_MAX_PAYLOAD && (n & 1u) == 0;
    newCall();
}

void DtmfReceiver::newCall()
{
    std::memset(&state, 0, sizeof(state));
    std::memset(&last, 0, sizeof(last));
    std::memset(dialled, 0, sizeof(dialled));
    count = 0;
}

int DtmfReceiver::feed(const int16_t *frame)
{
    if (!ok || !frame) return IGDSP_EINVAL;
    const int rc = igdsp_tdet_frame(&plan, &state, frame, n, &last);
    if (rc != IGDSP_OK) return rc;
    if (!(last.flags & (IGDSP_TDET_ON0 | IGDSP_TDET_ON1))) return 0;
    const int ch = igdsp_tdet_digit(state.cur ? state.cur : last.code);    // the digit that is up (an ON is the frame's last event unless it also ended)
    if (ch) {
        if (count == sizeof(dialled) - 1) { std::memmove(dialled, dialled + 1, count - 1); --count; }
        dialled[count++] = (char)ch;
        dialled[count] = 0;
    }
    return ch;
}

void *igdsp_host_dtmf_new(uint32_t samples_per_frame, uint32_t clock_rate)
{
    DtmfReceiver *r = new (std::nothrow) DtmfReceiver(samples_per_frame, clock_rate);
    if (r && !r->ok) { delete r; r = nullptr; }
    return r;
}
void igdsp_host_dtmf_free(void *v) { delete static_cast<DtmfReceiver *>(v); }
int igdsp_host_dtmf_feed(void *v, const int16_t *frame)
{
    if (!v || !frame) return IGDSP_EINVAL;
    return static_cast<DtmfReceiver *>(v)->feed(frame);
}
const char *igdsp_host_dtmf_digits(void *v) { return v ? static_cast<DtmfReceiver *>(v)->digits() : nullptr; }
void igdsp_host_dtmf_new_call(void *v) { if (v) static_cast<DtmfReceiver *>(v)->newCall(); }

// ---- the sound port's echo canceller on one leg, no context needed
EchoCanceller::EchoCanceller(uint32_t samples_per_frame, uint32_t tail) : n(samples_per_frame)
{
    igdsp_ec_cfg_default(tail, &cfg);
    ok = (tail == 128 || tail == 256) && n >= 2 && n <= IGDSP_MAX_PAYLOAD && (n & 1u) == 0;
    reset();
}

void EchoCanceller::reset()
{
    std::memset(&state, 0, sizeof(state));
    std::memset(&last, 0, sizeof(last));
}

int EchoCanceller::cancel(const int16_t *near_frame, const int16_t *far_frame, int16_t *out, uint32_t ctl)
{
    if (!ok || !near_frame || !out) return IGDSP_EINVAL;
    return igdsp_ec_frame(&cfg, &state, near_frame, far_frame, n, ctl, out, &last);
}

float EchoCanceller::erleDb() const
{
    if (!last.near_e || !last.out_e) return 0.0f;
    return 10.0f * std::log10((float)last.near_e / (float)last.out_e);
}

void *igdsp_host_ec_new(uint32_t samples_per_frame, uint32_t tail)
{
    EchoCanceller *e = new (std::nothrow) EchoCanceller(samples_per_frame, tail);
    if (e && !e->ok) { delete e; e = nullptr; }
    return e;
}
void igdsp_host_ec_free(void *v) { delete static_cast<EchoCanceller *>(v); }
int igdsp_host_ec_cancel(void *v, const int16_t *near_frame, const int16_t *far_frame, int16_t *out, uint32_t ctl)
{
    if (!v) return IGDSP_EINVAL;
    return static_cast<EchoCanceller *>(v)->cancel(near_frame, far_frame, out, ctl);
}
int igdsp_host_ec_rec(void *v, igdsp_ec_rec *out)
{
    if (!v || !out) return IGDSP_EINVAL;
    *out = static_cast<EchoCanceller *>(v)->last;
    return IGDSP_OK;
}
float igdsp_host_ec_erle_db(void *v) { return v ? static_cast<EchoCanceller *>(v)->erleDb() : 0.0f; }
void igdsp_host_ec_reset(void *v) { if (v) static_cast<EchoCanceller *>(v)->reset(); }

// ---- the level control on one leg, no context needed
LevelControl::LevelControl(uint32_t samples_per_frame) : n(samples_per_frame)
{
    igdsp_agc_cfg_default(&cfg);
    ok = n >= 8 && n <= IGDSP_MAX_PAYLOAD && (n & 7u) == 0;
    reset();
}

void LevelControl::reset()
{
    std::memset(&state, 0, sizeof(state));
    std::memset(&last, 0, sizeof(last));
}

int LevelControl::process(const int16_t *frame, int16_t *out, uint32_t ctl)
{
    if (!ok || !frame || !out) return IGDSP_EINVAL;
    return igdsp_agc_frame(&cfg, &state, frame, n, ctl, out, &last);
}

float LevelControl::gainDb() const
{
    if (!last.gain) return 0.0f;
    return 20.0f * std::log10((float)last.gain / (float)IGDSP_AGC_UNITY);
}

void *igdsp_host_agc_new(uint32_t samples_per_frame)
{
    LevelControl *e = new (std::nothrow) LevelControl(samples_per_frame);
    if (e && !e->ok) { delete e; e = nullptr; }
    return e;
}
void igdsp_host_agc_free(void *v) { delete static_cast<LevelControl *>(v); }
int igdsp_host_agc_process(void *v, const int16_t *frame, int16_t *out, uint32_t ctl)
{
    if (!v) return IGDSP_EINVAL;
    return static_cast<LevelControl *>(v)->process(frame, out, ctl);
}
int igdsp_host_agc_rec(void *v, igdsp_agc_rec *out)
{
    if (!v || !out) return IGDSP_EINVAL;
    *out = static_cast<LevelControl *>(v)->last;
    return IGDSP_OK;
}
float igdsp_host_agc_gain_db(void *v) { return v ? static_cast<LevelControl *>(v)->gainDb() : 0.0f; }
void igdsp_host_agc_reset(void *v) { if (v) static_cast<LevelControl *>(v)->reset(); }

// ---- the silence detector on one leg, no context needed
VoiceDetector::VoiceDetector(uint32_t samples_per_frame) : n(samples_per_frame)
{
    igdsp_vad_cfg_default(&cfg);
    ok = n >= 16 && n <= IGDSP_MAX_PAYLOAD && (n & 7u) == 0;
    reset();
}

void VoiceDetector::reset()
{
    std::memset(&state, 0, sizeof(state));
    std::memset(&last, 0, sizeof(last));
    std::memset(sid, 0, sizeof(sid));
}

int VoiceDetector::process(const int16_t *frame, uint32_t ctl)
{
    if (!ok || !frame) return IGDSP_EINVAL;
    return igdsp_vad_frame(&cfg, &state, frame, n, ctl, &last, sid);
}

void *igdsp_host_vad_new(uint32_t samples_per_frame)
{
    VoiceDetector *e = new (std::nothrow) VoiceDetector(samples_per_frame);
    if (e && !e->ok) { delete e; e = nullptr; }
    return e;
}
void igdsp_host_vad_free(void *v) { delete static_cast<VoiceDetector *>(v); }
int igdsp_host_vad_process(void *v, const int16_t *frame, uint32_t ctl)
{
    if (!v) return IGDSP_EINVAL;
    return static_cast<VoiceDetector *>(v)->process(frame, ctl);
}
int igdsp_host_vad_rec(void *v, igdsp_vad_rec *out)
{
    if (!v || !out) return IGDSP_EINVAL;
    *out = static_cast<VoiceDetector *>(v)->last;
    return IGDSP_OK;
}
int igdsp_host_vad_sid(void *v, uint8_t out[16])
{
    if (!v || !out) return IGDSP_EINVAL;
    std::memcpy(out, static_cast<VoiceDetector *>(v)->sid, 16);
    return (int)static_cast<VoiceDetector *>(v)->sidLen();
}
int igdsp_host_vad_cfg(void *v, const igdsp_vad_cfg *cfg)
{
    if (!v || !cfg) return IGDSP_EINVAL;
    static_cast<VoiceDetector *>(v)->cfg = *cfg;
    return IGDSP_OK;
}
void igdsp_host_vad_reset(void *v) { if (v) static_cast<VoiceDetector *>(v)->reset(); }

// ---- comfort noise on one leg, no context needed
ComfortNoise::ComfortNoise(uint32_t samples_per_frame, uint32_t seed_) : n(samples_per_frame), seed(seed_)
{
    ok = n >= 16 && n <= IGDSP_MAX_PAYLOAD && (n & 7u) == 0;
    reset();
}

void ComfortNoise::reset()
{
    std::memset(&state, 0, sizeof(state));                   // no tag: the RESET state, which takes the seed
    std::memset(&last, 0, sizeof(last));
}

int ComfortNoise::process(uint32_t kind, const uint8_t *sid, uint32_t sid_len, const int16_t *voice, int16_t *out, uint32_t ctl)
{
    if (!ok || !out) return IGDSP_EINVAL;
    return igdsp_cng_frame(&state, kind, sid, sid_len, voice, n, ctl, seed, out, &last);
}

void *igdsp_host_cng_new(uint32_t samples_per_frame, uint32_t seed)
{
    ComfortNoise *e = new (std::nothrow) ComfortNoise(samples_per_frame, seed);
    if (e && !e->ok) { delete e; e = nullptr; }
    return e;
}
void igdsp_host_cng_free(void *v) { delete static_cast<ComfortNoise *>(v); }
int igdsp_host_cng_process(void *v, uint32_t kind, const uint8_t *sid, uint32_t sid_len, const int16_t *voice, int16_t *out, uint32_t ctl)
{
    if (!v) return IGDSP_EINVAL;
    return static_cast<ComfortNoise *>(v)->process(kind, sid, sid_len, voice, out, ctl);
}
int igdsp_host_cng_rec(void *v, igdsp_cng_rec *out)
{
    if (!v || !out) return IGDSP_EINVAL;
    *out = static_cast<ComfortNoise *>(v)->last;
    return IGDSP_OK;
}
void igdsp_host_cng_reset(void *v) { if (v) static_cast<ComfortNoise *>(v)->reset(); }

// ---- a filter on one leg, no context needed
LegFilter::LegFilter(uint32_t samples_per_frame) : n(samples_per_frame), planned(false)
{
    ok = n >= 8 && n <= IGDSP_MAX_PAYLOAD && (n & 7u) == 0;
    std::memset(&plan, 0, sizeof(plan));
    reset();
}

void LegFilter::reset()
{
    std::memset(&state, 0, sizeof(state));                   // no tag: all-zero histories
    std::memset(&last, 0, sizeof(last));
}

int LegFilter::setPlan(const igdsp_filt_plan *p)
{
    if (!p || igdsp_filt_plan_check(p) != IGDSP_OK) return IGDSP_EINVAL;
    plan = *p;
    planned = true;
    reset();
    return IGDSP_OK;
}

int LegFilter::setPreset(uint32_t preset, uint32_t clock_rate)
{
    igdsp_filt_plan p;
    if (igdsp_filt_plan_preset(preset, clock_rate, &p) != IGDSP_OK) return IGDSP_EINVAL;
    return setPlan(&p);
}

int LegFilter::process(const int16_t *pcm, int16_t *out, uint32_t ctl)
{
    if (!ok || !pcm || !out) return IGDSP_EINVAL;
    return igdsp_filt_frame(planned ? &plan : nullptr, &state, pcm, n, ctl, out, &last);
}

void *igdsp_host_filt_new(uint32_t samples_per_frame)
{
    LegFilter *e = new (std::nothrow) LegFilter(samples_per_frame);
    if (e && !e->ok) { delete e; e = nullptr; }
    return e;
}
void igdsp_host_filt_free(void *v) { delete static_cast<LegFilter *>(v); }
int igdsp_host_filt_plan(void *v, const igdsp_filt_plan *plan) { return v ? static_cast<LegFilter *>(v)->setPlan(plan) : IGDSP_EINVAL; }
int igdsp_host_filt_preset(void *v, uint32_t preset, uint32_t clock_rate)
{
    return v ? static_cast<LegFilter *>(v)->setPreset(preset, clock_rate) : IGDSP_EINVAL;
}
int igdsp_host_filt_process(void *v, const int16_t *pcm, int16_t *out, uint32_t ctl)
{
    if (!v) return IGDSP_EINVAL;
    return static_cast<LegFilter *>(v)->process(pcm, out, ctl);
}
int igdsp_host_filt_rec(void *v, igdsp_filt_rec *out)
{
    if (!v || !out) return IGDSP_EINVAL;
    *out = static_cast<LegFilter *>(v)->last;
    return IGDSP_OK;
}
void igdsp_host_filt_reset(void *v) { if (v) static_cast<LegFilter *>(v)->reset(); }

// ---- a noise suppressor on one leg, no context needed
LegDenoiser::LegDenoiser(uint32_t samples_per_frame) : n(samples_per_frame), ctl(IGDSP_NS_RUN)
{
    ok = n == 80 || n == 160 || n == 240 || n == 320;
    igdsp_ns_cfg_default(&cfg);
    reset();
}

void LegDenoiser::reset()
{
    std::memset(&state, 0, sizeof(state));                   // no tag: a fresh state
    std::memset(&last, 0, sizeof(last));
}

int LegDenoiser::setConfig(const igdsp_ns_cfg *c)
{
    if (!c) return IGDSP_EINVAL;
    igdsp_ns_state probe;
    int16_t zero[80] = {0};
    std::memset(&probe, 0, sizeof(probe));
    if (igdsp_ns_frame(c, &probe, zero, 80, IGDSP_NS_RUN, nullptr, nullptr) != IGDSP_OK) return IGDSP_EINVAL;   // the library's range check
    cfg = *c;
    return IGDSP_OK;
}

int LegDenoiser::process(const int16_t *pcm, int16_t *out)
{
    if (!ok || !pcm || !out) return IGDSP_EINVAL;
    return igdsp_ns_frame(&cfg, &state, pcm, n, ctl, out, &last);
}

void *igdsp_host_ns_new(uint32_t samples_per_frame)
{
    LegDenoiser *e = new (std::nothrow) LegDenoiser(samples_per_frame);
    if (e && !e->ok) { delete e; e = nullptr; }
    return e;
}
void igdsp_host_ns_free(void *v) { delete static_cast<LegDenoiser *>(v); }
int igdsp_host_ns_config(void *v, const igdsp_ns_cfg *cfg) { return v ? static_cast<LegDenoiser *>(v)->setConfig(cfg) : IGDSP_EINVAL; }
int igdsp_host_ns_control(void *v, uint32_t ctl)
{
    if (!v || ctl > IGDSP_NS_BYPASS) return IGDSP_EINVAL;
    static_cast<LegDenoiser *>(v)->ctl = ctl;
    return IGDSP_OK;
}
int igdsp_host_ns_process(void *v, const int16_t *pcm, int16_t *out)
{
    if (!v) return IGDSP_EINVAL;
    return static_cast<LegDenoiser *>(v)->process(pcm, out);
}
int igdsp_host_ns_rec(void *v, igdsp_ns_rec *out)
{
    if (!v || !out) return IGDSP_EINVAL;
    *out = static_cast<LegDenoiser *>(v)->last;
    return IGDSP_OK;
}
void igdsp_host_ns_reset(void *v) { if (v) static_cast<LegDenoiser *>(v)->reset(); }

// ---- SRTP on one leg and direction, no context needed
LegSrtp::LegSrtp(const uint8_t key_salt[30], uint32_t tag_len, uint32_t roc0) : ctl(IGDSP_SRTP_RUN), resetNext(false)
{
    std::memset(&state, 0, sizeof(state));                   // no tag word: NO_KEY until a key is derived
    std::memset(&last, 0, sizeof(last));
    ok = key_salt && igdsp_srtp_derive(key_salt, tag_len, roc0, &state) == IGDSP_OK;
}

void LegSrtp::reset() { resetNext = true; }

int LegSrtp::protect(const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity)
{
    if (!ok || !in || !out) return IGDSP_EINVAL;
    uint32_t n = 0;
    const uint32_t c = (resetNext && ctl == IGDSP_SRTP_RUN) ? (uint32_t)IGDSP_SRTP_RESET : ctl;
    if (igdsp_srtp_protect_packet(&state, c, in, size, out, out_capacity, &n, &last) != IGDSP_OK) return IGDSP_EINVAL;
    if (c == IGDSP_SRTP_RESET) resetNext = false;
    return (int)n;
}

int LegSrtp::unprotect(const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity)
{
    if (!ok || !in || !out) return IGDSP_EINVAL;
    uint32_t n = 0;
    const uint32_t c = (resetNext && ctl == IGDSP_SRTP_RUN) ? (uint32_t)IGDSP_SRTP_RESET : ctl;
    if (igdsp_srtp_unprotect_packet(&state, c, in, size, out, out_capacity, &n, &last) != IGDSP_OK) return IGDSP_EINVAL;
    if (c == IGDSP_SRTP_RESET) resetNext = false;
    return (int)n;
}

// ---- SRTP with AES-GCM on one leg and direction, no context needed
LegSrtpGcm::LegSrtpGcm(const uint8_t *key_salt, uint32_t key_bytes, uint32_t roc0) : ctl(IGDSP_SRTP_RUN), resetNext(false)
{
    std::memset(&state, 0, sizeof(state));                   // no tag word: NO_KEY until a key is derived
    std::memset(&last, 0, sizeof(last));
    ok = key_salt && igdsp_srtp_gcm_derive(key_salt, key_bytes, roc0, &state) == IGDSP_OK;
}

void LegSrtpGcm::reset() { resetNext = true; }

int LegSrtpGcm::protect(const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity)
{
    if (!ok || !in || !out) return IGDSP_EINVAL;
    uint32_t n = 0;
    const uint32_t c = (resetNext && ctl == IGDSP_SRTP_RUN) ? (uint32_t)IGDSP_SRTP_RESET : ctl;
    if (igdsp_srtp_gcm_protect_packet(&state, c, in, size, out, out_capacity, &n, &last) != IGDSP_OK) return IGDSP_EINVAL;
    if (c == IGDSP_SRTP_RESET) resetNext = false;
    return (int)n;
}

int LegSrtpGcm::unprotect(const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity)
{
    if (!ok || !in || !out) return IGDSP_EINVAL;
    uint32_t n = 0;
    const uint32_t c = (resetNext && ctl == IGDSP_SRTP_RUN) ? (uint32_t)IGDSP_SRTP_RESET : ctl;
    if (igdsp_srtp_gcm_unprotect_packet(&state, c, in, size, out, out_capacity, &n, &last) != IGDSP_OK) return IGDSP_EINVAL;
    if (c == IGDSP_SRTP_RESET) resetNext = false;
    return (int)n;
}

// ---- RTCP on one leg, clear or under SRTCP, no context needed
LegRtcp::LegRtcp(uint32_t ssrc_, const char *cname_, const uint8_t *key_salt, const uint8_t *peer_key_salt, uint32_t index0)
    : secure(key_salt && peer_key_salt), ssrc(ssrc_), cnameLen(0)
{
    std::memset(cname, 0, sizeof(cname));
    std::memset(&state, 0, sizeof(state));
    std::memset(&tx, 0, sizeof(tx));                          // no tag word: NO_KEY
    std::memset(&rx, 0, sizeof(rx));
    std::memset(&lastBuilt, 0, sizeof(lastBuilt));
    std::memset(&lastSeen, 0, sizeof(lastSeen));
    std::memset(&lastSrtcp, 0, sizeof(lastSrtcp));
    if (cname_) {
        cnameLen = (uint32_t)std::strlen(cname_);
        if (cnameLen > IGDSP_RTCP_CNAME_MAX) cnameLen = IGDSP_RTCP_CNAME_MAX;
        std::memcpy(cname, cname_, cnameLen);
    }
    if (secure) secure = igdsp_srtcp_derive(key_salt, index0, &tx) == IGDSP_OK && igdsp_srtcp_derive(peer_key_salt, 0, &rx) == IGDSP_OK;
}

int LegRtcp::report(const igdsp_jb_state *jb, uint32_t rtp_ts, uint32_t packets, uint32_t octets, uint64_t now_ntp, bool bye, uint8_t *out, uint32_t out_capacity)
{
    if (!out) return IGDSP_EINVAL;
    const igdsp_rtcp_src src = {ssrc, rtp_ts, packets, octets};
    uint32_t n = 0;
    if (igdsp_rtcp_build_packet(&state, bye ? IGDSP_RTCP_BYE : IGDSP_RTCP_REPORT, jb, &src, now_ntp, cname, cnameLen, out, out_capacity, &n, &lastBuilt) != IGDSP_OK)
        return IGDSP_EINVAL;
    if (secure && igdsp_srtcp_protect_packet(&tx, IGDSP_SRTP_RUN, out, n, out, out_capacity, &n, &lastSrtcp) != IGDSP_OK) return IGDSP_EINVAL;
    return (int)n;
}

int LegRtcp::received(const uint8_t *in, uint32_t size, uint32_t arrival)
{
    if (!in) return IGDSP_EINVAL;
    uint8_t clear[IGDSP_SRTP_MAX_PACKET];
    if (secure) {
        uint32_t n = 0;
        if (igdsp_srtcp_unprotect_packet(&rx, IGDSP_SRTP_RUN, in, size, clear, sizeof(clear), &n, &lastSrtcp) != IGDSP_OK) return IGDSP_EINVAL;
        if (!(lastSrtcp.flags & IGDSP_SRTP_OK)) return 0;
        in = clear;
        size = n;
    }
    if (igdsp_rtcp_parse_packet(&state, in, size, arrival, ssrc, &lastSeen) != IGDSP_OK) return IGDSP_EINVAL;
    return (lastSeen.flags & IGDSP_RTCP_PARSED) ? 1 : 0;
}

void *igdsp_host_rtcp_new(uint32_t ssrc, const char *cname, const uint8_t *key_salt, const uint8_t *peer_key_salt, uint32_t index0)
{
    if ((key_salt == 0) != (peer_key_salt == 0)) return 0;
    LegRtcp *e = new (std::nothrow) LegRtcp(ssrc, cname, key_salt, peer_key_salt, index0);
    if (e && key_salt && !e->secure) { delete e; e = 0; }
    return e;
}
void igdsp_host_rtcp_free(void *v) { delete static_cast<LegRtcp *>(v); }
int igdsp_host_rtcp_report(void *v, const igdsp_jb_state *jb, uint32_t rtp_ts, uint32_t packets, uint32_t octets, uint64_t now_ntp, int bye, uint8_t *out,
                           uint32_t out_capacity)
{
    return v ? static_cast<LegRtcp *>(v)->report(jb, rtp_ts, packets, octets, now_ntp, bye != 0, out, out_capacity) : IGDSP_EINVAL;
}
int igdsp_host_rtcp_received(void *v, const uint8_t *in, uint32_t size, uint32_t arrival)
{
    return v ? static_cast<LegRtcp *>(v)->received(in, size, arrival) : IGDSP_EINVAL;
}
int igdsp_host_rtcp_state(void *v, igdsp_rtcp_state *out)
{
    if (!v || !out) return IGDSP_EINVAL;
    *out = static_cast<LegRtcp *>(v)->state;
    return IGDSP_OK;
}

void *igdsp_host_srtp_new(const uint8_t *key_salt, uint32_t tag_len, uint32_t roc0)
{
    LegSrtp *e = new (std::nothrow) LegSrtp(key_salt, tag_len, roc0);
    if (e && !e->ok) { delete e; e = nullptr; }
    return e;
}
void igdsp_host_srtp_free(void *v) { delete static_cast<LegSrtp *>(v); }
int igdsp_host_srtp_control(void *v, uint32_t ctl)
{
    if (!v || ctl > IGDSP_SRTP_BYPASS) return IGDSP_EINVAL;
    static_cast<LegSrtp *>(v)->ctl = ctl;
    return IGDSP_OK;
}
int igdsp_host_srtp_protect(void *v, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity)
{
    return v ? static_cast<LegSrtp *>(v)->protect(in, size, out, out_capacity) : IGDSP_EINVAL;
}
int igdsp_host_srtp_unprotect(void *v, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity)
{
    return v ? static_cast<LegSrtp *>(v)->unprotect(in, size, out, out_capacity) : IGDSP_EINVAL;
}
int igdsp_host_srtp_rec(void *v, igdsp_srtp_rec *out)
{
    if (!v || !out) return IGDSP_EINVAL;
    *out = static_cast<LegSrtp *>(v)->last;
    return IGDSP_OK;
}
void igdsp_host_srtp_reset(void *v) { if (v) static_cast<LegSrtp *>(v)->reset(); }

void *igdsp_host_srtp_gcm_new(const uint8_t *key_salt, uint32_t key_bytes, uint32_t roc0)
{
    LegSrtpGcm *e = new (std::nothrow) LegSrtpGcm(key_salt, key_bytes, roc0);
    if (e && !e->ok) { delete e; e = nullptr; }
    return e;
}
void igdsp_host_srtp_gcm_free(void *v) { delete static_cast<LegSrtpGcm *>(v); }
int igdsp_host_srtp_gcm_control(void *v, uint32_t ctl)
{
    if (!v || ctl > IGDSP_SRTP_BYPASS) return IGDSP_EINVAL;
    static_cast<LegSrtpGcm *>(v)->ctl = ctl;
    return IGDSP_OK;
}
int igdsp_host_srtp_gcm_protect(void *v, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity)
{
    return v ? static_cast<LegSrtpGcm *>(v)->protect(in, size, out, out_capacity) : IGDSP_EINVAL;
}
int igdsp_host_srtp_gcm_unprotect(void *v, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity)
{
    return v ? static_cast<LegSrtpGcm *>(v)->unprotect(in, size, out, out_capacity) : IGDSP_EINVAL;
}
int igdsp_host_srtp_gcm_rec(void *v, igdsp_srtp_rec *out)
{
    if (!v || !out) return IGDSP_EINVAL;
    *out = static_cast<LegSrtpGcm *>(v)->last;
    return IGDSP_OK;
}
void igdsp_host_srtp_gcm_reset(void *v) { if (v) static_cast<LegSrtpGcm *>(v)->reset(); }

// ---- conference receive levels, no context needed
void *igdsp_host_levels_new(uint32_t n_channels)
{
    ConfLevels *l = new (std::nothrow) ConfLevels(n_channels);
    if (l && l->channels() != n_channels) { delete l; return nullptr; }
    return l;
}
void igdsp_host_levels_free(void *l) { delete static_cast<ConfLevels *>(l); }
int igdsp_host_levels_map_call(void *l, int call_id, uint32_t channel) { return l ? static_cast<ConfLevels *>(l)->mapCall(call_id, channel) : IGDSP_EINVAL; }
int igdsp_host_levels_bind_radio(void *l, int slot, int call_id)
{
    if (!l || slot < 0 || slot > 3) return IGDSP_EINVAL;
    static_cast<ConfLevels *>(l)->radio_call[slot] = call_id;
    return IGDSP_OK;
}
int igdsp_host_levels_set(void *l, float slot_volume, float sidetone)
{
    if (!l) return IGDSP_EINVAL;
    static_cast<ConfLevels *>(l)->SLOT_VOLUME = slot_volume;
    static_cast<ConfLevels *>(l)->sidetone = sidetone;
    return IGDSP_OK;
}
float igdsp_host_levels_slot_volume(void *l) { return l ? static_cast<ConfLevels *>(l)->SLOT_VOLUME : -1.0f; }
int igdsp_host_set_slot_volume(void *l, int call_id, int increase, int current)
{
    return l && static_cast<ConfLevels *>(l)->setSlotVolume(call_id, increase != 0, current != 0) ? 1 : 0;
}
int igdsp_host_set_volume_sidetone(void *l, int call_id)
{
    if (!l) return IGDSP_EINVAL;
    static_cast<ConfLevels *>(l)->setvolumeSiteTone(call_id);
    return IGDSP_OK;
}
const uint16_t *igdsp_host_levels_gains(void *l) { return l ? static_cast<ConfLevels *>(l)->gains() : nullptr; }
