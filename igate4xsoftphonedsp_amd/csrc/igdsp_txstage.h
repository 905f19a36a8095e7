// igdsp_txstage.h — the staging half of the ED-137 send path (igdsp_on_tx_frame / igdsp_tx_set_* / igdsp_tx_flush): per-leg
// single-producer rings of pjmedia stream packets, the pending setter word, and the flush's snapshot into one compacted upload
// block.  Host-only C++17, no HIP include: igdsp_capi_tx.hip uses it, and tests/san/tx_stage_tsan.cpp drives it under ThreadSanitizer.
//
// One producer per leg (pjmedia serialises send_rtp per stream), one consumer (the flush's owner thread).  Staging is wait-free:
// no lock or spin flag, only the leg's own head / tail and setter word.
//   head   frames the producer has published (written only by the producer, release)
//   tail   frames the consumer has taken (written only by the consumer, release); head - tail <= kTxDepth
//   setw   the leg's pending setter values and their dirty bits in one 64-bit word.  A setter ORs its values in (CAS); staging a
//          frame exchanges the word for 0 and carries it in the frame's record, so a setter lands on exactly one frame: the first
//          one staged after it, or the next one if the two race.  Setters after the last staged frame wait for the next one.
// A full ring refuses the NEW frame (IGDSP_EBUSY, counted in `refused`): dropping the oldest would need the producer to move tail.
#pragma once
#include "igdsp.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>

namespace igdsp_tx {

constexpr uint32_t kTxDepth = IGDSP_STAGE_DEPTH;   // frames a leg can stage between two flushes
constexpr uint32_t kTxMaxN = IGDSP_TX_MAX_N;        // send_pkt_buff[256] holds 20 + n (TransportAdapter.h:69)
constexpr uint32_t kTxStreamMax = 12 + kTxMaxN;     // stream packet: 12-byte RTP header + n G.711 bytes
constexpr uint32_t kTxSlot = 256;                   // output slot per frame (packet bytes [0, size))

// ---- the setter word (also the low 48 bits of an upload record's `word`) ----
// values
constexpr uint64_t kSwPtt = 1ull << 0, kSwSql = 1ull << 1, kSwRec = 1ull << 2, kSwSlaveRx = 1ull << 3, kSwSlaveTx = 1ull << 4;
constexpr int kSwCtShift = 5;                       // 3 bits: IGDSP_TX_CT_*
constexpr int kSwPrioShift = 8, kSwBssiShift = 16, kSwPttIdShift = 24;   // 8 bits each
// dirty bits: which fields the frame's step assigns before it runs
constexpr uint64_t kSdPtt = 1ull << 32;             // ptt + pttpriority           setAdapterPtt
constexpr uint64_t kSdRec = 1ull << 33;             // call_recorder              setAdapterPtt (userRec), setcallRecorder
constexpr uint64_t kSdSql = 1ull << 34;             // sql                        setAdapterQslOn
constexpr uint64_t kSdBssi = 1ull << 35;            // bssi                       setAdapterQslOn, 4-argument overload
constexpr uint64_t kSdPttId = 1ull << 36;           // pttid                      setAdapterPttId
constexpr uint64_t kSdSlave = 1ull << 37;           // rx / tx_slave_changed, slave_count = 0   setTxRxSlaveEnable
constexpr uint64_t kSdCt = 1ull << 38;              // calltype bits              setCallType
constexpr uint64_t kSwMask = (1ull << 39) - 1u;
constexpr int kRecNShift = 48;                      // upload record: n in bits 48..55 of `word`

// the value bits each dirty bit owns (a later setter of the same field replaces them)
inline uint64_t setter_fields(uint64_t dirty)
{
    uint64_t m = 0;
    if (dirty & kSdPtt) m |= kSwPtt | 0xFFull << kSwPrioShift;
    if (dirty & kSdRec) m |= kSwRec;
    if (dirty & kSdSql) m |= kSwSql;
    if (dirty & kSdBssi) m |= 0xFFull << kSwBssiShift;
    if (dirty & kSdPttId) m |= 0xFFull << kSwPttIdShift;
    if (dirty & kSdSlave) m |= kSwSlaveRx | kSwSlaveTx;
    if (dirty & kSdCt) m |= 7ull << kSwCtShift;
    return m;
}

// Apply a setter word to a leg state (the device does the same in k_tx_staged; tests/tx_stage_model.py restates it).
inline void apply_setters(igdsp_tx_chan &s, uint64_t w)
{
    if (w & kSdPtt) { s.ptt = (w & kSwPtt) ? 1 : 0; s.pttpriority = (uint8_t)(w >> kSwPrioShift); }
    if (w & kSdRec) s.call_recorder = (w & kSwRec) ? 1 : 0;
    if (w & kSdSql) s.sql = (w & kSwSql) ? 1 : 0;
    if (w & kSdBssi) s.bssi = (uint8_t)(w >> kSwBssiShift);
    if (w & kSdPttId) s.pttid = (uint8_t)(w >> kSwPttIdShift);
    if (w & kSdSlave) { s.rx_slave_changed = (w & kSwSlaveRx) ? 1 : 0; s.tx_slave_changed = (w & kSwSlaveTx) ? 1 : 0; s.slave_count = 0; }
    if (w & kSdCt) s.calltype = (uint8_t)((w >> kSwCtShift) & 7u);
}

// ---- the upload block of one flush ----
// [runs: n_runs x TxRun][records: n_frames x TxRec][stream dwords], every section 256-byte aligned.  A run is one leg's staged
// frames, legs in channel order; its records are consecutive, frames in staging order, and each frame's 12 + n stream bytes sit at
// a dword offset of their own, rounded up to 4 bytes.
struct TxRun { uint32_t leg, first, count, off_dw; };       // first record, frames, dword offset of the first frame's stream bytes
struct TxRec { uint64_t now_ms, word; };                    // word = setter word | n << kRecNShift
static_assert(sizeof(TxRun) == 16 && sizeof(TxRec) == 16, "16-byte upload records");
constexpr uint32_t stream_dwords(uint32_t n) { return (12u + n + 3u) / 4u; }
struct TxUploadLayout { size_t runs, recs, bytes, total; };
inline TxUploadLayout upload_layout(size_t n_runs, size_t n_frames, size_t n_dwords)
{
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    TxUploadLayout L;
    L.runs = 0;
    L.recs = up(n_runs * sizeof(TxRun));
    L.bytes = L.recs + up(n_frames * sizeof(TxRec));
    L.total = L.bytes + up(n_dwords * 4u);
    return L;
}
// The download block: [info: n_frames x igdsp_tx_info][chan: n_runs x igdsp_tx_chan][packets: n_frames x kTxSlot]
struct TxOutLayout { size_t info, chan, pkts, total; };
inline TxOutLayout out_layout(size_t n_runs, size_t n_frames)
{
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    TxOutLayout L;
    L.info = 0;
    L.chan = up(n_frames * sizeof(igdsp_tx_info));
    L.pkts = L.chan + up(n_runs * sizeof(igdsp_tx_chan));
    L.total = L.pkts + n_frames * (size_t)kTxSlot;
    return L;
}

// What pjmedia's own stream hands over: RTP version 2, no padding, no extension, no CSRC (first byte exactly 0x80), 1 <= n <= 236.
inline bool stream_packet_ok(const uint8_t *pkt, uint32_t size)
{
    return pkt && size >= 13u && size <= kTxStreamMax && pkt[0] == 0x80u;
}

class Stager {
public:
    bool init(uint32_t legs)
    {
        legs_ = legs;
        head_.reset(new (std::nothrow) std::atomic<uint32_t>[legs]);
        tail_.reset(new (std::nothrow) std::atomic<uint32_t>[legs]);
        setw_.reset(new (std::nothrow) std::atomic<uint64_t>[legs]);
        refused_.reset(new (std::nothrow) std::atomic<uint32_t>[legs]);
        dropped_.reset(new (std::nothrow) std::atomic<uint32_t>[legs]);
        open_.reset(new (std::nothrow) std::atomic<uint32_t>[legs]);
        rec_.reset(new (std::nothrow) TxRec[(size_t)legs * kTxDepth]);
        bytes_.reset(new (std::nothrow) uint8_t[(size_t)legs * kTxDepth * kTxStreamMax]);   // not value-initialised: pages on first use
        snap_.reset(new (std::nothrow) uint32_t[legs]);
        if (!head_ || !tail_ || !setw_ || !refused_ || !dropped_ || !open_ || !rec_ || !bytes_ || !snap_) return false;
        for (uint32_t l = 0; l < legs; ++l) {
            head_[l].store(0, std::memory_order_relaxed); tail_[l].store(0, std::memory_order_relaxed);
            setw_[l].store(0, std::memory_order_relaxed); refused_[l].store(0, std::memory_order_relaxed);
            dropped_[l].store(0, std::memory_order_relaxed); open_[l].store(0, std::memory_order_relaxed);
        }
        return true;
    }
    uint32_t legs() const { return legs_; }
    bool is_open(uint32_t leg) const { return open_[leg].load(std::memory_order_acquire) != 0; }

    // ---- producer side (any thread; one at a time per leg) ----
    int stage(uint32_t leg, const uint8_t *pkt, uint32_t size, uint64_t now_ms)
    {
        if (!stream_packet_ok(pkt, size)) return IGDSP_EINVAL;
        if (!is_open(leg)) return IGDSP_ENOENT;
        const uint32_t h = head_[leg].load(std::memory_order_relaxed);
        if (h - tail_[leg].load(std::memory_order_acquire) >= kTxDepth) {
            refused_[leg].fetch_add(1, std::memory_order_relaxed);
            return IGDSP_EBUSY;
        }
        const size_t slot = (size_t)leg * kTxDepth + h % kTxDepth;
        std::memcpy(bytes_.get() + slot * kTxStreamMax, pkt, size);
        const uint64_t w = setw_[leg].exchange(0, std::memory_order_acq_rel);
        rec_[slot] = TxRec{now_ms, (w & kSwMask) | (uint64_t)(size - 12u) << kRecNShift};
        head_[leg].store(h + 1, std::memory_order_release);
        return IGDSP_OK;
    }
    // a setter: `dirty` names the fields (kSd*), `values` carries them in setter-word positions
    int set(uint32_t leg, uint64_t dirty, uint64_t values)
    {
        if (!is_open(leg)) return IGDSP_ENOENT;
        const uint64_t m = setter_fields(dirty);
        uint64_t w = setw_[leg].load(std::memory_order_relaxed);
        while (!setw_[leg].compare_exchange_weak(w, (w & ~m) | (values & m) | dirty, std::memory_order_acq_rel, std::memory_order_relaxed)) {}
        return IGDSP_OK;
    }
    uint32_t refused(uint32_t leg) const { return refused_[leg].load(std::memory_order_relaxed); }
    uint32_t dropped(uint32_t leg) const { return dropped_[leg].load(std::memory_order_relaxed); }

    // ---- consumer side (the owner thread) ----
    // open: staged leftovers and pending setters of an earlier leg on this channel are dropped; close: the staged frames are
    // dropped (counted).  A producer must not race with either on the same leg (pjmedia stops the stream before its transport).
    void open(uint32_t leg)
    {
        discard(leg);
        setw_[leg].store(0, std::memory_order_relaxed);
        refused_[leg].store(0, std::memory_order_relaxed);
        dropped_[leg].store(0, std::memory_order_relaxed);
        open_[leg].store(1, std::memory_order_release);
    }
    void close(uint32_t leg)
    {
        open_[leg].store(0, std::memory_order_release);
        discard(leg);
    }

    struct Counts { uint32_t runs = 0, frames = 0, dwords = 0; };
    // Snapshot pass 1 over legs [l0, l1): fixes each open leg's head for pass 2 and counts what it will emit.
    Counts count(uint32_t l0, uint32_t l1)
    {
        Counts c;
        for (uint32_t l = l0; l < l1; ++l) {
            uint32_t k = 0;
            if (open_[l].load(std::memory_order_acquire)) {
                const uint32_t h = head_[l].load(std::memory_order_acquire), t = tail_[l].load(std::memory_order_relaxed);
                k = h - t;
                for (uint32_t i = 0; i < k; ++i) c.dwords += stream_dwords(rec_n((size_t)l * kTxDepth + (t + i) % kTxDepth));
                snap_[l] = h;
            }
            if (k == 0) snap_[l] = tail_[l].load(std::memory_order_relaxed);
            c.runs += k ? 1u : 0u;
            c.frames += k;
        }
        return c;
    }
    // Snapshot pass 2 over the same legs: runs, records and stream bytes into the upload block at the given bases (this part's
    // share of each section), then the frames are released to their producers.
    void emit(uint32_t l0, uint32_t l1, uint8_t *up, const TxUploadLayout &L, Counts base)
    {
        TxRun *runs = reinterpret_cast<TxRun *>(up + L.runs);
        TxRec *recs = reinterpret_cast<TxRec *>(up + L.recs);
        uint32_t *dw = reinterpret_cast<uint32_t *>(up + L.bytes);
        for (uint32_t l = l0; l < l1; ++l) {
            const uint32_t t = tail_[l].load(std::memory_order_relaxed), h = snap_[l], k = h - t;
            if (k == 0) continue;
            runs[base.runs++] = TxRun{l, base.frames, k, base.dwords};
            for (uint32_t i = 0; i < k; ++i) {
                const size_t slot = (size_t)l * kTxDepth + (t + i) % kTxDepth;
                const uint32_t n = rec_n(slot), nd = stream_dwords(n);
                recs[base.frames++] = rec_[slot];
                dw[base.dwords + nd - 1u] = 0;                       // the rounding bytes of the last dword
                std::memcpy(dw + base.dwords, bytes_.get() + slot * kTxStreamMax, 12u + n);
                base.dwords += nd;
            }
            tail_[l].store(h, std::memory_order_release);
        }
    }

private:
    uint32_t rec_n(size_t slot) const { return (uint32_t)(rec_[slot].word >> kRecNShift) & 0xFFu; }
    void discard(uint32_t leg)
    {
        const uint32_t h = head_[leg].load(std::memory_order_acquire), t = tail_[leg].load(std::memory_order_relaxed);
        if (h != t) dropped_[leg].fetch_add(h - t, std::memory_order_relaxed);
        tail_[leg].store(h, std::memory_order_release);
    }

    uint32_t legs_ = 0;
    std::unique_ptr<std::atomic<uint32_t>[]> head_, tail_, refused_, dropped_, open_;
    std::unique_ptr<std::atomic<uint64_t>[]> setw_;
    std::unique_ptr<TxRec[]> rec_;
    std::unique_ptr<uint8_t[]> bytes_;
    std::unique_ptr<uint32_t[]> snap_;                 // pass 1 -> pass 2: each leg's head as pass 1 saw it
};

}  // namespace igdsp_tx
