// igdsp_rxstage.h — the staging half of the drop-in receive path (igdsp_on_rtp_frame / igdsp_set_ed137 / igdsp_flush_begin /
// igdsp_flush_end / igdsp_poll): per-channel rings of received frames, the flush's snapshot into one compacted upload block, and
// the double buffer the flush publishes its results in.  Host-only C++17, no HIP include: igdsp_capi_ctx.hip uses it (and allocates
// the pinned memory both halves work in), tests/rxstage/rx_stage_driver.cpp checks the upload block it builds, and
// tests/san/rx_stage_tsan.cpp drives the staging under ThreadSanitizer.
//
// Any number of producers per channel (a call's frames may arrive on more than one media thread), one consumer (the flush's
// owner thread, its snapshot possibly shared out to a SnapshotPool, one channel range per thread).  Each channel's ring is
// guarded by its own spin flag, held for one <= 256-byte copy:
//   lock     the channel's flag: taken with acquire and released with release, by a producer around one frame and by the
//            snapshot around one channel.  head and tail are plain words read and written only under it.
//   head     frames written; tail frames taken by a flush or overwritten (head - tail <= kStageDepth).  A producer that finds the
//            ring full moves tail itself: the OLDEST frame is overwritten and counted in `dropped`, and stage says IGDSP_EBUSY.
//   cur      the word frames staged from now on carry (set_word, relaxed; a producer reads it relaxed under the flag).
//   seen / dropped   counters, relaxed: frames taken by a flush (snapshot) / overwritten before one took them (stage).
//   hi_water 1 + the highest channel ever staged (relaxed CAS after the flag is released): the channels a flush walks.
// The published double buffer (Published / PublishedSet below) has its own rules, written there.
#pragma once
#include "igdsp.h"
#include "igdsp_snappool.h"

#include <atomic>
#include <cstdint>
#include <cstring>
#include <vector>

namespace igdsp_rx {

constexpr uint32_t kSlot = IGDSP_MAX_PAYLOAD;          // staging slot bytes (tp_adapter::payload_buff[256])
constexpr uint32_t kStageDepth = IGDSP_STAGE_DEPTH;    // frames per channel between two flushes (8 x 20 ms)
constexpr uint32_t kRecB = 0x80000000u;                // seq entry of a group B frame: record id | kRecB

// Layout of the flush upload block (same offsets in the pinned host copy and in its device mirror; every section starts on
// a 256-byte boundary).  Group A = whole 160-byte frames, dense at stride 160 (the tuned chunk kernel's layout); group B =
// every other length, slots of 256 bytes with a length per frame (the general kernel).  seq = every staged frame in the
// order its channel received it: {record id (group B: | 0x80000000), ED-137 word}; runs[c] = {first seq entry, count} of
// channel c (count 0: nothing staged).
struct UploadLayout { size_t payA, payB, lenB, ptA, ptB, seq, runs, total; };
inline UploadLayout upload_layout(size_t max_frames, size_t max_channels)
{
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    UploadLayout L;
    size_t o = 0;
    L.payA = o; o = up(o + max_frames * IGDSP_SAMPLES_PER_FRAME);
    L.payB = o; o = up(o + max_frames * kSlot);
    L.lenB = o; o = up(o + max_frames * sizeof(uint16_t));
    L.ptA = o;  o = up(o + max_frames);
    L.ptB = o;  o = up(o + max_frames);
    L.seq = o;  o = up(o + max_frames * 2 * sizeof(uint32_t));
    L.runs = o; o = up(o + max_channels * 2 * sizeof(uint32_t));
    L.total = o;
    return L;
}

// What one snapshot worker found in its channel range [c0, c1): its frames sit in ITS region of every section (frame index
// c0 * kStageDepth onwards), so workers never touch each other's bytes.
struct SnapPart { uint32_t c0 = 0, c1 = 0, nA = 0, nB = 0, nSeq = 0; };

// The ring storage, owned by the caller (the C API keeps it in pinned memory: the flush copies out of it): kStageDepth slots per
// channel, slot-major — the frames all calls staged at the same tick position sit next to each other, so the snapshot reads each
// slot plane sequentially.  tp_adapter::payload_buff[256] semantics per slot (TransportAdapter.h:66): the reference's hook runs
// on EVERY frame (TransportAdapter.cpp:303), so every frame is kept.
struct RingMem {
    uint8_t *pay = nullptr;                             // [slot][channel][kSlot]
    uint16_t *len = nullptr;                            // [slot][channel] payload bytes
    uint8_t *pt = nullptr;                              // [slot][channel] RTP payload type
    uint32_t *word = nullptr;                           // [slot][channel] the call's ED-137 word when the frame was staged
    static constexpr int kArrays = 4;
    void **array(int i) { void **a[kArrays] = {(void **)&pay, (void **)&len, (void **)&pt, (void **)&word}; return a[i]; }
    static size_t bytes(uint32_t channels, int i)       // bytes of array i for `channels` channels
    {
        constexpr size_t per_frame[kArrays] = {kSlot, sizeof(uint16_t), 1, sizeof(uint32_t)};
        return (size_t)channels * kStageDepth * per_frame[i];
    }
};

class Stager {
public:
    // `ring` must hold RingMem::bytes(channels, i) bytes per array and outlive the stager.
    void init(uint32_t channels, const RingMem &ring)
    {
        channels_ = channels;
        ring_ = ring;
        lock_ = std::vector<std::atomic_flag>(channels);
        for (auto &f : lock_) f.clear();
        cur_ = std::vector<std::atomic<uint32_t>>(channels);
        seen_ = std::vector<std::atomic<uint32_t>>(channels);
        dropped_ = std::vector<std::atomic<uint32_t>>(channels);
        for (uint32_t c = 0; c < channels; ++c) { cur_[c].store(0); seen_[c].store(0); dropped_[c].store(0); }
        head_.assign(channels, 0);
        tail_.assign(channels, 0);
    }

    // ---- producer side (any thread, any number per channel) ----
    // One frame of 0 < len <= kSlot bytes for channel ch (len 0: nothing staged).  IGDSP_EBUSY: staged, but the owner thread is
    // > 160 ms late and the channel's oldest frame was overwritten.
    int stage(uint32_t ch, uint8_t pt, const uint8_t *payload, uint32_t len)
    {
        if (len == 0) return IGDSP_OK;
        lock(ch);                                                            // held by another producer / the flush for one <= 256-byte copy
        int rc = IGDSP_OK;
        if (head_[ch] - tail_[ch] == kStageDepth) {                          // the owner thread is > 160 ms late: the oldest frame goes
            tail_[ch] += 1;
            dropped_[ch].fetch_add(1, std::memory_order_relaxed);
            rc = IGDSP_EBUSY;
        }
        const size_t slot = (size_t)(head_[ch] % kStageDepth) * channels_ + ch;   // slot-major: the flush walks each slot plane sequentially
        std::memcpy(ring_.pay + slot * kSlot, payload, len);
        ring_.len[slot] = (uint16_t)len;
        ring_.pt[slot] = pt;
        ring_.word[slot] = cur_[ch].load(std::memory_order_relaxed);
        head_[ch] += 1;
        unlock(ch);
        uint32_t hw = hi_water_.load(std::memory_order_relaxed);
        while (hw < ch + 1 && !hi_water_.compare_exchange_weak(hw, ch + 1, std::memory_order_relaxed)) {}
        return rc;
    }
    // setIncomingED137Value (roip_ed137.h:273): the word the channel's frames carry from now on
    void set_word(uint32_t ch, uint32_t w) { cur_[ch].store(w, std::memory_order_relaxed); }

    uint32_t channels_seen() const { return hi_water_.load(std::memory_order_relaxed); }
    uint32_t frames_seen(uint32_t ch) const { return seen_[ch].load(std::memory_order_relaxed); }
    uint32_t frames_dropped(uint32_t ch) const { return dropped_[ch].load(std::memory_order_relaxed); }

    // ---- consumer side (the owner thread, or one pool thread per part) ----
    // One worker's share of the snapshot: every channel of [part.c0, part.c1), staged frames oldest first, compacted into the
    // worker's own region of the upload block `up`, under the channel's flag.
    void snapshot(SnapPart &part, uint8_t *up, const UploadLayout &L)
    {
        uint16_t *lenB = reinterpret_cast<uint16_t *>(up + L.lenB);
        uint32_t *seq = reinterpret_cast<uint32_t *>(up + L.seq), *runs = reinterpret_cast<uint32_t *>(up + L.runs);
        const uint32_t base = part.c0 * kStageDepth;                       // first frame index of this worker's regions
        uint32_t nA = 0, nB = 0, nS = 0;
        for (uint32_t c = part.c0; c < part.c1; ++c) {
            lock(c);
            const uint32_t t0 = tail_[c], h0 = head_[c];
            const uint32_t s0 = nS;
            for (uint32_t k = t0; k != h0; ++k) {
                const size_t slot = (size_t)(k % kStageDepth) * channels_ + c;
                const uint16_t l = ring_.len[slot];
                uint32_t id;
                if (l == IGDSP_SAMPLES_PER_FRAME) {
                    id = base + nA++;
                    std::memcpy(up + L.payA + (size_t)id * IGDSP_SAMPLES_PER_FRAME, ring_.pay + slot * kSlot, l);
                    up[L.ptA + id] = ring_.pt[slot];
                } else {
                    const uint32_t ib = base + nB++;
                    std::memcpy(up + L.payB + (size_t)ib * kSlot, ring_.pay + slot * kSlot, l);
                    lenB[ib] = l;
                    up[L.ptB + ib] = ring_.pt[slot];
                    id = ib | kRecB;
                }
                seq[2 * (size_t)(base + nS)] = id;
                seq[2 * (size_t)(base + nS) + 1] = ring_.word[slot];
                ++nS;
            }
            tail_[c] = h0;
            unlock(c);
            runs[2 * (size_t)c] = base + s0;
            runs[2 * (size_t)c + 1] = nS - s0;
            if (h0 != t0) seen_[c].fetch_add(h0 - t0, std::memory_order_relaxed);
        }
        part.nA = nA; part.nB = nB; part.nSeq = nS;
    }

private:
    void lock(uint32_t ch) { while (lock_[ch].test_and_set(std::memory_order_acquire)) igdsp::cpu_relax(); }
    void unlock(uint32_t ch) { lock_[ch].clear(std::memory_order_release); }

    uint32_t channels_ = 0;
    RingMem ring_;
    std::vector<uint32_t> head_, tail_;
    std::vector<std::atomic<uint32_t>> cur_;
    std::vector<std::atomic_flag> lock_;
    std::atomic<uint32_t> hi_water_{0};
    std::vector<std::atomic<uint32_t>> seen_, dropped_;
};

// ---- what the flush publishes ----
// Each flush writes {newest record, hold, probe} of every channel into the BACK set of two pinned host sets (by DMA: the device's
// download), flush_end makes it the front set (flip), and the poll entries copy out of the front set without taking the flush's
// mutex (read).  The owner allocates the sets; everything but read() runs on the owner thread, under its mutex.
//   front  which set the readers read (release in flip, acquire in read).
//   seq    a sequence counter: +2 with every flip, odd while rewrite_front changes the front set in place.  A reader retries when it
//          moved under its copy, and waits while it is odd.
struct Published { igdsp_frame_stats *last; igdsp_chan_hold *hold; igdsp_chan_probe *probe; };

class PublishedSet {
public:
    Published &set(uint32_t i) { return pub_[i]; }                     // the owner: allocation, the first fill, free
    Published &back() { return pub_[front_.load(std::memory_order_relaxed) ^ 1u]; }
    uint64_t sequence() const { return seq_.load(std::memory_order_acquire); }

    // Read one channel's published state: copy out of the front set, retry if a flip moved it meanwhile (two flushes would
    // have to complete within the copy of ~60 bytes for a second retry).
    template <typename Fn>
    void read(Fn &&fn) const
    {
        for (;;) {
            const uint64_t s1 = seq_.load(std::memory_order_acquire);
            if (s1 & 1u) { igdsp::cpu_relax(); continue; }                   // rewrite_front is rewriting the front set
            fn(static_cast<const Published &>(pub_[front_.load(std::memory_order_acquire)]));
            std::atomic_thread_fence(std::memory_order_acquire);
            if (seq_.load(std::memory_order_relaxed) == s1) return;
        }
    }
    // The back set is complete: make it the front set.  Readers that were half way through the old one notice seq moving.
    void flip()
    {
        front_.store(front_.load(std::memory_order_relaxed) ^ 1u, std::memory_order_release);
        seq_.fetch_add(2, std::memory_order_release);
    }
    // Change the front set in place: fn(front, back) runs with seq odd, so readers wait instead of copying a half-written state.
    template <typename Fn>
    void rewrite_front(Fn &&fn)
    {
        const uint32_t f = front_.load(std::memory_order_relaxed);
        seq_.fetch_add(1, std::memory_order_acq_rel);                       // odd: readers wait
        fn(pub_[f], static_cast<const Published &>(pub_[f ^ 1u]));
        seq_.fetch_add(1, std::memory_order_release);
    }

private:
    Published pub_[2] = {};
    std::atomic<uint32_t> front_{0};
    std::atomic<uint64_t> seq_{0};
};

}  // namespace igdsp_rx
