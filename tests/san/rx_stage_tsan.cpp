// ThreadSanitizer harness for csrc/igdsp_rxstage.h (the drop-in receive path's staging) and csrc/igdsp_snappool.h: four producer
// threads stage frames — producers 0 and 1 on the same channels, 2 and 3 on channels of their own — a setter thread changes every
// channel's ED-137 word, and one owner thread snapshots repeatedly, split into 4 parts over a real pool of 3 helper threads.
// Each payload carries its producer, channel and sequence number.  Checks: every staged frame was taken by exactly one snapshot
// or overwritten and counted as dropped, each producer's frames keep their order per channel, frames_seen + dropped == staged,
// and every frame carries a word the setter wrote (never decreasing per producer and channel).  The published double buffer is
// not driven here: its writer is a DMA engine, whose overlap with a reader the seqlock allows by design.
// Built and run by tests/test_rx_stage_tsan_cpu.py; test infrastructure only.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "igdsp_rxstage.h"

using namespace igdsp_rx;

static constexpr uint32_t kChannels = 32, kShared = 16, kProducers = 4, kFrames = 1500, kWords = 300;
static constexpr uint32_t kWordBase = 0x5A000000u;

// producer p stages on channels [lo, hi)
static void channels_of(uint32_t p, uint32_t *lo, uint32_t *hi)
{
    if (p < 2) { *lo = 0; *hi = kShared; }
    else { *lo = kShared + (p - 2) * (kChannels - kShared) / 2; *hi = *lo + (kChannels - kShared) / 2; }
}

struct Frame { uint32_t producer, seq, word; };

int main()
{
    RingMem ring;
    std::vector<std::unique_ptr<uint8_t[]>> mem;
    for (int i = 0; i < RingMem::kArrays; ++i) {
        mem.emplace_back(new uint8_t[RingMem::bytes(kChannels, i)]());
        *ring.array(i) = mem.back().get();
    }
    Stager st;
    st.init(kChannels, ring);
    std::vector<uint32_t> staged(kChannels, 0);
    for (uint32_t p = 0; p < kProducers; ++p) {
        uint32_t lo, hi;
        channels_of(p, &lo, &hi);
        for (uint32_t c = lo; c < hi; ++c) staged[c] += kFrames;
    }

    std::atomic<uint32_t> producers_left{kProducers};
    std::vector<std::thread> th;
    for (uint32_t p = 0; p < kProducers; ++p)
        th.emplace_back([&, p] {
            uint32_t lo, hi;
            channels_of(p, &lo, &hi);
            uint8_t pay[kSlot];
            for (uint32_t s = 0; s < kFrames; ++s, std::this_thread::yield())   // a tick's worth per round: most frames reach a snapshot
                for (uint32_t c = lo; c < hi; ++c) {
                    const uint32_t len = (s + c) % 5 == 0 ? 24u + (s % 200u) : 160u;   // both groups
                    std::memset(pay, 0xEE, len);
                    pay[0] = (uint8_t)p; pay[1] = (uint8_t)c;
                    std::memcpy(pay + 2, &s, 4);
                    const int rc = st.stage(c, (s & 1) ? 8 : 0, pay, len);
                    if (rc != IGDSP_OK && rc != IGDSP_EBUSY) { std::printf("stage rc %d\n", rc); std::abort(); }
                }
            producers_left.fetch_sub(1);
        });
    th.emplace_back([&] {                                      // setter: words kWordBase + 1, + 2, ... on every channel
        for (uint32_t v = 1; v <= kWords; ++v)
            for (uint32_t c = 0; c < kChannels; ++c) st.set_word(c, kWordBase + v);
    });

    // the owner thread: snapshots split into 4 parts over a pool of 3 helpers
    igdsp::SnapshotPool pool(3);
    const UploadLayout L = upload_layout((size_t)kChannels * kStageDepth, kChannels);
    std::vector<uint8_t> up(L.total);
    std::vector<std::vector<Frame>> got(kChannels);
    uint32_t snapshots = 0;
    auto snapshot = [&] {
        const uint32_t nch = st.channels_seen();
        SnapPart parts[igdsp::kMaxParts];
        const uint32_t n = igdsp::for_each_part(&pool, nch, [&](uint32_t i, uint32_t c0, uint32_t c1) {
            parts[i].c0 = c0;
            parts[i].c1 = c1;
            st.snapshot(parts[i], up.data(), L);
        });
        if (nch && n != 4) { std::printf("%u parts\n", n); std::abort(); }
        ++snapshots;
        const uint32_t *seq = reinterpret_cast<const uint32_t *>(up.data() + L.seq), *runs = reinterpret_cast<const uint32_t *>(up.data() + L.runs);
        const uint16_t *lenB = reinterpret_cast<const uint16_t *>(up.data() + L.lenB);
        for (uint32_t c = 0; c < nch; ++c)
            for (uint32_t k = runs[2 * c]; k < runs[2 * c] + runs[2 * c + 1]; ++k) {
                const uint32_t id = seq[2 * (size_t)k], b = id & kRecB ? 1u : 0u, i = id & ~kRecB;
                const uint8_t *pay = b ? up.data() + L.payB + (size_t)i * kSlot : up.data() + L.payA + (size_t)i * IGDSP_SAMPLES_PER_FRAME;
                const uint8_t pt = b ? up[L.ptB + i] : up[L.ptA + i];
                const uint32_t len = b ? lenB[i] : IGDSP_SAMPLES_PER_FRAME;
                Frame f{pay[0], 0, seq[2 * (size_t)k + 1]};
                std::memcpy(&f.seq, pay + 2, 4);
                const uint32_t want_len = (f.seq + c) % 5 == 0 ? 24u + (f.seq % 200u) : 160u;
                if (pay[1] != c || f.producer >= kProducers || len != want_len || pt != ((f.seq & 1) ? 8 : 0) || pay[len - 1] != 0xEE ||
                    (b != 0) != (len != IGDSP_SAMPLES_PER_FRAME)) {
                    std::printf("bad frame on channel %u\n", c); std::abort();
                }
                got[c].push_back(f);
            }
    };
    while (producers_left.load() != 0) snapshot();
    for (auto &t : th) t.join();
    snapshot();

    uint64_t total = 0, dropped = 0;
    for (uint32_t c = 0; c < kChannels; ++c) {
        std::vector<std::vector<uint8_t>> taken(kProducers, std::vector<uint8_t>(kFrames, 0));
        std::vector<int64_t> last_seq(kProducers, -1);
        std::vector<uint32_t> last_word(kProducers, 0);
        for (const Frame &f : got[c]) {
            if (f.seq >= kFrames || taken[f.producer][f.seq]) { std::printf("channel %u: frame taken twice or never staged\n", c); return 1; }
            taken[f.producer][f.seq] = 1;
            if ((int64_t)f.seq <= last_seq[f.producer]) { std::printf("channel %u: producer %u reordered\n", c, f.producer); return 1; }
            last_seq[f.producer] = f.seq;
            if (f.word != 0 && (f.word <= kWordBase || f.word > kWordBase + kWords)) { std::printf("channel %u: word %08x never set\n", c, f.word); return 1; }
            if (f.word < last_word[f.producer]) { std::printf("channel %u: word went back\n", c); return 1; }
            last_word[f.producer] = f.word;
        }
        const uint32_t seen = st.frames_seen(c), drop = st.frames_dropped(c);
        if (seen != got[c].size() || seen + drop != staged[c]) {
            std::printf("channel %u: seen %u (taken %zu) + dropped %u != staged %u\n", c, seen, got[c].size(), drop, staged[c]);
            return 1;
        }
        total += seen;
        dropped += drop;
    }
    std::printf("rx stage ok: %llu frames taken in %u snapshots, %llu dropped\n", (unsigned long long)total, snapshots, (unsigned long long)dropped);
    return 0;
}
