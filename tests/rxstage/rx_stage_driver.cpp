// Drives csrc/igdsp_rxstage.h for tests/test_rx_stage_cpu.py.  One command per stdin line:
//   init <channels>                      a fresh stager over plain heap ring memory
//   word <ch> <w>                        set_word
//   stage <ch> <pt> <len> <tag>          one frame, payload byte i = (tag + i) & 0xFF; prints "rc <code>"
//   snap <parts>                         one snapshot, split over a real SnapshotPool of parts - 1 helpers (1: none), into a zeroed
//                                        upload block; prints the parts and the used span of every section (below)
//   counts                               "count <ch> <frames_seen> <frames_dropped>" per channel seen
//   pubtest                              the PublishedSet checks; prints "pub ok" or what failed
// A snap prints "snap <nch> <parts>", one "part <c0> <c1> <nA> <nB> <nSeq>" per part, then each section from its start to the end
// of the last part's share: "payA <hex>", "ptA <hex>", "payB <hex>", "lenB <u16 ...>", "ptB <hex>", "seq <u32 ...>", "runs <u32 ...>".
#include <atomic>
#include <chrono>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "igdsp_rxstage.h"

using namespace igdsp_rx;

static void hex(const char *name, const uint8_t *p, size_t n)
{
    std::printf("%s ", name);
    for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
    std::printf("\n");
}
template <typename T>
static void ints(const char *name, const T *p, size_t n)
{
    std::printf("%s", name);
    for (size_t i = 0; i < n; ++i) std::printf(" %u", (unsigned)p[i]);
    std::printf("\n");
}

static int pubtest()
{
    igdsp_frame_stats last[2] = {};
    igdsp_chan_hold hold[2] = {};
    igdsp_chan_probe probe[2] = {};
    PublishedSet pub;
    for (uint32_t i = 0; i < 2; ++i) {
        pub.set(i) = Published{&last[i], &hold[i], &probe[i]};
        last[i].peak = (uint16_t)(100 * (i + 1));
    }
    // a read whose copy a flip overtakes is retried and returns the new front
    int calls = 0;
    uint16_t got = 0;
    pub.read([&](const Published &p) {
        got = p.last->peak;
        if (++calls == 1) pub.flip();
    });
    if (calls != 2 || got != 200 || pub.sequence() != 2) { std::printf("pub retry: calls %d peak %u seq %llu\n", calls, got, (unsigned long long)pub.sequence()); return 1; }
    // rewrite_front: fn(front, back), the sequence odd meanwhile, even and 2 further afterwards
    hold[0].peak_hold = 7;
    uint64_t inside = 0;
    pub.rewrite_front([&](Published &f, const Published &b) {
        inside = pub.sequence();
        f.hold->peak_hold = b.hold->peak_hold;
    });
    if (inside != 3 || pub.sequence() != 4 || hold[1].peak_hold != 7) { std::printf("pub rewrite: inside %llu seq %llu\n", (unsigned long long)inside, (unsigned long long)pub.sequence()); return 1; }
    // an odd sequence holds a reader back until the rewrite ends (a reader thread, since the wait is a spin: it cannot return
    // while the sequence is odd, whatever the timing)
    std::atomic<int> done{0};
    uint16_t seen = 0;
    std::thread reader;
    pub.rewrite_front([&](Published &f, const Published &) {
        reader = std::thread([&] {
            pub.read([&](const Published &p) { seen = p.hold->peak_hold; });
            done.store(1);
        });
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
        if (done.load()) return;
        f.hold->peak_hold = 9;
    });
    reader.join();
    if (seen != 9) { std::printf("pub odd: the reader did not wait (saw %u)\n", seen); return 1; }
    std::printf("pub ok\n");
    return 0;
}

int main()
{
    std::vector<std::unique_ptr<uint8_t[]>> mem;
    std::unique_ptr<Stager> st;
    uint32_t channels = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "init") {
            in >> channels;
            RingMem ring;
            mem.clear();
            for (int i = 0; i < RingMem::kArrays; ++i) {
                mem.emplace_back(new uint8_t[RingMem::bytes(channels, i)]());
                *ring.array(i) = mem.back().get();
            }
            st.reset(new Stager());
            st->init(channels, ring);
        } else if (cmd == "word") {
            uint32_t ch, w;
            in >> ch >> w;
            st->set_word(ch, w);
        } else if (cmd == "stage") {
            uint32_t ch, pt, len, tag;
            in >> ch >> pt >> len >> tag;
            uint8_t pay[kSlot];
            for (uint32_t i = 0; i < len; ++i) pay[i] = (uint8_t)(tag + i);
            std::printf("rc %d\n", st->stage(ch, (uint8_t)pt, pay, len));
        } else if (cmd == "snap") {
            uint32_t want = 1;
            in >> want;
            const uint32_t nch = st->channels_seen();
            const size_t max_frames = (size_t)channels * kStageDepth;
            const UploadLayout L = upload_layout(max_frames, channels);
            std::vector<uint8_t> up(L.total, 0);
            std::unique_ptr<igdsp::SnapshotPool> pool(want > 1 ? new igdsp::SnapshotPool(want - 1) : nullptr);
            SnapPart parts[igdsp::kMaxParts];
            const uint32_t n = igdsp::for_each_part(pool.get(), nch, [&](uint32_t i, uint32_t c0, uint32_t c1) {
                parts[i].c0 = c0;
                parts[i].c1 = c1;
                st->snapshot(parts[i], up.data(), L);
            });
            std::printf("snap %u %u\n", nch, n);
            uint32_t endA = 0, endB = 0, endS = 0;
            for (uint32_t i = 0; i < n; ++i) {
                const SnapPart &p = parts[i];
                std::printf("part %u %u %u %u %u\n", p.c0, p.c1, p.nA, p.nB, p.nSeq);
                if (p.nA) endA = p.c0 * kStageDepth + p.nA;
                if (p.nB) endB = p.c0 * kStageDepth + p.nB;
                if (p.nSeq) endS = p.c0 * kStageDepth + p.nSeq;
            }
            hex("payA", up.data() + L.payA, (size_t)endA * IGDSP_SAMPLES_PER_FRAME);
            hex("ptA", up.data() + L.ptA, endA);
            hex("payB", up.data() + L.payB, (size_t)endB * kSlot);
            ints("lenB", reinterpret_cast<const uint16_t *>(up.data() + L.lenB), endB);
            hex("ptB", up.data() + L.ptB, endB);
            ints("seq", reinterpret_cast<const uint32_t *>(up.data() + L.seq), 2 * (size_t)endS);
            ints("runs", reinterpret_cast<const uint32_t *>(up.data() + L.runs), 2 * (size_t)nch);
        } else if (cmd == "counts") {
            for (uint32_t c = 0; c < st->channels_seen(); ++c) std::printf("count %u %u %u\n", c, st->frames_seen(c), st->frames_dropped(c));
        } else if (cmd == "pubtest") {
            if (pubtest()) return 1;
        } else if (!cmd.empty()) {
            std::printf("unknown command %s\n", cmd.c_str());
            return 2;
        }
        std::fflush(stdout);
    }
    return 0;
}
