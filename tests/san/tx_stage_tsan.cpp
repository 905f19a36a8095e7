// ThreadSanitizer harness for csrc/igdsp_txstage.h (the staged send path's host side): four producer threads, each owning
// disjoint legs, stage frames; a setter thread raises each leg's ptt id; one consumer snapshots repeatedly into upload blocks.
// Checks: no frame lost or duplicated beyond the counted refusals, per-leg order kept, every setter value observed by exactly one
// frame or still pending at the end.  Built and run by tests/test_tx_stage_tsan_cpu.py; test infrastructure only.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "igdsp_txstage.h"

using namespace igdsp_tx;

static constexpr uint32_t kLegs = 64, kProducers = 4, kFrames = 4000, kSetterRounds = 200;

int main()
{
    Stager st;
    if (!st.init(kLegs)) { std::puts("init failed"); return 1; }
    for (uint32_t l = 0; l < kLegs; ++l) st.open(l);
    std::atomic<uint32_t> producers_left{kProducers};
    std::vector<std::vector<uint32_t>> accepted(kLegs);   // per leg: sequence numbers the producer saw accepted
    std::vector<std::thread> th;
    for (uint32_t p = 0; p < kProducers; ++p)
        th.emplace_back([&, p] {
            uint8_t pkt[12 + 160];
            std::memset(pkt, 0, sizeof pkt);
            pkt[0] = 0x80;
            for (uint32_t s = 0; s < kFrames; ++s)
                for (uint32_t l = p; l < kLegs; l += kProducers) {
                    const uint32_t n = 1 + (s * 7 + l) % 160;
                    pkt[2] = (uint8_t)(s >> 8); pkt[3] = (uint8_t)s;
                    pkt[12] = (uint8_t)l;
                    const int rc = st.stage(l, pkt, 12 + n, s);
                    if (rc == IGDSP_OK) accepted[l].push_back(s);
                    else if (rc != IGDSP_EBUSY) { std::printf("stage rc %d\n", rc); std::abort(); }
                }
            producers_left.fetch_sub(1);
        });
    th.emplace_back([&] {                                      // setter thread: ptt id 1, 2, ... on every leg
        for (uint32_t v = 1; v <= kSetterRounds; ++v)
            for (uint32_t l = 0; l < kLegs; ++l) st.set(l, kSdPttId, (uint64_t)(v & 0xFF) << kSwPttIdShift);
    });
    std::vector<std::vector<uint32_t>> got(kLegs), ids(kLegs);
    std::vector<uint8_t> up;
    auto snapshot = [&] {
        const Stager::Counts c = st.count(0, kLegs);
        const TxUploadLayout L = upload_layout(c.runs, c.frames, c.dwords);
        up.assign(L.total, 0);
        st.emit(0, kLegs, up.data(), L, Stager::Counts{});
        const TxRun *runs = reinterpret_cast<const TxRun *>(up.data() + L.runs);
        const TxRec *recs = reinterpret_cast<const TxRec *>(up.data() + L.recs);
        const uint8_t *bytes = up.data() + L.bytes;
        for (uint32_t r = 0; r < c.runs; ++r) {
            uint32_t off = runs[r].off_dw;
            for (uint32_t k = 0; k < runs[r].count; ++k) {
                const TxRec &rc = recs[runs[r].first + k];
                const uint8_t *p = bytes + 4u * off;
                const uint32_t n = (uint32_t)(rc.word >> kRecNShift) & 0xFFu, s = (uint32_t)p[2] << 8 | p[3];
                if (p[0] != 0x80 || p[12] != runs[r].leg || s != (uint32_t)rc.now_ms || n != 1 + (s * 7 + runs[r].leg) % 160) {
                    std::printf("bad record leg %u\n", runs[r].leg); std::abort();
                }
                got[runs[r].leg].push_back(s);
                if (rc.word & kSdPttId) ids[runs[r].leg].push_back((uint32_t)(rc.word >> kSwPttIdShift) & 0xFFu);
                off += stream_dwords(n);
            }
        }
    };
    while (producers_left.load() != 0) snapshot();
    for (auto &t : th) t.join();
    snapshot();
    uint64_t total = 0, refused = 0;
    for (uint32_t l = 0; l < kLegs; ++l) {
        if (got[l] != accepted[l]) { std::printf("leg %u: frames lost, duplicated or reordered\n", l); return 1; }
        total += got[l].size();
        refused += st.refused(l);
        if (got[l].size() + st.refused(l) != kFrames) { std::printf("leg %u: %zu + %u refused != %u\n", l, got[l].size(), st.refused(l), kFrames); return 1; }
        // setter values: strictly rising, the last one observed or still pending
        for (size_t i = 1; i < ids[l].size(); ++i)
            if (ids[l][i] <= ids[l][i - 1]) { std::printf("leg %u: setter order\n", l); return 1; }
        uint8_t pkt[13] = {0x80};
        if (st.stage(l, pkt, 13, 0) != IGDSP_OK) { std::printf("leg %u: final stage\n", l); return 1; }
    }
    // the setter values still pending reach the final frames: every leg ends on the last value
    const Stager::Counts c = st.count(0, kLegs);
    const TxUploadLayout L = upload_layout(c.runs, c.frames, c.dwords);
    up.assign(L.total, 0);
    st.emit(0, kLegs, up.data(), L, Stager::Counts{});
    const TxRec *recs = reinterpret_cast<const TxRec *>(up.data() + L.recs);
    for (uint32_t l = 0; l < kLegs; ++l) {
        uint32_t last = ids[l].empty() ? 0u : ids[l].back();
        if (recs[l].word & kSdPttId) last = (uint32_t)(recs[l].word >> kSwPttIdShift) & 0xFFu;
        if (last != (kSetterRounds & 0xFFu)) { std::printf("leg %u: setter value lost (%u)\n", l, last); return 1; }
    }
    std::printf("tx stage ok: %llu frames, %llu refused\n", (unsigned long long)total, (unsigned long long)refused);
    return 0;
}
