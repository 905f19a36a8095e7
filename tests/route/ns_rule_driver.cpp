// Runs the noise suppressor's rule (csrc/igdsp_ns.h: what igdsp_ns_frame calls and the functions k_ns compiles) as a program of its
// own for tests/test_ns_cpu.py.  Input, one case: n frames ctl lanes floor_q15 over_q4 init_hops track_shift rise_shift, the state's
// 1 072 bytes as 134 hexadecimal numbers, then per frame the n samples.  ctl holds for the case as d_ctl holds for a launch: RESET on the
// first frame only.  lanes = 1: ns_frame_run, the host's walk.  lanes = 16: the kernel's walk, ns_open_state / ns_frame_core /
// ns_close_state worked by 16 threads as the 16 lanes of a channel, sync() a barrier between them.  Output per case, one line: per
// frame the record's sixteen bytes as two hexadecimal numbers and the n samples, then the state's 134 numbers.  A cfg out of range
// prints -22.
// A line "T" prints the tables: the window's 160 entries and the 256 twiddle entries.
#include <pthread.h>

#include <cstdio>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "igdsp_ns.h"

using namespace igdsp;

struct Barrier {
    pthread_barrier_t *b;
    void operator()() const { pthread_barrier_wait(b); }
};

static void frame_lanes(const igdsp_ns_cfg &cfg, igdsp_ns_state &st, const int16_t *pcm, uint32_t n, uint32_t ctl_in, int16_t *out, igdsp_ns_rec *rec,
                        uint32_t L)
{
    const uint32_t ctl = ns_ctl(ctl_in);
    const bool fresh = ns_fresh(st.tag, ctl == (uint32_t)IGDSP_NS_RESET);
    static NsWork ws;
    static int16_t row[kNsMaxFrame];
    std::memcpy(row, pcm, n * sizeof(int16_t));
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, L);
    std::vector<std::thread> th;
    uint32_t w0[4];
    for (uint32_t lane = 0; lane < L; ++lane)
        th.emplace_back([&, lane] {
            uint32_t w[4], peak = 0u;
            uint64_t sq = 0u;
            ns_open_state(st, fresh, lane, L, Barrier{&bar});
            ns_frame_core(cfg, st, ws, kNsWin, kNsTw, row, n, ctl, fresh ? (uint32_t)IGDSP_NS_WAS_RESET : 0u, lane, L, Barrier{&bar}, w, sq, peak);
            if (lane == 0u) std::memcpy(w0, w, 16);
        });
    for (auto &t : th) t.join();
    pthread_barrier_destroy(&bar);
    ns_close_state(st, w0[3] >> 8);
    std::memcpy(out, row, n * sizeof(int16_t));
    std::memcpy(rec, w0, 16);
}

int main()
{
    std::string head;
    while (std::cin >> head) {
        if (head == "T") {
            for (int16_t v : kNsWin) std::printf("%d ", (int)v);
            for (int32_t v : kNsTw) std::printf("%d ", (int)v);
            std::printf("\n");
            continue;
        }
        unsigned n = (unsigned)std::stoul(head), frames, ctl, lanes, c[5];
        std::cin >> frames >> ctl >> lanes;
        for (auto &v : c) std::cin >> v;
        unsigned long long sw[sizeof(igdsp_ns_state) / 8];
        for (auto &w : sw) std::cin >> std::hex >> w >> std::dec;
        if (!ns_n_ok(n) || (lanes != 1u && lanes != kNsMaxLanes)) return 2;
        igdsp_ns_cfg cfg;
        ns_cfg_default(cfg);
        cfg.floor_q15 = c[0]; cfg.over_q4 = (uint16_t)c[1]; cfg.init_hops = (uint16_t)c[2]; cfg.track_shift = (uint16_t)c[3]; cfg.rise_shift = (uint16_t)c[4];
        const bool ok = ns_cfg_ok(cfg) && c[1] < 65536u && c[2] < 65536u && c[3] < 65536u && c[4] < 65536u;
        igdsp_ns_state st;
        std::memcpy(&st, sw, sizeof st);
        std::vector<int16_t> x(n), out(n);
        for (unsigned f = 0; f < frames; ++f) {
            for (unsigned i = 0; i < n; ++i) {
                int s;
                if (!(std::cin >> s)) return 3;
                x[i] = (int16_t)s;
            }
            if (!ok) continue;
            igdsp_ns_rec rec;
            const unsigned cf = f == 0 ? ctl : (ns_ctl(ctl) == IGDSP_NS_RESET ? (unsigned)IGDSP_NS_RUN : ctl);
            if (lanes == 1u) ns_frame_run(cfg, st, x.data(), n, cf, out.data(), &rec);
            else frame_lanes(cfg, st, x.data(), n, cf, out.data(), &rec, lanes);
            unsigned long long w[2];
            std::memcpy(w, &rec, 16);
            std::printf("%llx %llx", w[0], w[1]);
            for (unsigned i = 0; i < n; ++i) std::printf(" %d", (int)out[i]);
            std::printf(" ");
        }
        if (!ok) { std::printf("%d\n", IGDSP_EINVAL); continue; }
        std::memcpy(sw, &st, sizeof st);
        for (auto w : sw) std::printf("%llx ", w);
        std::printf("\n");
    }
    return 0;
}
