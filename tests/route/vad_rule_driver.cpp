// Runs the voice detector's rule (vad_frame_run in csrc/igdsp_vad.h, the functions k_vad compiles) as a program of its own for
// tests/test_vad_cpu.py.  Input: one case per stdin line: n frames ctl, the state's 128 bytes as sixteen hexadecimal numbers, the cfg's
// thr_abs nf_min nf_max sid_every ratio_on_q4 ratio_off_q4 dn up up_v asm_shift burst hang_long hang_short order dtx sid_delta sid_gap
// vox_on vox_off, then frames * n samples.  ctl holds for the case as d_ctl holds for a launch: RESET on the first frame only.
// A line "L n e" prints level(e) for n samples per frame; a line "D len b0 .. b(len-1)" prints igdsp_sid_decode's level and ten k.
// Output per case, one line: per frame the kind, the record's sixteen bytes and the payload's sixteen bytes as two hexadecimal numbers
// each, then the state's sixteen numbers.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "igdsp_vad.h"

using namespace igdsp;

int main()
{
    std::string head;
    while (std::cin >> head) {
        if (head == "L") {
            unsigned n;
            long long e;
            std::cin >> n >> e;
            std::printf("%u\n", vad_level((int64_t)e, VadHostTab{n}));
            continue;
        }
        if (head == "D") {
            unsigned len;
            std::cin >> len;
            std::printf("%d", len ? 0 : -1);
            for (unsigned i = 0; i < len; ++i) {
                unsigned b;
                std::cin >> b;
                if (i == 0) std::printf(" %u", b);
                else if (i <= 10) std::printf(" %d", vad_dequant(b));
            }
            std::printf("\n");
            continue;
        }
        unsigned n = (unsigned)std::stoul(head), frames, ctl, v[19];
        unsigned long long sw[16];
        std::cin >> frames >> ctl;
        for (auto &w : sw) std::cin >> std::hex >> w >> std::dec;
        for (unsigned &u : v) std::cin >> u;
        const igdsp_vad_cfg cfg{v[0], v[1], v[2], (uint16_t)v[3], (uint8_t)v[4], (uint8_t)v[5], (uint8_t)v[6], (uint8_t)v[7], (uint8_t)v[8], (uint8_t)v[9],
                                (uint8_t)v[10], (uint8_t)v[11], (uint8_t)v[12], (uint8_t)v[13], (uint8_t)v[14], (uint8_t)v[15], (uint8_t)v[16],
                                (uint8_t)v[17], (uint8_t)v[18], {0, 0, 0}};
        if (!vad_n_ok(n) || !vad_cfg_ok(&cfg)) return 2;
        igdsp_vad_state st;
        std::memcpy(&st, sw, 128);
        std::vector<int16_t> x(n);
        for (unsigned f = 0; f < frames; ++f) {
            for (unsigned i = 0; i < n; ++i) {
                int s;
                if (!(std::cin >> s)) return 3;
                x[i] = (int16_t)s;
            }
            igdsp_vad_rec rec;
            uint8_t sid[16];
            const unsigned kind = vad_frame_run(cfg, st, x.data(), n, f == 0 ? ctl : (vad_ctl(ctl) == IGDSP_VAD_RESET ? (unsigned)IGDSP_VAD_RUN : ctl), &rec, sid);
            unsigned long long w[4];
            std::memcpy(w, &rec, 16);
            std::memcpy(w + 2, sid, 16);
            std::printf("%u %llx %llx %llx %llx ", kind, w[0], w[1], w[2], w[3]);
        }
        std::memcpy(sw, &st, 128);
        for (auto w : sw) std::printf("%llx ", w);
        std::printf("\n");
    }
    return 0;
}
