// Runs the level control's rule (agc_frame_run in csrc/igdsp_agc.h, the functions k_agc compiles) as a program of its own for
// tests/test_agc_cpu.py.  Input: one case per stdin line: n frames ctl, the state's tag env gain cap flags reserved, the cfg's target ceil gate gmin
// gmax att rel up down lrel, then frames * n samples.  ctl holds for the case as d_ctl holds for a launch: RESET on the first frame
// only.  Output per case, one line: per frame the record's sixteen bytes as two hexadecimal numbers and the n output samples, then the
// state's sixteen bytes as two hexadecimal numbers.
#include <cstdio>
#include <iostream>
#include <vector>

#include "igdsp_agc.h"

using namespace igdsp;

int main()
{
    unsigned n, frames, ctl, tag, env, gain, cap, flags, reserved, v[10];
    while (std::cin >> n >> frames >> ctl >> tag >> env >> gain >> cap >> flags >> reserved) {
        for (unsigned &u : v) std::cin >> u;
        const igdsp_agc_cfg cfg{(uint16_t)v[0], (uint16_t)v[1], (uint16_t)v[2], (uint16_t)v[3], (uint16_t)v[4], (uint8_t)v[5], (uint8_t)v[6], (uint8_t)v[7],
                                (uint8_t)v[8], (uint8_t)v[9], 0};
        if (!agc_n_ok(n) || !agc_cfg_ok(&cfg)) return 2;
        igdsp_agc_state st{tag, (uint16_t)env, (uint16_t)gain, (uint16_t)cap, (uint16_t)flags, reserved};
        std::vector<int16_t> x(n), out(n);
        for (unsigned f = 0; f < frames; ++f) {
            for (unsigned i = 0; i < n; ++i) {
                int s;
                if (!(std::cin >> s)) return 3;
                x[i] = (int16_t)s;
            }
            igdsp_agc_rec rec;
            agc_frame_run(cfg, st, x.data(), n, f == 0 ? ctl : (agc_ctl(ctl) == IGDSP_AGC_RESET ? (unsigned)IGDSP_AGC_RUN : ctl), out.data(), &rec);
            unsigned long long w[2];
            std::memcpy(w, &rec, 16);
            std::printf("%llx %llx ", w[0], w[1]);
            for (unsigned i = 0; i < n; ++i) std::printf("%d ", (int)out[i]);
        }
        unsigned long long w[2];
        std::memcpy(w, &st, 16);
        std::printf("%llx %llx\n", w[0], w[1]);
    }
    return 0;
}
