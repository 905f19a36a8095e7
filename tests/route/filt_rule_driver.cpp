// Runs the filter's rule (filt_frame_run in csrc/igdsp_filt.h, what igdsp_filt_frame calls and the functions k_filt compiles) as a
// program of its own for tests/test_filt_cpu.py.  Input, one case: n frames ctl has_plan, the plan's 48 bytes and the state's 48 bytes
// as six hexadecimal numbers each, then per frame the n samples.  ctl holds for the case as d_ctl holds for a launch: RESET on the
// first frame only.  Output per case, one line: per frame the record's sixteen bytes as two hexadecimal numbers and the n samples, then
// the state's six numbers.
// A line "D kind rate f0 q gain_db" prints igdsp_filt_design's verdict: 0 and the five coefficients, or -22.  A line "P preset rate"
// prints igdsp_filt_plan_preset's: 0 and the plan's six numbers, or -22.  A line "K" with a plan's six numbers prints filt_plan_ok.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "igdsp_filt.h"

using namespace igdsp;

int main()
{
    std::string head;
    while (std::cin >> head) {
        if (head == "D") {
            unsigned kind, rate;
            double f0, q, g;
            int16_t c[5] = {77, 77, 77, 77, 77};
            std::cin >> kind >> rate >> f0 >> q >> g;
            if (filt_design(kind, rate, f0, q, g, c)) std::printf("0 %d %d %d %d %d\n", c[0], c[1], c[2], c[3], c[4]);
            else std::printf("%d %d\n", IGDSP_EINVAL, (c[0] == 77 && c[1] == 77 && c[2] == 77 && c[3] == 77 && c[4] == 77) ? 0 : 1);   // 1: it wrote
            continue;
        }
        if (head == "P") {
            unsigned preset, rate;
            std::cin >> preset >> rate;
            igdsp_filt_plan p;
            unsigned long long w[6];
            if (!filt_preset(preset, rate, p)) { std::printf("%d\n", IGDSP_EINVAL); continue; }
            std::memcpy(w, &p, 48);
            std::printf("0 %llx %llx %llx %llx %llx %llx\n", w[0], w[1], w[2], w[3], w[4], w[5]);
            continue;
        }
        unsigned long long pw[6], sw[6];
        if (head == "K") {
            for (auto &w : pw) std::cin >> std::hex >> w >> std::dec;
            igdsp_filt_plan p;
            std::memcpy(&p, pw, 48);
            std::printf("%d\n", filt_plan_ok(p) ? 0 : IGDSP_EINVAL);
            continue;
        }
        unsigned n = (unsigned)std::stoul(head), frames, ctl, has_plan;
        std::cin >> frames >> ctl >> has_plan;
        for (auto &w : pw) std::cin >> std::hex >> w >> std::dec;
        for (auto &w : sw) std::cin >> std::hex >> w >> std::dec;
        if (!filt_n_ok(n)) return 2;
        igdsp_filt_plan plan;
        igdsp_filt_state st;
        std::memcpy(&plan, pw, 48);
        std::memcpy(&st, sw, 48);
        std::vector<int16_t> x(n), out(n);
        for (unsigned f = 0; f < frames; ++f) {
            for (unsigned i = 0; i < n; ++i) {
                int s;
                if (!(std::cin >> s)) return 3;
                x[i] = (int16_t)s;
            }
            igdsp_filt_rec rec;
            const unsigned c = f == 0 ? ctl : (filt_ctl(ctl) == IGDSP_FILT_RESET ? (unsigned)IGDSP_FILT_RUN : ctl);
            filt_frame_run(has_plan ? &plan : nullptr, st, x.data(), n, c, out.data(), &rec);
            unsigned long long w[2];
            std::memcpy(w, &rec, 16);
            std::printf("%llx %llx", w[0], w[1]);
            for (unsigned i = 0; i < n; ++i) std::printf(" %d", (int)out[i]);
            std::printf(" ");
        }
        std::memcpy(sw, &st, 48);
        for (auto w : sw) std::printf("%llx ", w);
        std::printf("\n");
    }
    return 0;
}
