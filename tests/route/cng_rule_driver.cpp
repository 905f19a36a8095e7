// Runs the comfort-noise generator's rule (cng_frame_run in csrc/igdsp_cng.h, the functions k_cng compiles) as a program of its own for
// tests/test_cng_cpu.py.  Input: one case per stdin line: n frames ctl seed, the state's 96 bytes as twelve hexadecimal numbers, then
// per frame: kind sid_len has_voice, sixteen payload bytes, and with has_voice the n samples.  ctl holds for the case as d_ctl holds
// for a launch: RESET on the first frame only.  A line "G len b0 .. b(len-1)" prints step 2's g_tgt of a payload.
// Output per case, one line: per frame len_out, the record's sixteen bytes as two hexadecimal numbers and the n samples, then the
// state's twelve numbers.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "igdsp_cng.h"

using namespace igdsp;

int main()
{
    std::string head;
    while (std::cin >> head) {
        if (head == "G") {
            unsigned len;
            uint8_t pay[16] = {0};
            std::cin >> len;
            if (len == 0 || len > 16) return 2;
            for (unsigned i = 0; i < len; ++i) {
                unsigned b;
                std::cin >> b;
                pay[i] = (uint8_t)b;
            }
            std::printf("%u\n", cng_gain_host(pay, len));
            continue;
        }
        unsigned n = (unsigned)std::stoul(head), frames, ctl, seed;
        unsigned long long sw[12];
        std::cin >> frames >> ctl >> seed;
        for (auto &w : sw) std::cin >> std::hex >> w >> std::dec;
        if (!cng_n_ok(n)) return 2;
        igdsp_cng_state st;
        std::memcpy(&st, sw, 96);
        std::vector<int16_t> x(n), out(n);
        for (unsigned f = 0; f < frames; ++f) {
            unsigned kind, sid_len, has_voice;
            uint8_t sid[16];
            if (!(std::cin >> kind >> sid_len >> has_voice)) return 3;
            for (auto &b : sid) {
                unsigned v;
                std::cin >> v;
                b = (uint8_t)v;
            }
            if (has_voice)
                for (unsigned i = 0; i < n; ++i) {
                    int s;
                    if (!(std::cin >> s)) return 3;
                    x[i] = (int16_t)s;
                }
            igdsp_cng_rec rec;
            const unsigned c = f == 0 ? ctl : (cng_ctl(ctl) == IGDSP_CNG_RESET ? (unsigned)IGDSP_CNG_RUN : ctl);
            const unsigned len_out = cng_frame_run(st, kind, sid, sid_len, has_voice ? x.data() : nullptr, n, c, seed, out.data(), &rec);
            unsigned long long w[2];
            std::memcpy(w, &rec, 16);
            std::printf("%u %llx %llx", len_out, w[0], w[1]);
            for (unsigned i = 0; i < n; ++i) std::printf(" %d", (int)out[i]);
            std::printf(" ");
        }
        std::memcpy(sw, &st, 96);
        for (auto w : sw) std::printf("%llx ", w);
        std::printf("\n");
    }
    return 0;
}
