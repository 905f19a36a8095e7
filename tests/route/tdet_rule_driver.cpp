// Runs the tone detector's rule (tdet_frame_run in csrc/igdsp_tdet.h, the text k_tdet compiles) as a program of its own for
// tests/test_tdet_route_cpu.py.  Input: one case per stdin line: n frames seed garbage (0 | 1) plan (0: DTMF, 1: 8 + 8, 2: one tone at
// 1 000 Hz, 3: one tone at 3 999 Hz).  The rows are a xorshift sequence the test restates (full-scale values, -32768 among them);
// garbage = 1 fills the state's bytes from the same sequence first.  Output per case: per frame the record's eight bytes as one
// hexadecimal number, then the state's bytes as a 64-bit FNV-1a hash.
#include <cstdio>
#include <iostream>
#include <vector>

#include "igdsp_tdet.h"

using namespace igdsp;

static uint32_t rng_state;
static uint32_t rng()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

int main()
{
    unsigned n, frames, seed, garbage, which;
    while (std::cin >> n >> frames >> seed >> garbage >> which) {
        if (!tdet_n_ok(n)) return 2;
        igdsp_tdet_plan plan{};
        const uint16_t dtmf[8] = {697, 770, 852, 941, 1209, 1336, 1477, 1633};
        const uint16_t wide[16] = {350, 440, 480, 620, 697, 770, 852, 941, 1209, 1336, 1477, 1633, 1800, 2000, 2200, 2400};
        const uint16_t one[1] = {1000}, high[1] = {3999};
        const bool ok = which == 0 ? tdet_plan_make(8000, dtmf, 4, 4, nullptr, plan) : which == 1 ? tdet_plan_make(8000, wide, 8, 8, nullptr, plan)
                      : which == 2 ? tdet_plan_make(8000, one, 1, 0, nullptr, plan) : tdet_plan_make(8000, high, 1, 0, nullptr, plan);
        if (!ok) return 3;
        rng_state = seed ? seed : 1u;
        igdsp_tdet_state st{};
        if (garbage) {
            uint8_t *b = reinterpret_cast<uint8_t *>(&st);
            for (size_t i = 0; i < sizeof(st); ++i) b[i] = (uint8_t)rng();
        }
        std::vector<int16_t> row(n);
        for (unsigned f = 0; f < frames; ++f) {
            for (unsigned i = 0; i < n; ++i) {
                const uint32_t r = rng();
                row[i] = (r & 0x30000u) == 0 ? (int16_t)-32768 : (int16_t)(r & 0xFFFFu);
            }
            igdsp_tdet_rec rec;
            tdet_frame_run(plan, st, row.data(), n, &rec);
            unsigned long long w = 0;
            std::memcpy(&w, &rec, 8);
            std::printf("%llx ", w);
        }
        unsigned long long hsh = 1469598103934665603ull;
        const uint8_t *b = reinterpret_cast<const uint8_t *>(&st);
        for (size_t i = 0; i < sizeof(st); ++i) hsh = (hsh ^ b[i]) * 1099511628211ull;
        std::printf("%llx\n", hsh);
    }
    return 0;
}
