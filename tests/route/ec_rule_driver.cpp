// Runs the echo canceller's rule (ec_frame_run in csrc/igdsp_ec.h, the functions k_ec compiles) as a program of its own for
// tests/test_ec_route_cpu.py.  Input: one case per stdin line: n frames seed garbage (0 | 1 | 2) tail mu_shift hang ctl.  The rows are a
// xorshift sequence the test restates (full-scale values, -32768 among them); garbage = 1 fills the state's bytes from the same
// sequence first and sets the tag, garbage = 2 then puts every weight at an end of int32 as well.  Output per case: per frame the
// record's sixteen bytes as two hexadecimal numbers and a 64-bit FNV-1a hash of the output row, then the hash of the state's bytes.
#include <cstdio>
#include <iostream>
#include <vector>

#include "igdsp_ec.h"

using namespace igdsp;

static uint32_t rng_state;
static uint32_t rng()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}
static unsigned long long fnv(const void *p, size_t bytes)
{
    unsigned long long h = 1469598103934665603ull;
    const uint8_t *b = static_cast<const uint8_t *>(p);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

int main()
{
    unsigned n, frames, seed, garbage, tail, mu, hang, ctl;
    while (std::cin >> n >> frames >> seed >> garbage >> tail >> mu >> hang >> ctl) {
        igdsp_ec_cfg cfg = ec_cfg_default(tail);
        cfg.mu_shift = (uint8_t)mu;
        cfg.hang = (uint16_t)hang;
        cfg.pmin = 0;
        if (!ec_n_ok(n) || !ec_cfg_ok(&cfg)) return 2;
        rng_state = seed ? seed : 1u;
        igdsp_ec_state st{};
        if (garbage) {
            uint8_t *b = reinterpret_cast<uint8_t *>(&st);
            for (size_t i = 0; i < sizeof(st); ++i) b[i] = (uint8_t)rng();
            st.tag = (uint32_t)IGDSP_EC_TAG | tail;
            st.hang &= 3u;
            if (garbage == 2)
                for (int k = 0; k < IGDSP_EC_MAX_TAIL; ++k) st.w[k] = (rng() & 1u) ? 2147483647 : (int32_t)-2147483648ll;
        }
        std::vector<int16_t> near(n), far(n), out(n);
        for (unsigned f = 0; f < frames; ++f) {
            for (unsigned i = 0; i < 2 * n; ++i) {
                const uint32_t r = rng();
                (i < n ? near[i] : far[i - n]) = (r & 0x30000u) == 0 ? (int16_t)-32768 : (int16_t)(r & 0xFFFFu);
            }
            igdsp_ec_rec rec;
            ec_frame_run(cfg, st, near.data(), far.data(), n, f == 0 ? ctl : (ctl == IGDSP_EC_RESET ? (unsigned)IGDSP_EC_RUN : ctl), out.data(), &rec);
            unsigned long long w[2];
            std::memcpy(w, &rec, 16);
            std::printf("%llx %llx %llx ", w[0], w[1], fnv(out.data(), n * 2u));
        }
        std::printf("%llx\n", fnv(&st, sizeof(st)));
    }
    return 0;
}
