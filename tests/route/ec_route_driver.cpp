// Prints ec_route (csrc/igdsp_route.h) for tests/test_ec_route_cpu.py.  One case per stdin line: C F n tail; one output line per case:
// grid threads lds tail blocks, then what the geometry has to cover for the kernel's indices to stay in bounds, over every block of a
// frame and every lane: the lowest and one past the highest value of the far buffer a block's window reads, the same of the near
// buffer, the last value the history's move reads, and the constants.
#include <algorithm>
#include <cstdio>
#include <iostream>

#include "igdsp_route.h"

using namespace igdsp;

int main()
{
    unsigned long long C, F, n, tail;
    while (std::cin >> C >> F >> n >> tail) {
        const EcRoute r = ec_route((uint32_t)C, (uint32_t)F, (uint32_t)n, (uint32_t)tail);
        long long x_lo = 1 << 30, x_hi = -1, n_lo = 1 << 30, n_hi = -1, move_hi = -1;
        if (r.grid) {
            const long long L = (long long)tail, T = L / 16;
            for (long long s = 0; s < (long long)n; s += 8) {
                const long long b = std::min(8ll, (long long)n - s), E = s + b;
                for (long long k = 0; k < 16; ++k) {
                    const long long a0 = kEcPad + L + E - 8 - k * T - T;   // the window: T + 8 values
                    x_lo = std::min(x_lo, a0);
                    x_hi = std::max(x_hi, a0 + T + 8);
                }
                n_lo = std::min(n_lo, (long long)kEcPad + E - 8);
                n_hi = std::max(n_hi, (long long)kEcPad + E);
            }
            move_hi = kEcPad + (long long)n + L;                           // one past the last value the move reads
        }
        std::printf("%u %u %u %u %u %lld %lld %lld %lld %lld %u %u %u %u %u\n", r.grid, r.threads, r.lds, r.tail, r.blocks, x_lo, x_hi, n_lo, n_hi, move_hi,
                    kEcXBuf, kEcNBuf, kEcPad, kEcChans, kEcResident);
    }
    return 0;
}
