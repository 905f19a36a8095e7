// Prints agc_route (csrc/igdsp_route.h) for tests/test_agc_route_cpu.py.  One case per stdin line: C F n g711 yardstick; one output line
// per case: grid threads lds g711 copy blocks, then what the geometry has to cover for the kernel's indices to stay in bounds: the
// highest channel a thread of the grid maps to, one past the highest sample a busy lane's block of 8 reaches in its row, the number
// of busy lanes per channel, and the constants.
#include <cstdio>
#include <iostream>

#include "igdsp_route.h"

using namespace igdsp;

int main()
{
    unsigned long long C, F, n, g711, yard;
    while (std::cin >> C >> F >> n >> g711 >> yard) {
        const AgcRoute r = agc_route((uint32_t)C, (uint32_t)F, (uint32_t)n, g711 != 0, yard != 0);
        long long top_chan = -1, row_hi = -1, busy = 0;
        if (r.grid) {
            top_chan = (long long)(r.grid - 1u) * kAgcChans + (r.threads - 1u) / kAgcLanes;   // the kernel's c64 of the last thread
            for (unsigned b = 0; b < kAgcLanes; ++b)
                if (b < r.blocks) { ++busy; row_hi = 8ll * b + 8; }
        }
        std::printf("%u %u %u %d %d %u %lld %lld %lld %u %u %u %d\n", r.grid, r.threads, r.lds, r.g711 ? 1 : 0, r.copy ? 1 : 0, r.blocks, top_chan, row_hi, busy,
                    kAgcLanes, kAgcChans, kAgcResident, kAgcWaves);
    }
    return 0;
}
