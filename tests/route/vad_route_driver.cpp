// Prints vad_route (csrc/igdsp_route.h) for tests/test_vad_route_cpu.py.  One case per stdin line: C F n g711 yardstick list with_rec; one
// output line per case: grid threads lds g711 copy pieces waves list_grid counts_bytes work_bytes, then what the geometry has to cover
// for the kernel's indices to stay in bounds: the highest channel a thread of the grid maps to, one past the highest sample a busy lane's
// piece of 8 reaches in its row (lane p takes pieces p and p + 16), the number of pieces taken, the lowest and one past the highest value
// of a channel's LDS row that the lag sums and the packing of the second copy read (in values, the row's first sample at kVadPad), and
// the constants.
#include <algorithm>
#include <cstdio>
#include <iostream>

#include "igdsp_route.h"

using namespace igdsp;

int main()
{
    unsigned long long C, F, n, g711, yard, list, with_rec;
    while (std::cin >> C >> F >> n >> g711 >> yard >> list >> with_rec) {
        const VadRoute r = vad_route((uint32_t)C, (uint32_t)F, (uint32_t)n, g711 != 0, yard != 0, list != 0, with_rec != 0);
        long long top_chan = -1, row_hi = -1, taken = 0, read_lo = 1 << 30, read_hi = -1;
        if (r.grid) {
            top_chan = (long long)(r.grid - 1u) * kVadChans + (r.threads - 1u) / kVadLanes;   // the kernel's c64 of the last thread
            for (unsigned k = 0; k < kVadLanes; ++k) {
                for (unsigned p : {k, k + 16u})
                    if (p < r.pieces) { ++taken; row_hi = std::max(row_hi, 8ll * p + 8); }
                const long long kd = k / 2u;                               // the kernel's lp = dword of sample 0 + 4 j - kd, four dwords, j < pieces
                read_lo = std::min(read_lo, (long long)kVadPad - 2 * kd);
                read_hi = std::max(read_hi, (long long)kVadPad + 2 * (4ll * (r.pieces - 1u) - kd + 4));
                for (unsigned p : {k, k + 16u})                            // the second copy is packed from five dwords of the lane's piece
                    if (p < r.pieces) read_hi = std::max(read_hi, (long long)kVadPad + 2 * (4ll * p + 5));
            }
        }
        std::printf("%u %u %u %d %d %u %u %u %llu %llu %lld %lld %lld %lld %lld %u %u %u %d %u %u %u\n", r.grid, r.threads, r.lds, r.g711 ? 1 : 0, r.copy ? 1 : 0,
                    r.pieces, r.waves, r.list_grid, (unsigned long long)r.counts_bytes, (unsigned long long)r.work_bytes, top_chan, row_hi, taken, read_lo,
                    read_hi, kVadLanes, kVadChans, kVadResident, kVadWaves, kVadPad, kVadBuf, kVadLdsBytes);
    }
    return 0;
}
