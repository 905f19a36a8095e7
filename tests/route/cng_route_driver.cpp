// Prints cng_route (csrc/igdsp_route.h) for tests/test_cng_route_cpu.py.  One case per stdin line: C F n g711 pcm yardstick; one output
// line per case: grid threads lds in copy pieces passes inv, then what the geometry has to cover for the kernel's indices to stay in
// bounds, walked as the kernel walks a full tile: the number of items a pass visits below kCngChans * pieces, whether every item's row
// and piece by the multiplier are item / pieces and item % pieces, one past the highest dword a piece reaches in its row, one past the
// highest byte of the tile and of the row bytes behind it, the highest channel the grid's last block maps to, and the constants.
#include <algorithm>
#include <cstdio>
#include <iostream>

#include "igdsp_route.h"

using namespace igdsp;

int main()
{
    unsigned long long C, F, n, g711, pcm, yard;
    while (std::cin >> C >> F >> n >> g711 >> pcm >> yard) {
        const CngRoute r = cng_route((uint32_t)C, (uint32_t)F, (uint32_t)n, g711 != 0, pcm != 0, yard != 0);
        long long visited = 0, exact = 1, row_hi = -1, tile_hi = -1, who_hi = -1, top_chan = -1;
        if (r.grid) {
            const unsigned items = kCngChans * r.pieces, stride = cng_row_dwords((uint32_t)n);
            for (unsigned it = 0; it < r.passes; ++it)
                for (unsigned lane = 0; lane < 64u; ++lane) {
                    const unsigned i = it * 64u + lane, rw = (i * r.inv) >> 20, pc = i - rw * r.pieces;
                    if (i >= items) continue;
                    ++visited;
                    if (rw != i / r.pieces || pc != i % r.pieces) exact = 0;
                    row_hi = std::max(row_hi, 4ll * pc + 4);
                    tile_hi = std::max(tile_hi, 4ll * ((long long)rw * stride + 4 * pc + 4));
                }
            who_hi = 4ll * kCngChans * stride + kCngChans;
            top_chan = (long long)(r.grid - 1u) * kCngChans + kCngChans - 1u;
        }
        std::printf("%u %u %u %d %d %u %u %u %lld %lld %lld %lld %lld %lld %u %u %u\n", r.grid, r.threads, r.lds, r.in, r.copy ? 1 : 0, r.pieces, r.passes, r.inv,
                    visited, exact, row_hi, tile_hi, who_hi, top_chan, kCngChans, kCngResident, kCngVgprs);
    }
    return 0;
}
