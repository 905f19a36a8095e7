// Prints filt_route (csrc/igdsp_route.h) for tests/test_filt_route_cpu.py.  One case per stdin line: C F n g711 max_sections yardstick;
// one output line per case: grid threads lds in sections copy pieces inv max_sections, then what the geometry has to cover for the
// kernel's indices to stay in bounds, walked as the kernel walks a full tile, early turns then late: the number of items the turns
// visit below kFiltChans * pieces, whether every item's row and piece by the multiplier are item / pieces and item % pieces, one past
// the highest dword a piece reaches in its row, one past the highest byte of the tile and of the law bytes behind it, the highest
// item a clamped fetch of a one-row block reads, the highest channel the grid's last block maps to, and the constants.
#include <algorithm>
#include <cstdio>
#include <iostream>

#include "igdsp_route.h"

using namespace igdsp;

int main()
{
    unsigned long long C, F, n, g711, max_s, yard;
    while (std::cin >> C >> F >> n >> g711 >> max_s >> yard) {
        const FiltRoute r = filt_route((uint32_t)C, (uint32_t)F, (uint32_t)n, g711 != 0, (uint32_t)max_s, yard != 0);
        long long visited = 0, exact = 1, row_hi = -1, tile_hi = -1, law_hi = -1, fetch_hi = -1, top_chan = -1;
        if (r.grid) {
            const unsigned items = kFiltChans * r.pieces, stride = filt_row_dwords((uint32_t)n);
            for (unsigned u0 = 0; u0 < kFiltMaxPieces; u0 += kFiltAhead) {
                if (u0 && r.pieces <= kFiltAhead) break;                   // the late turns: rows of more than kFiltAhead pieces only
                for (unsigned u = u0; u < u0 + kFiltAhead; ++u)
                    for (unsigned lane = 0; lane < 64u; ++lane) {
                        const unsigned i = u * 64u + lane, rw = (i * r.inv) >> 20, pc = i - rw * r.pieces;
                        fetch_hi = std::max(fetch_hi, (long long)std::min(i, r.pieces - 1u));   // a block of one row: items = pieces
                        if (i >= items) continue;
                        ++visited;
                        if (rw != i / r.pieces || pc != i % r.pieces) exact = 0;
                        row_hi = std::max(row_hi, 4ll * pc + 4);
                        tile_hi = std::max(tile_hi, 4ll * ((long long)rw * stride + 4 * pc + 4));
                    }
            }
            law_hi = 4ll * kFiltChans * stride + kFiltChans;
            top_chan = (long long)(r.grid - 1u) * kFiltChans + kFiltChans - 1u;
        }
        std::printf("%u %u %u %d %d %d %u %u %u %lld %lld %lld %lld %lld %lld %lld %u %u %u %u %u\n", r.grid, r.threads, r.lds, r.in, r.sections, r.copy ? 1 : 0,
                    r.pieces, r.inv, r.max_sections, visited, exact, row_hi, tile_hi, law_hi, fetch_hi, top_chan, kFiltChans, kFiltResident, kFiltVgprs,
                    kFiltAhead, kFiltMaxPieces);
    }
    return 0;
}
