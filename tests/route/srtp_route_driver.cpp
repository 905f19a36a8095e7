// Prints srtp_route (csrc/igdsp_route.h) for tests/test_srtp_route_cpu.py.  One case per stdin line: C F stride ostride dir yardstick;
// one output line per case: grid threads lds dir move max_pieces, then what the geometry has to cover for the kernel's indices to stay
// in bounds, walked as the kernel walks: over every piece j < max_pieces and the four turns of the 64 lanes, with every packet of the
// frame as long as its slot, the number of items visited and whether each (row, quarter) of a piece is visited once, one past the
// highest word an item reaches in the tile, the tile's words, one past the highest byte a load reaches in its slot (16-byte loads
// where they fit the slot, dwords behind), the highest channel the grid's last block maps to, and the constants.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <vector>

#include "igdsp_route.h"
#include "igdsp_srtp.h"

using namespace igdsp;

int main()
{
    unsigned long long C, F, stride, ostride, dir, yard;
    while (std::cin >> C >> F >> stride >> ostride >> dir >> yard) {
        const SrtpRoute r = srtp_route((uint32_t)C, (uint32_t)F, (uint32_t)stride, (uint32_t)ostride, (int)dir, yard != 0);
        long long visited = 0, once = 1, tile_hi = -1, slot_hi = -1, top_chan = -1, covered = 0;
        if (r.grid) {
            for (unsigned j = 0; j < r.max_pieces; ++j) {
                std::vector<int> seen(kSrtpChans * 4u, 0);
                for (unsigned u = 0; u < kSrtpTurns; ++u)
                    for (unsigned lane = 0; lane < 64u; ++lane) {
                        const unsigned i = u * 64u + lane, row = i >> 2, q = i & 3u, off = 64u * j + 16u * q;
                        ++seen[row * 4u + q];
                        tile_hi = std::max(tile_hi, (long long)(row * kSrtpPitch + 4u * q + 4u));
                        if (off >= stride) continue;                       // s_lim <= stride: nothing is loaded
                        ++visited;
                        if (off + 16u <= stride) slot_hi = std::max(slot_hi, (long long)off + 16);
                        else slot_hi = std::max(slot_hi, (long long)std::min<unsigned long long>(off + 12u, stride));
                        covered += std::min<unsigned long long>(16u, stride - off);
                    }
                once &= std::all_of(seen.begin(), seen.end(), [](int v) { return v == 1; }) ? 1 : 0;
            }
            top_chan = (long long)(r.grid - 1u) * kSrtpChans + kSrtpChans - 1u;
        }
        std::printf("%u %u %u %d %d %u %lld %lld %lld %u %lld %lld %lld %u %u %u %u %u %u %zu %zu\n", r.grid, r.threads, r.lds, r.dir, r.move ? 1 : 0, r.max_pieces,
                    visited, once, tile_hi, kSrtpChans * kSrtpPitch, slot_hi, covered, top_chan, kSrtpChans, kSrtpPitch, kSrtpTurns, kSrtpResident, kSrtpVgprs,
                    kSrtpLdsBytes, sizeof(igdsp_srtp_state), sizeof(igdsp_srtp_rec));
    }
    return 0;
}
