// Prints rtcp_build_route, rtcp_parse_route and srtcp_route (csrc/igdsp_route.h) for tests/test_rtcp_route_cpu.py.  One case per stdin
// line: kind (0 build, 1 parse, 2 srtcp) C F stride ostride dir yardstick; one output line per case: grid threads lds dir move
// max_pieces, then what the geometry has to cover for the kernel's indices to stay in bounds, walked as the kernel walks.  Build: the
// nine turns of the 64 lanes with every packet at its largest: the items visited, whether each (row, sixteenth) is visited at most
// once and every one below the largest packet once, one past the highest word an item reaches in the rows, the rows' words, one past
// the highest byte a store (the owner's tail included) reaches in its slot.  Parse: SRTP's walk over every piece j < max_pieces with
// every packet as long as its slot: items, once, the tile's reach, the slot's reach, the bytes covered.  Then the highest leg the
// grid's last block maps to and the constants.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <vector>

#include "igdsp_route.h"
#include "igdsp_rtcp.h"

using namespace igdsp;

int main()
{
    unsigned long long kind, C, F, stride, ostride, dir, yard;
    while (std::cin >> kind >> C >> F >> stride >> ostride >> dir >> yard) {
        uint32_t grid = 0, threads = 0, lds = 0, max_pieces = 0;
        int rdir = 0, move = 0;
        long long visited = 0, once = 1, tile_hi = -1, tile_words = 0, slot_hi = -1, covered = 0, top = -1;
        if (kind == 2) {
            const SrtpRoute r = srtcp_route((uint32_t)C, (uint32_t)F, (uint32_t)stride, (uint32_t)ostride, (int)dir, yard != 0);
            grid = r.grid; threads = r.threads; lds = r.lds; max_pieces = r.max_pieces; rdir = r.dir; move = r.move ? 1 : 0;
        } else {
            const RtcpRoute r = kind == 0 ? rtcp_build_route((uint32_t)C, (uint32_t)F, (uint32_t)stride, yard != 0) : rtcp_parse_route((uint32_t)C, (uint32_t)F, (uint32_t)stride, yard != 0);
            grid = r.grid; threads = r.threads; lds = r.lds; max_pieces = r.max_pieces; move = r.move ? 1 : 0;
        }
        if (grid && kind == 0) {
            const unsigned size = IGDSP_RTCP_MAX_BUILT;
            std::vector<int> seen(kRtcpChans * kRtcpRowItems, 0);
            tile_words = kRtcpChans * kRtcpRowPitch;
            for (unsigned u = 0; u < kRtcpRowItems; ++u)
                for (unsigned lane = 0; lane < 64u; ++lane) {
                    const unsigned i = u * 64u + lane, row = i / kRtcpRowItems, q = i - row * kRtcpRowItems;
                    if (row >= kRtcpChans) { once = 0; continue; }
                    ++seen[row * kRtcpRowItems + q];
                    if (16u * q + 16u > (size & ~15u)) continue;
                    ++visited;
                    tile_hi = std::max(tile_hi, (long long)(row * kRtcpRowPitch + 4u * q + 4u));
                    slot_hi = std::max(slot_hi, (long long)(16u * q + 16u));
                    covered += 16;
                }
            once &= std::all_of(seen.begin(), seen.end(), [](int v) { return v == 1; }) ? 1 : 0;
            for (unsigned lane = 0; lane < 64u; ++lane) {                    // the owner's tail
                const unsigned t0 = size & ~15u, nt = size & 15u;
                for (unsigned k = 0; k < 3u; ++k)
                    if (4u * k + 4u <= nt) {
                        tile_hi = std::max(tile_hi, (long long)(lane * kRtcpRowPitch + (t0 >> 2) + k + 1u));
                        slot_hi = std::max(slot_hi, (long long)(t0 + 4u * k + 4u));
                        covered += 4;
                    }
            }
        }
        if (grid && kind == 1) {
            tile_words = kSrtpChans * kSrtpPitch;
            for (unsigned j = 0; j < max_pieces; ++j) {
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
        }
        if (grid) top = (long long)(grid - 1u) * kRtcpChans + kRtcpChans - 1u;
        std::printf("%u %u %u %d %d %u %lld %lld %lld %lld %lld %lld %lld %u %u %u %u %u %u %u %u %u %zu %zu %zu %zu\n", grid, threads, lds, rdir, move, max_pieces, visited,
                    once, tile_hi, tile_words, slot_hi, covered, top, kRtcpChans, kRtcpRowWords, kRtcpRowPitch, kRtcpRowItems, kRtcpResident, kRtcpVgprs,
                    kRtcpBuildLdsBytes, kRtcpParseLdsBytes, kSrtpLdsBytes, sizeof(igdsp_rtcp_state), sizeof(igdsp_rtcp_src), sizeof(igdsp_rtcp_built),
                    sizeof(igdsp_rtcp_seen));
    }
    return 0;
}
