// Prints ns_route (csrc/igdsp_route.h) for tests/test_ns_route_cpu.py.  One case per stdin line: C F n g711 yardstick; one output line
// per case: grid threads lds in copy pieces, then what the geometry has to cover for the kernel's indices to stay in bounds, walked as
// the kernel walks: the number of pieces the kNsTurns turns of a channel's 16 lanes visit below `pieces` and whether each is visited
// once, one past the highest byte a piece reaches in its row, the row's size, one past the highest byte the last channel of a block
// reaches in LDS (state, work, row), the highest piece a clamped fetch reads, the highest channel the grid's last block maps to, and
// the constants.
// A line "X" prints the index arithmetic of the transform (csrc/igdsp_ns.h), as the 16 lanes walk it: per pass (span 2 << sh, sh = 0
// .. 6) whether the 64 butterflies' points are a permutation of 0 .. 127 and the highest twiddle index; then whether rev7 is an
// involution on 0 .. 127, whether the split pass's pairs (rev7(k), rev7(128 - k)), k = 0 .. 64, cover every position once (k = 0 and 64
// alone), the highest twiddle index the split reads, and whether ns_band_of maps bins 1 .. 128 onto 32 bands of four.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "igdsp_ns.h"
#include "igdsp_route.h"

using namespace igdsp;

int main()
{
    std::string head;
    while (std::cin >> head) {
        if (head == "X") {
            for (unsigned sh = 0; sh < 7u; ++sh) {
                std::vector<int> seen(kNsPoints, 0);
                unsigned tmax = 0;
                for (unsigned lane = 0; lane < kNsLanes; ++lane)
                    for (unsigned b = lane; b < kNsPoints / 2u; b += kNsLanes) {
                        const NsFly f = ns_fly(b, sh);
                        if (f.i < kNsPoints) ++seen[f.i];
                        if (f.j < kNsPoints) ++seen[f.j];
                        tmax = std::max(tmax, f.t);
                    }
                std::printf("%d %u ", std::all_of(seen.begin(), seen.end(), [](int v) { return v == 1; }) ? 1 : 0, tmax);
            }
            int invol = 1, bands = 1;
            std::vector<int> seen(kNsPoints, 0), per(kNsBands, 0);
            unsigned tmax = 0;
            for (unsigned k = 0; k < kNsPoints; ++k) invol &= ns_rev7(k) < kNsPoints && ns_rev7(ns_rev7(k)) == k;
            for (unsigned lane = 0; lane < kNsLanes; ++lane)
                for (unsigned k = lane; k <= kNsPoints / 2u; k += kNsLanes) {
                    ++seen[ns_rev7(k)];
                    if (k != 0u && k != kNsPoints / 2u) ++seen[ns_rev7(kNsPoints - k)];
                    if (k != 0u) tmax = std::max(tmax, std::max(k, kNsPoints - k));
                }
            for (unsigned k = 1; k <= kNsPoints; ++k) {
                if (ns_band_of(k) < kNsBands) ++per[ns_band_of(k)]; else bands = 0;
                bands &= ns_band_of(k) == (k - 1u) / 4u;
            }
            bands &= std::all_of(per.begin(), per.end(), [](int v) { return v == 4; }) && ns_band_of(0) == 0u;
            std::printf("%d %d %u %d\n", invol, std::all_of(seen.begin(), seen.end(), [](int v) { return v == 1; }) ? 1 : 0, tmax, bands);
            continue;
        }
        unsigned long long C = std::stoull(head), F, n, g711, yard;
        std::cin >> F >> n >> g711 >> yard;
        const NsRoute r = ns_route((uint32_t)C, (uint32_t)F, (uint32_t)n, g711 != 0, yard != 0);
        long long visited = 0, once = 1, row_hi = -1, row_bytes = -1, lds_hi = -1, fetch_hi = -1, top_chan = -1;
        if (r.grid) {
            std::vector<int> seen(r.pieces, 0);
            for (unsigned u = 0; u < kNsTurns; ++u)
                for (unsigned lane = 0; lane < kNsLanes; ++lane) {
                    const unsigned p = u * kNsLanes + lane;
                    fetch_hi = std::max(fetch_hi, (long long)std::min(p, r.pieces - 1u));
                    if (p >= r.pieces) continue;
                    ++visited; ++seen[p];
                    row_hi = std::max(row_hi, 16ll * p + 16);
                }
            once = std::all_of(seen.begin(), seen.end(), [](int v) { return v == 1; }) ? 1 : 0;
            row_bytes = 2ll * (long long)n;
            lds_hi = (long long)(kNsChans - 1u) * ns_chan_bytes((uint32_t)n) + kNsStateBytes + kNsWorkBytes + row_hi;
            top_chan = (long long)(r.grid - 1u) * kNsChans + kNsChans - 1u;
        }
        std::printf("%u %u %u %d %d %u %lld %lld %lld %lld %lld %lld %lld %u %u %u %u %u %u %u %zu %zu\n", r.grid, r.threads, r.lds, r.in, r.copy ? 1 : 0, r.pieces, visited,
                    once, row_hi, row_bytes, lds_hi, fetch_hi, top_chan, kNsLanes, kNsChans, kNsResident, kNsVgprs, kNsTurns, kNsStateBytes, kNsWorkBytes,
                    sizeof(igdsp_ns_state), sizeof(NsWork));
    }
    return 0;
}
