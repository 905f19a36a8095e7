// Prints srtp_gcm_route (csrc/igdsp_route.h) for tests/test_srtp_gcm_route_cpu.py.  One case per stdin line: C F stride ostride dir
// yardstick; one output line per case: grid threads lds dir move max_pieces, then what the geometry has to cover for the kernel's indices
// to stay in bounds, walked as the kernel walks (tests/route/srtp_route_driver.cpp's walk over every piece j < max_pieces and the four
// turns of the 64 lanes: items visited, each (row, quarter) once, the highest tile word, the highest byte of a slot a load reaches, the
// bytes covered, the grid's highest leg), then GHASH's slots: over every header length h = 12, 16, .. and every end in [h, stride] the
// most pieces a pass walks (srtp_gcm_pieces) and whether, within those pieces' 4 slots each, exactly ceil(h / 16) slots are AAD blocks
// and exactly ceil((end - h) / 16) are ciphertext blocks, each block once and in order; and the constants.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <vector>

#include "igdsp_route.h"
#include "igdsp_srtp_gcm.h"

using namespace igdsp;

int main()
{
    unsigned long long C, F, stride, ostride, dir, yard;
    while (std::cin >> C >> F >> stride >> ostride >> dir >> yard) {
        const SrtpRoute r = srtp_gcm_route((uint32_t)C, (uint32_t)F, (uint32_t)stride, (uint32_t)ostride, (int)dir, yard != 0);
        long long visited = 0, once = 1, tile_hi = -1, slot_hi = -1, top_chan = -1, covered = 0, pieces_hi = 0, slots_ok = 1;
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
            for (uint32_t h = 12; h <= stride; h += 4u)
                for (uint32_t end = h; end <= stride; ++end) {
                    const uint32_t nb = srtp_gcm_pieces(h, end), hw = h >> 2, hq = hw >> 2, nct = (end - h + 15u) >> 4;
                    pieces_hi = std::max(pieces_hi, (long long)nb);
                    uint32_t aad = 0, ct = 0, next_ct = 0;
                    bool ok = nb >= (end + 63u) / 64u;                     // the data's pieces are all walked
                    for (uint32_t slot = 0; slot < 4u * nb; ++slot) {
                        const bool a = 4u * slot < hw;
                        const int32_t idx = (int32_t)slot - 1 - (int32_t)hq;
                        if (a) { ok = ok && ct == 0; ++aad; }
                        else if (idx >= 0 && (uint32_t)idx < nct) { ok = ok && (uint32_t)idx == next_ct; ++next_ct; ++ct; }
                    }
                    if (!ok || aad != (h + 15u) / 16u || ct != nct) slots_ok = 0;
                }
        }
        std::printf("%u %u %u %d %d %u %lld %lld %lld %u %lld %lld %lld %u %u %u %u %u %u %zu %zu %lld %lld\n", r.grid, r.threads, r.lds, r.dir, r.move ? 1 : 0,
                    r.max_pieces, visited, once, tile_hi, kSrtpChans * kSrtpPitch, slot_hi, covered, top_chan, kSrtpChans, kSrtpPitch, kSrtpTurns, kSrtpGcmResident,
                    kSrtpGcmVgprs, kSrtpGcmLdsBytes, sizeof(igdsp_srtp_gcm_state), sizeof(igdsp_srtp_rec), pieces_hi, slots_ok);
    }
    return 0;
}
