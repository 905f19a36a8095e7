// Prints tdet_route (csrc/igdsp_route.h) for tests/test_tdet_route_cpu.py.  One case per stdin line: C F n list with_rec; one output line
// per case: grid threads lds e0 waves list_grid counts_bytes work_bytes, then what the geometry has to cover for the kernel's indices
// to stay in bounds: the last LDS value a frame of n touches (store behind the history, the history's move), the table entries a plan
// fills, and the last byte of d_work the list's passes touch.
#include <cstdio>
#include <iostream>

#include "igdsp_route.h"

using namespace igdsp;

int main()
{
    unsigned long long C, F, n, list, with_rec;
    while (std::cin >> C >> F >> n >> list >> with_rec) {
        const TdetRoute r = tdet_route((uint32_t)C, (uint32_t)F, (uint32_t)n, list != 0, with_rec != 0);
        const unsigned long long h = n / 2;
        const unsigned long long last_store = 128 + 4 * ((h + 1) / 2) - 1;         // the last value the sums read: the frame, rounded up to two pairs
        const unsigned long long last_move = 2 * (h + 63) + 1;                     // the last value the history's move reads
        const unsigned long long tab_entries = ((h + 1) / 2) * 16;           // 16-byte entries: two sample pairs each
        const unsigned long long counts_end = kLinkWorkHead + F * r.waves * 4ull;
        const unsigned long long rec_end = r.counts_bytes + (with_rec ? 0 : C * F * 8ull);
        std::printf("%u %u %u %u %u %u %llu %llu %llu %llu %llu %llu %llu %u %u\n", r.grid, r.threads, r.lds, r.e0, r.waves, r.list_grid,
                    (unsigned long long)r.counts_bytes, (unsigned long long)r.work_bytes, last_store, last_move, tab_entries, counts_end, rec_end,
                    kTdetBuf, kTdetChans);
    }
    return 0;
}
