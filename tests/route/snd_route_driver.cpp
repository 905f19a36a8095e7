// Prints the routes of igdsp_snd_combine / igdsp_snd_split (snd_route in csrc/igdsp_route.h) for tests/test_snd_route_cpu.py.  One case
// per stdin line: key=value pairs (numbers in any base strtoull reads): D, K, F, n, bulk, stats, yardstick (0 / 1), in, out (addresses:
// only their alignment matters), cus.  One output line per case: the route's fields as key=value.  The line "divcheck" instead checks
// snd_div against the division over the whole range the kernel uses (r < 4096, d = 1 .. 256) and prints bad=<number of mismatches>.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "igdsp_route.h"

using namespace igdsp;

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line == "divcheck") {
            unsigned bad = 0;
            for (uint32_t d = 1; d <= 256u; ++d)
                for (uint32_t r = 0; r < 4096u; ++r) bad += snd_div(r, snd_div_magic(d)) != r / d ? 1u : 0u;
            std::printf("bad=%u\n", bad);
            continue;
        }
        std::istringstream in(line);
        std::string kv;
        std::map<std::string, unsigned long long> a;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            a[kv.substr(0, eq)] = std::strtoull(kv.substr(eq + 1).c_str(), nullptr, 0);
        }
        auto g = [&](const char *key, unsigned long long dflt = 0) { return a.count(key) ? a[key] : dflt; };
        const SndRoute r = snd_route((uint32_t)g("D"), (uint32_t)g("K"), (uint32_t)g("F"), (uint32_t)g("n", 160), g("bulk", 1) != 0, g("stats", 1) != 0,
                                     g("yardstick") != 0, (uintptr_t)g("in", 0x1000), (uintptr_t)g("out", 0x2000), (uint32_t)g("cus", 256));
        std::printf("mode=%d vec=%u pieces=%u tail_dwords=%u items=%u grid=%u threads=%u lds=%u\n", r.mode, r.vec, r.pieces, r.tail_dwords, r.items,
                    r.grid, r.threads, r.mode == kSndCopy ? 0u : (uint32_t)kSndWaves * kSndTileBytes);
    }
    return 0;
}
