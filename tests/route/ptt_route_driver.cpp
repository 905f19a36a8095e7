// Prints the routes of igdsp_ptt_arbitrate (ptt_route in igdsp_route.h) for tests/test_ptt_route_cpu.py.  One case per stdin line:
// key=value pairs (numbers in any base strtoull reads): G, F, n (160), members, form (0 G.711 / 1 PCM / 2 none), in, out (buffer
// addresses, alignment only).  One output line per case: the route's fields as key=value.
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
        std::istringstream in(line);
        std::string kv;
        std::map<std::string, unsigned long long> a;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            a[kv.substr(0, eq)] = std::strtoull(kv.substr(eq + 1).c_str(), nullptr, 0);
        }
        auto g = [&](const char *key, unsigned long long dflt = 0) { return a.count(key) ? a[key] : dflt; };
        const PttRoute r = ptt_route((uint32_t)g("G"), (uint32_t)g("F"), (uint32_t)g("n", 160), (uint32_t)g("members"), (int)g("form"),
                                     g("in", 0x1000), g("out", 0x1000));
        std::printf("form=%d gpw=%u vec_in=%u vec_out=%u grid=%u threads=%u part_frames=%u parts=%u pass_frames=%u slots_grid=%u\n", r.form, r.gpw,
                    r.vec_in, r.vec_out, r.grid, r.threads, r.part_frames, r.parts, r.pass_frames, r.slots_grid);
    }
    return 0;
}
