// Prints the routes of igdsp_jb_receive (jb_route and jb_ring_bytes in igdsp_route.h) for tests/test_jb_route_cpu.py.  One case per
// stdin line: key=value pairs (C, T, n, out: the payload output's address, alignment only).  One output line per case: the route's
// fields and the ring size as key=value.
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
        auto g = [&](const char *key, unsigned long long dflt) { return a.count(key) ? a[key] : dflt; };
        const uint32_t C = (uint32_t)g("C", 0), n = (uint32_t)g("n", 160);
        const JbRoute r = jb_route(C, (uint32_t)g("T", 0), n, g("out", 0x1000));
        std::printf("vec=%u pieces=%u grid=%u threads=%u part_ticks=%u parts=%u ring=%llu\n", r.vec, r.pieces, r.grid, r.threads, r.part_ticks,
                    r.parts, (unsigned long long)jb_ring_bytes(C, n));
    }
    return 0;
}
