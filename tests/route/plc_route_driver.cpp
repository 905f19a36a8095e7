// Prints the routes of igdsp_plc_conceal (plc_route in igdsp_route.h) for tests/test_plc_route_cpu.py.  One case per stdin line:
// key=value pairs (C, T, n, pcm: 1 for the PCM input, in / out: the input's and the output's addresses, alignment only).  One output
// line per case: the route's fields as key=value.
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
        const PlcRoute r = plc_route((uint32_t)g("C", 0), (uint32_t)g("T", 0), (uint32_t)g("n", 160), g("pcm", 0) != 0, g("in", 0x1000),
                                     g("out", 0x1000));
        std::printf("vec=%u pieces=%u batch_rows=%u grid=%u threads=%u part_ticks=%u parts=%u\n", r.vec, r.pieces, r.batch_rows, r.grid,
                    r.threads, r.part_ticks, r.parts);
    }
    return 0;
}
