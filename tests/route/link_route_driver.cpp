// Prints the routes of igdsp_link_watch (link_route and link_work_bytes in igdsp_route.h) for tests/test_link_route_cpu.py.  One case
// per stdin line: key=value pairs (numbers in any base strtoull reads): C, T, list (0 / 1: an event list is requested).  One output
// line per case: the route's fields as key=value, and work = link_work_bytes(C, T) whether or not a list is requested.
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
        const LinkRoute r = link_route((uint32_t)g("C"), (uint32_t)g("T"), g("list") != 0);
        std::printf("waves=%u grid=%u threads=%u part_ticks=%u parts=%u passes=%u scan_threads=%u work_bytes=%llu work=%llu\n", r.waves, r.grid,
                    r.threads, r.part_ticks, r.parts, r.passes, r.scan_threads, (unsigned long long)r.work_bytes,
                    (unsigned long long)link_work_bytes((uint32_t)g("C"), (uint32_t)g("T")));
    }
    return 0;
}
