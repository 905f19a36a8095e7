// Prints the verdicts of the rate converter's argument rule (resample in csrc/igdsp_args.h) for tests/test_rs_args_cpu.py.  One case per
// stdin line: key=value pairs: payload, codec, pcm, len, state, out, stats (a pointer is 0, x or x+k with x the buffer's own fixed
// 4096-aligned number, never dereferenced, or the name of another buffer for the same address), dir, R, layout, C, F, n, rn, rw
// (anything strtoull reads).  One output line per case: rc=<code> run=<0|1> why=<0|1>.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "igdsp_args.h"

using namespace igdsp::args;

int main()
{
    const std::map<std::string, uintptr_t> base = {{"payload", 0x7f0000001000ull}, {"codec", 0x7f0000101000ull}, {"pcm", 0x7f0000201000ull},
                                                   {"len", 0x7f0000301000ull}, {"state", 0x7f0000401000ull}, {"out", 0x7f0000501000ull},
                                                   {"stats", 0x7f0000601000ull}};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kv;
        std::map<std::string, std::string> a;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            a[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        auto u = [&](const char *key) { return (uint32_t)std::strtoull(a.at(key).c_str(), nullptr, 0); };
        auto p = [&](const char *key) -> const void * {
            const std::string &v = a.at(key);
            if (base.count(v)) return reinterpret_cast<const void *>(base.at(v));                         // another buffer's address
            if (v[0] != 'x') return reinterpret_cast<const void *>((uintptr_t)std::strtoull(v.c_str(), nullptr, 0));
            return reinterpret_cast<const void *>(base.at(key) + (v.size() > 1 ? std::strtoull(v.c_str() + 1, nullptr, 0) : 0));
        };
        const Verdict v = resample(u("dir"), u("R"), u("layout"), p("payload"), p("codec"), p("pcm"), p("len"), p("state"), u("C"), u("F"), u("n"),
                                   u("rn"), u("rw"), p("out"), p("stats"));
        if (v.run && (v.rc != IGDSP_OK || v.why)) return 3;                // a verdict that launches carries no code and no text
        std::printf("rc=%d run=%d why=%d\n", v.rc, v.run ? 1 : 0, v.why ? 1 : 0);
    }
    return 0;
}
