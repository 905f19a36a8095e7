// Prints the verdicts of the AES-GCM SRTP entries' argument rule (srtp_gcm_run in csrc/igdsp_args.h) for tests/test_srtp_gcm_args_cpu.py.  One case per
// stdin line: key=value pairs: ctl, packets, sizes, state, out, sizes_out, rec (a pointer is 0, x or x+k with x the buffer's own fixed
// 4096-aligned number, never dereferenced, or the name of another buffer with an optional +k for an address inside it), C, F, stride,
// ostride.  The buffers' numbers are 2^44 apart: no shape the rule accepts makes two of them overlap by accident.  One output line per
// case: rc=<code> run=<0|1> why=<0|1>.
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
    const char *names[7] = {"ctl", "packets", "sizes", "state", "out", "sizes_out", "rec"};
    std::map<std::string, uintptr_t> base;
    for (int i = 0; i < 7; ++i) base[names[i]] = 0x100000001000ull + ((uintptr_t)i << 44);
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
            const size_t plus = v.find('+');
            const std::string head = v.substr(0, plus);
            const uintptr_t off = plus == std::string::npos ? 0 : (uintptr_t)std::strtoull(v.c_str() + plus + 1, nullptr, 0);
            if (base.count(head)) return reinterpret_cast<const void *>(base.at(head) + off);                     // (inside) another buffer
            if (v[0] != 'x') return reinterpret_cast<const void *>((uintptr_t)std::strtoull(v.c_str(), nullptr, 0));
            return reinterpret_cast<const void *>(base.at(key) + (v.size() > 1 ? std::strtoull(v.c_str() + 1, nullptr, 0) : 0));
        };
        const Verdict v = srtp_gcm_run(p("ctl"), p("packets"), p("sizes"), u("C"), u("F"), u("stride"), p("state"), p("out"), u("ostride"), p("sizes_out"), p("rec"));
        if (v.run && (v.rc != IGDSP_OK || v.why)) return 3;                // a verdict that launches carries no code and no text
        std::printf("rc=%d run=%d why=%d\n", v.rc, v.run ? 1 : 0, v.why ? 1 : 0);
    }
    return 0;
}
