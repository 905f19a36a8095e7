// Prints the verdicts of the sound-card argument rules (snd_combine / snd_split in csrc/igdsp_args.h) for tests/test_snd_args_cpu.py.
// One case per stdin line: the rule's name, then key=value pairs: in, bulk, stats (a pointer is 0, a or a+k; a: a fixed 4096-aligned
// number, never dereferenced; "in" for bulk passes the input pointer itself), D, K, F, n (anything strtoull reads).  One output line
// per case: rc=<code> run=<0|1> why=<0|1>.
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
    constexpr uintptr_t kA = 0x7f0000001000ull, kB = 0x7f0000801000ull, kS = 0x7f0001001000ull;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string entry, kv;
        std::map<std::string, std::string> a;
        in >> entry;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            a[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        auto u = [&](const char *key) { return (uint32_t)std::strtoull(a.at(key).c_str(), nullptr, 0); };
        auto p = [&](const char *key, uintptr_t base) -> const void * {
            const std::string &v = a.at(key);
            if (v[0] != 'a') return reinterpret_cast<const void *>((uintptr_t)std::strtoull(v.c_str(), nullptr, 0));
            return reinterpret_cast<const void *>(base + (v.size() > 1 ? std::strtoull(v.c_str() + 1, nullptr, 0) : 0));
        };
        const void *src = p("in", kA);
        const void *bulk = a.at("bulk") == "in" ? src : p("bulk", kB);
        const void *stats = p("stats", kS);
        Verdict v{};
        if (entry == "snd_combine") v = snd_combine(src, u("D"), u("K"), u("F"), u("n"), bulk, stats);
        else if (entry == "snd_split") v = snd_split(src, u("D"), u("K"), u("F"), u("n"), bulk, stats);
        else { std::fprintf(stderr, "unknown entry %s\n", entry.c_str()); return 2; }
        if (v.run && (v.rc != IGDSP_OK || v.why)) return 3;                // a verdict that launches carries no code and no text
        std::printf("rc=%d run=%d why=%d\n", v.rc, v.run ? 1 : 0, v.why ? 1 : 0);
    }
    return 0;
}
