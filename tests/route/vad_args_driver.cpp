// Prints the verdicts of the voice detector's argument rule (vad_run in csrc/igdsp_args.h) for tests/test_vad_args_cpu.py.  One case per
// stdin line: key=value pairs: g711, codec, pcm, ctl, state, kind, rec, sid, txctl, events, count, work (a pointer is 0, x or x+k with x
// the buffer's own fixed 4096-aligned number, never dereferenced, or the name of another buffer with an optional +k for an address
// inside it), C, F, n, cap, and cfg=0 (NULL) or cfg=<thr_abs>:<nf_min>:<nf_max>:<sid_every>:<ratio_on_q4>:<ratio_off_q4>:<dn>:<up>:<up_v>:
// <asm_shift>:<burst>:<hang_long>:<hang_short>:<order>:<dtx>:<sid_delta>:<sid_gap>:<vox_on>:<vox_off>.  The buffers' numbers are 2^44
// apart: no shape the rule accepts makes two of them overlap by accident.  One output line per case: rc=<code> run=<0|1> why=<0|1>.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "igdsp_args.h"

using namespace igdsp::args;

int main()
{
    const char *names[12] = {"g711", "codec", "pcm", "ctl", "state", "kind", "rec", "sid", "txctl", "events", "count", "work"};
    std::map<std::string, uintptr_t> base;
    for (int i = 0; i < 12; ++i) base[names[i]] = 0x100000001000ull + ((uintptr_t)i << 44);
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
        igdsp_vad_cfg cfg{};
        const std::string &cs = a.at("cfg");
        const bool has_cfg = cs != "0";
        if (has_cfg) {
            unsigned long f[19] = {};
            const char *q = cs.c_str();
            for (int i = 0; i < 19 && q; ++i) {
                f[i] = std::strtoul(q, nullptr, 0);
                q = std::strchr(q, ':');
                if (q) ++q;
            }
            cfg = igdsp_vad_cfg{(uint32_t)f[0], (uint32_t)f[1], (uint32_t)f[2], (uint16_t)f[3], (uint8_t)f[4], (uint8_t)f[5], (uint8_t)f[6], (uint8_t)f[7],
                                (uint8_t)f[8], (uint8_t)f[9], (uint8_t)f[10], (uint8_t)f[11], (uint8_t)f[12], (uint8_t)f[13], (uint8_t)f[14],
                                (uint8_t)f[15], (uint8_t)f[16], (uint8_t)f[17], (uint8_t)f[18], {0, 0, 0}};
        }
        const Verdict v = vad_run(p("g711"), p("codec"), p("pcm"), p("ctl"), has_cfg ? &cfg : nullptr, u("C"), u("F"), u("n"), p("state"), p("kind"), p("rec"),
                                  p("sid"), p("txctl"), p("events"), u("cap"), p("count"), p("work"));
        if (v.run && (v.rc != IGDSP_OK || v.why)) return 3;                // a verdict that launches carries no code and no text
        std::printf("rc=%d run=%d why=%d\n", v.rc, v.run ? 1 : 0, v.why ? 1 : 0);
    }
    return 0;
}
