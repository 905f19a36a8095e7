// Prints the routes of igdsp_tone_generate (tone_route in csrc/igdsp_route.h) for tests/test_tone_route_cpu.py, and runs the constexpr
// tone rules k_tone and igdsp_tone_frame share.  One case per stdin line, the first word picks the kind, then key=value pairs (numbers
// in any base strtoull reads):
//   route   P, F, n, pcm, stats, yardstick (0 / 1), out (an address: only its alignment matters), cus -> the route's fields
//   sample  step1, step2, vol, on, fade_in, fade_out, k0, count -> tone_sample at k0 .. k0 + count - 1
//   frames  clock, options, tones (f1:f2:on_ms:off_ms:vol, comma separated), pos, flags, cmd (applied to the first frame), n, frames
//           -> per frame one line: len pos flags, then the n samples (tone_plan_make, tone_cmd, tone_frame_sample, tone_advance)
//   static  -> the compile-time checks below passed (the rules are usable in constant expressions)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "igdsp_route.h"

using namespace igdsp;

constexpr igdsp_tone_seg kSeg{0u, 800u, 236223201u, 257698038u, 12288u, 8u, 16u, 0u};    // 440 + 480 Hz at 8 kHz
static_assert(tone_sample(kTonePairs.w, kSeg, 0u) == 0 && tone_osc(kTonePairs.w, 1u << 30) == 32767 && tone_osc(kTonePairs.w, 3u << 30) == -32767);
static_assert(kToneSin[256] == 32767 && kToneSin[768] == -32767 && (kTonePairs.w[255] >> 16) == 1u && sizeof(igdsp_tone_plan) == 208);

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, kv;
        std::map<std::string, std::string> a;
        in >> kind;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            a[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        auto g = [&](const char *key, unsigned long long dflt = 0) { return a.count(key) ? std::strtoull(a[key].c_str(), nullptr, 0) : dflt; };
        if (kind == "static") {
            std::printf("ok=1\n");
        } else if (kind == "route") {
            const ToneRoute r = tone_route((uint32_t)g("P"), (uint32_t)g("F"), (uint32_t)g("n", 160), g("pcm", 1) != 0, g("stats", 1) != 0,
                                           g("yardstick") != 0, (uintptr_t)g("out", 0x1000), (uint32_t)g("cus", 256));
            std::printf("mode=%d vec=%u pieces=%u groups=%u chunk_frames=%u chunks=%u grid=%u threads=%u state_grid=%u lds=%u\n", r.mode, r.vec, r.pieces,
                        r.groups, r.chunk_frames, r.chunks, r.grid, r.threads, r.state_grid, r.mode == kToneFill ? 0u : 4096u);
        } else if (kind == "sample") {
            const igdsp_tone_seg sg{0u, (uint32_t)g("on"), (uint32_t)g("step1"), (uint32_t)g("step2"), (uint16_t)g("vol"), (uint16_t)g("fade_in"),
                                    (uint16_t)g("fade_out"), 0u};
            for (uint32_t k = (uint32_t)g("k0"), e = k + (uint32_t)g("count"); k < e; ++k) std::printf("%d ", tone_sample(kTonePairs.w, sg, k));
            std::printf("\n");
        } else if (kind == "frames") {
            igdsp_tone_desc d[IGDSP_TONE_MAX + 1] = {};
            uint32_t count = 0;
            std::istringstream ts(a["tones"]);
            std::string t;
            while (std::getline(ts, t, ',') && count <= IGDSP_TONE_MAX) {
                unsigned v[5] = {0, 0, 0, 0, 0};
                std::sscanf(t.c_str(), "%u:%u:%u:%u:%u", &v[0], &v[1], &v[2], &v[3], &v[4]);
                d[count++] = igdsp_tone_desc{(uint16_t)v[0], (uint16_t)v[1], (uint16_t)v[2], (uint16_t)v[3], (uint16_t)v[4], 0};
            }
            igdsp_tone_plan plan{};
            if (!tone_plan_make(d, count, (uint32_t)g("clock", 8000), (uint32_t)g("options", 1), plan)) { std::printf("einval\n"); continue; }
            igdsp_tone_state st{(uint32_t)g("pos"), (uint32_t)g("flags", 1)};
            const uint32_t n = (uint32_t)g("n", 160);
            for (uint32_t f = 0, F = (uint32_t)g("frames", 1); f < F; ++f) {
                const uint32_t cmd = f == 0 ? (uint32_t)g("cmd") : 0u;
                const igdsp_tone_state s = tone_cmd(st, cmd);
                const bool hold = (cmd & IGDSP_TONE_CMD_HOLD) != 0u, live = !hold && tone_plays(plan, s) && tone_live(plan, s.pos);
                st = hold ? s : tone_advance(plan, s, n);
                std::printf("%u %u %u", live ? n : 0u, st.pos, st.flags);
                for (uint32_t i = 0; i < n; ++i) std::printf(" %d", live ? tone_frame_sample(kTonePairs.w, plan, s.pos, i) : 0);
                std::printf("\n");
            }
        } else {
            std::fprintf(stderr, "unknown kind %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
