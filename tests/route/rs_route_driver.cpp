// Prints the routes of igdsp_resample (rs_route in csrc/igdsp_route.h) for tests/test_rs_route_cpu.py, and runs the constexpr rules k_rs
// and igdsp_rs_frame share.  One case per stdin line, the first word picks the kind, then key=value pairs (numbers in any base
// strtoull reads):
//   route   dir, R, C, F, n, g711, yardstick (0 / 1), in, out (addresses: only their alignment matters), cus, blocks (the
//           IGDSP_RS_BLOCKS knob, absent: none) -> the route's fields and rs_resident
//   pairs   dir, R -> rs_pair of every phase (UP: R of them, DOWN: one) and even window offset: the dwords k_rs multiplies by
//   frames  dir, R, n_in, hist (144 values, comma separated, or absent: silence), x (the input of all frames, comma separated)
//           -> per frame one line: the clamp flag, the state's frames, then the outputs; at the end one line with the history
//   static  -> the compile-time checks below passed (the rules are usable in constant expressions)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "igdsp_route.h"

using namespace igdsp;

constexpr int16_t kOnes[24] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
static_assert(rs_up_raw(kRsUp2, 0, kOnes + 23) == 1 && rs_up_raw(kRsUp6, 5, kOnes + 23) == 1, "a phase sums to 16384");
static_assert(kRsUp2[0] == -3 && kRsUp2[12] == 14141 && kRsDown2[23] == 7074 && kRsDown6[72] == 2567 && kRsUp6[11] == 2209);
static_assert(rs_pair(IGDSP_RS_UP, 2, 0, 0) == ((uint32_t)(uint16_t)kRsUp2[23] | ((uint32_t)(uint16_t)kRsUp2[22] << 16)));
static_assert(rs_pair(IGDSP_RS_DOWN, 6, 0, 142) == ((uint32_t)(uint16_t)kRsDown6[1] | ((uint32_t)(uint16_t)kRsDown6[0] << 16)));
static_assert(rs_table(2, 2) == nullptr && rs_table(0, 5) == nullptr && rs_clamp16(69900) == 32767 && rs_round(-1) == 0 && rs_round(-8193) == -1);
static_assert(sizeof(igdsp_rs_state) == 296 && rs_lds_bytes(IGDSP_RS_DOWN, 6) <= 65536 && rs_hist(IGDSP_RS_DOWN, 6) == kRsHist);
static_assert(rs_resident(IGDSP_RS_UP, 6) == 3 && rs_resident(IGDSP_RS_DOWN, 6) == 2 && rs_resident(IGDSP_RS_DOWN, 2) == 3);

static std::vector<int16_t> numbers(const std::string &s)
{
    std::vector<int16_t> v;
    std::istringstream in(s);
    std::string t;
    while (std::getline(in, t, ',')) v.push_back((int16_t)std::strtol(t.c_str(), nullptr, 0));
    return v;
}

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
            const uint32_t dir = (uint32_t)g("dir"), R = (uint32_t)g("R", 2);
            const RsRoute r = rs_route(dir, R, (uint32_t)g("C"), (uint32_t)g("F"), (uint32_t)g("n", 160), g("g711") != 0, g("yardstick") != 0,
                                       (uintptr_t)g("in", 0x1000), (uintptr_t)g("out", 0x2000), (uint32_t)g("cus", 256),
                                       a.count("blocks") ? std::optional<int>((int)g("blocks")) : std::nullopt);
            std::printf("vec=%u pieces=%u ch=%u groups=%u chunk_frames=%u chunks=%u grid=%u threads=%u lds=%u state_grid=%u resident=%u\n", r.vec, r.pieces,
                        r.ch, r.groups, r.chunk_frames, r.chunks, r.grid, r.threads, r.lds, r.state_grid, rs_table(dir, R) ? rs_resident(dir, R) : 0u);
        } else if (kind == "pairs") {
            const uint32_t dir = (uint32_t)g("dir"), R = (uint32_t)g("R", 2), phases = dir == IGDSP_RS_UP ? R : 1u;
            const uint32_t len = dir == IGDSP_RS_UP ? kRsTaps : kRsTaps * R;
            for (uint32_t p = 0; p < phases; ++p)
                for (uint32_t t0 = 0; t0 < len; t0 += 2) std::printf("%u ", rs_pair(dir, R, p, t0));
            std::printf("\n");
        } else if (kind == "frames") {
            const uint32_t dir = (uint32_t)g("dir"), R = (uint32_t)g("R", 2), n_in = (uint32_t)g("n_in", 160);
            const std::vector<int16_t> x = numbers(a["x"]), h = numbers(a["hist"]);
            if (!rs_table(dir, R) || n_in == 0 || n_in > IGDSP_MAX_PAYLOAD * R || x.size() % n_in) { std::printf("einval\n"); continue; }
            igdsp_rs_state st{};
            for (size_t i = 0; i < h.size() && i < kRsHist; ++i) st.hist[i] = h[i];
            std::vector<int16_t> out(n_in * R);
            for (size_t at = 0; at < x.size(); at += n_in) {
                bool sat = false;
                rs_frame_run(st, dir, R, x.data() + at, n_in, out.data(), &sat);
                std::printf("%d %u", sat ? 1 : 0, st.frames);
                for (uint32_t i = 0, n_out = dir == IGDSP_RS_UP ? n_in * R : n_in / R; i < n_out; ++i) std::printf(" %d", out[i]);
                std::printf("\n");
            }
            for (uint32_t i = 0; i < kRsHist; ++i) std::printf("%d ", st.hist[i]);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown kind %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
