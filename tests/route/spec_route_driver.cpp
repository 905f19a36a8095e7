// Prints the routes of igdsp_spectrum (spec_route in csrc/igdsp_route.h) for tests/test_spec_route_cpu.py, and runs the rule k_spec and
// igdsp_spec_frame share (csrc/igdsp_spec.h).  One case per stdin line, the first word picks the kind, then key=value pairs (numbers in
// any base strtoull reads):
//   route   C, F, n -> the route's fields
//   flow    -> the data flow's index functions checked over all 64 lanes and 8 registers: every pass's tile stores hit distinct slots
//           inside the tile, its loads read exactly the slots stored, pass 3 covers every bin once, the mirror is an involution that pairs
//           bin k with bin (512 - k) % 512; and the bank spread of each exchange: the largest number of lanes of a 32-lane group on one of
//           the 64 dword banks (an 8-byte access takes two)
//   frames  n, hop, alpha, x (the rows' samples in order, comma separated; their count picks the frames) -> per frame one line: the
//           record's flags, peak_bin, peak_db (%a) and, on a hop, the 512 raw values (%a); at the end the state: since, hops, flags, then
//           the 1 024 history samples and the 512 averaged values (%a)
//   static  -> the compile-time checks below passed
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "igdsp_route.h"
#include "igdsp_spec.h"

using namespace igdsp;

static_assert(kSpecLdsBytes == 4 * (2048 + 4608) && kSpecLdsBytes * kSpecResident <= 160u * 1024u, "the residency's LDS");
static_assert(spec_since_read(0, 1) == 0 && spec_since_read(5, 3) == 2 && spec_since_read(2, 3) == 2 && spec_since_read(0xFFFFFFFFu, 0xFFFFFFFFu) == 0xFFFFFFFEu);
static_assert(spec_first_hop(0, 1) == 0 && spec_first_hop(0, 7) == 6 && spec_first_hop(6, 7) == 0 && spec_last_hop(0, 1, 13) == 12 && spec_last_hop(0, 7, 13) == 6);
static_assert(spec_last_hop(0, 7, 14) == 13 && spec_last_hop(3, 7, 3) == 3 && spec_last_hop(3, 7, 4) == 3 && spec_last_hop(0, 20, 13) == 13, "F: no hop in the launch");
static_assert(spec_cfg_ok(igdsp_spec_cfg{1, 1.0f}) && !spec_cfg_ok(igdsp_spec_cfg{0, 0.25f}) && !spec_cfg_ok(igdsp_spec_cfg{1, 0.0f}) && spec_cfg_or_default(nullptr).alpha == 0.25f);
static_assert(spec_mirror_lane(0) == 0 && spec_mirror_lane(1) == 63 && spec_mirror_reg(0, 0) == 0 && spec_mirror_reg(0, 1) == 7 && spec_mirror_reg(5, 0) == 7);
static_assert(kSpecWin[0] == 0.0f && kSpecWin[512] == 1.0f && kSpecTw[0] == 1.0f && kSpecTw[2 * 256 + 1] == -1.0f && kSpecTw[2 * 512] == -1.0f, "the tables");

static std::vector<long> numbers(const std::string &s)
{
    std::vector<long> v;
    std::istringstream in(s);
    std::string t;
    while (std::getline(in, t, ',')) v.push_back(std::strtol(t.c_str(), nullptr, 0));
    return v;
}

// the most lanes of one 32-lane group on one dword bank, for 8-byte accesses at the given complex-point slots
template <class Fn> static unsigned worst_bank(Fn slot)
{
    unsigned worst = 0;
    for (uint32_t q = 0; q < 8; ++q)
        for (uint32_t g = 0; g < 2; ++g) {
            unsigned count[64] = {};
            for (uint32_t l = 0; l < 32; ++l) {
                const uint32_t dw = 2u * slot(32u * g + l, q);
                ++count[dw % 64u];
            }
            for (unsigned c : count) worst = std::max(worst, c);
        }
    return worst;
}

static int flow()
{
    std::set<uint32_t> s1, s2, l1, l2, bins;
    for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint32_t q = 0; q < 8; ++q) {
            s1.insert(spec_x1_store(lane, q)); l1.insert(spec_x1_load(lane, q));
            s2.insert(spec_x2_store(lane, q)); l2.insert(spec_x2_load(lane, q));
            bins.insert(spec_bin(lane, q));
            if (spec_x1_store(lane, q) >= kSpecTile || spec_x2_store(lane, q) >= kSpecTile) return 1;
            if (spec_tw1(lane, q) >= kSpecN || spec_tw2(lane, q) >= kSpecN || spec_in_point(lane, q) >= kSpecN / 2) return 2;
            // the point pass 2's lane (k0, c) loads as register b is the one pass 1's lane (b, c) stored as register k0
            const uint32_t k0 = lane >> 3, c = lane & 7u;
            if (spec_x1_load(lane, q) != spec_x1_store(8u * q + c, k0)) return 3;
            // the point pass 3's lane k0 + 8 k1 loads as register c is the one pass 2's lane (k0, c) stored as register k1
            const uint32_t kk0 = lane & 7u, kk1 = lane >> 3;
            if (spec_x2_load(lane, q) != spec_x2_store(8u * kk0 + q, kk1)) return 4;
            const uint32_t k = spec_bin(lane, q), pk = spec_bin(spec_mirror_lane(lane), spec_mirror_reg(lane, q));
            if (pk != (512u - k) % 512u) return 5;
        }
    if (s1.size() != 512 || s2.size() != 512 || l1 != s1 || l2 != s2 || bins.size() != 512 || *bins.rbegin() != 511) return 6;
    std::printf("ok=1 x1_store=%u x1_load=%u x2_store=%u x2_load=%u\n", worst_bank(spec_x1_store), worst_bank(spec_x1_load), worst_bank(spec_x2_store),
                worst_bank(spec_x2_load));
    return 0;
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
            const SpecRoute r = spec_route((uint32_t)g("C"), (uint32_t)g("F"), (uint32_t)g("n", 160));
            std::printf("grid=%u threads=%u lds=%u\n", r.grid, r.threads, r.lds);
        } else if (kind == "flow") {
            if (const int rc = flow()) { std::printf("ok=0 at=%d\n", rc); return 5; }
        } else if (kind == "frames") {
            const uint32_t n = (uint32_t)g("n", 160);
            const igdsp_spec_cfg cfg{(uint32_t)g("hop", 1), a.count("alpha") ? std::strtof(a["alpha"].c_str(), nullptr) : 0.25f};
            const std::vector<long> x = numbers(a["x"]);
            if (!spec_n_ok(n) || !spec_cfg_ok(cfg)) { std::printf("einval\n"); continue; }
            igdsp_spec_state st{};
            std::vector<int16_t> row(n);
            std::vector<float> raw(kSpecBins);
            for (size_t at = 0; at + n <= x.size(); at += n) {
                for (uint32_t i = 0; i < n; ++i) row[i] = (int16_t)x[at + i];
                igdsp_spec_rec rec;
                spec_frame_run(st, row.data(), n, cfg, &rec, raw.data());
                std::printf("%u %u %a", rec.flags, rec.peak_bin, rec.peak_db);
                if (rec.flags & IGDSP_SPEC_HOP) for (float v : raw) std::printf(" %a", v);
                std::printf("\n");
            }
            std::printf("%u %u %u", st.since, st.hops, st.flags);
            for (int16_t v : st.hist) std::printf(" %d", v);
            for (float v : st.avg) std::printf(" %a", v);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown kind %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
