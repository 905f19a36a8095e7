// Prints the routes of igdsp_dbuf_run (dbuf_route in csrc/igdsp_route.h) for tests/test_dbuf_route_cpu.py, and runs the constexpr rule
// k_dbuf and igdsp_dbuf_step share (csrc/igdsp_dbuf.h).  One case per stdin line, the first word picks the kind, then key=value pairs
// (numbers in any base strtoull reads):
//   route   C, T, n, M, in, out (addresses: only their alignment matters) -> the route's fields
//   steps   n, M, ops (comma separated, one per step), x (the rows of the PUT steps in order, comma separated), and optionally the
//           scalars head, len, eff, level, max_level, since, last_op of the state to start from (the ring starts as zeros)
//           -> per step one line: the flag, len after the step, then the row of a GET; at the end one line with the scalars, the six
//           counters and the live samples
//   static  -> the compile-time checks below passed (the rule is usable in constant expressions)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "igdsp_dbuf.h"
#include "igdsp_route.h"

using namespace igdsp;

constexpr DbufSc after_update(DbufSc s, uint32_t op, uint32_t n, uint32_t M) { dbuf_update(s, op, n, M); return s; }
constexpr DbufSc after_read(DbufSc s, uint32_t M) { dbuf_read(s, M); return s; }
constexpr DbufSc kReset{};
static_assert(after_read(kReset, 960).eff == 480 && after_read(DbufSc{5000, 2000, 0, 0, 0, 60000, 9}, 960).head == 920, "the read rule");
static_assert(after_read(DbufSc{5000, 2000, 0, 0, 0, 60000, 9}, 960).since == 199 && after_read(DbufSc{0, 0, 5000, 0, 0, 0, 2}, 960).eff == 960);
static_assert(after_update(DbufSc{0, 0, 480, 7, 3, 0, 1}, 1, 160, 960).level == 8 && after_update(DbufSc{0, 0, 480, 65535, 3, 0, 1}, 1, 160, 960).level == 65535);
static_assert(after_update(DbufSc{0, 0, 480, 7, 3, 100, 1}, 2, 160, 960).since == 107 && after_update(DbufSc{0, 0, 480, 7, 3, 100, 1}, 2, 160, 960).max_level == 7);
static_assert(after_update(DbufSc{0, 0, 480, 2, 1, 198, 1}, 2, 160, 960).eff == (3 * 480 + 480) / 4 && after_update(DbufSc{0, 0, 480, 2, 1, 198, 1}, 2, 160, 960).since == 0);
static_assert(after_update(DbufSc{0, 0, 100, 9, 1, 198, 1}, 2, 160, 960).eff == (300 + 960) / 4, "the burst is capped at the maximum");
static_assert(pitch_key(5, 40) < pitch_key(5, 41) && pitch_key(4, 120) < pitch_key(5, 40) && pitch_w(0, 40) == 32768 / 41 && pitch_w(39, 40) == (40 << 15) / 41);
static_assert(dbuf_blend(-32768, -32768, 0, 40) == -32768 && dbuf_blend(32767, 32767, 119, 120) == 32767 && dbuf_blend(-32768, 32767, 59, 119) == 0);
static_assert(pitch_q15(-16385) == -1 && pitch_q15(-16384) == 0 && pitch_q15(16383) == 0 && pitch_q15(16384) == 1, "round half up, floor shift");
static_assert(kDbufLdsBytes * kDbufResident <= 160u * 1024u && kDbufLdsBytes == 4480 && dbuf_shape_ok(1, 2) && !dbuf_shape_ok(160, 319));

static std::vector<long> numbers(const std::string &s)
{
    std::vector<long> v;
    std::istringstream in(s);
    std::string t;
    while (std::getline(in, t, ',')) v.push_back(std::strtol(t.c_str(), nullptr, 0));
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
            const DbufRoute r = dbuf_route((uint32_t)g("C"), (uint32_t)g("T"), (uint32_t)g("n", 160), (uint32_t)g("M", 960), (uintptr_t)g("in", 0x1000),
                                           (uintptr_t)g("out", 0x2000));
            std::printf("vec=%u grid=%u threads=%u lds=%u part_steps=%u parts=%u\n", r.vec, r.grid, r.threads, r.lds, r.part_steps, r.parts);
        } else if (kind == "steps") {
            const uint32_t n = (uint32_t)g("n", 160), M = (uint32_t)g("M", 960);
            const std::vector<long> ops = numbers(a["ops"]), x = numbers(a["x"]);
            if (!dbuf_shape_ok(n, M)) { std::printf("einval\n"); continue; }
            igdsp_dbuf_state st{};
            st.head = (uint16_t)g("head"); st.len = (uint16_t)g("len"); st.eff = (uint16_t)g("eff"); st.level = (uint16_t)g("level");
            st.max_level = (uint16_t)g("max_level"); st.since = (uint16_t)g("since"); st.last_op = (uint16_t)g("last_op");
            std::vector<int16_t> row(n), out(n);
            size_t at = 0;
            for (long op : ops) {
                if (op & IGDSP_DBUF_PUT) {
                    if (at + n > x.size()) return 4;
                    for (uint32_t i = 0; i < n; ++i) row[i] = (int16_t)x[at + i];
                    at += n;
                }
                const uint32_t flag = dbuf_step_run(st, (uint32_t)op & 3u, row.data(), n, M, out.data());
                std::printf("%u %u", flag, st.len);
                if (op & IGDSP_DBUF_GET) for (uint32_t i = 0; i < n; ++i) std::printf(" %d", out[i]);
                std::printf("\n");
            }
            std::printf("%u %u %u %u %u %u %u %u %u %u %u %u %u", st.head, st.len, st.eff, st.level, st.max_level, st.since, st.last_op, st.underruns,
                        st.shrinks, st.shrunk, st.dropped, st.puts, st.gets);
            for (uint32_t k = 0; k < st.len; ++k) std::printf(" %d", st.ring[(st.head + k) % IGDSP_DBUF_CAP]);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown kind %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
