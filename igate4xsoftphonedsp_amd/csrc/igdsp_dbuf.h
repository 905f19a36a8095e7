// igdsp_dbuf.h — the delay buffer's rule (include/igdsp.h, "Delay buffer"; independent restatement: tests/dbuf_model.py) as constexpr
// functions in plain C++17, so that the host entry igdsp_dbuf_step (dbuf_step_run below), the kernel k_dbuf and
// tests/route/dbuf_route_driver.cpp run the same code.  The rule works on the scalars of a channel (DbufSc, every field widened to
// 32 bits); where the samples live is the caller's business: dbuf_step_run moves them in the state's ring on the host, k_dbuf moves
// them wave-wide.  The shrink's search key, weight and rounding are the concealment's (igdsp_pitch.h).
#pragma once
#include <cstddef>
#include <cstdint>

#include "igdsp.h"
#include "igdsp_pitch.h"

namespace igdsp {

static_assert(sizeof(igdsp_dbuf_state) == 2112 && alignof(igdsp_dbuf_state) == 4, "igdsp_dbuf_state layout (capi.DBUF_STATE mirrors it)");
static_assert(IGDSP_DBUF_WIN == IGDSP_PLC_HIST && 2 * IGDSP_PLC_PMAX <= IGDSP_DBUF_WIN, "the blend reads two periods inside the search window");
static_assert(offsetof(igdsp_dbuf_state, gets) == offsetof(igdsp_dbuf_state, underruns) + 20, "the six counters are one array of dwords");
static_assert(2 * IGDSP_MAX_PAYLOAD <= IGDSP_DBUF_CAP && (IGDSP_DBUF_CAP & (IGDSP_DBUF_CAP - 1)) == 0, "two of the largest frames fit; CAP is a power of two");

constexpr uint32_t kDbufCap = IGDSP_DBUF_CAP, kDbufWin = IGDSP_DBUF_WIN;

constexpr bool dbuf_shape_ok(uint32_t n, uint32_t M) { return n != 0 && n <= IGDSP_MAX_PAYLOAD && M >= 2u * n && M <= kDbufCap; }

// a channel's scalars (igdsp_dbuf_state without the ring)
struct DbufSc {
    uint32_t head, len, eff, level, max_level, since, last_op;
    uint32_t underruns, shrinks, shrunk, dropped, puts, gets;
};

// ring position of buffered sample k
constexpr uint32_t dbuf_pos(const DbufSc &s, uint32_t k) { return (s.head + k) % kDbufCap; }

// ---- on reading a state: a garbage state stays in bounds
constexpr void dbuf_read(DbufSc &s, uint32_t M)
{
    s.head %= kDbufCap;
    if (s.len > M) { s.head = (s.head + (s.len - M)) % kDbufCap; s.len = M; }
    s.eff = s.eff == 0 ? M >> 1 : (s.eff < M ? s.eff : M);
    if (s.last_op != IGDSP_DBUF_PUT && s.last_op != IGDSP_DBUF_GET) s.last_op = 0;
    if (s.since > IGDSP_DBUF_RECALC - 1u) s.since = IGDSP_DBUF_RECALC - 1u;
}
constexpr DbufSc dbuf_load(const igdsp_dbuf_state &st, uint32_t M)
{
    DbufSc s{st.head, st.len, st.eff, st.level, st.max_level, st.since, st.last_op, st.underruns, st.shrinks, st.shrunk, st.dropped, st.puts, st.gets};
    dbuf_read(s, M);
    return s;
}
constexpr void dbuf_store_live(igdsp_dbuf_state &st, const DbufSc &s)             // reserved0 and reserved[] stay as they are
{
    st.head = (uint16_t)s.head; st.len = (uint16_t)s.len; st.eff = (uint16_t)s.eff; st.level = (uint16_t)s.level;
    st.max_level = (uint16_t)s.max_level; st.since = (uint16_t)s.since; st.last_op = (uint16_t)s.last_op;
}
constexpr void dbuf_store(igdsp_dbuf_state &st, const DbufSc &s)
{
    dbuf_store_live(st, s);
    st.underruns = s.underruns; st.shrinks = s.shrinks; st.shrunk = s.shrunk; st.dropped = s.dropped; st.puts = s.puts; st.gets = s.gets;
}
// the six counters in the state's order: counter j of the scalars, and all of them back to 0 (k_dbuf keeps lane j's running counter j)
constexpr uint32_t kDbufCounters = 6;
constexpr uint32_t dbuf_counter(const DbufSc &s, uint32_t j)
{
    return j == 0 ? s.underruns : j == 1 ? s.shrinks : j == 2 ? s.shrunk : j == 3 ? s.dropped : j == 4 ? s.puts : j == 5 ? s.gets : 0u;
}
constexpr void dbuf_counters_clear(DbufSc &s) { s.underruns = 0; s.shrinks = 0; s.shrunk = 0; s.dropped = 0; s.puts = 0; s.gets = 0; }

// ---- update(op): the burst level, learnt per direction switch
constexpr void dbuf_update(DbufSc &s, uint32_t op, uint32_t n, uint32_t M)
{
    if (s.last_op == op) { s.level = s.level + 1u < 65535u ? s.level + 1u : 65535u; return; }
    if (s.last_op != 0) { s.max_level = s.max_level > s.level ? s.max_level : s.level; s.since += s.level; }
    s.last_op = op;
    s.level = 1;
    if (s.since >= (uint32_t)IGDSP_DBUF_RECALC) {
        const uint32_t want = (s.max_level + 1u) * n;
        s.eff = (3u * s.eff + (want < M ? want : M)) >> 2;
        s.max_level = 0;
        s.since = 0;
    }
}

// ---- PUT in three steps: begin (does this PUT shrink?), the shrink's samples (the caller's), end (drop; returns k: x goes to y[k .. k + n))
constexpr bool dbuf_put_begin(DbufSc &s, uint32_t n, uint32_t M)
{
    dbuf_update(s, IGDSP_DBUF_PUT, n, M);
    s.puts += 1u;
    return (s.len > n + s.eff || s.len + n > M) && s.len >= kDbufWin;
}
// the shrink: b[i] from the window z (z[k] = y[len - WIN + k]) replaces y[len - 2 p + i], i < p; then dbuf_shrunk
constexpr int32_t dbuf_blend(int32_t z_old, int32_t z_new, uint32_t i, uint32_t p)      // z_old = z[WIN - 2 p + i], z_new = z[WIN - p + i]
{
    const int32_t w = pitch_w(i, p);
    return pitch_q15(z_old * (32768 - w) + z_new * w);
}
constexpr void dbuf_shrunk(DbufSc &s, uint32_t p) { s.len -= p; s.shrinks += 1u; s.shrunk += p; }
constexpr uint32_t dbuf_put_end(DbufSc &s, uint32_t n, uint32_t M)
{
    if (s.len + n > M) {
        const uint32_t d = s.len + n - M;
        s.head = (s.head + d) % kDbufCap;
        s.len -= d;
        s.dropped += d;
    }
    const uint32_t k = s.len;
    s.len += n;
    return k;
}

// ---- GET in two steps: begin (true: the row is y[0 .. n) of the scalars as they are now; false: an underrun, a row of zeros), end
constexpr bool dbuf_get_begin(DbufSc &s, uint32_t n, uint32_t M)
{
    dbuf_update(s, IGDSP_DBUF_GET, n, M);
    s.gets += 1u;
    return s.len >= n;
}
constexpr uint32_t dbuf_get_end(DbufSc &s, uint32_t n, bool played)                      // the step's flag
{
    const uint32_t take = played ? n : s.len;
    s.head = (s.head + take) % kDbufCap;
    s.len -= take;
    if (!played) s.underruns += 1u;
    return played ? IGDSP_JB_PLAYED : IGDSP_JB_LOST;
}

// ---- one step of one channel on the host: the state's ring holds the samples (igdsp_dbuf_step; the route driver)
inline uint32_t dbuf_step_run(igdsp_dbuf_state &st, uint32_t op, const int16_t *in, uint32_t n, uint32_t M, int16_t *out)
{
    DbufSc s = dbuf_load(st, M);
    uint32_t flag = IGDSP_JB_IDLE;
    if (op & IGDSP_DBUF_PUT) {
        if (dbuf_put_begin(s, n, M)) {
            int16_t z[IGDSP_DBUF_WIN];
            for (uint32_t k = 0; k < kDbufWin; ++k) z[k] = st.ring[dbuf_pos(s, s.len - kDbufWin + k)];
            const uint32_t p = pitch_search(z);
            for (uint32_t i = 0; i < p; ++i)
                st.ring[dbuf_pos(s, s.len - 2u * p + i)] = (int16_t)dbuf_blend(z[kDbufWin - 2u * p + i], z[kDbufWin - p + i], i, p);
            dbuf_shrunk(s, p);
        }
        const uint32_t k = dbuf_put_end(s, n, M);
        for (uint32_t i = 0; i < n; ++i) st.ring[dbuf_pos(s, k + i)] = in[i];
    }
    if (op & IGDSP_DBUF_GET) {
        const bool played = dbuf_get_begin(s, n, M);
        for (uint32_t i = 0; i < n; ++i) out[i] = played ? st.ring[dbuf_pos(s, i)] : (int16_t)0;
        flag = dbuf_get_end(s, n, played);
    }
    dbuf_store(st, s);
    return flag;
}

}  // namespace igdsp
