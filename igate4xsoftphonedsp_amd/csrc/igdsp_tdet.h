// igdsp_tdet.h — the tone detector's rule (include/igdsp.h, "Tone detector"; independent restatement: tests/tdet_model.py) in plain
// C++17, so that the host entries (igdsp_tdet_plan_build, igdsp_tdet_table, igdsp_tdet_frame) and the kernel k_tdet run the same code:
// the reference table's values, the thresholds of a hit, the final decision from the two groups' chosen bins, and the debounce.
// What the two sides do differently is only how they find a group's strongest bin: the host walks the bins, the kernel takes maxima
// over the eight lanes of a group (igdsp_k_tdet.hip); both then call tdet_decide.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "igdsp.h"
#include "igdsp_route.h"

#if defined(__HIPCC__)
#define IGDSP_TDET_HD __host__ __device__ __forceinline__
#else
#define IGDSP_TDET_HD inline
#endif

namespace igdsp {

static_assert(sizeof(igdsp_tdet_thr) == 12 && sizeof(igdsp_tdet_plan) == 84 && offsetof(igdsp_tdet_plan, step) == 20, "capi.TDET_PLAN mirrors it");
static_assert(sizeof(igdsp_tdet_state) == 264 && offsetof(igdsp_tdet_state, cur) == 256 && alignof(igdsp_tdet_state) == 2, "capi.TDET_STATE");
static_assert(sizeof(igdsp_tdet_rec) == 8 && sizeof(igdsp_tdet_event) == 16, "capi.TDET_REC, capi.TDET_EVENT");
static_assert(IGDSP_TDET_HIST == 128 && IGDSP_MAX_PAYLOAD == 256 && IGDSP_TDET_MAX_FREQ == 16, "half a window of 256 is the history; 8 + 8 bins");
// the bound of I and Q: |v| <= 4096, |w| <= 2047, n <= 256
static_assert(4096ll * 2047ll * 256ll < (1ll << 31), "I_k and Q_k fit int32");

constexpr igdsp_tdet_thr kTdetThr{400, 1024, 673, 1615, 150, 3, 2};
constexpr bool tdet_n_ok(uint32_t n) { return n >= 2u && n <= IGDSP_MAX_PAYLOAD && (n & 1u) == 0u; }
// a plan as it is READ: group sizes above 8 count as 8 (a plan the builder did not make stays in bounds)
constexpr uint32_t tdet_nlo(const igdsp_tdet_plan &p) { return p.n_lo < 8u ? p.n_lo : 8u; }
constexpr uint32_t tdet_nhi(const igdsp_tdet_plan &p) { return p.n_hi < 8u ? p.n_hi : 8u; }

// ---- the table: T is the generator's sine list (1 024 values)
IGDSP_TDET_HD int32_t tdet_osc(const int16_t *T, uint32_t ph)
{
    const uint32_t i = ph >> 22;
    const int32_t v = T[i], d = T[(i + 1u) & 1023u] - v;
    return v + ((d * (int32_t)((ph >> 6) & 0xFFFFu)) >> 16);
}
IGDSP_TDET_HD int32_t tdet_ws(const int16_t *T, uint32_t step, uint32_t i) { return tdet_osc(T, i * step) / 16; }
IGDSP_TDET_HD int32_t tdet_wc(const int16_t *T, uint32_t step, uint32_t i) { return tdet_osc(T, i * step + 0x40000000u) / 16; }

// ---- the thresholds
IGDSP_TDET_HD uint64_t tdet_floor(uint32_t min_amp, uint32_t n)
{
    const uint64_t a = (uint64_t)(min_amp >> 3) * 2047u * (n / 2u);        // < 2^32
    return a * a;
}
IGDSP_TDET_HD uint64_t tdet_eref(uint64_t E, uint32_t n) { return (E * (n / 2u) * (2047ull * 2047ull)) >> 16; }   // E <= 2^32: below 2^61 before the shift
// a bin k of a group against the group's chosen power: true = the chosen bin does not stand out enough
IGDSP_TDET_HD bool tdet_rel_fails(uint64_t p_chosen, uint64_t p_other, uint32_t rel_q8) { return (p_chosen >> 16) * 256u < (uint64_t)rel_q8 * (p_other >> 16); }

// the groups' chosen bins -> the hit code.  ok_lo / ok_hi: the group has a bin, it reaches the floor and no other bin fails tdet_rel_fails
IGDSP_TDET_HD uint32_t tdet_decide(const igdsp_tdet_thr &t, uint32_t nhi, bool ok_lo, uint32_t i_lo, uint64_t p_lo, bool ok_hi, uint32_t i_hi,
                                   uint64_t p_hi, uint64_t eref)
{
    const bool two = nhi != 0u;
    const uint64_t s_lo = p_lo >> 16, s_hi = two ? p_hi >> 16 : 0u;
    bool hit = ok_lo;
    if (two) hit = hit && ok_hi && s_hi * 256u <= (uint64_t)t.fwd_q8 * s_lo && s_lo * 256u <= (uint64_t)t.rev_q8 * s_hi;
    hit = hit && (s_lo + s_hi) * 256u >= (uint64_t)t.frac_q8 * eref;
    if (!hit) return 0u;
    return two ? 1u + i_lo * nhi + i_hi : i_lo + 1u;
}

// ---- the debounce: one evaluation with hit code h; returns IGDSP_TDET_ON0 / _OFF0 bits (the caller shifts evaluation 1's)
struct TdetDeb { uint32_t cur, cand, run, off, len; };
IGDSP_TDET_HD uint32_t tdet_debounce(TdetDeb &d, uint32_t h, uint32_t min_on, uint32_t min_off, uint32_t &code)
{
    uint32_t fl = 0u;
    if (d.cur != 0u) {
        d.len = d.len < 65535u ? d.len + 1u : 65535u;
        d.off = h == d.cur ? 0u : (d.off < 255u ? d.off + 1u : 255u);
    }
    if (d.cur != 0u && h == d.cur) { d.cand = 0u; d.run = 0u; }
    else if (h != 0u && h == d.cand) d.run = d.run < 255u ? d.run + 1u : 255u;
    else { d.cand = h; d.run = h != 0u ? 1u : 0u; }
    if (d.cur != 0u && d.off >= min_off) {
        fl |= IGDSP_TDET_OFF0;
        code = d.cur;
        d.len = d.len > d.off ? d.len - d.off : 0u;
        d.cur = 0u; d.off = 0u;
    }
    if (d.cur == 0u && d.cand != 0u && d.run >= min_on) {
        fl |= IGDSP_TDET_ON0;
        d.cur = d.cand; code = d.cur;
        d.len = d.run;
        d.off = 0u; d.cand = 0u; d.run = 0u;
    }
    return fl;
}

// a record's two words: {hit0 | hit1 << 8 | cur << 16 | flags << 24, len | code << 16}
IGDSP_TDET_HD uint32_t tdet_rec_w0(uint32_t h0, uint32_t h1, uint32_t cur, uint32_t flags) { return h0 | h1 << 8 | cur << 16 | flags << 24; }
IGDSP_TDET_HD uint32_t tdet_rec_w1(uint32_t len, uint32_t code) { return len | code << 16; }

// ---- the host: plan, table, one frame of one channel
inline bool tdet_plan_make(uint32_t clock_rate, const uint16_t *freq, uint32_t n_lo, uint32_t n_hi, const igdsp_tdet_thr *thr, igdsp_tdet_plan &out)
{
    if (!freq || clock_rate < 8000u || clock_rate > 48000u || clock_rate % 1000u != 0u || n_lo < 1u || n_lo > 8u || n_hi > 8u) return false;
    const igdsp_tdet_thr t = thr ? *thr : kTdetThr;
    if (t.min_amp < 8u || t.min_amp > 32767u || !t.rel_q8 || !t.fwd_q8 || !t.rev_q8 || !t.frac_q8 || !t.min_on || !t.min_off) return false;
    igdsp_tdet_plan p{};
    p.clock_rate = clock_rate;
    p.n_lo = (uint8_t)n_lo; p.n_hi = (uint8_t)n_hi;
    p.thr = t;
    for (uint32_t k = 0; k < n_lo + n_hi; ++k) {
        if (freq[k] < 1u || freq[k] > clock_rate / 2u - 1u) return false;
        p.step[k] = (uint32_t)((((uint64_t)freq[k] << 32) + clock_rate / 2u) / clock_rate);
    }
    out = p;
    return true;
}

inline void tdet_eval(const igdsp_tdet_plan &p, const int16_t *v, uint32_t n, uint32_t &hit)
{
    const uint32_t nlo = tdet_nlo(p), nhi = tdet_nhi(p);
    uint64_t P[IGDSP_TDET_MAX_FREQ] = {}, E = 0;
    for (uint32_t i = 0; i < n; ++i) E += (uint64_t)((int32_t)v[i] * v[i]);
    for (uint32_t k = 0; k < nlo + nhi; ++k) {
        int32_t I = 0, Q = 0;                                              // wraps like the kernel's if a garbage history exceeds |v| <= 4096
        for (uint32_t i = 0; i < n; ++i) {
            I = (int32_t)((uint32_t)I + (uint32_t)(v[i] * tdet_wc(kToneSin, p.step[k], i)));
            Q = (int32_t)((uint32_t)Q + (uint32_t)(v[i] * tdet_ws(kToneSin, p.step[k], i)));
        }
        P[k] = (uint64_t)((int64_t)I * I) + (uint64_t)((int64_t)Q * Q);
    }
    const uint64_t floor = tdet_floor(p.thr.min_amp, n);
    auto group = [&](uint32_t first, uint32_t count, uint32_t &idx, uint64_t &pw) {
        if (count == 0u) { idx = 0u; pw = 0u; return false; }
        idx = 0u;
        for (uint32_t j = 1; j < count; ++j) if (P[first + j] > P[first + idx]) idx = j;
        pw = P[first + idx];
        bool ok = pw >= floor;
        for (uint32_t j = 0; j < count; ++j) if (j != idx && tdet_rel_fails(pw, P[first + j], p.thr.rel_q8)) ok = false;
        return ok;
    };
    uint32_t i_lo, i_hi;
    uint64_t p_lo, p_hi;
    const bool ok_lo = group(0u, nlo, i_lo, p_lo), ok_hi = group(nlo, nhi, i_hi, p_hi);
    hit = tdet_decide(p.thr, nhi, ok_lo, i_lo, p_lo, ok_hi, i_hi, p_hi, tdet_eref(E, n));
}

// one frame of one channel; n checked by the caller, rec may be nullptr
inline void tdet_frame_run(const igdsp_tdet_plan &p, igdsp_tdet_state &st, const int16_t *row, uint32_t n, igdsp_tdet_rec *rec)
{
    const uint32_t h = n / 2u;
    int16_t buf[IGDSP_TDET_HIST + IGDSP_MAX_PAYLOAD];
    std::memcpy(buf, st.hist, sizeof(st.hist));
    for (uint32_t i = 0; i < n; ++i) buf[IGDSP_TDET_HIST + i] = (int16_t)(row[i] >> 3);
    TdetDeb d{st.cur, st.cand, st.run, st.off, st.len};
    uint32_t hit[2], flags = 0, code = 0;
    for (uint32_t e = 0; e < 2u; ++e) {
        tdet_eval(p, buf + IGDSP_TDET_HIST - (e ? 0u : h), n, hit[e]);
        flags |= tdet_debounce(d, hit[e], p.thr.min_on, p.thr.min_off, code) << (2u * e);
    }
    std::memcpy(st.hist, buf + n, sizeof(st.hist));
    st.cur = (uint8_t)d.cur; st.cand = (uint8_t)d.cand; st.run = (uint8_t)d.run; st.off = (uint8_t)d.off;
    st.len = (uint16_t)d.len; st.reserved = 0;
    if (rec) *rec = igdsp_tdet_rec{{(uint8_t)hit[0], (uint8_t)hit[1]}, (uint8_t)d.cur, (uint8_t)flags, (uint16_t)d.len, (uint8_t)code, 0};
}

}  // namespace igdsp
