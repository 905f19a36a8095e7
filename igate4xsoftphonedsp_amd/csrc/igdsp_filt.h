// igdsp_filt.h — the filter's rule (include/igdsp.h, "Filter"; independent restatement: tests/filt_model.py) in plain C++17, so that
// the host entry igdsp_filt_frame and the kernel k_filt run the same code: how a plan and a state are read and written, which sections
// run, one sample through one section.  What the two sides do differently is only who walks: the host runs one channel's frame in a
// loop, the kernel gives a lane a channel.  Every step is an exact integer operation and ">>" on a signed value an arithmetic shift on
// both sides.  Nothing here indexes an array by a run-time value: the loops over the sections have constant bounds and unroll, so
// coefficients and histories stay registers in the kernel.  Also here, host only: the designs (RBJ cookbook sections in double,
// rounded to Q13) and the presets.
// The rule is the library's own, UNVERIFIED against any other filter implementation.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "igdsp.h"

#if defined(__HIPCC__)
#define IGDSP_FILT_HD __host__ __device__ inline __attribute__((always_inline))   // (no HIP header need come first)
#define IGDSP_FILT_UNROLL _Pragma("unroll")
#else
#define IGDSP_FILT_HD inline
#define IGDSP_FILT_UNROLL
#endif

namespace igdsp {

static_assert(sizeof(igdsp_filt_section) == 10 && sizeof(igdsp_filt_plan) == 48 && sizeof(igdsp_filt_hist) == 10 && sizeof(igdsp_filt_state) == 48 &&
              sizeof(igdsp_filt_rec) == 16, "capi.FILT_PLAN, FILT_STATE, FILT_REC");
static_assert(offsetof(igdsp_filt_plan, s) == 8 && offsetof(igdsp_filt_state, s) == 4 && offsetof(igdsp_filt_state, flags) == 44 &&
              offsetof(igdsp_filt_rec, flags) == 8 && alignof(igdsp_filt_plan) == 4,
              "a plan and a state go as 12 dwords, their sections from half-word 4 and 2, the record as one 16-byte store");

constexpr uint32_t kFiltMaxSections = IGDSP_FILT_MAX_SECTIONS, kFiltPlanWords = 12, kFiltStateWords = 12;
constexpr int32_t kFiltUnity = IGDSP_FILT_UNITY, kFiltEMask = 8191, kFiltShift = 13;
constexpr int64_t kFiltSumMax = 65535, kFiltStateMax = 32768;
// a valid section's accumulator and every partial sum of it fit int32: each term is a coefficient times a state of magnitude <= 32768,
// the magnitudes of the coefficients sum to <= 65535, and e <= 8191 joins once.  Both factors of a product fit 24 bits (v_mad_i32_i24:
// -a1 may be +32768)
static_assert(kFiltSumMax * kFiltStateMax + kFiltEMask == 2147459071ll && kFiltSumMax * kFiltStateMax + kFiltEMask < (1ll << 31) &&
              kFiltStateMax < (1 << 23) && kFiltEMask == (1 << kFiltShift) - 1 && kFiltUnity == (1 << kFiltShift), "the widths");
// the identity section on any int16 input and any e as read: y = (8192 v + e) >> 13 = v, e stays
static_assert(((8192 * -32768 + 8191) >> 13) == -32768 && ((8192 * 32767 + 8191) >> 13) == 32767 && ((8192 * -32768 + 8191) & 8191) == 8191,
              "the identity returns its input");

constexpr bool filt_n_ok(uint32_t n) { return n >= 8u && n <= IGDSP_MAX_PAYLOAD && (n & 7u) == 0u; }
constexpr uint32_t filt_ctl(uint32_t v) { return v <= 2u ? v : (uint32_t)IGDSP_FILT_RUN; }

// one section as it runs: -a1 and -a2 (<= 32768 in magnitude), the history
struct FiltSec {
    int32_t b0, b1, b2, na1, na2, x1, x2, y1, y2, e;
};

// a * b + c for factors that fit 24 bits and a sum that fits 32 (the static_assert above).  On the device the instruction is named:
// left to itself the compiler folds a chain of these into the quarter-rate 64-bit mad
IGDSP_FILT_HD int32_t filt_mad24(int32_t a, int32_t b, int32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int32_t r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
#else
    return a * b + c;
#endif
}
IGDSP_FILT_HD int32_t filt_abs(int32_t v) { return v < 0 ? -v : v; }
// half-word h of a run of dwords, sign-extended; h is a constant wherever this is called
template <uint32_t N>
IGDSP_FILT_HD int32_t filt_half(const uint32_t (&w)[N], uint32_t h) { return (int32_t)(int16_t)(w[h >> 1] >> (16u * (h & 1u))); }
template <uint32_t N>
IGDSP_FILT_HD void filt_set_half(uint32_t (&w)[N], uint32_t h, uint32_t v)
{
    w[h >> 1] = (h & 1u) ? ((w[h >> 1] & 0xFFFFu) | (v << 16)) : ((w[h >> 1] & 0xFFFF0000u) | (v & 0xFFFFu));
}

// min(n_sections, 4) of a plan's first dword
IGDSP_FILT_HD uint32_t filt_plan_sections(uint32_t w0) { return (w0 & 0xFFFFu) < kFiltMaxSections ? (w0 & 0xFFFFu) : kFiltMaxSections; }
IGDSP_FILT_HD bool filt_valid(int32_t b0, int32_t b1, int32_t b2, int32_t a1, int32_t a2)
{
    return filt_abs(b0) + filt_abs(b1) + filt_abs(b2) + filt_abs(a1) + filt_abs(a2) <= (int32_t)kFiltSumMax;
}
// section s of a plan's 12 dwords into q's coefficients; want = s < the plan's section count.  Returns whether the section RUNS
// (wanted and valid); one that does not gets the identity's coefficients, so no product of an invalid section is ever executed
IGDSP_FILT_HD bool filt_load_section(const uint32_t (&pw)[kFiltPlanWords], uint32_t s, bool want, FiltSec &q)
{
    const int32_t b0 = filt_half(pw, 4u + 5u * s), b1 = filt_half(pw, 5u + 5u * s), b2 = filt_half(pw, 6u + 5u * s);
    const int32_t a1 = filt_half(pw, 7u + 5u * s), a2 = filt_half(pw, 8u + 5u * s);
    const bool run = want && filt_valid(b0, b1, b2, a1, a2);
    q.b0 = run ? b0 : kFiltUnity; q.b1 = run ? b1 : 0; q.b2 = run ? b2 : 0; q.na1 = run ? -a1 : 0; q.na2 = run ? -a2 : 0;
    return run;
}
// a state as it is READ, from its 12 dwords: another tag (or RESET) is all-zero histories, under the tag e is masked and every other
// value stands.  sw itself is brought to what was read, so that a section that does not run is written back from it
IGDSP_FILT_HD bool filt_zeroed(uint32_t tag, bool reset) { return reset || tag != (uint32_t)IGDSP_FILT_TAG; }
IGDSP_FILT_HD void filt_read_state(uint32_t (&sw)[kFiltStateWords], bool zero)
{
    IGDSP_FILT_UNROLL
    for (uint32_t i = 1; i < 11u; ++i) sw[i] = zero ? 0u : sw[i];
    IGDSP_FILT_UNROLL
    for (uint32_t s = 0; s < kFiltMaxSections; ++s) filt_set_half(sw, 6u + 5u * s, (uint32_t)filt_half(sw, 6u + 5u * s) & (uint32_t)kFiltEMask);
}
IGDSP_FILT_HD void filt_read_section(const uint32_t (&sw)[kFiltStateWords], uint32_t s, FiltSec &q)
{
    q.x1 = filt_half(sw, 2u + 5u * s); q.x2 = filt_half(sw, 3u + 5u * s); q.y1 = filt_half(sw, 4u + 5u * s); q.y2 = filt_half(sw, 5u + 5u * s);
    q.e = filt_half(sw, 6u + 5u * s);                                      // masked by filt_read_state: 0..8191
}
// and as it is WRITTEN: a section that ran puts its history back, one that did not stays as read
IGDSP_FILT_HD void filt_write_section(uint32_t (&sw)[kFiltStateWords], uint32_t s, bool ran, const FiltSec &q)
{
    if (ran) {
        filt_set_half(sw, 2u + 5u * s, (uint32_t)q.x1); filt_set_half(sw, 3u + 5u * s, (uint32_t)q.x2); filt_set_half(sw, 4u + 5u * s, (uint32_t)q.y1);
        filt_set_half(sw, 5u + 5u * s, (uint32_t)q.y2); filt_set_half(sw, 6u + 5u * s, (uint32_t)q.e);
    }
}
IGDSP_FILT_HD void filt_close_state(uint32_t (&sw)[kFiltStateWords], uint32_t flags) { sw[0] = (uint32_t)IGDSP_FILT_TAG; sw[11] = flags & 0xFFFFu; }

// one sample through one section; returns y and counts a clip
IGDSP_FILT_HD int32_t filt_step(FiltSec &q, int32_t v, uint32_t &clipped)
{
    int32_t acc = filt_mad24(q.b0, v, q.e);
    acc = filt_mad24(q.b1, q.x1, acc);
    acc = filt_mad24(q.b2, q.x2, acc);
    acc = filt_mad24(q.na1, q.y1, acc);
    acc = filt_mad24(q.na2, q.y2, acc);
    const int32_t y = acc >> kFiltShift;
    const int32_t yc = y < -32768 ? -32768 : (y > 32767 ? 32767 : y);     // one v_med3_i32
    const bool clip = yc != y;
    clipped += clip ? 1u : 0u;
    q.e = clip ? 0 : (acc & kFiltEMask);
    q.x2 = q.x1; q.x1 = v; q.y2 = q.y1; q.y1 = yc;
    return yc;
}
// what a frame's record carries of the plan: flags NO_PLAN / BAD_PLAN and the section count.  w0 = the plan's first dword, have =
// the channel's index is below n_plans, max_s = the launch's max_sections, 1..4 (filt_route)
IGDSP_FILT_HD uint32_t filt_plan_flags(uint32_t w0, bool have, uint32_t max_s, uint32_t &ns)
{
    ns = have ? filt_plan_sections(w0) : 0u;
    if (ns == 0u) return (uint32_t)IGDSP_FILT_NO_PLAN;
    if (ns > max_s) return (uint32_t)IGDSP_FILT_NO_PLAN | (uint32_t)IGDSP_FILT_BAD_PLAN;
    return 0u;
}
IGDSP_FILT_HD uint32_t filt_sat16(uint32_t v) { return v < 65535u ? v : 65535u; }
IGDSP_FILT_HD void filt_pack_rec(uint32_t in_peak, uint32_t out_peak, uint32_t n_clipped, uint32_t plan, uint32_t flags, uint32_t ns, uint32_t (&w)[4])
{
    w[0] = in_peak | out_peak << 16; w[1] = filt_sat16(n_clipped) | (plan & 0xFFFFu) << 16; w[2] = (flags & 0xFFu) | ns << 8; w[3] = 0u;
}

// ---- the host: one frame of one channel with all four sections in play (max_sections 4).  n checked by the caller; plan may be
// nullptr (a channel without a plan), out and rec may be nullptr
inline void filt_frame_run(const igdsp_filt_plan *plan, igdsp_filt_state &st, const int16_t *pcm, uint32_t n, uint32_t ctl_in, int16_t *out,
                           igdsp_filt_rec *rec)
{
    const uint32_t ctl = filt_ctl(ctl_in);
    uint32_t pw[kFiltPlanWords] = {0}, sw[kFiltStateWords], ns = 0u, w[4];
    if (plan) std::memcpy(pw, plan, sizeof *plan);
    std::memcpy(sw, &st, sizeof st);
    const uint32_t pflags = filt_plan_flags(pw[0], plan != nullptr, kFiltMaxSections, ns);
    const bool pass = ctl == IGDSP_FILT_BYPASS || (pflags & IGDSP_FILT_NO_PLAN) != 0u;
    const bool zero = filt_zeroed(sw[0], ctl == IGDSP_FILT_RESET);
    FiltSec q[kFiltMaxSections];
    bool ran[kFiltMaxSections];
    uint32_t flags = ctl == IGDSP_FILT_BYPASS ? (uint32_t)IGDSP_FILT_BYPASSED : pflags;
    if (!pass) {
        filt_read_state(sw, zero);
        if (zero) flags |= (uint32_t)IGDSP_FILT_WAS_RESET;
    }
    for (uint32_t s = 0; s < kFiltMaxSections; ++s) {
        ran[s] = filt_load_section(pw, s, !pass && s < ns, q[s]);
        if (!pass && s < ns && !ran[s]) flags |= (uint32_t)IGDSP_FILT_BAD_PLAN;
        filt_read_section(sw, s, q[s]);
    }
    uint32_t in_peak = 0u, out_peak = 0u, clipped = 0u;
    for (uint32_t j = 0; j < n; ++j) {
        int32_t v = pcm[j];
        in_peak = (uint32_t)filt_abs(v) > in_peak ? (uint32_t)filt_abs(v) : in_peak;
        for (uint32_t s = 0; s < kFiltMaxSections; ++s)
            if (ran[s]) v = filt_step(q[s], v, clipped);
        out_peak = (uint32_t)filt_abs(v) > out_peak ? (uint32_t)filt_abs(v) : out_peak;
        if (out) out[j] = (int16_t)v;
    }
    if (clipped) flags |= (uint32_t)IGDSP_FILT_CLIPPED;
    if (!pass) {
        for (uint32_t s = 0; s < kFiltMaxSections; ++s) filt_write_section(sw, s, ran[s], q[s]);
        filt_close_state(sw, flags);
        std::memcpy(&st, sw, sizeof st);
    }
    filt_pack_rec(in_peak, out_peak, clipped, 0u, flags, ns, w);
    if (rec) std::memcpy(rec, w, 16);
}
inline bool filt_plan_ok(const igdsp_filt_plan &plan)
{
    if (plan.n_sections == 0u || plan.n_sections > kFiltMaxSections) return false;
    for (uint32_t s = 0; s < plan.n_sections; ++s)
        if (!filt_valid(plan.s[s].b0, plan.s[s].b1, plan.s[s].b2, plan.s[s].a1, plan.s[s].a2)) return false;
    return true;
}

// ---- the designs (host only, double).  c = {b0, b1, b2, a1, a2} over a0 = 1, scaled by g; quantised to the nearest Q13 and checked
inline bool filt_quantise(const double (&c)[5], int16_t (&out)[5])
{
    int32_t r[5];
    for (int i = 0; i < 5; ++i) {
        if (!std::isfinite(c[i])) return false;
        const double v = std::nearbyint(c[i] * (double)kFiltUnity);        // the default rounding mode: to nearest, ties to even
        if (v < -32768.0 || v > 32767.0) return false;
        r[i] = (int32_t)v;
    }
    if (!filt_valid(r[0], r[1], r[2], r[3], r[4])) return false;
    if (!(filt_abs(r[4]) < kFiltUnity && filt_abs(r[3]) < kFiltUnity + r[4])) return false;      // the quantised poles, strictly inside
    for (int i = 0; i < 5; ++i) out[i] = (int16_t)r[i];
    return true;
}
constexpr double kFiltPi = 3.14159265358979323846;
// |H| of the section c at f Hz
inline double filt_gain_at(const double (&c)[5], double f, double rate)
{
    const double w = 2.0 * kFiltPi * f / rate, c1 = std::cos(w), s1 = std::sin(w), c2 = std::cos(2.0 * w), s2 = std::sin(2.0 * w);
    const double nr = c[0] + c[1] * c1 + c[2] * c2, ni = -(c[1] * s1 + c[2] * s2), dr = 1.0 + c[3] * c1 + c[4] * c2, di = -(c[3] * s1 + c[4] * s2);
    return std::sqrt((nr * nr + ni * ni) / (dr * dr + di * di));
}
inline bool filt_design_real(uint32_t kind, double rate, double f0, double q, double gain_db, double (&c)[5])
{
    if (!(rate > 0.0) || !(f0 > 0.0) || !(f0 < rate / 2.0) || !std::isfinite(rate) || !std::isfinite(gain_db)) return false;
    if (kind == IGDSP_FILT_LP1 || kind == IGDSP_FILT_HP1) {
        const double K = std::tan(kFiltPi * f0 / rate);
        c[3] = (K - 1.0) / (K + 1.0); c[2] = 0.0; c[4] = 0.0;
        if (kind == IGDSP_FILT_LP1) { c[0] = K / (1.0 + K); c[1] = c[0]; }
        else { c[0] = 1.0 / (1.0 + K); c[1] = -c[0]; }
        return true;
    }
    if (!(q > 0.0) || !std::isfinite(q)) return false;
    const double w0 = 2.0 * kFiltPi * f0 / rate, cs = std::cos(w0), sn = std::sin(w0), al = sn / (2.0 * q), A = std::pow(10.0, gain_db / 40.0);
    double b0, b1, b2, a0, a1, a2;
    switch (kind) {
    case IGDSP_FILT_LOWPASS:  b0 = (1.0 - cs) / 2.0; b1 = 1.0 - cs; b2 = b0; a0 = 1.0 + al; a1 = -2.0 * cs; a2 = 1.0 - al; break;
    case IGDSP_FILT_HIGHPASS: b0 = (1.0 + cs) / 2.0; b1 = -(1.0 + cs); b2 = b0; a0 = 1.0 + al; a1 = -2.0 * cs; a2 = 1.0 - al; break;
    case IGDSP_FILT_BANDPASS: b0 = al; b1 = 0.0; b2 = -al; a0 = 1.0 + al; a1 = -2.0 * cs; a2 = 1.0 - al; break;
    case IGDSP_FILT_NOTCH:    b0 = 1.0; b1 = -2.0 * cs; b2 = 1.0; a0 = 1.0 + al; a1 = -2.0 * cs; a2 = 1.0 - al; break;
    case IGDSP_FILT_PEAK:     b0 = 1.0 + al * A; b1 = -2.0 * cs; b2 = 1.0 - al * A; a0 = 1.0 + al / A; a1 = -2.0 * cs; a2 = 1.0 - al / A; break;
    case IGDSP_FILT_LOWSHELF: {
        const double r = 2.0 * std::sqrt(A) * al;
        b0 = A * ((A + 1.0) - (A - 1.0) * cs + r); b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cs); b2 = A * ((A + 1.0) - (A - 1.0) * cs - r);
        a0 = (A + 1.0) + (A - 1.0) * cs + r; a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cs); a2 = (A + 1.0) + (A - 1.0) * cs - r;
        break;
    }
    case IGDSP_FILT_HIGHSHELF: {
        const double r = 2.0 * std::sqrt(A) * al;
        b0 = A * ((A + 1.0) + (A - 1.0) * cs + r); b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cs); b2 = A * ((A + 1.0) + (A - 1.0) * cs - r);
        a0 = (A + 1.0) - (A - 1.0) * cs + r; a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cs); a2 = (A + 1.0) - (A - 1.0) * cs - r;
        break;
    }
    default: return false;
    }
    c[0] = b0 / a0; c[1] = b1 / a0; c[2] = b2 / a0; c[3] = a1 / a0; c[4] = a2 / a0;
    return true;
}
inline bool filt_design(uint32_t kind, uint32_t rate, double f0, double q, double gain_db, int16_t (&out)[5])
{
    double c[5];
    return filt_design_real(kind, (double)rate, f0, q, gain_db, c) && filt_quantise(c, out);
}
inline bool filt_preset(uint32_t preset, uint32_t rate, igdsp_filt_plan &plan)
{
    if (rate < 8000u || rate > 48000u) return false;
    int16_t s[2][5] = {{0}};
    uint32_t ns = 1u;
    double c[5];
    switch (preset) {
    case IGDSP_FILT_VOICE_BAND:
        ns = 2u;
        if (!filt_design(IGDSP_FILT_HIGHPASS, rate, 300.0, std::sqrt(0.5), 0.0, s[0]) || !filt_design(IGDSP_FILT_LOWPASS, rate, 3400.0, std::sqrt(0.5), 0.0, s[1]))
            return false;
        break;
    case IGDSP_FILT_CTCSS_HP:
        ns = 2u;
        if (!filt_design(IGDSP_FILT_HIGHPASS, rate, 300.0, 1.0 / (2.0 * std::cos(kFiltPi / 8.0)), 0.0, s[0]) ||
            !filt_design(IGDSP_FILT_HIGHPASS, rate, 300.0, 1.0 / (2.0 * std::cos(3.0 * kFiltPi / 8.0)), 0.0, s[1]))
            return false;
        break;
    case IGDSP_FILT_DEEMPH:
    case IGDSP_FILT_PREEMPH: {
        // the corners matched in z, not warped: a bilinear corner at 3400 Hz of an 8 kHz clock lifts the band's top by 9 dB more
        if (!(3400.0 < (double)rate / 2.0)) return false;
        const double za = std::exp(-2.0 * kFiltPi * 300.0 / (double)rate), zp = std::exp(-2.0 * kFiltPi * 3400.0 / (double)rate);
        const bool pre = preset == IGDSP_FILT_PREEMPH;
        c[0] = 1.0; c[1] = pre ? -za : -zp; c[2] = 0.0; c[3] = pre ? -zp : -za; c[4] = 0.0;
        const double g = 1.0 / filt_gain_at(c, 1000.0, (double)rate);
        c[0] *= g; c[1] *= g;
        if (!filt_quantise(c, s[0])) return false;
        break;
    }
    case IGDSP_FILT_DC_BLOCK:
        if (!filt_design(IGDSP_FILT_HP1, rate, 20.0, 1.0, 0.0, s[0])) return false;
        break;
    default: return false;
    }
    std::memset(&plan, 0, sizeof plan);
    plan.n_sections = (uint16_t)ns;
    plan.clock_rate = rate;
    for (uint32_t i = 0; i < kFiltMaxSections; ++i) {
        const int16_t ident[5] = {(int16_t)kFiltUnity, 0, 0, 0, 0}, *src = i < ns ? s[i] : ident;
        plan.s[i].b0 = src[0]; plan.s[i].b1 = src[1]; plan.s[i].b2 = src[2]; plan.s[i].a1 = src[3]; plan.s[i].a2 = src[4];
    }
    return true;
}

}  // namespace igdsp
