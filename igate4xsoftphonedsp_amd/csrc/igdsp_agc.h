// igdsp_agc.h — the level control's rule (include/igdsp.h, "Level control"; independent restatement: tests/agc_model.py) in plain
// C++17, so that the host entry igdsp_agc_frame and the kernel k_agc run the same code: how a state is read, the envelope and the slow
// gain of a frame, the limiter's ratio of a block and its release step, a knot's slow gain, a sample's gain and output.  What the two
// sides do differently is only who walks: the host walks blocks and knots in loops, the kernel gives a lane a block and its right knot
// (igdsp_k_agc.hip).  Every step is an exact integer operation, "/" is C division toward zero on both sides.
// The rule is the library's own and is UNVERIFIED against ITU-T G.169 and against any other level control.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "igdsp.h"

#if defined(__HIPCC__)
#define IGDSP_AGC_HD __host__ __device__ inline __attribute__((always_inline))   // (no HIP header need come first)
#else
#define IGDSP_AGC_HD inline
#endif

namespace igdsp {

static_assert(sizeof(igdsp_agc_cfg) == 16 && sizeof(igdsp_agc_state) == 16 && sizeof(igdsp_agc_rec) == 16, "capi.AGC_CFG, AGC_STATE, AGC_REC");
static_assert(offsetof(igdsp_agc_state, env) == 4 && offsetof(igdsp_agc_state, flags) == 10 && offsetof(igdsp_agc_rec, flags) == 10 &&
              offsetof(igdsp_agc_rec, reserved) == 12, "state and record go as one 16-byte store of four dwords");
static_assert(IGDSP_AGC_BLOCK == 8 && IGDSP_MAX_PAYLOAD == 256 && IGDSP_MAX_PAYLOAD / IGDSP_AGC_BLOCK == 32, "a lane owns a block, 32 lanes a channel");

constexpr uint32_t kAgcCap = IGDSP_AGC_CAP, kAgcUnity = IGDSP_AGC_UNITY, kAgcCeilMax = 32767;
// ---- the two properties of the rule.
// (a) r_b = min(CAP, (ceil << 12) / p_b), so p_b * r_b <= ceil << 12.  Knot b has c_b <= m_b <= r_b and knot b + 1 has
//     c_(b+1) <= m_(b+1) <= r_b, T <= c, and t_j = T_b + ((T_(b+1) - T_b) * i) / 8 with 0 <= i < 8 lies between the two knots (division
//     toward zero never overshoots).  So t_j <= r_b and |x_j| * t_j <= p_b * r_b <= ceil << 12 <= 32767 << 12 < 2^27: 32 bits hold it.
static_assert(((uint64_t)kAgcCeilMax << 12) < (1ull << 27), "|x t| <= ceil << 12 < 2^27");
// (b) out_j = (x_j t_j + 2048) >> 12.  x t <= ceil << 12 gives out <= (ceil * 4096 + 2048) >> 12 = ceil; x t >= -(ceil << 12) gives
//     out >= (-ceil * 4096 + 2048) >> 12 = -ceil (the arithmetic shift floors -ceil + 1/2).  |out_j| <= ceil: no clamp exists.
static_assert((((int64_t)kAgcCeilMax << 12) + 2048) >> 12 == kAgcCeilMax && ((-((int64_t)kAgcCeilMax << 12)) + 2048) >> 12 == -(int64_t)kAgcCeilMax,
              "the rounding stays inside the ceiling");
// the slow gain's ramp: |Gn - G| <= 65535 times k <= 32 fits int32; target << 12 and ceil << 12 fit uint32
static_assert(65535ll * 32 < (1ll << 31) && ((uint64_t)kAgcCeilMax << 12) < (1ull << 32), "the intermediates are 32-bit");

constexpr bool agc_n_ok(uint32_t n) { return n >= 8u && n <= IGDSP_MAX_PAYLOAD && (n & 7u) == 0u; }
constexpr igdsp_agc_cfg agc_cfg_default() { return igdsp_agc_cfg{8192, 23170, 256, 1024, 32768, 1, 5, 5, 2, 6, 0}; }
constexpr bool agc_cfg_ok(const igdsp_agc_cfg *c)
{
    return !c || (c->gate >= 1u && c->target >= 1u && c->target <= c->ceil && c->ceil <= kAgcCeilMax && c->gmin >= 1u && c->gmin <= kAgcUnity &&
                  c->gmax >= kAgcUnity && c->att <= 15u && c->rel <= 15u && c->up <= 15u && c->down <= 15u && c->lrel >= 1u && c->lrel <= 15u);
}
constexpr igdsp_agc_cfg agc_cfg_or_default(const igdsp_agc_cfg *c) { return c ? *c : agc_cfg_default(); }
constexpr uint32_t agc_ctl(uint32_t v) { return v <= 3u ? v : (uint32_t)IGDSP_AGC_RUN; }

// the rule's numbers as the kernel carries them: 32-bit copies of the cfg
struct AgcK { uint32_t target, ceil, gate, gmin, gmax, att, rel, up, down, lrel; };
constexpr AgcK agc_k(const igdsp_agc_cfg &c) { return AgcK{c.target, c.ceil, c.gate, c.gmin, c.gmax, c.att, c.rel, c.up, c.down, c.lrel}; }

// what runs through a channel's frames
struct AgcRun { uint32_t env, G, cap; };
IGDSP_AGC_HD uint32_t agc_clamp(uint32_t v, uint32_t lo, uint32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
// a state as it is READ: another tag (or RESET) is the reset state, under the tag gain is clamped and every other value stands
IGDSP_AGC_HD AgcRun agc_read(uint32_t tag, uint32_t env, uint32_t gain, uint32_t cap, bool reset, const AgcK &k)
{
    if (reset || tag != (uint32_t)IGDSP_AGC_TAG) return AgcRun{0u, kAgcUnity, kAgcCap};   // gmin <= 4096 <= gmax
    return AgcRun{env & 0xFFFFu, agc_clamp(gain & 0xFFFFu, k.gmin, k.gmax), cap & 0xFFFFu};
}
// step 2 of an ACTIVE frame that is not frozen: env and G move, flags takes AT_MAX / AT_MIN; returns Gn
IGDSP_AGC_HD uint32_t agc_slow(AgcRun &r, uint32_t pk, const AgcK &k, uint32_t &flags)
{
    if (r.env == 0u) r.env = pk;
    else if (pk > r.env) r.env += (pk - r.env + (1u << k.att) - 1u) >> k.att;
    else r.env -= (r.env - pk) >> k.rel;
    const uint32_t q = (k.target << 12) / r.env;                           // env >= min(pk, old env) >= 1
    if (q > k.gmax) flags |= IGDSP_AGC_AT_MAX;
    if (q < k.gmin) flags |= IGDSP_AGC_AT_MIN;
    const uint32_t Gt = agc_clamp(q, k.gmin, k.gmax);
    if (Gt >= r.G) return r.G + ((Gt - r.G + (1u << k.up) - 1u) >> k.up);
    return r.G - ((r.G - Gt + (1u << k.down) - 1u) >> k.down);
}
// A_k: the slow gain at knot k of B
IGDSP_AGC_HD uint32_t agc_knot(uint32_t G, uint32_t Gn, uint32_t k, uint32_t B)
{
    return (uint32_t)((int32_t)G + (((int32_t)Gn - (int32_t)G) * (int32_t)k) / (int32_t)B);
}
// r_b: the largest gain block b takes under the ceiling
IGDSP_AGC_HD uint32_t agc_ratio(uint32_t p, uint32_t ceil)
{
    if (p == 0u) return kAgcCap;
    const uint32_t q = (ceil << 12) / p;
    return q < kAgcCap ? q : kAgcCap;
}
// one block of release
IGDSP_AGC_HD uint32_t agc_release(uint32_t c, uint32_t lrel)
{
    const uint32_t s = c >> lrel, v = c + (s > 1u ? s : 1u);
    return v < kAgcCap ? v : kAgcCap;
}
IGDSP_AGC_HD uint32_t agc_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
// sample i of a block between the knots Ta and Tb, and its output
IGDSP_AGC_HD uint32_t agc_gain_at(uint32_t Ta, uint32_t Tb, uint32_t i)
{
    return (uint32_t)((int32_t)Ta + (((int32_t)Tb - (int32_t)Ta) * (int32_t)i) / 8);
}
IGDSP_AGC_HD int32_t agc_out(int32_t x, uint32_t t) { return (x * (int32_t)t + 2048) >> 12; }
IGDSP_AGC_HD uint32_t agc_abs(int32_t v) { return (uint32_t)(v < 0 ? -v : v); }

// ---- the host: one frame of one channel.  cfg, n checked by the caller; out, rec may be nullptr
inline void agc_frame_run(const igdsp_agc_cfg &cfg, igdsp_agc_state &st, const int16_t *x, uint32_t n, uint32_t ctl_in, int16_t *out, igdsp_agc_rec *rec)
{
    const AgcK k = agc_k(cfg);
    const uint32_t ctl = agc_ctl(ctl_in), B = n / IGDSP_AGC_BLOCK;
    AgcRun r = agc_read(st.tag, st.env, st.gain, st.cap, ctl == IGDSP_AGC_RESET, k);
    uint32_t p[32], pk = 0;
    for (uint32_t b = 0; b < B; ++b) {
        p[b] = 0;
        for (uint32_t i = 0; i < 8u; ++i) { const uint32_t a = agc_abs(x[8u * b + i]); p[b] = a > p[b] ? a : p[b]; }
        pk = p[b] > pk ? p[b] : pk;
    }
    if (ctl == IGDSP_AGC_BYPASS) {
        if (out) std::memcpy(out, x, n * 2u);
        if (rec) *rec = igdsp_agc_rec{(uint16_t)r.G, (uint16_t)kAgcUnity, (uint16_t)pk, (uint16_t)pk, (uint16_t)r.env, IGDSP_AGC_BYPASSED, 0, 0};
        return;
    }
    uint32_t flags = pk >= k.gate ? (uint32_t)IGDSP_AGC_ACTIVE : 0u;
    if (ctl == IGDSP_AGC_FREEZE) flags |= IGDSP_AGC_FROZEN;
    const bool moves = pk >= k.gate && ctl != IGDSP_AGC_FREEZE;
    const uint32_t G = r.G, Gn = moves ? agc_slow(r, pk, k, flags) : G;
    uint32_t T[33], n_limited = 0, tmin = kAgcCap, c = 0;
    for (uint32_t q = 0; q <= B; ++q) {
        const uint32_t m = agc_min(q > 0u ? agc_ratio(p[q - 1u], k.ceil) : kAgcCap, q < B ? agc_ratio(p[q], k.ceil) : kAgcCap);
        if (q == 0u) {
            if (m < r.cap) flags |= IGDSP_AGC_ATTACKED;
            c = agc_min(m, r.cap);
        } else {
            c = agc_min(m, agc_release(c, k.lrel));
        }
        const uint32_t A = agc_knot(G, Gn, q, B);
        if (c < A) ++n_limited;
        T[q] = agc_min(A, c);
        tmin = agc_min(tmin, T[q]);
    }
    if (n_limited) flags |= IGDSP_AGC_LIMITED;
    uint32_t opk = 0;
    for (uint32_t b = 0; b < B; ++b)
        for (uint32_t i = 0; i < 8u; ++i) {
            const int32_t o = agc_out(x[8u * b + i], agc_gain_at(T[b], T[b + 1u], i));
            opk = agc_abs(o) > opk ? agc_abs(o) : opk;
            if (out) out[8u * b + i] = (int16_t)o;
        }
    st = igdsp_agc_state{(uint32_t)IGDSP_AGC_TAG, (uint16_t)r.env, (uint16_t)Gn, (uint16_t)c, (uint16_t)flags, 0};
    if (rec) *rec = igdsp_agc_rec{(uint16_t)Gn, (uint16_t)tmin, (uint16_t)pk, (uint16_t)opk, (uint16_t)r.env, (uint8_t)flags, (uint8_t)n_limited, 0};
}

}  // namespace igdsp
