// igdsp_cng.h — the comfort-noise generator's rule (include/igdsp.h, "Comfort noise"; independent restatement: tests/cng_model.py) in
// plain C++17, so that the host entry igdsp_cng_frame and the kernel k_cng run the same code: how a state is read and written, which
// frames take a SID, the model of a payload (coefficients, gain target), the gain's step, the excitation and the lattice's sample.
// What the two sides do differently is only who walks: the host runs one channel's frame in a loop, the kernel gives a lane a channel
// and puts the SID step behind a wave-uniform test.  Every step is an exact integer operation, "/" is C division toward zero and ">>"
// on a signed value an arithmetic shift on both sides.  Nothing here indexes an array by a run-time value: the loops over the ten
// stages have constant bounds and unroll, so b[] and kq[] stay registers in the kernel.
// The rule is the library's own.  UNVERIFIED against RFC 3389 and G.711 Appendix II.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "igdsp.h"
#include "igdsp_cng_tab.h"

#if defined(__HIPCC__)
#define IGDSP_CNG_HD __host__ __device__ inline __attribute__((always_inline))   // (no HIP header need come first)
#define IGDSP_CNG_UNROLL _Pragma("unroll")
#else
#define IGDSP_CNG_HD inline
#define IGDSP_CNG_UNROLL
#endif

namespace igdsp {

static_assert(sizeof(igdsp_cng_state) == 96 && sizeof(igdsp_cng_rec) == 16, "capi.CNG_STATE, CNG_REC");
static_assert(offsetof(igdsp_cng_state, b) == 20 && offsetof(igdsp_cng_state, kq) == 60 && offsetof(igdsp_cng_state, since_sid) == 80 &&
              offsetof(igdsp_cng_state, have) == 84 && offsetof(igdsp_cng_rec, since_sid) == 8 && offsetof(igdsp_cng_rec, order) == 12,
              "the state goes as 24 dwords, the record as one 16-byte store");

constexpr uint32_t kCngOrder = 10;
constexpr int32_t kCngBMax = 131071, kCngKqMax = 16383;
constexpr uint32_t kCngGMax = IGDSP_CNG_GMAX, kCngGainMul = 7095, kCngStateWords = 24;
constexpr uint32_t kCngG[128] = {IGDSP_CNG_G_VALUES};
// every product of the sample loop fits int32; both factors of a stage product fit 24 bits
static_assert(16383ll * 131071 + 8192 < (1ll << 31) && 510ll * kCngGMax + 2048 < (1ll << 31) && kCngBMax < (1 << 23) && kCngKqMax < (1 << 23) &&
              kCngG[0] == 131072u && kCngG[105] == 1u && kCngG[106] == 0u && ((131072ull * 32768u * kCngGainMul) >> 23) == kCngGMax, "the widths");

constexpr bool cng_n_ok(uint32_t n) { return n >= 16u && n <= IGDSP_MAX_PAYLOAD && (n & 7u) == 0u; }
constexpr uint32_t cng_ctl(uint32_t v) { return v <= 3u ? v : (uint32_t)IGDSP_CNG_RUN; }

// what runs through a channel's frames
struct CngRun {
    uint32_t seed, ctr, g, g_tgt, since_sid, level, order, have;
    int32_t b[kCngOrder], kq[kCngOrder];
};

IGDSP_CNG_HD int32_t cng_clamp(int32_t v, int32_t m) { return v < -m ? -m : (v > m ? m : v); }             // one v_med3_i32
// a * b + c for factors that fit 24 bits (|kq| <= 16383, |b|, |f| <= 131071) and a sum that fits 32.  On the device the instruction is
// named: left to itself the compiler folds product and rounding term into the quarter-rate v_mad_u64_u32
IGDSP_CNG_HD int32_t cng_mad24(int32_t a, int32_t b, int32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int32_t r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
#else
    return a * b + c;
#endif
}
IGDSP_CNG_HD uint32_t cng_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// e(q): the four bytes of mix(q ^ hs) summed (one v_sad_u8 against 0), minus 510
IGDSP_CNG_HD int32_t cng_exc(uint32_t q, uint32_t hs)
{
    const uint32_t r = cng_mix(q ^ hs);
#if defined(__HIP_DEVICE_COMPILE__)
    return (int32_t)__builtin_amdgcn_sad_u8(r, 0u, 0u) - 510;
#else
    return (int32_t)((r & 255u) + ((r >> 8) & 255u) + ((r >> 16) & 255u) + (r >> 24)) - 510;
#endif
}
// the floor square root of v <= 2^30
IGDSP_CNG_HD uint32_t cng_isqrt(uint32_t v)
{
    uint32_t r = 0u;
    for (uint32_t bit = 1u << 15; bit; bit >>= 1) {
        const uint32_t t = r | bit;
        if (t * t <= v) r = t;                                             // t <= 65535: the square fits
    }
    return r;
}

// a state as it is READ, from its 24 dwords: another tag (or RESET) is the RESET state with the caller's seed; under the tag b, kq, g
// and g_tgt are clamped, have is its bit 0 and every other value stands
IGDSP_CNG_HD bool cng_is_reset(uint32_t tag, bool reset) { return reset || tag != (uint32_t)IGDSP_CNG_TAG; }
IGDSP_CNG_HD CngRun cng_read(const uint32_t (&w)[kCngStateWords], bool reset, uint32_t seed)
{
    CngRun r;
    const bool z = cng_is_reset(w[0], reset);
    r.seed = z ? seed : w[1];
    r.ctr = z ? 0u : w[2];
    r.g = z ? 0u : (w[3] < kCngGMax ? w[3] : kCngGMax);
    r.g_tgt = z ? 0u : (w[4] < kCngGMax ? w[4] : kCngGMax);
    IGDSP_CNG_UNROLL
    for (uint32_t i = 0; i < kCngOrder; ++i) {
        r.b[i] = z ? 0 : cng_clamp((int32_t)w[5u + i], kCngBMax);
        r.kq[i] = z ? 0 : cng_clamp((int32_t)(int16_t)(w[15u + (i >> 1)] >> (16u * (i & 1u))), kCngKqMax);
    }
    r.since_sid = z ? 0u : (w[20] & 0xFFFFu);
    r.level = z ? 0u : ((w[20] >> 16) & 0xFFu);
    r.order = z ? 0u : (w[20] >> 24);
    r.have = z ? 0u : (w[21] & 1u);
    return r;
}
// and as it is WRITTEN: the tag, flags the last frame's (the yardstick: as read), reserved 0
IGDSP_CNG_HD void cng_write(const CngRun &r, uint32_t flags, uint32_t (&w)[kCngStateWords])
{
    w[0] = (uint32_t)IGDSP_CNG_TAG; w[1] = r.seed; w[2] = r.ctr; w[3] = r.g; w[4] = r.g_tgt;
    IGDSP_CNG_UNROLL
    for (uint32_t i = 0; i < kCngOrder; ++i) w[5u + i] = (uint32_t)r.b[i];
    IGDSP_CNG_UNROLL
    for (uint32_t i = 0; i < kCngOrder; i += 2u) w[15u + (i >> 1)] = ((uint32_t)r.kq[i] & 0xFFFFu) | ((uint32_t)r.kq[i + 1u] << 16);
    w[20] = r.since_sid | r.level << 16 | r.order << 24;
    w[21] = r.have | (flags & 0xFFu) << 8;
    w[22] = 0u; w[23] = 0u;
}
IGDSP_CNG_HD void cng_pack_rec(const CngRun &r, uint32_t flags, uint32_t (&w)[4])
{
    w[0] = r.g; w[1] = r.g_tgt; w[2] = r.since_sid | flags << 16 | r.level << 24; w[3] = r.order;
}

// step 1: the frame's flags FROZEN, SID_EMPTY and VOICE, and whether it takes a SID.  len = min(sid_len, 11)
IGDSP_CNG_HD uint32_t cng_len(uint32_t sid_len) { return sid_len < 11u ? sid_len : 11u; }
IGDSP_CNG_HD uint32_t cng_classify(uint32_t kind, bool frozen, uint32_t len, bool &take)
{
    const bool sid = kind == (uint32_t)IGDSP_VAD_SID;
    take = sid && !frozen && len > 0u;
    return (frozen ? (uint32_t)IGDSP_CNG_F_FROZEN : 0u) | (sid && len == 0u ? (uint32_t)IGDSP_CNG_F_SID_EMPTY : 0u) |
           (!sid && kind != (uint32_t)IGDSP_VAD_NONE ? (uint32_t)IGDSP_CNG_F_VOICE : 0u);
}
// step 2's model of a payload: pw = its first twelve bytes as dwords (bytes at and past len are not read), len = 1..11.
// k = 258 * (min(N, 254) - 127) is igdsp_sid_decode's
IGDSP_CNG_HD uint32_t cng_model(const uint32_t (&pw)[3], uint32_t len, int32_t (&kq)[kCngOrder])
{
    uint64_t p = 1ull << 30;
    IGDSP_CNG_UNROLL
    for (uint32_t i = 0; i < kCngOrder; ++i) {
        const uint32_t N = (pw[(i + 1u) >> 2] >> (8u * ((i + 1u) & 3u))) & 0xFFu;
        const int32_t k = i + 1u < len ? 258 * ((int32_t)(N > 254u ? 254u : N) - 127) : 0;
        kq[i] = k / 2;
        p = (p * (uint64_t)((1 << 30) - k * k)) >> 30;                     // |k| <= 32766
    }
    return cng_isqrt((uint32_t)p);
}
IGDSP_CNG_HD uint32_t cng_gain_of(uint32_t G, uint32_t sp) { return (uint32_t)(((uint64_t)G * sp * kCngGainMul) >> 23); }
// the rest of step 2 for a taken SID: G = G[min(level, 127)] (the caller's table), sp and kq from cng_model
IGDSP_CNG_HD void cng_take(CngRun &r, uint32_t level, uint32_t len, uint32_t G, uint32_t sp)
{
    r.level = level; r.order = len - 1u;
    r.g_tgt = cng_gain_of(G, sp);
    if (!r.have) { r.g = r.g_tgt; r.have = 1u; }
}
// what every frame that is not bypassed does behind steps 1 and 2: since_sid, the flags SID, NO_MODEL and GENERATED, step 5's gain.
// The caller generates the row when the flags carry GENERATED, and adds n to ctr
IGDSP_CNG_HD uint32_t cng_step(CngRun &r, uint32_t flags, bool take)
{
    if (take) { r.since_sid = 0u; flags |= (uint32_t)IGDSP_CNG_F_SID; }
    else r.since_sid = r.since_sid < 65535u ? r.since_sid + 1u : 65535u;
    if (flags & (uint32_t)IGDSP_CNG_F_VOICE) return flags;
    if (!r.have) return flags | (uint32_t)IGDSP_CNG_F_NO_MODEL;
    const int32_t d = (int32_t)r.g_tgt - (int32_t)r.g;
    r.g = (uint32_t)((int32_t)r.g + (d - d / 2));
    return flags | (uint32_t)IGDSP_CNG_F_GENERATED;
}
// step 5 for one sample: excitation e through the gain and the ten stages; returns f (the output is cng_out(f))
IGDSP_CNG_HD int32_t cng_sample(int32_t e, int32_t g, int32_t (&b)[kCngOrder], const int32_t (&kq)[kCngOrder])
{
    int32_t f = cng_clamp((e * g + 2048) >> 12, kCngBMax);
    IGDSP_CNG_UNROLL
    for (uint32_t i = kCngOrder; i >= 1u; --i) {
        f = cng_clamp(f - (cng_mad24(kq[i - 1u], b[i - 1u], 8192) >> 14), kCngBMax);
        if (i < kCngOrder) b[i] = cng_clamp(b[i - 1u] + (cng_mad24(kq[i - 1u], f, 8192) >> 14), kCngBMax);
    }
    b[0] = f;
    return f;
}
IGDSP_CNG_HD int32_t cng_out(int32_t f)
{
    const int32_t o = (f + 2) >> 2;
    return o < -32768 ? -32768 : (o > 32767 ? 32767 : o);
}
IGDSP_CNG_HD bool cng_clips(int32_t o) { return o >= 32767 || o <= -32767; }

// ---- the host: step 2 of a payload; one frame of one channel.  n checked by the caller
inline void cng_payload_words(const uint8_t *sid, uint32_t len, uint32_t (&pw)[3])
{
    uint8_t pay[12] = {0};
    if (sid && len) std::memcpy(pay, sid, len);                            // len <= 11
    std::memcpy(pw, pay, 12);
}
inline uint32_t cng_gain_host(const uint8_t *payload, uint32_t len)
{
    uint32_t pw[3];
    int32_t kq[kCngOrder];
    cng_payload_words(payload, cng_len(len), pw);
    const uint32_t level = pw[0] & 0xFFu, sp = cng_model(pw, cng_len(len), kq);
    return cng_gain_of(kCngG[level < 127u ? level : 127u], sp);
}
// returns len_out.  sid is read on a taken SID only; voice may be nullptr; rec may be nullptr
inline uint32_t cng_frame_run(igdsp_cng_state &st, uint32_t kind, const uint8_t *sid, uint32_t sid_len, const int16_t *voice, uint32_t n, uint32_t ctl_in,
                              uint32_t seed, int16_t *out, igdsp_cng_rec *rec)
{
    uint32_t ctl = cng_ctl(ctl_in), sw[kCngStateWords], w[4];
    std::memcpy(sw, &st, sizeof st);
    CngRun r = cng_read(sw, ctl == IGDSP_CNG_RESET, seed);
    if (ctl == IGDSP_CNG_RESET) ctl = IGDSP_CNG_RUN;
    const uint32_t len = cng_len(sid_len);
    bool take = false;
    uint32_t flags = cng_classify(kind, ctl == IGDSP_CNG_FREEZE, len, take), len_out = 0u;
    const bool is_voice = (flags & IGDSP_CNG_F_VOICE) != 0u;
    if (ctl == IGDSP_CNG_BYPASS) {
        flags = IGDSP_CNG_F_BYPASSED;
    } else {
        if (take) {
            uint32_t pw[3];
            cng_payload_words(sid, len, pw);
            const uint32_t level = pw[0] & 0xFFu, sp = cng_model(pw, len, r.kq);
            cng_take(r, level, len, kCngG[level < 127u ? level : 127u], sp);
        }
        flags = cng_step(r, flags, take);
    }
    if (is_voice && voice) {
        std::memcpy(out, voice, (size_t)n * 2u);
        len_out = n;
    } else if (flags & IGDSP_CNG_F_GENERATED) {
        const uint32_t hs = cng_mix(r.seed);
        for (uint32_t j = 0; j < n; ++j) {
            const int32_t o = cng_out(cng_sample(cng_exc(r.ctr + j, hs), (int32_t)r.g, r.b, r.kq));
            if (cng_clips(o)) flags |= IGDSP_CNG_F_CLIPPED;
            out[j] = (int16_t)o;
        }
        len_out = n;
    } else {
        std::memset(out, 0, (size_t)n * 2u);
    }
    if (ctl != IGDSP_CNG_BYPASS) {
        r.ctr += n;
        cng_write(r, flags, sw);
        std::memcpy(&st, sw, sizeof st);
    }
    cng_pack_rec(r, flags, w);
    if (rec) std::memcpy(rec, w, 16);
    return len_out;
}

}  // namespace igdsp
