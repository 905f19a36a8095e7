// igdsp_ec.h — the echo canceller's rule (include/igdsp.h, "Echo canceller"; independent restatement: tests/ec_model.py) in plain
// C++17, so that the host entry igdsp_ec_frame and the kernel k_ec run the same code: how a state is read, the output of an exact
// sum, the double-talk step, the update's shift and the saturating update of one weight.  What the two sides do differently is only
// how they form the sums: the host walks the taps in 64 bits, the kernel gives a lane 16 (or 8) taps in 32 bits and adds the lanes of a
// row (igdsp_k_ec.hip).  Every sum is an exact integer, so the order does not matter.
// The rule is the library's own and is UNVERIFIED against ITU-T G.168, against speex, WebRTC and any other canceller.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "igdsp.h"

#if defined(__HIPCC__)
#define IGDSP_EC_HD __host__ __device__ __forceinline__
#else
#define IGDSP_EC_HD inline
#endif

namespace igdsp {

static_assert(sizeof(igdsp_ec_cfg) == 12 && sizeof(igdsp_ec_rec) == 16, "capi.EC_CFG, capi.EC_REC");
static_assert(sizeof(igdsp_ec_state) == 1552 && sizeof(igdsp_ec_state) <= 1664 && sizeof(igdsp_ec_state) % 16 == 0 &&
              offsetof(igdsp_ec_state, hist) == 1024 && offsetof(igdsp_ec_state, hang) == 1536, "capi.EC_STATE; 16-byte pieces");
static_assert(IGDSP_EC_MAX_TAIL == 256 && IGDSP_EC_BLOCK == 8 && IGDSP_MAX_PAYLOAD == 256, "a lane owns L / 16 taps; a block is four sample pairs");

// the magnitudes: wh = w >> 18 and xs = far >> 2 (a stored value is read clamped to the same range), es = e / 4
constexpr int64_t kEcWhMax = 1ll << 13, kEcXsMax = 1ll << 13, kEcEsMax = 1ll << 13;
static_assert(kEcWhMax * kEcXsMax * 16 <= (1ll << 30), "16 taps of a lane: |sum wh xs| <= 2^30 fits int32");
static_assert(kEcEsMax * kEcXsMax * IGDSP_EC_BLOCK <= (1ll << 29), "a block's gradient of one tap: |sum es xs| <= 2^29 fits int32");
static_assert(kEcWhMax * kEcXsMax * IGDSP_EC_MAX_TAIL <= (1ll << 34), "a whole tail needs 64 bits (or a split): the row's sum");
static_assert(kEcXsMax * kEcXsMax * 16 <= (1ll << 30) && kEcXsMax * kEcXsMax * IGDSP_EC_MAX_TAIL <= (1ll << 34), "P: a lane in 32 bits, the row in 64");
// the update: |g| <= 2^29 shifted left by at most 31 stays below 2^60; added to |w| <= 2^31 it cannot leave int64
static_assert(29 + 31 < 62, "the update's intermediate fits int64");

constexpr bool ec_n_ok(uint32_t n) { return n >= 2u && n <= IGDSP_MAX_PAYLOAD && (n & 1u) == 0u; }
constexpr bool ec_tail_ok(uint32_t L) { return L == 128u || L == 256u; }
constexpr igdsp_ec_cfg ec_cfg_default(uint32_t tail) { return igdsp_ec_cfg{(uint16_t)tail, 2, 0, 1u << 16, 80, 256}; }
constexpr bool ec_cfg_ok(const igdsp_ec_cfg *cfg) { return !cfg || (ec_tail_ok(cfg->tail) && cfg->mu_shift <= 6u); }
constexpr igdsp_ec_cfg ec_cfg_or_default(const igdsp_ec_cfg *cfg) { return cfg ? *cfg : ec_cfg_default(128u); }
constexpr uint32_t ec_ctl(uint32_t v) { return v <= 3u ? v : (uint32_t)IGDSP_EC_RUN; }

IGDSP_EC_HD int32_t ec_clamp16(int32_t v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
// a far sample as the filter sees it, and a stored one as it is READ (a state the stage did not write stays inside the bounds above)
IGDSP_EC_HD int32_t ec_xs(int32_t far) { return far >> 2; }
IGDSP_EC_HD int32_t ec_hist(int32_t v) { return v < -8192 ? -8192 : (v > 8191 ? 8191 : v); }
IGDSP_EC_HD int32_t ec_wh(int32_t w) { return w >> 18; }
// the output sample from the exact sum over the tail
IGDSP_EC_HD int32_t ec_out(int32_t near, int64_t acc) { return ec_clamp16(near - ec_clamp16((int32_t)((acc + 1024) >> 11))); }
IGDSP_EC_HD int32_t ec_es(int32_t e) { return e / 4; }
// the double-talk step of one block: xm = max |xs| over the last L + b values, dmax = max |near| over the block
IGDSP_EC_HD uint32_t ec_hang(uint32_t hang, uint32_t xm, uint32_t dmax, uint32_t hang_cfg, uint32_t dmin)
{
    if (2u * dmax > 4u * xm && dmax >= dmin) return hang_cfg;
    return hang > 0u ? hang - 1u : 0u;
}
IGDSP_EC_HD int32_t ec_bit_length(uint64_t P)
{
    return P ? 64 - (int32_t)__builtin_clzll((unsigned long long)P) : 0;
}
// one weight: returns the new value, sets sat when it was clipped
IGDSP_EC_HD int32_t ec_update(int32_t w, int32_t g, int32_t sh, bool &sat)
{
    const int64_t d = sh >= 0 ? (int64_t)((uint64_t)(int64_t)g << sh) : ((int64_t)g >> -sh);
    const int64_t s = (int64_t)w + d;
    if (s > 2147483647ll) { sat = true; return 2147483647; }
    if (s < -2147483648ll) { sat = true; return (int32_t)-2147483648ll; }
    return (int32_t)s;
}
IGDSP_EC_HD bool ec_tag_ok(uint32_t tag, uint32_t L) { return tag == ((uint32_t)IGDSP_EC_TAG | L); }

// ---- the host: one frame of one channel.  cfg, n checked by the caller; far nullptr = no far end; out, rec may be nullptr
inline void ec_frame_run(const igdsp_ec_cfg &cfg, igdsp_ec_state &st, const int16_t *near, const int16_t *far, uint32_t n, uint32_t ctl_in,
                         int16_t *out, igdsp_ec_rec *rec)
{
    const uint32_t L = cfg.tail;
    uint32_t ctl = ec_ctl(ctl_in);
    int32_t w[IGDSP_EC_MAX_TAIL] = {};
    int32_t x[IGDSP_EC_MAX_TAIL + IGDSP_MAX_PAYLOAD] = {};
    uint32_t hang = 0, sflags = 0;
    if (ctl != IGDSP_EC_RESET && ec_tag_ok(st.tag, L)) {
        for (uint32_t k = 0; k < L; ++k) { w[k] = st.w[k]; x[k] = ec_hist(st.hist[k]); }
        hang = st.hang;
        sflags = st.flags & (uint32_t)IGDSP_EC_W_SATURATED;
    }
    if (ctl == IGDSP_EC_RESET) ctl = IGDSP_EC_RUN;
    if (!far) ctl = IGDSP_EC_BYPASS;
    for (uint32_t i = 0; i < n; ++i) x[L + i] = far ? ec_xs(far[i]) : 0;
    int16_t e[IGDSP_MAX_PAYLOAD];
    uint32_t flags = ctl == IGDSP_EC_BYPASS ? (uint32_t)IGDSP_EC_BYPASSED : 0u, n_adapt = 0, n_dt = 0;
    uint64_t se = 0, sn = 0;
    for (uint32_t s = 0; s < n; s += IGDSP_EC_BLOCK) {
        const uint32_t b = n - s < IGDSP_EC_BLOCK ? n - s : (uint32_t)IGDSP_EC_BLOCK;
        if (ctl == IGDSP_EC_BYPASS) {
            for (uint32_t j = 0; j < b; ++j) e[s + j] = near[s + j];
            continue;
        }
        int32_t wh[IGDSP_EC_MAX_TAIL];
        for (uint32_t k = 0; k < L; ++k) wh[k] = ec_wh(w[k]);
        uint32_t dmax = 0;
        for (uint32_t j = 0; j < b; ++j) {
            int64_t acc = 0;
            for (uint32_t k = 0; k < L; ++k) acc += (int64_t)wh[k] * x[L + s + j - k];
            e[s + j] = (int16_t)ec_out(near[s + j], acc);
            const uint32_t a = (uint32_t)(near[s + j] < 0 ? -(int32_t)near[s + j] : (int32_t)near[s + j]);
            dmax = a > dmax ? a : dmax;
        }
        const uint32_t end = L + s + b;                                    // one past the block's last value
        uint64_t P = 0;
        uint32_t xm = 0;
        for (uint32_t k = 0; k < L; ++k) P += (uint64_t)((int64_t)x[end - 1u - k] * x[end - 1u - k]);
        for (uint32_t k = 0; k < L + b; ++k) {
            const uint32_t a = (uint32_t)(x[end - 1u - k] < 0 ? -x[end - 1u - k] : x[end - 1u - k]);
            xm = a > xm ? a : xm;
        }
        hang = ec_hang(hang, xm, dmax, cfg.hang, cfg.dmin);
        if (hang > 0u) { ++n_dt; flags |= IGDSP_EC_DOUBLETALK; }
        if (P >= cfg.pmin) flags |= IGDSP_EC_FAR_ACTIVE;
        if (hang == 0u && P >= cfg.pmin && ctl != IGDSP_EC_FREEZE) {
            const int32_t sh = 31 - (int32_t)cfg.mu_shift - ec_bit_length(P);
            bool sat = false;
            for (uint32_t k = 0; k < L; ++k) {
                int32_t g = 0;
                for (uint32_t j = 0; j < b; ++j) g += ec_es(e[s + j]) * x[L + s + j - k];
                w[k] = ec_update(w[k], g, sh, sat);
            }
            ++n_adapt;
            flags |= IGDSP_EC_ADAPTED;
            if (sat) { flags |= IGDSP_EC_W_SATURATED; sflags |= IGDSP_EC_W_SATURATED; }
        }
    }
    uint32_t wmax = 0;
    for (uint32_t k = 0; k < L; ++k) {
        const int32_t v = ec_wh(w[k]);
        const uint32_t a = (uint32_t)(v < 0 ? -v : v);
        wmax = a > wmax ? a : wmax;
    }
    for (uint32_t i = 0; i < n; ++i) {
        sn += (uint64_t)((int64_t)near[i] * near[i]);
        se += (uint64_t)((int64_t)e[i] * e[i]);
        if (out) out[i] = e[i];
    }
    std::memset(st.w, 0, sizeof(st.w));
    std::memset(st.hist, 0, sizeof(st.hist));
    for (uint32_t k = 0; k < L; ++k) { st.w[k] = w[k]; st.hist[k] = (int16_t)x[n + k]; }
    st.hang = hang; st.flags = sflags; st.tag = (uint32_t)IGDSP_EC_TAG | L; st.reserved = 0;
    if (rec) *rec = igdsp_ec_rec{(uint32_t)(sn >> 8), (uint32_t)(se >> 8), (uint8_t)flags, (uint8_t)n_adapt, (uint8_t)n_dt, 0, (uint16_t)wmax, 0};
}

}  // namespace igdsp
