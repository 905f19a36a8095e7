// igdsp_q7.h — the per-member level rule shared by igdsp_conf_mix (igdsp_k_conf.hip) and igdsp_bss_select (igdsp_k_bss.hip): a frame
// row's samples as magnitude + sign (q7_sample), and clamp16(trunc(x * gain / 128)) on them (IGDSP_Q7_LEVEL) (include/igdsp.h,
// "Conference mix").  A lane owns samples 4 lane .. 4 lane + 3 of the row.
#pragma once
#include "igdsp_device.h"
#include "igdsp_pcmrec.h"

namespace igdsp {

// the lane's four input samples of frame row `row` (G.711 codes in .x, or PCM in .x / .y); zeros past n.  vec: n % 4 == 0 and the rows
// 4-byte (G.711) / 8-byte (PCM) aligned
template <int IN>
__device__ __forceinline__ uint2 q7_load(const uint8_t *g711, const int16_t *pcm, uint32_t n, uint32_t vec, uint64_t row, uint32_t lane)
{
    const uint32_t b0 = 4u * lane;
    if (b0 >= n) return make_uint2(0u, 0u);
    if (IN == kConfG711) {
        const uint8_t *p = g711 + row * n + b0;
        if (vec) return make_uint2(*reinterpret_cast<const uint32_t *>(p), 0u);
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4u && b0 + k < n; ++k) w |= (uint32_t)p[k] << (8u * k);
        return make_uint2(w, 0u);
    } else {
        const int16_t *p = pcm + row * n + b0;
        if (vec) return *reinterpret_cast<const uint2 *>(p);
        uint32_t x = 0, y = 0;
        for (uint32_t k = 0; k < 4u && b0 + k < n; ++k) {
            const uint32_t v = (uint16_t)p[k];
            if (k < 2u) x |= v << (16u * k); else y |= v << (16u * (k - 2u));
        }
        return make_uint2(x, y);
    }
}

// sample k of a loaded value: magnitude and sign (law80: 0x80808080 for A-law rows, else 0; off: the lane's LUT replica)
template <int IN>
__device__ __forceinline__ void q7_sample(const uint2 *lut, uint2 v, uint32_t law80, uint32_t off, uint32_t k, uint32_t &ax, uint32_t &neg)
{
    if (IN == kConfG711) {
        const uint32_t t = (v.x & 0x7F7F7F7Fu) | law80;
        ax = lut_at(lut, t, off, 0x0C0C0400u + (k << 8)).y;
        neg = ((v.x >> (8u * k + 7u)) & 1u) ^ 1u;                  // a G.711 code is negative iff its bit 7 is clear
    } else {
        const int32_t x = (int32_t)(int16_t)(((k < 2u ? v.x : v.y) >> (16u * (k & 1u))) & 0xFFFFu);
        ax = (uint32_t)(x < 0 ? -x : x);
        neg = x < 0 ? 1u : 0u;
    }
}

// q = |clamp16(trunc(x * g / 128))| of x = neg ? -ax : ax at sample position pos of a row of len l (0 at and past l); sat |= 1 when
// the clamp fired.  A statement macro, not a function: igdsp_conf_mix's code is this exact sequence, and an inlined call schedules
// differently.
#define IGDSP_Q7_LEVEL(q, ax, neg, g, pos, l, sat)                                                                                 \
    uint32_t q = (g) == 128u ? (ax) : ((ax) * (g)) >> 7;               /* |x| * g / 128 truncated = |trunc(x * g / 128)| */       \
    if ((pos) >= (l)) q = 0u;                                          /* past the row's len (and past n) */                        \
    if ((g) > 128u) {                                                  /* only a gain above unity can leave int16 */                \
        const uint32_t lim_ = 32767u + (neg);                                                                                       \
        (sat) |= q > lim_ ? 1u : 0u;                                                                                                \
        q = min(q, lim_);                                                                                                           \
    }

// The frame's PCM row out[item][n] and record stats[item] from the lane's output samples o (samples 4 lane + k), the lane's sum of
// squares sq and peak, a clamp flag sat; empty: the len-0 record.  Either pointer may be nullptr; every lane of the wave active.
// (igdsp_conf_mix's conf_finish ends here too.)
__device__ __forceinline__ void q7_store(int16_t *out, igdsp_frame_stats *stats, uint64_t item, uint32_t n, uint32_t vec_out, uint32_t lane,
                                         const int32_t (&o)[4], bool empty, uint32_t sat, uint64_t sq, uint32_t peak)
{
    const uint32_t b0 = 4u * lane;
    if (out != nullptr && b0 < n) {
        int16_t *dst = out + item * n + b0;
        if (vec_out) {
            *reinterpret_cast<uint2 *>(dst) = make_uint2(((uint32_t)o[0] & 0xFFFFu) | ((uint32_t)o[1] << 16), ((uint32_t)o[2] & 0xFFFFu) | ((uint32_t)o[3] << 16));
        } else {
            for (uint32_t k = 0; k < 4u && b0 + k < n; ++k) dst[k] = (int16_t)o[k];
        }
    }
    if (stats == nullptr) return;
    const uint64_t sumsq = wave_sum_u64(sq);
    peak = wave_reduce_dpp(peak, OpMax{});
    const uint32_t any_sat = __builtin_amdgcn_ballot_w64(sat != 0u) != 0u ? 1u : 0u;
    if (lane == 0u) stats[item] = as_stats(empty ? pcm_record_empty() : pcm_record(sumsq, peak, n, any_sat ? (uint32_t)IGDSP_FLAG_SATURATED : 0u));
}

}  // namespace igdsp
