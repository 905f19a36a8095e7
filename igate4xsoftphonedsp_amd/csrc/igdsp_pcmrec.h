// igdsp_pcmrec.h — the PCM record: the 16-byte igdsp_frame_stats over a row of n int16 samples, as igdsp_conf_mix, igdsp_bss_select,
// igdsp_ptt_arbitrate, igdsp_plc_conceal, igdsp_snd_combine / split, igdsp_tone_generate and igdsp_resample write it (include/igdsp.h;
// independent restatement: tests/record_model.py).  Three things: the per-lane accumulate, the fold of a group of lanes, the rule.
// (The G.711 record of igdsp_decode_meter, with probe, CLIPPED and byte_mean, is not this one: pack_stats, igdsp_device.h.)
#pragma once
#include "igdsp_internal.h"

namespace igdsp {

typedef short v2i16 __attribute__((ext_vector_type(2)));
typedef unsigned short v2u16_t __attribute__((ext_vector_type(2)));

// ---- accumulate: a lane's sum of squares and peak ----
__device__ __forceinline__ void pcm_acc(uint32_t x, uint64_t &sq, uint32_t &pk)    // one sample, as its 16 bits
{
    const int32_t s = (int16_t)x;
    const uint32_t ax = (uint32_t)(s < 0 ? -s : s);
    sq += ax * ax;                                                                 // <= 2^30
    pk = max(pk, ax);
}
// two samples in one dword, packed math: x . x as one dot product (2^31 for two -32768: the 32 bits hold it), |x| as max(x, 0 - x)
// in 16 bits (-32768 stays 0x8000 = 32768 unsigned) folded into two running unsigned maxima
__device__ __forceinline__ void pcm_acc2(uint32_t w, uint64_t &sq, v2u16_t &pk)
{
    const v2i16 x = __builtin_bit_cast(v2i16, w);
    sq += (uint32_t)__builtin_amdgcn_sdot2(x, x, 0, false);
    const v2u16_t neg = (v2u16_t)(0) - __builtin_bit_cast(v2u16_t, w);             // wraps: well defined
    pk = __builtin_elementwise_max(pk, __builtin_bit_cast(v2u16_t, __builtin_elementwise_max(x, __builtin_bit_cast(v2i16, neg))));
}

// ---- fold: lane G g + G - 1 gets op over lanes G g .. G g + G - 1 (G = 4, 8, a DPP row of 16) ----
// An inclusive scan by row_shr steps on the VALU's DPP path (no LDS round trip); a lane without a source takes the identity 0, which
// suits unsigned add and max.  Every lane of the wave active.
struct OpAdd { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct OpMax { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return max(a, b); } };

template <int G, typename Op>
__device__ __forceinline__ uint32_t group_fold(uint32_t v, Op op)
{
    static_assert(G == 4 || G == 8 || G == 16, "a group inside a DPP row");
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false));                       // row_shr:1
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false));                       // row_shr:2
    if constexpr (G > 4) v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false));  // row_shr:4
    if constexpr (G > 8) v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false));  // row_shr:8
    return v;
}
// The 64-bit sum over a group as two 24-bit limbs {the low 24 bits, the rest}, each folded in 32 bits: exact while the group's total is
// below 2^56.  group_sum_u64 folds and joins; a kernel whose one storing lane needs the sum may fold with group_limbs (every lane) and
// join with limbs_u64 in that lane.
template <int G>
__device__ __forceinline__ uint2 group_limbs(uint64_t v)
{
    const uint32_t lo = group_fold<G>((uint32_t)v & 0xFFFFFFu, OpAdd{});
    const uint32_t hi = group_fold<G>((uint32_t)(v >> 24), OpAdd{});
    return make_uint2(lo, hi);
}
__device__ __forceinline__ uint64_t limbs_u64(const uint2 l) { return (uint64_t)l.x + ((uint64_t)l.y << 24); }
template <int G>
__device__ __forceinline__ uint64_t group_sum_u64(uint64_t v) { return limbs_u64(group_limbs<G>(v)); }

// ---- the rule: {sumsq lo, sumsq hi, rms bits, peak | byte_mean 0 << 16 | flags << 24} ----
// sumsq exact, rms the correctly rounded float expression (IEEE divide + sqrt, hipcc's default), peak = max |x| (32768 for -32768),
// SILENT when peak <= 8; extra: the stage's own flag (SATURATED, CONCEALED).  A kernel that stores the struct bit-casts this value.
// (its three steps are functions of their own for k_snd, which keeps its schedule only with its address arithmetic between them)
__device__ __forceinline__ float pcm_rms(uint64_t sumsq, uint32_t n) { return sqrtf((float)sumsq / (float)n); }
__device__ __forceinline__ uint32_t pcm_flags(uint32_t peak, uint32_t extra) { return (peak <= 8u ? (uint32_t)IGDSP_FLAG_SILENT : 0u) | extra; }
__device__ __forceinline__ uint4 pcm_pack(uint64_t sumsq, float rms, uint32_t peak, uint32_t flags)
{
    return make_uint4((uint32_t)sumsq, (uint32_t)(sumsq >> 32), __float_as_uint(rms), peak | (flags << 24));
}
__device__ __forceinline__ uint4 pcm_record(uint64_t sumsq, uint32_t peak, uint32_t n, uint32_t extra)
{
    const float rms = pcm_rms(sumsq, n);
    const uint32_t flags = pcm_flags(peak, extra);
    return pcm_pack(sumsq, rms, peak, flags);
}
// a row that does not exist (len 0, no member, an IDLE tick)
__device__ __forceinline__ uint4 pcm_record_empty() { return make_uint4(0u, 0u, 0u, (uint32_t)IGDSP_FLAG_EMPTY << 24); }

__device__ __forceinline__ igdsp_frame_stats as_stats(const uint4 rec)
{
    static_assert(sizeof(igdsp_frame_stats) == sizeof(uint4), "the record is one dwordx4");
    return __builtin_bit_cast(igdsp_frame_stats, rec);
}

}  // namespace igdsp
