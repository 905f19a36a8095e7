// igdsp_lanes.h — the lane primitives the stage kernels share (HIP only): the DPP row of 16 lanes and its reductions, the packed
// int16 pair, G.711 codes to signed samples one, two and eight at a time, the lane-per-channel tile's addressing (k_cng, k_filt) and
// the event list's pass over dense records (k_tdet_list, k_vad_list).  One copy and one comment each; a stage keeps only what is its
// own shape (tdet_max8, agc_half_all, vad_levels, ...) and builds it on these.  Header-only, namespace igdsp.
#pragma once
#include "igdsp_device.h"

namespace igdsp {

// ---- the DPP row: v of another lane of the row of 16, on the VALU's DPP path (no LDS round trip).  Every lane of the wave active ----
template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false); }
template <int CTRL>
__device__ __forceinline__ uint64_t dpp64(uint64_t v) { return (uint64_t)dpp<CTRL>((uint32_t)v) | (uint64_t)dpp<CTRL>((uint32_t)(v >> 32)) << 32; }
// the sum / the maximum over the 16 lanes of a row, in each of them (row_ror 8, 4, 2, 1)
__device__ __forceinline__ uint32_t row16_sum(uint32_t v)
{
    v += dpp<0x128>(v);
    v += dpp<0x124>(v);
    v += dpp<0x122>(v);
    return v + dpp<0x121>(v);
}
__device__ __forceinline__ uint32_t row16_max(uint32_t v)
{
    v = max(v, dpp<0x128>(v));
    v = max(v, dpp<0x124>(v));
    v = max(v, dpp<0x122>(v));
    return max(v, dpp<0x121>(v));
}
// a 64-bit sum as two 24-bit limbs, each folded in 32 bits: exact while the row's total is below 2^56
__device__ __forceinline__ uint64_t row16_sum64(uint64_t v)
{
    return (uint64_t)row16_sum((uint32_t)v & 0xFFFFFFu) + ((uint64_t)row16_sum((uint32_t)(v >> 24)) << 24);
}

// ---- two int16 in a dword: acc + x.lo * w.lo + x.hi * w.hi (v_dot2_i32_i16), and the pack (no clamp: the values fit) ----
__device__ __forceinline__ uint32_t dot2(uint32_t x, uint32_t w, uint32_t acc)
{
    return (uint32_t)__builtin_amdgcn_sdot2(__builtin_bit_cast(v2i16, x), __builtin_bit_cast(v2i16, w), (int)acc, false);
}
__device__ __forceinline__ uint32_t pack2(int32_t lo, int32_t hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }

// ---- G.711 codes to signed samples, as igdsp_decode_meter decodes: the ITU magnitude of the law (ulaw_abs / alaw_abs), the sign applied
// outside it: a code is negative iff its bit 7 is clear.  g711_abs and g711_signed are the two halves for a stage that works on the
// magnitude between them: k_agc zeroes an idle lane's, and igdsp_vad_run shifts the MAGNITUDE right by 2 before the sign (-(m >> 2)).
// igdsp_tone_detect shifts the SIGNED sample (x >> 3, which rounds a negative sample toward minus infinity) and so decodes whole
// samples first.  The two shift rules differ bit for bit on negative samples and stay apart: no helper here shifts ----
__device__ __forceinline__ uint32_t g711_abs(uint32_t code, bool alaw) { return alaw ? alaw_abs(code) : ulaw_abs(code); }
__device__ __forceinline__ int32_t g711_signed(uint32_t code, int32_t m) { return (code & 0x80u) ? m : -m; }
__device__ __forceinline__ int32_t g711_s16(uint32_t code, bool alaw) { return g711_signed(code, (int32_t)g711_abs(code, alaw)); }
// the two codes in the low 16 bits of u as two samples (g711_two) or as one dword of two int16 (g711_pair)
struct G711Two { int32_t x0, x1; };
__device__ __forceinline__ G711Two g711_two(uint32_t u, bool alaw)
{
    const uint32_t c0 = u & 0xFFu, c1 = (u >> 8) & 0xFFu;
    const int32_t m0 = (int32_t)g711_abs(c0, alaw), m1 = (int32_t)g711_abs(c1, alaw);
    return G711Two{g711_signed(c0, m0), g711_signed(c1, m1)};
}
__device__ __forceinline__ uint32_t g711_pair(uint32_t u, bool alaw) { const G711Two x = g711_two(u, alaw); return pack2(x.x0, x.x1); }
// eight codes (two dwords, as they lie in memory) as eight int16 in four dwords
__device__ __forceinline__ uint4 g711_decode8(uint32_t lo, uint32_t hi, bool alaw)
{
    return make_uint4(g711_pair(lo, alaw), g711_pair(lo >> 16, alaw), g711_pair(hi, alaw), g711_pair(hi >> 16, alaw));
}

// ---- the lane-per-channel tile (k_cng, k_filt; the rule: tile_row_dwords, tile_inv, igdsp_route.h): the wave walks the tile's 16-byte
// pieces in memory order, item i is piece i % P of row i / P, the division done by the multiplier inv ----
struct TileItem { uint32_t row, piece; };                                  // i < 2^12: the product fits (tile_inv)
__device__ __forceinline__ TileItem tile_item(uint32_t i, uint32_t inv, uint32_t P) { const uint32_t rw = (i * inv) >> 20; return TileItem{rw, i - rw * P}; }
__device__ __forceinline__ uint32_t *tile_piece(uint32_t *tile, uint32_t stride, const TileItem t) { return tile + t.row * stride + 4u * t.piece; }

// ---- the event list's pass over a stage's dense records [F][C]: a wave is 64 consecutive channels of one frame (item = f * W + w).
// The count pass leaves the wave's number of event lanes at counts[item]; the store pass, behind k_link_scan, finds the wave's offset
// there and stores each event at the offset plus the lane's rank among the wave's event lanes (events past cap are dropped).
// Rule: Vec, the record as a vector; is_event(rec, mask); make_event(c, f, rec), the 16 bytes of the stage's event.
template <bool WRITE, class Rule, class Rec, class Event>
__device__ __forceinline__ void event_list_pass(const Rec *rec, uint32_t C, uint32_t F, uint32_t W, uint32_t mask, uint32_t *counts, Event *events,
                                                uint32_t cap)
{
    using Vec = typename Rule::Vec;
    static_assert(sizeof(Vec) == sizeof(Rec) && sizeof(Event) == sizeof(uint4), "a record is one load, an event one 16-byte store");
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = (uint64_t)blockIdx.x * kListWaves + (threadIdx.x >> 6);
    if (item >= (uint64_t)F * W) return;                                   // wave-uniform
    const uint32_t f = (uint32_t)(item / W), w = (uint32_t)(item - (uint64_t)f * W);
    const uint64_t c = (uint64_t)w * 64u + lane;
    Vec r(0u);                                                             // a lane past the last channel: no event
    if (c < C) r = *reinterpret_cast<const Vec *>(rec + (uint64_t)f * C + c);
    const bool ev = Rule::is_event(r, mask);
    const uint64_t bal = __builtin_amdgcn_ballot_w64(ev);
    if (!WRITE) {
        if (lane == 0u) counts[item] = (uint32_t)__popcll(bal);
    } else if (ev) {
        const uint4 e = Rule::make_event((uint32_t)c, f, r);               // ahead of the offset's load
        const uint32_t idx = counts[item] + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (idx < cap) *reinterpret_cast<uint4 *>(events + idx) = e;
    }
}

}  // namespace igdsp
