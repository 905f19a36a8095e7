// igdsp_k_spec.hip — the spectrum graph (igdsp_spectrum): per channel a 1 024-point windowed transform every hop_frames frames, the raw
// dBFS array, its peak, and the array averaged in the dB domain.  Semantics: include/igdsp.h, section "Spectrum"; the rule itself, its
// arithmetic and the index arithmetic of the data flow: igdsp_spec.h (the host entry igdsp_spec_frame walks the same functions over 64
// lanes in a loop); independent restatement: tests/spec_model.py.
//
// Shape (route: spec_route).  A wave owns one channel for the launch's frames; the waves of a block are independent.  The history is a
// ring of 1 024 int16 in the wave's LDS, loaded from the state (oldest first there) at the start and stored back at the end; the averaged
// array lives in registers, 8 bins per lane (bin = lane + 64 j), as do the twiddle factors of pass 2 and of the split pass, which are the
// same at every hop; the window values and pass 1's twiddle factors are read at the hop from the 12 KiB of tables, which the CU's L1
// keeps (registers for them too would cost the fourth wave per SIMD).  Per frame: the row (loaded a frame ahead, up to 4 samples per lane) is decoded and appended to the ring; at a
// hop the lane reads its 8 complex points (sample pairs, one dword each while the ring's head is even), windows them, and runs
//   pass 1 (8-point butterflies over a)  -> twiddle -> tile, row k0     -> loads over b
//   pass 2 (over b)                      -> twiddle -> tile, row k1     -> loads over c
//   pass 3 (over c): the lane holds Z[lane + 64 k2]; the partner Z[512 - k] comes from the mirror lane by ds_bpermute (__shfl)
//   split, power, 10 log10f, the peak by two wave reductions (the value, then the lowest bin that has it), the average.
// The tile is the wave's own: LDS operations of one wave execute in order, wave_lds_fence keeps the compiler from moving them.  A row of the
// tile is 72 points: stores of a pass go row-wise (64 consecutive points), loads of the next go 8 points apart in 8 rows, and the
// padding spreads a 32-lane group of those over all 64 banks.
// COPY (the compute-free yardstick, tools/spec_bench.py): the same rows into the ring, the same ring loads, tile stores and loads and
// global stores at a hop, no window, butterfly, twiddle, mirror fetch, split, log or average: raw is the lane's points as they came back
// from the tile, a record carries only IGDSP_SPEC_HOP, the averaged array is stored as it was read.
#include "igdsp_lanes.h"
#include "igdsp_spec.h"

namespace igdsp {

__device__ const float d_spec_win[kSpecN] = {IGDSP_SPEC_WIN_VALUES};
__device__ const float d_spec_tw[2 * kSpecN] = {IGDSP_SPEC_TW_VALUES};

struct SpecArgs {
    const uint8_t *g711, *codec;
    const int16_t *pcm;
    uint32_t C, F, n, hop;
    float alpha;
    igdsp_spec_state *state;
    igdsp_spec_rec *rec;
    float *avg, *raw;
};

// one wave's LDS
struct SpecLds {
    __attribute__((aligned(16))) int16_t ring[kSpecN];
    __attribute__((aligned(16))) SpecC tile[kSpecTile];
};
static_assert(sizeof(SpecLds) * kSpecWaves == kSpecLdsBytes, "spec_route's LDS");

__device__ __forceinline__ uint32_t spec_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ SpecC spec_tw_dev(uint32_t k) { return SpecC{d_spec_tw[2u * k], d_spec_tw[2u * k + 1u]}; }

// the lane's samples of row o (sample lane + 64 q in v[q]), as they lie in memory: codes or PCM bit patterns
__device__ __forceinline__ void spec_row_load(const SpecArgs &a, uint32_t o, uint32_t lane, uint32_t (&v)[4])
{
    const uint64_t base = (uint64_t)o * a.n;
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t i = lane + 64u * q;
        v[q] = 0u;
        if (i < a.n) v[q] = a.g711 ? (uint32_t)a.g711[base + i] : (uint32_t)(uint16_t)a.pcm[base + i];
    }
}
__device__ __forceinline__ int16_t spec_decode(uint32_t v, bool g711, bool alaw)
{
    return (int16_t)(g711 ? g711_s16(v, alaw) : (int32_t)v);
}
// sample pair m of the history (samples 2 m, 2 m + 1, oldest first) from the ring whose oldest sample is at head
__device__ __forceinline__ uint32_t spec_pair(const SpecLds &L, uint32_t head, uint32_t m)
{
    if (!(head & 1u)) return reinterpret_cast<const uint32_t *>(L.ring)[((head >> 1) + m) & (kSpecN / 2u - 1u)];
    const uint32_t lo = (uint16_t)L.ring[(head + 2u * m) & (kSpecN - 1u)], hi = (uint16_t)L.ring[(head + 2u * m + 1u) & (kSpecN - 1u)];
    return lo | (hi << 16);
}

template <bool COPY>
__global__ __launch_bounds__(kSpecWaves * 64, kSpecResident) void k_spec(const SpecArgs a)
{
    __shared__ SpecLds lds[kSpecWaves];
    const uint32_t lane = threadIdx.x & 63u, w = spec_uni(threadIdx.x >> 6);
    const uint64_t cl = (uint64_t)blockIdx.x * kSpecWaves + w;
    if (cl >= a.C) return;                                                 // waves are independent: no block barrier below
    const uint32_t c = (uint32_t)cl, n = a.n, hop = a.hop;
    SpecLds &L = lds[w];
    igdsp_spec_state *st = a.state + c;
    const bool g711 = a.g711 != nullptr;
    const bool alaw = g711 && a.codec[c] == IGDSP_PT_PCMA;

    // the state: the history into the ring (head 0), the scalars wave-uniform, the lane's 8 bins of the averaged array
    {
        const uint32_t *h32 = reinterpret_cast<const uint32_t *>(st->hist);
        uint32_t *r32 = reinterpret_cast<uint32_t *>(L.ring);
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) r32[lane + 64u * q] = h32[lane + 64u * q];
    }
    uint32_t head = 0;
    const uint32_t since0 = spec_uni(spec_since_read(st->since, hop));
    uint32_t since = since0, hops = spec_uni(st->hops);
    const bool live = (spec_uni(st->flags) & IGDSP_SPEC_LIVE) != 0u;
    float avg[8];
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) avg[j] = live ? st->avg[spec_bin(lane, j)] : IGDSP_SPEC_FLOOR_DB;
    const uint64_t last_hop = spec_last_hop(since0, hop, a.F);             // the frame whose raw array d_raw gets (F: none)

    // the lane's constants
    SpecC tw2[8], tw3[8];
    if (!COPY) {
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) {
            tw2[q] = spec_tw_dev(spec_tw2(lane, q));
            tw3[q] = spec_tw_dev(spec_bin(lane, q));
        }
    }
    wave_lds_fence();

    uint32_t nxt[4];
    spec_row_load(a, c, lane, nxt);
    for (uint32_t f = 0; f < a.F; ++f) {
        const uint32_t o = f * a.C + c;                                    // < 2^32 - 32: the argument rule
        uint32_t cur[4];
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) cur[q] = nxt[q];
        if (f + 1u < a.F) spec_row_load(a, o + a.C, lane, nxt);            // in flight during the transform
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            const uint32_t i = lane + 64u * q;
            if (i < n) L.ring[(head + i) & (kSpecN - 1u)] = spec_decode(cur[q], g711, alaw);
        }
        head = (head + n) & (kSpecN - 1u);
        wave_lds_fence();                                                  // the ring's new samples, for every lane
        ++since;
        uint32_t rec_lo = 0u;
        float rec_db = 0.0f;
        if (since == hop) {
            since = 0u;
            ++hops;
            SpecC v[8];
            float raw[8];
            uint32_t tl = lane;                                            // the lane, opaque: the table loads below stay inside the hop
            asm volatile("" : "+v"(tl));
#pragma unroll
            for (uint32_t q = 0; q < 8u; ++q) {
                const uint32_t m = spec_in_point(tl, q), p = spec_pair(L, head, m);
                const float x0 = (float)(int16_t)(p & 0xFFFFu), x1 = (float)(int16_t)(p >> 16);
                if (COPY) {
                    v[q] = SpecC{x0, x1};
                } else {
                    const float2 wn = *reinterpret_cast<const float2 *>(d_spec_win + 2u * m);   // 64 lanes, 512 consecutive bytes
                    v[q] = SpecC{x0 * wn.x, x1 * wn.y};
                }
            }
            if (!COPY) {
                spec_r8(v);
#pragma unroll
                for (uint32_t q = 1; q < 8u; ++q) v[q] = spec_mul(v[q], spec_tw_dev(spec_tw1(tl, q)));
            }
#pragma unroll
            for (uint32_t q = 0; q < 8u; ++q) L.tile[spec_x1_store(lane, q)] = v[q];
            wave_lds_fence();
#pragma unroll
            for (uint32_t q = 0; q < 8u; ++q) v[q] = L.tile[spec_x1_load(lane, q)];
            wave_lds_fence();
            if (!COPY) {
                spec_r8(v);
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q) v[q] = spec_mul(v[q], tw2[q]);
            }
#pragma unroll
            for (uint32_t q = 0; q < 8u; ++q) L.tile[spec_x2_store(lane, q)] = v[q];
            wave_lds_fence();
#pragma unroll
            for (uint32_t q = 0; q < 8u; ++q) v[q] = L.tile[spec_x2_load(lane, q)];
            wave_lds_fence();
            if (COPY) {
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q) raw[q] = v[q].re;
                rec_lo = (uint32_t)IGDSP_SPEC_HOP << 16;
            } else {
                spec_r8(v);
                const int src = (int)spec_mirror_lane(lane);
                uint32_t best = 0u, bin = 0u;
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q) {
                    SpecC zp{__shfl(v[7u - q].re, src), __shfl(v[7u - q].im, src)};
                    if (lane == 0u) zp = v[(8u - q) & 7u];
                    raw[q] = spec_db(spec_split2(v[q], zp, tw3[q]));
                    const uint32_t key = spec_key(raw[q]);
                    if (key > best) { best = key; bin = spec_bin(lane, q); }               // ascending bins: the lowest of a tie stays
                    avg[q] = spec_average(avg[q], raw[q], a.alpha);
                }
                const uint32_t top = wave_reduce_dpp(best, OpMax{});
                const uint32_t cand = best == top ? bin : kSpecN - 1u;
                const uint32_t peak_bin = (kSpecN - 1u) - wave_reduce_dpp((kSpecN - 1u) - cand, OpMax{});
                rec_lo = peak_bin | ((uint32_t)IGDSP_SPEC_HOP << 16);
                rec_db = spec_unkey(top);
            }
            if (a.raw && f == last_hop) {
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q) a.raw[(uint64_t)c * kSpecBins + spec_bin(lane, q)] = raw[q];
            }
        }
        if (a.rec && lane == 0u) {
            uint2 r;
            r.x = rec_lo;
            r.y = __float_as_uint(rec_db);
            *reinterpret_cast<uint2 *>(a.rec + o) = r;
        }
    }

    // the state back: the history oldest first, the averaged array, the scalars
    {
        uint32_t *h32 = reinterpret_cast<uint32_t *>(st->hist);
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) h32[lane + 64u * q] = spec_pair(L, head, lane + 64u * q);
    }
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
        st->avg[spec_bin(lane, j)] = avg[j];
        if (a.avg) a.avg[(uint64_t)c * kSpecBins + spec_bin(lane, j)] = avg[j];
    }
    if (lane == 0u) {
        st->since = since;
        st->hops = hops;
        st->flags = IGDSP_SPEC_LIVE;
    }
}

hipError_t launch_spectrum(const LaunchCfg &, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, uint32_t C, uint32_t F, uint32_t n,
                           uint32_t hop_frames, float alpha, igdsp_spec_state *state, igdsp_spec_rec *rec, float *avg, float *raw, bool yardstick,
                           hipStream_t s)
{
    const SpecRoute r = spec_route(C, F, n);
    if (r.grid == 0) return hipSuccess;
    const SpecArgs a{g711, codec, pcm, C, F, n, hop_frames, alpha, state, rec, avg, raw};
    hipLaunchKernelGGL(yardstick ? k_spec<true> : k_spec<false>, dim3(r.grid), dim3(r.threads), 0, s, a);
    return hipGetLastError();
}

}  // namespace igdsp
