// igdsp_device.h — device-side building blocks shared by the kernel translation units (igdsp_k_*.hip): G.711 expansion
// formulas, streaming load / store helpers (global and buffer form), the launch-aggregate commit, record packing, the
// 32-replica expansion LUT, probe helpers, the persistent-block work queue, the block-owned form's LDS window and
// item queue.  Header-only, namespace igdsp.
//
// Reference semantics the kernels reproduce (all citations /root/reference):
//   G.711 expansion / compression : performed by pjmedia around adapter->stream_rtp_cb (TransportAdapter.cpp:301) / before
//       transport_send_rtp (TransportAdapter.cpp:635); ITU-T G.711.
//   byte_mean "audioLevel"        : roip_ed137.cpp:6564-6568, 6513-6517.
//   silence probe                 : TransportAdapter.cpp:657-673.
//   hold / window aggregate       : Functions.cpp:2126-2145, 2155-2167.
#pragma once
#include "igdsp_internal.h"
#include "igdsp_pcmrec.h"
#include "igdsp_pitch.h"

#include <algorithm>
#include <cstdlib>

namespace igdsp {

// ----------------------------------------------------------------------------
// G.711 expansion magnitude by the ITU segment formula (used to build the LDS
// tables in-kernel; no table ever comes from host memory).
// ----------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ulaw_abs(uint32_t code)
{
    const uint32_t u = ~code & 0x7Fu;
    return ((((u & 15u) * 2u + 33u) << (u >> 4)) - 33u) << 2;
}

__device__ __forceinline__ uint32_t alaw_abs(uint32_t code)
{
    const uint32_t a = (code ^ 0x55u) & 0x7Fu;
    const uint32_t s = a >> 4, q = a & 15u;
    const uint32_t m = (s == 0u) ? (q * 2u + 1u) : ((q * 2u + 33u) << (s - 1u));
    return m << 3;
}

// streaming (read-once) 16-byte load: native vector type so the nontemporal builtin accepts it
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld_stream(const uint4 *p)
{
    const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

// 16 bytes at dword (not 16-byte) alignment: gfx950 global loads only need dword alignment for dwordx4 (measured < 1 %
// slower than aligned ones in a bare stream, tools/misaligned_loads.py).  Nontemporal like every other streaming load here.
typedef uint32_t u32x4_a4_t __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ uint4 ld16_dw(const uint8_t *p)
{
    const u32x4_a4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_a4_t *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

// write-once 16-byte store (records / PCM are never re-read by this launch)
#ifndef IGDSP_NT_STORE
#define IGDSP_NT_STORE 0      // cached stores measured ~1 % faster than nontemporal for the 1 KiB record blocks
#endif
__device__ __forceinline__ void st_stream(uint4 *p, const uint4 v)
{
#if IGDSP_NT_STORE
    u32x4_t t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    __builtin_nontemporal_store(t, reinterpret_cast<u32x4_t *>(p));
#else
    *p = v;
#endif
}

// Buffer-instruction form of the streaming accesses: a wave-uniform 128-bit descriptor (SGPRs) + one 32-bit lane offset
// (lane * 16) + a scalar offset.  The compiler never forms SGPR-base addressing for global_load / global_store on this path
// (every address is a per-lane 64-bit VGPR pair and 10 KiB spans need several of them), so the kernels that are short of
// registers describe their windows themselves.  Raw buffer, no swizzle, 32-bit data format; the range check is switched off
// by the largest record count (every offset used is < 2^32 because the base is re-seated per item / frame).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, 0xFFFFFFFFu, 0x00020000);
}
// the same with a range: raw buffer accesses at an offset >= bytes are dropped by the hardware (stores) / return zero (loads),
// which lets a lane opt out of a store without a branch
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc_ranged(const void *base, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint4 buf_ld_stream(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff)
{
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 2);          // aux 2 = nt
    return make_uint4(v.x, v.y, v.z, v.w);
}
#ifndef IGDSP_RTS_LOAD_AUX
#define IGDSP_RTS_LOAD_AUX 2      // A/B: cache policy of k_roundtrip_strided's dword-aligned input pieces (2 = nt, 0 = default)
#endif
__device__ __forceinline__ uint4 buf_ld_pieces(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff)
{
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, IGDSP_RTS_LOAD_AUX);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void buf_st(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff, const uint4 v)
{
    u32x4_t t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    __builtin_amdgcn_raw_buffer_store_b128(t, r, (int)voff, (int)soff, 0);
}

// The 1 KiB record block of k_meter_chunk64 (64 lanes x 16 B at `base`).  0 = cached (st_stream), 1 = nontemporal, 2 = write-through:
// a plain or nt store leaves its line dirty in the XCD's L2 and the launch's end then waits for the write-back of whatever is still
// there; an sc1 store (buffer cache policy 16) goes through to memory and drops the line.  Whole 1 KiB blocks either way.
// Measured: DESIGN 3.1, profiles/meter_launch_ledger.md.
#ifndef IGDSP_RECORD_STORE
#define IGDSP_RECORD_STORE 2
#endif
__device__ __forceinline__ void st_record_block(igdsp_frame_stats *base, uint32_t lane, const uint4 v)
{
#if IGDSP_RECORD_STORE == 2
    u32x4_t t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    __builtin_amdgcn_raw_buffer_store_b128(t, make_rsrc(base), (int)(lane * 16u), 0, 16);            // aux 16 = sc1
#elif IGDSP_RECORD_STORE == 1
    u32x4_t t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    __builtin_nontemporal_store(t, reinterpret_cast<u32x4_t *>(base) + lane);
#else
    st_stream(reinterpret_cast<uint4 *>(base) + lane, v);
#endif
}

__device__ __forceinline__ uint32_t full_scale(bool alaw) { return alaw ? 32256u : 32124u; }

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m)
{
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = (uint32_t)__shfl_xor((int)lo, m, 64);
    hi = (uint32_t)__shfl_xor((int)hi, m, 64);
    return ((uint64_t)hi << 32) | lo;
}

// Launch aggregate: wave butterfly -> one LDS slot per wave -> wave 0 folds the block -> ONE set of
// device-scope integer atomics per BLOCK (exact, order-independent u64 add / max).  Same-line atomics
// serialise at roughly 90 per microsecond, so per-wave commits (4096 waves x 7 words) cost ~0.3 ms;
// per-block commits keep it to a few microseconds that overlap with other blocks' tails.
// `slots` = nwaves x 4 uint2 of LDS.  Must be reached by every thread of the block.
__device__ __forceinline__ void agg_commit_block(igdsp_aggregate *agg, uint32_t rank, uint2 *slots, uint32_t nwaves,
                                                 uint64_t sumsq, uint64_t samples, uint32_t frames, uint32_t n_silent,
                                                 uint32_t n_clipped, uint32_t bm_sum, uint32_t peak)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sumsq += shfl_xor_u64(sumsq, m);
        samples += shfl_xor_u64(samples, m);
        frames += (uint32_t)__shfl_xor((int)frames, m, 64);
        n_silent += (uint32_t)__shfl_xor((int)n_silent, m, 64);
        n_clipped += (uint32_t)__shfl_xor((int)n_clipped, m, 64);
        bm_sum += (uint32_t)__shfl_xor((int)bm_sum, m, 64);
        peak = max(peak, (uint32_t)__shfl_xor((int)peak, m, 64));
    }
    __syncthreads();                       // every wave is done with its LDS strip
    if (lane == 0) {
        slots[wave * 4 + 0] = make_uint2((uint32_t)sumsq, (uint32_t)(sumsq >> 32));
        slots[wave * 4 + 1] = make_uint2((uint32_t)samples, (uint32_t)(samples >> 32));
        slots[wave * 4 + 2] = make_uint2(frames, n_silent);
        slots[wave * 4 + 3] = make_uint2(n_clipped | 0u, bm_sum);
    }
    // peak rides in a fifth word: reuse slot 2/3 would overflow nothing, keep it simple and separate
    __shared__ uint32_t peak_slots[kWavesPerBlock];
    if (lane == 0) peak_slots[wave] = peak;
    __syncthreads();
    if (wave == 0) {
        uint64_t s = 0, sm = 0;
        uint32_t fr = 0, sil = 0, cl = 0, bm = 0, pk = 0;
        if (lane < nwaves) {
            const uint2 a = slots[lane * 4 + 0], b = slots[lane * 4 + 1], c = slots[lane * 4 + 2], d = slots[lane * 4 + 3];
            s = ((uint64_t)a.y << 32) | a.x; sm = ((uint64_t)b.y << 32) | b.x;
            fr = c.x; sil = c.y; cl = d.x; bm = d.y; pk = peak_slots[lane];
        }
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) {   // nwaves <= 16
            s += shfl_xor_u64(s, m); sm += shfl_xor_u64(sm, m);
            fr += (uint32_t)__shfl_xor((int)fr, m, 64); sil += (uint32_t)__shfl_xor((int)sil, m, 64);
            cl += (uint32_t)__shfl_xor((int)cl, m, 64); bm += (uint32_t)__shfl_xor((int)bm, m, 64);
            pk = max(pk, (uint32_t)__shfl_xor((int)pk, m, 64));
        }
        if (lane == 0 && fr != 0) {
            atomicAdd((unsigned long long *)&agg->sumsq, (unsigned long long)s);
            atomicAdd((unsigned long long *)&agg->samples, (unsigned long long)sm);
            atomicAdd((unsigned long long *)&agg->frames, (unsigned long long)fr);
            atomicAdd((unsigned long long *)&agg->n_silent, (unsigned long long)sil);
            atomicAdd((unsigned long long *)&agg->n_clipped, (unsigned long long)cl);
            atomicAdd((unsigned long long *)&agg->byte_mean_sum, (unsigned long long)bm);
            atomicMax((unsigned long long *)&agg->peak_slot[rank & (IGDSP_AGG_MAX_RANKS - 1)], (unsigned long long)pk);
        }
    }
}

// the 16-byte record as one dwordx4 store: {sumsq lo, sumsq hi, rms bits, peak | byte_mean<<16 | flags<<24}
__device__ __forceinline__ uint4 pack_stats(uint64_t sumsq, uint32_t peak, uint32_t bsum, uint32_t n, bool alaw,
                                            bool probe, uint32_t &byte_mean, uint32_t &flags)
{
    byte_mean = (bsum / n) & 255u;
    flags = (peak <= 8u ? IGDSP_FLAG_SILENT : 0u) | (probe ? IGDSP_FLAG_PROBE_D5 : 0u) |
            (peak == full_scale(alaw) ? IGDSP_FLAG_CLIPPED : 0u);
    const float rms = sqrtf((float)sumsq / (float)n);
    return make_uint4((uint32_t)sumsq, (uint32_t)(sumsq >> 32), __float_as_uint(rms), peak | (byte_mean << 16) | (flags << 24));
}

__device__ __forceinline__ igdsp_frame_stats make_stats(uint64_t sumsq, uint32_t peak, uint32_t bsum, uint32_t n,
                                                        bool alaw, bool probe)
{
    igdsp_frame_stats st;
    st.sumsq = sumsq;
    st.rms = sqrtf((float)sumsq / (float)n);   // IEEE divide + sqrt (hipcc default: correctly rounded)
    st.peak = (uint16_t)peak;
    st.byte_mean = (uint8_t)(bsum / n);
    st.flags = (uint8_t)((peak <= 8u ? IGDSP_FLAG_SILENT : 0) | (probe ? IGDSP_FLAG_PROBE_D5 : 0) |
                         (peak == full_scale(alaw) ? IGDSP_FLAG_CLIPPED : 0));
    return st;
}

// Wave64 reductions on the VALU's DPP path (no LDS round trips): group_fold's inclusive scan inside each row of 16
// lanes (igdsp_pcmrec.h), then row_bcast15 / row_bcast31 carry the row totals upward; lane 63 ends up
// with the wave total and is read out with v_readlane.  Identity 0 suits unsigned add and max.
template <typename Op>
__device__ __forceinline__ uint32_t wave_reduce_dpp(uint32_t v, Op op)
{
    v = group_fold<16>(v, op);
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false));   // row_bcast:15 -> rows 1, 3
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false));   // row_bcast:31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// Barrier-free launch-aggregate commit for the persistent kernels: a wave that has run out of work reduces its partials with DPP (no LDS, no shuffle tree), lane 0 adds the
// wave totals into a 48-byte block accumulator with seven LDS atomics and bumps a counter; the
// wave that finds the counter at nwaves - 1 moves the block totals to the aggregate with device atomics.  No wave waits for
// another, so the kernel's tail is one LDS round trip instead of two barriers and two shuffle trees (agg_commit_block):
// measured on k_meter_chunk64, 0.2314 -> 0.2294 ms per launch (the kernel without any aggregate: 0.2281).
struct AggBlock { unsigned long long sumsq, samples; uint32_t frames, n_silent, n_clipped, bm_sum, peak, done; };

__device__ __forceinline__ void agg_block_init(AggBlock &b)      // one thread, before a barrier every wave passes
{
    b.sumsq = 0; b.samples = 0; b.frames = 0; b.n_silent = 0; b.n_clipped = 0; b.bm_sum = 0; b.peak = 0; b.done = 0;
}

// sumsq / bm_sum / peak: per lane.  samples / frames / n_silent / n_clipped: wave-uniform (lane 0 adds them).
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)      // 24-bit limbs: 64 of them fit 32 bits
{
    const uint32_t s0 = wave_reduce_dpp((uint32_t)v & 0xFFFFFFu, OpAdd{});
    const uint32_t s1 = wave_reduce_dpp((uint32_t)(v >> 24) & 0xFFFFFFu, OpAdd{});
    const uint32_t s2 = wave_reduce_dpp((uint32_t)(v >> 48), OpAdd{});
    return (uint64_t)s0 + ((uint64_t)s1 << 24) + ((uint64_t)s2 << 48);
}

// sumsq / samples / bm_sum / peak: per lane.  frames / n_silent / n_clipped: wave-uniform.  When the block's last wave is
// out, the last BLOCK out re-arms the device work queue gq (nullptr: static schedule) for the next launch.
// agg == nullptr: only the counters move.
__device__ __forceinline__ void wave_exit(igdsp_aggregate *agg, uint32_t rank, AggBlock &b, uint32_t nwaves, uint32_t lane,
                                          uint32_t *gq, uint32_t G, uint64_t sumsq, uint64_t samples, uint32_t bm_sum, uint32_t peak,
                                          uint32_t frames, uint32_t n_silent, uint32_t n_clipped)
{
    // (all 64 lanes adding into one LDS address measured 6 us per block: same-address LDS atomics run one lane at a time)
    uint64_t tot = 0, smp = 0;
    uint32_t bm = 0, pk = 0;
    if (agg != nullptr) {
        tot = wave_sum_u64(sumsq);
        smp = wave_sum_u64(samples);
        bm = wave_reduce_dpp(bm_sum, OpAdd{});
        pk = wave_reduce_dpp(peak, OpMax{});
    }
    if (lane == 0) {
        if (agg != nullptr) {
            atomicAdd(&b.sumsq, (unsigned long long)tot);
            atomicAdd(&b.samples, (unsigned long long)smp);
            atomicAdd(&b.bm_sum, bm);
            atomicMax(&b.peak, pk);
            atomicAdd(&b.frames, frames);
            atomicAdd(&b.n_silent, n_silent);
            atomicAdd(&b.n_clipped, n_clipped);
        }
        // LDS operations of one wave execute in order, so every add above has landed when the counter moves
        if (__hip_atomic_fetch_add(&b.done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) == nwaves - 1u) {
            if (agg != nullptr && b.frames != 0u) {
                atomicAdd((unsigned long long *)&agg->sumsq, b.sumsq);
                atomicAdd((unsigned long long *)&agg->samples, b.samples);
                atomicAdd((unsigned long long *)&agg->frames, (unsigned long long)b.frames);
                atomicAdd((unsigned long long *)&agg->n_silent, (unsigned long long)b.n_silent);
                atomicAdd((unsigned long long *)&agg->n_clipped, (unsigned long long)b.n_clipped);
                atomicAdd((unsigned long long *)&agg->byte_mean_sum, (unsigned long long)b.bm_sum);
                atomicMax((unsigned long long *)&agg->peak_slot[rank & (IGDSP_AGG_MAX_RANKS - 1)], (unsigned long long)b.peak);
            }
            if (gq != nullptr && atomicAdd(gq + 1, 1u) == G - 1u) { gq[0] = 0u; gq[1] = 0u; }
        }
    }
}

// Merge one work item's window into hold[c] when several items share a channel (frame segments): device-scope integer
// atomics (adds, and a CAS loop on the {peak_hold, level_max, level_min} word) — exact and order-independent, so the
// result is bit-identical to the sequential fold (keeplogAudioLevel, Functions.cpp:2126-2145).
__device__ __forceinline__ void hold_merge(igdsp_chan_hold *g, const igdsp_chan_hold &h)
{
    atomicAdd((unsigned long long *)&g->sumsq_acc, (unsigned long long)h.sumsq_acc);
    atomicAdd(&g->count, h.count); atomicAdd(&g->level_sum, h.level_sum); atomicAdd(&g->samples, h.samples);
    atomicAdd(&g->n_silent, h.n_silent); atomicAdd(&g->n_clipped, h.n_clipped);
    uint32_t *pw = reinterpret_cast<uint32_t *>(&g->peak_hold);
    uint32_t old = *pw, want;
    do {
        const uint32_t pk = max(old & 0xFFFFu, (uint32_t)h.peak_hold), mx = max((old >> 16) & 0xFFu, (uint32_t)h.level_max);
        const uint32_t mn = min(old >> 24, (uint32_t)h.level_min);
        want = pk | (mx << 16) | (mn << 24);
        if (want == old) break;
        const uint32_t seen = atomicCAS(pw, old, want);
        if (seen == old) break;
        old = seen;
    } while (true);
}

// the same when ONE work item owns the channel for the whole launch: plain read-modify-write
__device__ __forceinline__ void hold_add(igdsp_chan_hold *gp, const igdsp_chan_hold &h)
{
    igdsp_chan_hold g = *gp;
    g.sumsq_acc += h.sumsq_acc; g.count += h.count; g.level_sum += h.level_sum; g.samples += h.samples;
    g.peak_hold = max(g.peak_hold, h.peak_hold); g.level_max = max(g.level_max, h.level_max); g.level_min = min(g.level_min, h.level_min);
    g.n_silent += h.n_silent; g.n_clipped += h.n_clipped;
    *gp = g;
}

// ============================================================================
// Shared machinery of the tuned n == 160 kernels (k_meter_chunk64, k_meter_rtp64, k_roundtrip_chunk64).
//
// Expansion LUT: 256 entries (law<<7 | code&0x7F) x 32 replicas x 8 B = 64 KiB
// in LDS, entry = { (|x|/4)^2 , |x| }.  Replica r sits at byte offset r*8 of the
// entry's 256-byte row, and lane l always reads replica l&31, so every
// ds_read_b64 of a 32-lane group touches 32 distinct 8-byte slots = all 64
// banks once: conflict-free for ANY code distribution.  The address is built
// by ONE v_perm_b32: byte0 = replica offset, byte1 = law|code7.
// (|x|/4)^2 <= 8064^2 < 2^26 so 16 samples fit a u32 partial; x^2 = 16 * that.
// ============================================================================

__device__ __forceinline__ void fill_lut(uint2 *lut)
{
    for (uint32_t i = threadIdx.x; i < (uint32_t)kLutEntries; i += blockDim.x) {
        const uint32_t e = i >> 5;                 // law<<7 | code7
        const uint32_t ax = (e & 0x80u) ? alaw_abs(e) : ulaw_abs(e);
        const uint32_t m = ax >> 2;
        lut[i] = make_uint2(m * m, ax);
    }
}

// The same table with each value computed ONCE per block (k_meter_chunk64, whose prologue is on the launch's critical path):
// item i = (entry e = i >> 2, quarter r = i & 3) evaluates the segment formula of entry e and writes 8 of its 32 replicas as four 16-byte LDS stores (two replicas each).  Store k goes to 64-byte quarter (k + e) & 3 of the
// 256-byte row, so the 16 lanes of four neighbouring entries cover all 64 banks once per instruction.
__device__ __forceinline__ void fill_lut_once(uint2 *lut)                 // lut: 16-byte aligned
{
    for (uint32_t i = threadIdx.x; i < (uint32_t)kLutEntries / 8u; i += blockDim.x) {
        const uint32_t e = i >> 2, r = i & 3u;     // e = law<<7 | code7
        const uint32_t ax = (e & 0x80u) ? alaw_abs(e) : ulaw_abs(e);
        const uint32_t m = ax >> 2;
        const uint4 v = make_uint4(m * m, ax, m * m, ax);
        uint4 *row = reinterpret_cast<uint4 *>(lut + e * 32u);      // 16 x 16 B
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) row[((k + e) & 3u) * 4u + r] = v;
    }
}

__device__ __forceinline__ uint2 lut_at(const uint2 *lut, uint32_t t, uint32_t off, uint32_t sel)
{
    // byte address = off | (byte_k(t) << 8); v_perm_b32: sel bytes 4..7 pick from t, 0..3 from off, 0x0C = 0x00
    const uint32_t addr = __builtin_amdgcn_perm(t, off, sel);
    return *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(lut) + addr);
}

// The record-only kernels that are NOT bound by HBM (k_meter_strided: 6 % under the bare stream with its own access pattern,
// tools/stream_pieces.py) read a 4-byte LUT: entry = m * m alone (m = |x| >> 2, 26 bits).  A wave-wide ds_read_b32 moves 256 B
// through the 128 B/clk LDS port in 2 clocks where the ds_read_b64 of the 8-byte table takes 4, the lookup result needs one
// register instead of two, and NO per-sample masking is left: the row is the raw code byte (256 rows x 256 B, the v_perm address
// trick again; the sign bit just selects a duplicate), inside a row 32 replicas of the mu-law entry then 32 of the A-law entry,
// so the law is one bit of the per-piece offset instead of bit 7 of every code byte.  64 KiB for both laws.  The peak comes from
// the SAME value: max(m * m) is the square of max(m), and one float square root per 16-sample piece turns it back (isqrt_m2:
// exact, see there).  (k_meter_chunk64 IS bound by HBM: it measured 0.2278 ms with either table and keeps the 8-byte one, which
// the PCM variants need anyway.)
constexpr int kLut32Words = 256 * 64;
__device__ __forceinline__ void fill_lut32(uint32_t *lut)
{
    for (uint32_t i = threadIdx.x; i < (uint32_t)kLut32Words; i += blockDim.x) {
        const uint32_t e = ((i & 32u) << 2) | ((i >> 6) & 0x7Fu);   // law << 7 | code7
        const uint32_t m = ((e & 0x80u) ? alaw_abs(e) : ulaw_abs(e)) >> 2;
        lut[i] = m * m;
    }
}

__device__ __forceinline__ uint32_t lut32_at(const uint32_t *lut, uint32_t w, uint32_t off, uint32_t sel)
{
    // byte address = off | (byte_k(w) << 8), off = replica * 4 | law << 7; w holds raw code bytes
    const uint32_t addr = __builtin_amdgcn_perm(w, off, sel);
    return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(lut) + addr);
}

// m from m * m (m <= 8064): (float)v is off by <= 2^-24 relative, v_sqrt_f32 by 1 ulp, so the root is within 0.002 of the
// integer m and rounding to nearest returns it exactly (every G.711 magnitude of both laws is checked through the record's peak
// in tests/test_gpu_parity.py).
__device__ __forceinline__ uint32_t isqrt_m2(uint32_t v)
{
    return (uint32_t)(__builtin_amdgcn_sqrtf((float)v) + 0.5f);
}

// two magnitudes -> one dword of signed int16 PCM (codes k and k + 1 of word w; a code is negative iff its bit 7 is
// clear).  Packed 16-bit math: one v_perm puts the two inverted sign bits at bits 15 / 31, a packed arithmetic shift
// turns them into 0x0000 / 0xFFFF masks m, and (p ^ m) - m negates the selected halves: 5 VALU per PAIR.
__device__ __forceinline__ uint32_t pack_pcm(uint32_t w, uint32_t k, uint32_t ax0, uint32_t ax1)
{
    const uint32_t sb = __builtin_amdgcn_perm(~w, 0u, k == 0u ? 0x050C040Cu : 0x070C060Cu);
    const v2i16 m = __builtin_bit_cast(v2i16, sb) >> (v2i16)(15);
    const uint32_t p = ax0 | (ax1 << 16);
    const v2i16 r = __builtin_bit_cast(v2i16, p ^ __builtin_bit_cast(uint32_t, m)) - m;
    return __builtin_bit_cast(uint32_t, r);
}

__device__ __forceinline__ void wave_lds_fence()
{
    // same-wave LDS hand-off (lane A writes, lane B reads): the LDS pipe is in
    // order per wave; this only stops the compiler from moving accesses across.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The pitch search of igdsp_pitch.h, wave-wide: yb[k] = z[k] ^ 0x8000 (the window, biased for the unsigned SAD) and ys[k] = yb[k + 1]
// (odd lags read dword pairs from there), both 4-byte aligned in LDS and fenced by the caller.  AMDF over lags 40 .. 120: lag 40 + lane,
// and 104 + lane for the first 17 lanes; the key is min-reduced over the wave.  Every lane of the wave active; every lane gets p.
__device__ __forceinline__ uint32_t pitch_search_wave(const uint16_t *yb, const uint16_t *ys, uint32_t lane)
{
    constexpr uint32_t kH = IGDSP_PLC_HIST;
    uint32_t best = 0;                     // max of ~key = ~min of key
    for (uint32_t li = lane; li <= (uint32_t)(IGDSP_PLC_PMAX - IGDSP_PLC_PMIN); li += 64u) {
        const uint32_t p = IGDSP_PLC_PMIN + li, base = kH - IGDSP_PLC_SPAN - p;   // 120 - p
        const uint32_t *ref = reinterpret_cast<const uint32_t *>(yb + (kH - IGDSP_PLC_SPAN));
        const uint32_t *lag = (base & 1u) ? reinterpret_cast<const uint32_t *>(ys + base - 1u) : reinterpret_cast<const uint32_t *>(yb + base);
        uint32_t d = 0;
#pragma unroll 8
        for (uint32_t i = 0; i < IGDSP_PLC_SPAN / 2u; ++i) d = __builtin_amdgcn_sad_u16(ref[i], lag[i], d);
        best = max(best, ~pitch_key(d, p));
    }
    return (~wave_reduce_dpp(best, OpMax{})) & 127u;
}

// Silence-probe helper.  Bytes 28 / 38 / 48 of a frame sit in its pieces 1 / 2 / 3
// (byte 12 of piece 1, byte 6 of piece 2, byte 0 of piece 3).  Two constant-selector
// v_perm_b32 gather {d.w.b0, d.x.b0, d.y.b2} into one word; a per-lane mask keeps
// the byte this piece is responsible for.  Returns bit 31 set when the probe fails.
__device__ __forceinline__ uint32_t probe_fail(const uint4 d, const uint32_t pmask)
{
    const uint32_t y = __builtin_amdgcn_perm(d.w, d.x, 0x0C0C0004u);      // b0 = d.w.b0 (byte 28), b1 = d.x.b0 (byte 48)
    const uint32_t x = __builtin_amdgcn_perm(d.y, y, 0x0C060100u);        // b2 = d.y.b2 (byte 38)
    return min((x ^ 0x00D5D5D5u) & pmask, 1u) << 31;
}

__device__ __forceinline__ uint32_t probe_mask(uint32_t q)   // q = piece index within the frame
{
    return (q == 1u ? 0x000000FFu : 0u) | (q == 3u ? 0x0000FF00u : 0u) | (q == 2u ? 0x00FF0000u : 0u);
}

__device__ __forceinline__ uint64_t now_cycles() { return __builtin_readcyclecounter(); }

// Frame record for the tuned n == 160 path.  sumsq = 16 * s with s < 2^34; rms = sqrt(s / 10):
// two u32->f32 converts + one fma, one multiply, one v_sqrt_f32 (1 ulp) — total relative error
// < 4e-7 against the float64 definition, inside the 1e-5 contract; every integer field is exact.
__device__ __forceinline__ uint4 pack_stats160(uint64_t s, uint32_t peak, uint32_t bsum, bool alaw, bool probe,
                                               uint32_t &byte_mean, uint32_t &flags)
{
    byte_mean = bsum / 160u;
    flags = (peak <= 8u ? IGDSP_FLAG_SILENT : 0u) | (probe ? IGDSP_FLAG_PROBE_D5 : 0u) |
            (peak == full_scale(alaw) ? IGDSP_FLAG_CLIPPED : 0u);
    const float fs = fmaf((float)(uint32_t)(s >> 32), 4294967296.0f, (float)(uint32_t)s);
    const float rms = __builtin_amdgcn_sqrtf(fs * 0.1f);
    const uint64_t sumsq = s << 4;
    return make_uint4((uint32_t)sumsq, (uint32_t)(sumsq >> 32), __float_as_uint(rms), peak | (byte_mean << 16) | (flags << 24));
}

constexpr int kStripEntries = kSuperFrames * kPiecesPerFrame;  // 640 x 8 B = 5 KiB per wave

// Per-lane piece constants of a 32-frame half of 160-byte frames (five 16-byte pieces per lane), packed: five 5-bit frame
// indices (frame-in-half of piece j) in `fr5`, five 5-bit probe shifts in `pm5` (the probe byte a piece is responsible for
// sits at that bit of probe_fail's gathered word; 24 = none, that byte of the word is always zero).  Two registers instead
// of ten; one v_bfe_u32 (+ one shift) per piece to unpack.  Used by k_roundtrip_lut64 and k_roundtrip_blk64.
__device__ __forceinline__ void pack_piece_consts(uint32_t lane, uint32_t &fr5, uint32_t &pm5)
{
    fr5 = 0; pm5 = 0;
#pragma unroll
    for (int j = 0; j < kLoadsPerChunk; ++j) {
        const uint32_t p = (uint32_t)j * 64u + lane, f = p / 10u, q = p - f * 10u;
        const uint32_t sh = q == 1u ? 0u : (q == 3u ? 8u : (q == 2u ? 16u : 24u));
        fr5 |= f << (5 * j);
        pm5 |= sh << (5 * j);
    }
}

// Order in which batches of work items are visited: the two halves of the item range alternately, so that at any
// moment the launch reads and WRITES in two distant places of every buffer.  Write streams spread over two classes of
// device memory run 11-22 % faster on MI355X than the same stream into one class (tools/stream_calib2.py, DESIGN.md
// 7); a caller gets that by letting a bulk output buffer straddle a class boundary.  A bijection on [0, nb); ids >=
// nb (queue exhausted) are returned unchanged.
#ifndef IGDSP_SPREAD_METER
#define IGDSP_SPREAD_METER 0
#endif
__device__ __forceinline__ uint32_t spread_batch(uint32_t b, uint32_t nb)
{
#ifdef IGDSP_NO_SPREAD          // A/B builds only: ascending order everywhere
    return b;
#endif
    const uint32_t half = (nb + 1u) >> 1;
    return b >= nb ? b : ((b & 1u) ? half + (b >> 1) : (b >> 1));
}

// Work queue of a persistent block (the mechanism k_meter_chunk64 carries inline): a batch = W consecutive items; the
// block's first batch is its blockIdx, later ones come from one device-wide counter (gq[0]; nullptr = static
// blockIdx + j * G); the waves draw slots from an LDS counter and the wave that draws the first slot of local batch j
// announces batch j + 1, so nobody waits on the device atomic.  gq[1] counts finished blocks; the last one re-arms.
template <int W>
struct BlockQueue { uint32_t next, batch[8], tag[8]; };

template <int W>
__device__ __forceinline__ void bq_init(BlockQueue<W> &q, uint32_t *gq, uint32_t G, uint32_t gb1)   // thread 0, before a barrier;
{                                                                 // gb1 = atomicAdd(gq, 1u) issued earlier (its latency hides under the LUT fill)
    q.next = (uint32_t)W;
    for (int i = 0; i < 8; ++i) q.tag[i] = 0xFFFFFFFFu;
    q.batch[0] = blockIdx.x; q.tag[0] = 0u;
    q.batch[1] = gq ? gb1 + G : blockIdx.x + G; q.tag[1] = 1u;
}

template <int W>
__device__ __forceinline__ uint32_t bq_grab(BlockQueue<W> &q, uint32_t *gq, uint32_t G, uint32_t lane, uint32_t nb)   // wave-uniform item id; nb = number of batches
{
    uint32_t v = 0;
    if (lane == 0) {
        const uint32_t s = atomicAdd(&q.next, 1u);
        const uint32_t j = s / (uint32_t)W, w = s - j * (uint32_t)W;
        if (w == 0u) {
            const uint32_t nb = gq ? atomicAdd(gq, 1u) + G : blockIdx.x + (j + 1u) * G;
            __hip_atomic_store(&q.batch[(j + 1u) & 7u], nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_store(&q.tag[(j + 1u) & 7u], j + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        while (__hip_atomic_load(&q.tag[j & 7u], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != j)
            __builtin_amdgcn_s_sleep(2);                         // published by a wave of this block that never waits on us
        v = spread_batch(__hip_atomic_load(&q.batch[j & 7u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), nb) * (uint32_t)W + w;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

__device__ __forceinline__ void bq_finish(uint32_t *gq, uint32_t G)                     // all threads, end of the kernel
{
    if (gq == nullptr) return;
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(gq + 1, 1u) == G - 1u) { gq[0] = 0u; gq[1] = 0u; }
}

// The block-owned form (k_roundtrip_blk64, k_roundtrip_strided<BLK>; k_meter_rtp64<WIN == 2>): block b owns the gpb = 1 << gsh
// consecutive channel groups of 64 from b * gpb (at most kBlkCh channels: groups_per_block, igdsp_route.h) for the whole launch and
// hands their F * gpb items — one frame of one group — to its waves one at a time.
template <typename T> __device__ __forceinline__ void lds_add(T *p, T v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_max(uint32_t *p, uint32_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_min(uint32_t *p, uint32_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ uint32_t wave_draw(uint32_t *counter, uint32_t lane)      // the next number of an LDS counter, wave-uniform
{
    uint32_t v = 0;
    if (lane == 0) v = atomicAdd(counter, 1u);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// The hold windows of the channels a block owns, in LDS: 7 dwords per channel, channel cl = (group within the block) * 64 + lane.
// Every wave adds the frames it folds by workgroup-scope relaxed integer atomics (add / max / min: exact in any order); when all
// items are through (a barrier), the wave that holds hold[c] of a group folds the group's windows into it — the block owns the
// channel for the launch: plain read-modify-write.  The round trips fold every frame of the launch (add / fold).  The packet kernel
// folds the frames its gate lets through and counts them and their samples in the two count planes (add_packet / fold_packets):
// 8-bit frame, silent and clipped counts, 16-bit byte-mean sum and samples — at most 255 frames per launch (the launcher splits).
template <bool ON = true>
struct BlkHoldWindowT {
    uint64_t sumsq[kBlkCh];                 // sum of squares << 4.  First member: the 64-bit LDS atomic needs the 8-byte alignment of its type
    uint32_t level_sum[kBlkCh];             // byte-mean sum (packets: | samples << 16)
    uint32_t peak[kBlkCh], level_max[kBlkCh], level_min[kBlkCh];
    uint32_t counts[kBlkCh];                // silent | clipped << 16 (packets: frames | silent << 8 | clipped << 16)

    __device__ __forceinline__ void init(uint32_t tid, uint32_t nthreads)       // all threads, before a barrier
    {   // (two loops: as one, k_roundtrip_strided<5, false, *, BLK> takes two more SGPRs)
        for (uint32_t i = tid; i < (uint32_t)kBlkCh; i += nthreads) { sumsq[i] = 0; level_sum[i] = 0u; counts[i] = 0u; }           // the sums
        for (uint32_t i = tid; i < (uint32_t)kBlkCh; i += nthreads) { peak[i] = 0u; level_max[i] = 0u; level_min[i] = 255u; }       // the extremes
    }
    __device__ __forceinline__ void add(uint32_t cl, uint64_t sumsq16, uint32_t pk, uint32_t bm, uint32_t fl)
    {
        lds_add(&sumsq[cl], sumsq16); lds_add(&level_sum[cl], bm);
        lds_max(&peak[cl], pk); lds_max(&level_max[cl], bm); lds_min(&level_min[cl], bm);
        const uint32_t sc = ((fl & IGDSP_FLAG_SILENT) ? 1u : 0u) + ((fl & IGDSP_FLAG_CLIPPED) ? 0x10000u : 0u);
        if (sc != 0u) lds_add(&counts[cl], sc);
    }
    __device__ __forceinline__ void add_packet(uint32_t cl, uint64_t sumsq16, uint32_t pk, uint32_t bm, uint32_t fl, uint32_t samples)
    {
        lds_add(&sumsq[cl], sumsq16);
        lds_add(&counts[cl], 1u | ((fl & IGDSP_FLAG_SILENT) ? 0x100u : 0u) | ((fl & IGDSP_FLAG_CLIPPED) ? 0x10000u : 0u));
        lds_add(&level_sum[cl], bm | (samples << 16));
        lds_max(&peak[cl], pk); lds_max(&level_max[cl], bm); lds_min(&level_min[cl], bm);
    }
    __device__ __forceinline__ void fold(uint32_t t, uint32_t frames, uint32_t samples, igdsp_chan_hold &g) const
    {
        fold_levels(t, g);
        g.count += frames; g.level_sum += level_sum[t]; g.samples += samples;
        g.n_silent += counts[t] & 0xFFFFu; g.n_clipped += counts[t] >> 16;
    }
    __device__ __forceinline__ bool fold_packets(uint32_t t, igdsp_chan_hold &g) const      // false (g untouched): no frame was folded
    {
        const uint32_t wa = counts[t], wb = level_sum[t];
        if ((wa & 0xFFu) == 0u) return false;
        fold_levels(t, g);
        g.count += wa & 0xFFu; g.level_sum += wb & 0xFFFFu; g.samples += wb >> 16;
        g.n_silent += (wa >> 8) & 0xFFu; g.n_clipped += (wa >> 16) & 0xFFu;
        return true;
    }
    __device__ __forceinline__ void fold_levels(uint32_t t, igdsp_chan_hold &g) const
    {
        g.sumsq_acc += sumsq[t];
        g.peak_hold = (uint16_t)max((uint32_t)g.peak_hold, peak[t]);
        g.level_max = (uint8_t)max((uint32_t)g.level_max, level_max[t]);
        g.level_min = (uint8_t)min((uint32_t)g.level_min, level_min[t]);
    }
};
template <> struct BlkHoldWindowT<false> {}; // a kernel template's instantiations without the block-owned form reserve no LDS for it
using BlkHoldWindow = BlkHoldWindowT<true>;
static_assert(sizeof(BlkHoldWindow) == 7 * 4 * kBlkCh && alignof(BlkHoldWindow) == 8, "7 dwords of LDS per channel, the 64-bit plane aligned");

// The item queue of the block-owned round trips.  Item id of the block (ids come in (frame, group) order from an LDS counter) is a
// frame of group b_first + (id & (gpb - 1)): frame id >> gsh, or, in the odd blocks of a launch whose output is spread over two
// memory classes (mid_start), that frame counted from the middle of the launch — at any moment half the chip then writes the first
// half of the output and half the second.  A global load at the block's end waits ~5 us behind the other blocks' streams, so the
// first gpb waves to start their last item (or to find they have none) fetch hold[c] of one group each, a whole item ahead, and fold it.
struct BlkQueueLds { uint32_t next, ticket; };       // in LDS, zero before the first grab: items handed out, waves that have started their last item
constexpr uint32_t kNoItem = 0xFFFFFFFFu;

struct BlkItemQueue {
    BlkQueueLds &q;
    const uint32_t lane, gpb, gsh, F, b_first, b_items, f_shift;       // (all but lane wave-uniform)
    igdsp_chan_hold e_hold = igdsp_chan_hold{};                        // hold[c] of group b_first + e_ticket, if its gate is open
    uint32_t e_ticket = kNoItem;                                       // (kNoItem: not drawn yet)
    bool e_open = false;
    __device__ __forceinline__ BlkItemQueue(BlkQueueLds &q_, uint32_t lane_, uint32_t gpb_, uint32_t gsh_, uint32_t F_, bool mid_start)
        : q(q_), lane(lane_), gpb(gpb_), gsh(gsh_), F(F_), b_first(blockIdx.x * gpb_), b_items(F_ * gpb_), f_shift((mid_start && (blockIdx.x & 1u)) ? F_ / 2u : 0u) {}
    __device__ __forceinline__ uint32_t grab() { const uint32_t v = wave_draw(&q.next, lane); return v < b_items ? v : kNoItem; }   // block-local item number
    __device__ __forceinline__ uint32_t frame_of(uint32_t id) const { const uint32_t f = (id >> gsh) + f_shift; return f >= F ? f - F : f; }
    __device__ __forceinline__ uint32_t group_of(uint32_t id) const { return b_first + (id & (gpb - 1u)); }
    __device__ __forceinline__ uint32_t chan_of(uint32_t id) const { return (id & (gpb - 1u)) * (uint32_t)kSuperFrames + lane; }   // this lane's channel within the block
    __device__ __forceinline__ void end_prefetch(const igdsp_chan_hold *hold, const uint8_t *gate)     // when the wave starts its last item
    {
        e_ticket = wave_draw(&q.ticket, lane);
        if (e_ticket < gpb) {
            const uint32_t c = (b_first + e_ticket) * (uint32_t)kSuperFrames + lane;
            e_open = gate == nullptr || gate[c] != 0;
            if (e_open) e_hold = hold[c];
        }
    }
    __device__ __forceinline__ void finish(const BlkHoldWindow &w, uint32_t n, igdsp_chan_hold *hold, const uint8_t *gate)
    {   // every wave of the block, after its last item: the windows of F frames of n samples each go into hold[c]
        if (e_ticket == kNoItem) end_prefetch(hold, gate);                     // a wave that never had an item
        __syncthreads();
        if (e_ticket < gpb && e_open) {
            const uint32_t t = e_ticket * (uint32_t)kSuperFrames + lane;
            w.fold(t, F, F * n, e_hold);
            hold[b_first * (uint32_t)kSuperFrames + t] = e_hold;
        }
    }
};

// ============================================================================
// a2 — G.711 compression.  ONE branch-free formulation serves both laws and both encoder lineages
// (include/igdsp.h): per-law constants select bias / rounding, the segment comes from count-leading-
// zeros.  With msb = 31 - clz(mag):
//   SUN16  mu : mag = min(|v| + 0x84, 0x7FFF)                 A : mag = v >= 0 ? v : max(-v - 8, 0)
//          seg = max(msb,7) - 7        step = (mag >> (max(msb, mu?7:8) - 4)) & 15
//   G191   mu : mag = min(|v>>2| + 0x21, 0x1FFF)              A : mag = (v>>3) ^ sign   (= -x-1 for x < 0)
//          seg = max(msb, mu?5:4) - (mu?5:4)   step = (mag >> (max(msb,5) - 4)) & 15
//   code = (seg<<4 | step) ^ (mu ? 0xFF : 0xD5) ^ (v < 0 ? 0x80 : 0)
// (clamping mag is identical to the classic "segment 8 -> 0x7F ^ mask" overflow rule).
// ============================================================================
struct EncK { int k_and, k_add, sh; uint32_t c_shift, c_seg, base; };

template <int VARIANT>
__device__ __forceinline__ EncK enc_consts(bool alaw)
{
    EncK k;
    if (VARIANT == IGDSP_ENC_SUN16) {
        k.k_and = alaw ? -8 : 0; k.k_add = alaw ? 0 : 0x84; k.sh = 0;
        k.c_shift = alaw ? 23u : 24u;      // 31 - floor(msb) for the step shift
        k.c_seg = 24u;                     // 31 - 7
    } else {
        k.k_and = alaw ? 0 : 1; k.k_add = alaw ? 0 : 0x21; k.sh = alaw ? 3 : 2;
        k.c_shift = 26u;                   // 31 - 5
        k.c_seg = alaw ? 27u : 26u;        // 31 - {4,5}
    }
    k.base = alaw ? 0xD5u : 0xFFu;
    return k;
}

template <int VARIANT>
__device__ __forceinline__ uint32_t enc_uni(int v, const EncK k)
{
    int mag;
    const int sign = v >> 31;                                   // -1 for negative samples
    if (VARIANT == IGDSP_ENC_SUN16) {
        const int av = (v ^ sign) - sign;                       // |v|, 32768 for -32768
        mag = min(max(av + ((sign & k.k_and) + k.k_add), 0), 0x7FFF);
    } else {
        const int vd = v >> k.sh;                               // arithmetic: floors negatives
        const int t = vd ^ sign;                                // x >= 0 ? x : -x - 1
        mag = min(t + (sign & k.k_and) + k.k_add, 0x1FFF);      // mu: |x| + 0x21 ; A: -x - 1
    }
    const uint32_t c = (uint32_t)__clz(mag);                    // 32 for mag == 0
    const uint32_t shift = 27u - min(c, k.c_shift);             // max(msb, floor) - 4
    const uint32_t sg = k.c_seg - min(c, k.c_seg);              // max(msb, f) - f
    const uint32_t step = ((uint32_t)mag >> shift) & 15u;
    return ((sg << 4) | step) ^ k.base ^ ((uint32_t)sign & 0x80u);
}

// ---- ED-137 TX (igdsp_k_tx.hip, igdsp_k_txstage.hip) ----
// Pass boundary inside one wavefront: LDS written by some lanes is read by others after it.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

__device__ __forceinline__ int sbyte_sum(uint32_t d, uint32_t k)   // sum of the first k bytes of d as signed char
{
    int s = 0;
    for (uint32_t i = 0; i < 4u; ++i) s += i < k ? (int)(int8_t)(d >> (8u * i)) : 0;
    return s;
}

// igdsp_tx_chan unpacked into registers (the packed struct kept whole ends up in scratch / LDS): read once, written once per launch
struct TxState {
    uint64_t r2s_send_ms = 0;
    uint32_t ts = 0, ssrc = 0, seq = 0, pt = 0, first_r2s = 0, tx_slave = 0, rx_slave = 0, tx_slave_changed = 0, rx_slave_changed = 0;
    int32_t keepalive_ms = 0, packet_cnt = 0, slave_count = 0, tx_run = 0;
    uint32_t ptt = 0, sql = 0, call_in = 0, call_recorder = 0, pttid = 0, pttpriority = 0, bssi = 0, calltype = 0, level = 0, w11 = 0;
    __device__ __forceinline__ void load(const igdsp_tx_chan *p)
    {
        const uint32_t *u = reinterpret_cast<const uint32_t *>(p);
        r2s_send_ms = *reinterpret_cast<const uint64_t *>(p);
        ts = u[2]; ssrc = u[3]; keepalive_ms = (int32_t)u[4]; packet_cnt = (int32_t)u[5];
        seq = u[6] & 0xFFFFu; pt = (u[6] >> 16) & 0xFFu; first_r2s = u[6] >> 24;
        tx_slave = u[7] & 0xFFu; rx_slave = (u[7] >> 8) & 0xFFu; tx_slave_changed = (u[7] >> 16) & 0xFFu; rx_slave_changed = u[7] >> 24;
        slave_count = (int32_t)u[8];
        ptt = u[9] & 0xFFu; sql = (u[9] >> 8) & 0xFFu; call_in = (u[9] >> 16) & 0xFFu; call_recorder = u[9] >> 24;
        pttid = u[10] & 0xFFu; pttpriority = (u[10] >> 8) & 0xFFu; bssi = (u[10] >> 16) & 0xFFu; calltype = u[10] >> 24;
        tx_run = (int32_t)(int16_t)(u[11] & 0xFFFFu); level = (u[11] >> 16) & 0xFFu; w11 = u[11] & 0xFF000000u;
    }
    __device__ __forceinline__ void store(igdsp_tx_chan *p) const     // reserved bytes 48 .. 63 are left as they are
    {
        uint32_t *u = reinterpret_cast<uint32_t *>(p);
        *reinterpret_cast<uint64_t *>(p) = r2s_send_ms;
        u[2] = ts; u[3] = ssrc; u[4] = (uint32_t)keepalive_ms; u[5] = (uint32_t)packet_cnt;
        u[6] = (seq & 0xFFFFu) | pt << 16 | first_r2s << 24;
        u[7] = tx_slave | rx_slave << 8 | tx_slave_changed << 16 | rx_slave_changed << 24;
        u[8] = (uint32_t)slave_count;
        u[9] = ptt | sql << 8 | call_in << 16 | call_recorder << 24;
        u[10] = pttid | pttpriority << 8 | bssi << 16 | calltype << 24;
        u[11] = ((uint32_t)tx_run & 0xFFFFu) | level << 16 | w11;
    }
};

}  // namespace igdsp
