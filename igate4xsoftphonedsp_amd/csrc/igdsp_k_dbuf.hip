// igdsp_k_dbuf.hip — the sound port's delay buffer (igdsp_dbuf_run): PUT and GET steps of two clocks on a ring per channel, with the
// drift compensation (one pitch period dropped by overlap-add) when the fill grows.  Semantics: include/igdsp.h, section "Delay buffer";
// the rule itself: igdsp_dbuf.h (the host entry igdsp_dbuf_step runs the same functions); independent restatement: tests/dbuf_model.py.
//
// Shape (route: dbuf_route).  A wave owns one channel for the steps of one part (<= kDbufPart); the waves of a block are independent.
// The channel's scalars live in registers, wave-uniform (the six counters in one VGPR, a lane each); the samples stay where the state
// keeps them, in the channel's ring in global memory, so a launch touches the n samples a PUT appends, the n a GET takes and the 280 of
// a shrink and nothing else: a one-step launch does not move the ring.  Per step:
//   PUT    the rule's begin (igdsp_dbuf.h) says whether this PUT shrinks.  A shrink gathers the newest 280 samples into LDS, biased for
//          the unsigned SAD, runs the concealment's search (pitch_search_wave, one lag per lane) and stores the p blended samples over
//          the newest 2 p.  Then the row goes from d_in into the ring behind the live samples.
//   GET    the row goes from the front of the ring to d_out, its sum of squares and peak are folded over the wave into the record; an
//          underrun stores zeros.
// Rows move as dwords where n is even, both buffers are dword aligned (route: vec) and the ring position is even (it is until a shrink
// by an odd period, and again after the next odd one), else a sample at a time.  A ring sample one lane stored is read by another lane
// of the same wave later in the launch: a CU's vector memory path serves one wave's accesses in order through the one L1 the workgroup
// shares, which is what workgroup scope means on this target, and wave_lds_fence's workgroup-scope release / acquire keeps the compiler
// from moving the global accesses across it.  The scalars are written once per part.
// COPY (the compute-free yardstick, tools/dbuf_bench.py): every step is taken as PUT|GET at a fixed fill of n, with no update, search,
// blend or record arithmetic: the rows go through the ring as above, the records carry only the length, the other scalars are stored
// as they were read.
#include "igdsp_device.h"
#include "igdsp_dbuf.h"
#include "igdsp_pcmrec.h"

namespace igdsp {

struct DbufArgs {
    const uint8_t *ops;
    const int16_t *in;
    uint32_t C, n, M, vec;
    uint32_t t0, pt;                       // this part: steps t0 .. t0 + pt - 1
    igdsp_dbuf_state *state;
    int16_t *out;
    uint8_t *flags;
    uint16_t *len_out, *fill;
    igdsp_frame_stats *stats;
};

// one wave's LDS: the shrink's window
struct DbufLds {
    __attribute__((aligned(16))) uint16_t yb[kDbufWin];    // z[k] ^ 0x8000, oldest first
    __attribute__((aligned(16))) uint16_t ys[kDbufWin];    // ys[k] = yb[k + 1]
};
static_assert(sizeof(DbufLds) * kDbufWaves == kDbufLdsBytes, "dbuf_route's LDS");

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the newest 2 p samples of the live region become p: z = y[len - 280 ..) into LDS, the search, the blend back into the ring
__device__ __forceinline__ uint32_t dbuf_shrink_wave(int16_t *ring, DbufLds &L, const DbufSc &s, uint32_t lane)
{
    const uint32_t base = s.len - kDbufWin;
    for (uint32_t k = lane; k < kDbufWin; k += 64u) {
        const uint32_t y = (uint32_t)(uint16_t)ring[dbuf_pos(s, base + k)] ^ 0x8000u;
        L.yb[k] = (uint16_t)y;
        if (k > 0u) L.ys[k - 1u] = (uint16_t)y;
    }
    wave_lds_fence();
    const uint32_t p = pitch_search_wave(L.yb, L.ys, lane);
    for (uint32_t i = lane; i < p; i += 64u) {
        const int32_t z_old = (int16_t)(L.yb[kDbufWin - 2u * p + i] ^ 0x8000u), z_new = (int16_t)(L.yb[kDbufWin - p + i] ^ 0x8000u);
        ring[dbuf_pos(s, s.len - 2u * p + i)] = (int16_t)dbuf_blend(z_old, z_new, i, p);
    }
    wave_lds_fence();
    return p;
}

// n samples from a row into the ring at position pos (the row's dwords where dw)
__device__ __forceinline__ void dbuf_row_in(int16_t *ring, uint32_t pos, const int16_t *row, uint32_t n, bool dw, uint32_t lane)
{
    if (dw) {
        uint32_t *r32 = reinterpret_cast<uint32_t *>(ring);
        const uint32_t *x32 = reinterpret_cast<const uint32_t *>(row);
        for (uint32_t j = lane; j < n / 2u; j += 64u) r32[((pos >> 1) + j) % (kDbufCap / 2u)] = x32[j];
    } else {
        for (uint32_t i = lane; i < n; i += 64u) ring[(pos + i) % kDbufCap] = row[i];
    }
}
// n samples from the ring at position pos into a row; the lane's sum of squares and peak
template <bool COPY>
__device__ __forceinline__ void dbuf_row_out(const int16_t *ring, uint32_t pos, int16_t *row, uint32_t n, bool dw, uint32_t lane, uint64_t &sq, uint32_t &pk)
{
    if (dw) {
        const uint32_t *r32 = reinterpret_cast<const uint32_t *>(ring);
        uint32_t *o32 = reinterpret_cast<uint32_t *>(row);
        v2u16_t pk2 = (v2u16_t)(0);
        for (uint32_t j = lane; j < n / 2u; j += 64u) {
            const uint32_t w = r32[((pos >> 1) + j) % (kDbufCap / 2u)];
            o32[j] = w;
            if (!COPY) pcm_acc2(w, sq, pk2);
        }
        pk = max(pk, max((uint32_t)pk2.x, (uint32_t)pk2.y));
    } else {
        for (uint32_t i = lane; i < n; i += 64u) {
            const int16_t v = ring[(pos + i) % kDbufCap];
            row[i] = v;
            if (!COPY) pcm_acc((uint32_t)(uint16_t)v, sq, pk);
        }
    }
}

template <bool COPY>
__global__ __launch_bounds__(kDbufWaves * 64) void k_dbuf(const DbufArgs a)
{
    __shared__ DbufLds lds[kDbufWaves];
    const uint32_t lane = threadIdx.x & 63u, w = uni(threadIdx.x >> 6);
    const uint64_t cl = (uint64_t)blockIdx.x * kDbufWaves + w;
    if (cl >= a.C) return;                                                 // waves are independent: no block barrier below
    const uint32_t c = (uint32_t)cl, n = a.n, M = a.M;
    DbufLds &L = lds[w];
    igdsp_dbuf_state *st = a.state + c;
    int16_t *ring = st->ring;

    DbufSc s = dbuf_load(*st, M);
    s.head = uni(s.head); s.len = uni(s.len); s.eff = uni(s.eff); s.level = uni(s.level); s.max_level = uni(s.max_level);
    s.since = uni(s.since); s.last_op = uni(s.last_op);
    if (COPY) s.len = n;                                                   // the fixed fill
    // the six telemetry counters ride in one VGPR, lane j holding counter j: the walk adds each step's increments
    uint32_t count = lane < kDbufCounters ? (&st->underruns)[lane] : 0u;
    dbuf_counters_clear(s);

    const uint32_t t_end = a.t0 + a.pt;
    uint32_t op_next = COPY ? 0u : a.ops[a.t0 * a.C + c];                  // a step's op byte is loaded a step ahead: off the walk's chain
    for (uint32_t t = a.t0; t < t_end; ++t) {
        const uint32_t o = t * a.C + c;                                    // < 2^32 - 32: the argument rule
        const uint32_t op = COPY ? (uint32_t)(IGDSP_DBUF_PUT | IGDSP_DBUF_GET) : uni(op_next) & 3u;
        if (!COPY && t + 1u < t_end) op_next = a.ops[o + a.C];
        const bool row_dw = a.vec != 0u;
        if (op & IGDSP_DBUF_PUT) {
            uint32_t k;
            if (COPY) {
                k = s.len;
                s.len += n;
            } else {
                if (dbuf_put_begin(s, n, M)) dbuf_shrunk(s, uni(dbuf_shrink_wave(ring, L, s, lane)));
                k = dbuf_put_end(s, n, M);
            }
            const uint32_t pos = dbuf_pos(s, k);
            dbuf_row_in(ring, pos, a.in + (uint64_t)o * n, n, row_dw && !(pos & 1u), lane);
            wave_lds_fence();                                              // the ring's new samples, for every lane
        }
        uint32_t flag = IGDSP_JB_IDLE;
        uint4 rec = pcm_record_empty();
        if (op & IGDSP_DBUF_GET) {
            const bool played = COPY ? true : dbuf_get_begin(s, n, M);
            int16_t *row = a.out + (uint64_t)o * n;
            uint64_t sq = 0;
            uint32_t pk = 0;
            if (played) {
                dbuf_row_out<COPY>(ring, s.head, row, n, row_dw && !(s.head & 1u), lane, sq, pk);
            } else if (row_dw) {
                for (uint32_t j = lane; j < n / 2u; j += 64u) reinterpret_cast<uint32_t *>(row)[j] = 0u;
            } else {
                for (uint32_t i = lane; i < n; i += 64u) row[i] = 0;
            }
            if (COPY) {
                s.head = (s.head + n) % kDbufCap;
                s.len -= n;
                flag = IGDSP_JB_PLAYED;
                rec = pcm_record(0u, 0u, n, 0u);
            } else {
                flag = dbuf_get_end(s, n, played);
                if (a.stats) {
                    const uint64_t sumsq = wave_sum_u64(sq);
                    pk = wave_reduce_dpp(pk, OpMax{});
                    rec = pcm_record(sumsq, pk, n, 0u);
                }
            }
            wave_lds_fence();                                              // the row is read before a later PUT may reuse its ring samples
        }
        if (lane == 0u) {
            if (a.flags) a.flags[o] = (uint8_t)flag;
            if (a.len_out) a.len_out[o] = (op & IGDSP_DBUF_GET) ? (uint16_t)n : (uint16_t)0;
            if (a.fill) a.fill[o] = (uint16_t)s.len;
            if (a.stats) a.stats[o] = as_stats(rec);
        }
        if (!COPY) {
            count += dbuf_counter(s, lane);
            dbuf_counters_clear(s);
        }
    }
    if (lane == 0u) dbuf_store_live(*st, s);
    if (lane < kDbufCounters) (&st->underruns)[lane] = count;
}

hipError_t launch_dbuf_run(const LaunchCfg &, const uint8_t *ops, const int16_t *in, uint32_t C, uint32_t T, uint32_t n, uint32_t M,
                           igdsp_dbuf_state *state, int16_t *out, uint8_t *flags, uint16_t *len_out, uint16_t *fill, igdsp_frame_stats *stats,
                           bool yardstick, hipStream_t s)
{
    const DbufRoute r = dbuf_route(C, T, n, M, reinterpret_cast<uintptr_t>(in), reinterpret_cast<uintptr_t>(out));
    if (r.grid == 0) return hipSuccess;
    DbufArgs a{ops, in, C, n, M, r.vec, 0u, 0u, state, out, flags, len_out, fill, stats};
    const auto kernel = yardstick ? k_dbuf<true> : k_dbuf<false>;
    for (uint32_t p = 0; p < r.parts; ++p) {
        a.t0 = p * kDbufPart;
        a.pt = std::min(kDbufPart, T - a.t0);
        hipLaunchKernelGGL(kernel, dim3(r.grid), dim3(r.threads), 0, s, a);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace igdsp
