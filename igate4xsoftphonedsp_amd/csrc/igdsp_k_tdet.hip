// igdsp_k_tdet.hip — the tone detector (igdsp_tone_detect): per channel and frame two evaluations of n samples against the plan's
// reference table, the hit decision and the debounce.  Semantics: include/igdsp.h, section "Tone detector"; the rule's arithmetic:
// igdsp_tdet.h (igdsp_tdet_frame runs the same functions on the host); independent restatement: tests/tdet_model.py.
//
// Shape (route: tdet_route).  A DPP row of 16 lanes owns one channel for the launch's frames: lanes 0..7 hold the low group's bins,
// lanes 8..15 the high group's; a wave is four channels, a block kTdetChans.  LDS: one plan's table, tab[j2][lane] = the cosine and the
// sine values of sample pairs 2 j2 and 2 j2 + 1 (window indices 4 j2 .. 4 j2 + 3) as four dwords of two int16 (zeros for a lane
// without a bin and for a pair past the window), built by the block from the generator's sine list; per channel buf = 128 values of
// history and the frame's n values v = x >> 3 behind them.  The block walks the distinct plans of its channels: build the table, every
// channel of that plan runs its frames, next plan.
// Per frame: the row (loaded a frame ahead, two samples per lane and load) is decoded, shifted and stored behind the history.  Both
// evaluations run in one loop over j2: one 16-byte table entry, 8 bytes of each window's samples (a broadcast within the row), eight
// v_dot2_i32_i16: the entry serves both windows, and the LDS array and the VALU are then level (16-byte and 8-byte reads move 256 B
// per clock).  A plan of at most 4 + 4 bins would leave half the lanes idle: there lane k + 4 takes the second half of lane k's window
// and one row_shl:4 adds the halves.  E: the lane squares the pairs j = k, k + 16, .. and the row adds the sums (row_ror).  The decision:
// a three-step butterfly over the eight lanes of a group gives the group's largest P; ballots give its lowest index and whether another
// bin fails the rel test; row_ror:8 hands each half the other group's result, and tdet_decide runs in every lane.  The debounce
// fields live in registers (every lane of a row holds the same values); lane 0 of the row stores the record.  Then the history moves
// up by n.  E0 (0, 1, 2): n % 8 == 0, n % 4 == 0, else: how evaluation 0's window, which starts n / 2 values before the frame, can be read.
// COPY (the compute-free yardstick, tools/tdet_bench.py): the same row loads, buffer stores, history move, records and state stores;
// no table, no pair reads, no dot product, decision or debounce.
// The list (launch_tone_detect, launch_event_list): k_tdet_list is event_list_pass over the records whose flags meet the mask.
// The row's DPP steps and sums, the packed dot product and the G.711 pair are igdsp_lanes.h's.  Everything is written with vector stores.
#include "igdsp_lanes.h"
#include "igdsp_tdet.h"

namespace igdsp {

__device__ const int16_t d_tdet_sin[1024] = {IGDSP_TONE_SIN_VALUES};

struct TdetArgs {
    const uint8_t *g711, *codec;
    const int16_t *pcm;
    const igdsp_tdet_plan *plans;
    const uint16_t *plan_of;
    uint32_t n_plans, C, F, n;
    igdsp_tdet_state *state;
    igdsp_tdet_rec *rec;
};

struct TdetLds {
    __attribute__((aligned(16))) uint4 tab[64 * 16];                      // [pair of sample pairs][lane]
    __attribute__((aligned(16))) int16_t buf[kTdetChans][kTdetBuf];
    uint32_t plan[kTdetChans];                                             // 0xFFFFFFFF: no channel, or a plan index out of range
};
static_assert(sizeof(TdetLds) == kTdetLdsBytes, "tdet_route's LDS");

constexpr uint32_t kTdetNone = 0xFFFFFFFFu;

// the maximum over the eight lanes of a group, in each of them: xor 1, xor 2 (quad_perm), then the other quad (row_half_mirror)
__device__ __forceinline__ uint64_t tdet_max8(uint64_t v)
{
    v = max(v, dpp64<0xB1>(v));
    v = max(v, dpp64<0x4E>(v));
    return max(v, dpp64<0x141>(v));
}
// two samples as they lie in memory (two codes, or two PCM samples) -> the two values v = x >> 3, the shift on the SIGNED sample
__device__ __forceinline__ uint32_t tdet_unit(uint32_t u, bool g711, bool alaw)
{
    int32_t x0, x1;
    if (g711) {
        const G711Two x = g711_two(u, alaw);
        x0 = x.x0;
        x1 = x.x1;
    } else {
        x0 = (int16_t)(u & 0xFFFFu);
        x1 = (int16_t)(u >> 16);
    }
    return pack2(x0 >> 3, x1 >> 3);
}
__device__ __forceinline__ void tdet_row_load(const TdetArgs &a, uint32_t o, uint32_t k, uint32_t (&u)[8])
{
    const uint32_t h = a.n >> 1;
#pragma unroll
    for (uint32_t q = 0; q < 8u; ++q) {
        const uint32_t m = k + 16u * q;
        u[q] = 0u;
        if (m < h) u[q] = a.g711 ? (uint32_t)reinterpret_cast<const uint16_t *>(a.g711 + (uint64_t)o * a.n)[m]      // d_g711 2-byte, d_pcm 4-byte aligned, n even: the argument rule
                                 : reinterpret_cast<const uint32_t *>(a.pcm + (uint64_t)o * a.n)[m];
    }
}

// sample pairs 2 j2 and 2 j2 + 1 of evaluation 0's window (it starts at value 128 - h of buf).  E0 = 0: h % 4 == 0, one 8-byte read;
// 1: h even, two dwords; 2: h odd, the window starts at an odd value and the pairs are read as halves
template <int E0>
__device__ __forceinline__ uint2 tdet_pairs0(const int16_t *buf, uint32_t h, uint32_t j2)
{
    const int16_t *p = buf + (IGDSP_TDET_HIST - h) + 4u * j2;
    if constexpr (E0 == 0) return *reinterpret_cast<const uint2 *>(p);
    if constexpr (E0 == 1) return make_uint2(reinterpret_cast<const uint32_t *>(p)[0], reinterpret_cast<const uint32_t *>(p)[1]);
    return make_uint2((uint32_t)(uint16_t)p[0] | (uint32_t)(uint16_t)p[1] << 16, (uint32_t)(uint16_t)p[2] | (uint32_t)(uint16_t)p[3] << 16);
}
template <int E0>
__device__ __forceinline__ uint32_t tdet_pair0(const int16_t *buf, uint32_t h, uint32_t j)
{
    const int16_t *p = buf + (IGDSP_TDET_HIST - h) + 2u * j;
    if constexpr (E0 != 2) return *reinterpret_cast<const uint32_t *>(p);
    return (uint32_t)(uint16_t)p[0] | (uint32_t)(uint16_t)p[1] << 16;
}

// both evaluations' sums of a frame: I and Q of the lane's bin (split: the half of the window the lane takes), E of the row
struct TdetSums { uint32_t I0, Q0, I1, Q1; uint64_t E0, E1; };
template <int E0>
__device__ __forceinline__ TdetSums tdet_sums(const TdetLds &L, const int16_t *buf, uint32_t h, uint32_t k, uint32_t kb, uint32_t jb, uint32_t je, bool split)
{
    TdetSums r{0u, 0u, 0u, 0u, 0u, 0u};
    const uint4 *tab = L.tab + kb;
    const int16_t *frame = buf + IGDSP_TDET_HIST;
#pragma unroll 1
    for (uint32_t j2 = jb; j2 < je; ++j2) {                                // one table entry serves four sums of two pairs each
        const uint4 t = tab[16u * j2];
        const uint2 s1 = *reinterpret_cast<const uint2 *>(frame + 4u * j2);
        const uint2 s0 = tdet_pairs0<E0>(buf, h, j2);
        r.I0 = dot2(s0.x, t.x, r.I0); r.Q0 = dot2(s0.x, t.y, r.Q0);
        r.I1 = dot2(s1.x, t.x, r.I1); r.Q1 = dot2(s1.x, t.y, r.Q1);
        r.I0 = dot2(s0.y, t.z, r.I0); r.Q0 = dot2(s0.y, t.w, r.Q0);
        r.I1 = dot2(s1.y, t.z, r.I1); r.Q1 = dot2(s1.y, t.w, r.Q1);
    }
    if (split) {                                                           // plan-uniform: lane k + 4 took the other half of lane k's window
        r.I0 += dpp<0x104>(r.I0); r.Q0 += dpp<0x104>(r.Q0);
        r.I1 += dpp<0x104>(r.I1); r.Q1 += dpp<0x104>(r.Q1);
    }
    uint64_t e0 = 0, e1 = 0;
    for (uint32_t j = k; j < h; j += 16u) {
        const uint32_t a0 = tdet_pair0<E0>(buf, h, j), a1 = *reinterpret_cast<const uint32_t *>(frame + 2u * j);
        e0 += dot2(a0, a0, 0u);
        e1 += dot2(a1, a1, 0u);
    }
    r.E0 = row16_sum64(e0);
    r.E1 = row16_sum64(e1);
    return r;
}

// the row's hit code from the lanes' sums, in every lane of the row
__device__ __forceinline__ uint32_t tdet_hit_dev(uint32_t I, uint32_t Q, uint64_t E, uint32_t n, uint32_t lane, bool valid, const igdsp_tdet_thr &thr,
                                                 uint32_t nhi, uint64_t floor)
{
    const uint32_t k = lane & 15u;
    const int64_t Is = (int32_t)I, Qs = (int32_t)Q;
    const uint64_t P = valid ? (uint64_t)(Is * Is) + (uint64_t)(Qs * Qs) : 0u;
    const uint64_t M = tdet_max8(P);
    const uint32_t sh = lane & 56u;
    const uint32_t tops = (uint32_t)(__builtin_amdgcn_ballot_w64(valid && P == M) >> sh) & 0xFFu;
    const uint32_t ci = tops ? (uint32_t)__builtin_ctz(tops) : 0u;
    const uint32_t bad = (uint32_t)(__builtin_amdgcn_ballot_w64(valid && (k & 7u) != ci && tdet_rel_fails(M, P, thr.rel_q8)) >> sh) & 0xFFu;
    const uint32_t ok = (tops != 0u && bad == 0u && M >= floor) ? 1u : 0u;
    const uint64_t Mo = dpp64<0x128>(M);
    const uint32_t cio = dpp<0x128>(ci), oko = dpp<0x128>(ok);
    const bool hi = (k & 8u) != 0u;
    return tdet_decide(thr, nhi, (hi ? oko : ok) != 0u, hi ? cio : ci, hi ? Mo : M, (hi ? ok : oko) != 0u, hi ? ci : cio, hi ? M : Mo, tdet_eref(E, n));
}

template <bool COPY, int E0>
__global__ __launch_bounds__(kTdetWaves * 64, kTdetWaves * kTdetResident / 4) void k_tdet(const TdetArgs a)
{
    __shared__ TdetLds L;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, k = lane & 15u, slot = tid >> 4, n = a.n, h = n >> 1;
    const uint64_t c64 = (uint64_t)blockIdx.x * kTdetChans + slot;
    const bool chan = c64 < a.C;
    const uint32_t c = chan ? (uint32_t)c64 : a.C - 1u;                    // rows past the end load the last channel and store nothing
    uint32_t my_plan = kTdetNone;
    if (chan) {
        const uint32_t pi = a.plan_of ? a.plan_of[c] : 0u;
        if (pi < a.n_plans) my_plan = COPY ? 0u : pi;
    }
    if (k == 0u) L.plan[slot] = my_plan;
    // a channel without a plan: all-zero records, nothing else
    if (chan && my_plan == kTdetNone && a.rec && k == 0u)
        for (uint32_t f = 0; f < a.F; ++f) *reinterpret_cast<uint2 *>(a.rec + (uint64_t)f * a.C + c) = make_uint2(0u, 0u);
    __syncthreads();

    int16_t *buf = L.buf[slot];
    const bool g711 = a.g711 != nullptr;
    const bool alaw = g711 && a.codec[c] == IGDSP_PT_PCMA;
    uint32_t done = 0;                                                     // the block's slots whose plan has had its pass
    for (;;) {
        uint32_t p = kTdetNone, mask = 0;
        for (uint32_t s = 0; s < kTdetChans; ++s) {
            const uint32_t sp = L.plan[s];
            if (sp == kTdetNone || (done >> s & 1u)) continue;
            if (p == kTdetNone) p = sp;
            if (sp == p) mask |= 1u << s;
        }
        if (p == kTdetNone) break;                                         // block-uniform
        done |= mask;
        const igdsp_tdet_plan &pl = a.plans[p];
        const uint32_t nlo = tdet_nlo(pl), nhi = tdet_nhi(pl);
        const igdsp_tdet_thr thr = pl.thr;
        const bool valid = k < 8u ? k < nlo : k - 8u < nhi;
        // a plan of at most 4 + 4 bins leaves lanes 4..7 and 12..15 without one: lane k + 4 takes the second half of lane k's window
        const bool split = nlo <= 4u && nhi <= 4u;
        const uint32_t h2 = (h + 1u) >> 1, per = split ? (h2 + 1u) >> 1 : h2;
        const uint32_t kb = split ? k & 11u : k, jb = min(h2, (split ? (k >> 2) & 1u : 0u) * per), je = min(h2, jb + per);
        if (!COPY) {
            for (uint32_t i = tid; i < h2 * 16u; i += kTdetWaves * 64u) {
                const uint32_t j2 = i >> 4, kk = i & 15u;
                const bool v = kk < 8u ? kk < nlo : kk - 8u < nhi;
                uint4 t = make_uint4(0u, 0u, 0u, 0u);
                if (v) {
                    const uint32_t step = pl.step[kk < 8u ? kk : nlo + kk - 8u];
                    auto two = [&](bool cosine, uint32_t pr) -> uint32_t {          // window indices 2 pr, 2 pr + 1; a pair past the window: 0
                        if (pr >= h) return 0u;
                        const int32_t w0 = cosine ? tdet_wc(d_tdet_sin, step, 2u * pr) : tdet_ws(d_tdet_sin, step, 2u * pr);
                        const int32_t w1 = cosine ? tdet_wc(d_tdet_sin, step, 2u * pr + 1u) : tdet_ws(d_tdet_sin, step, 2u * pr + 1u);
                        return ((uint32_t)w0 & 0xFFFFu) | ((uint32_t)w1 << 16);
                    };
                    t = make_uint4(two(true, 2u * j2), two(false, 2u * j2), two(true, 2u * j2 + 1u), two(false, 2u * j2 + 1u));
                }
                L.tab[i] = t;
            }
        }
        __syncthreads();
        const bool mine = chan && (mask >> slot & 1u) != 0u;
        if (__builtin_amdgcn_ballot_w64(mine) != 0u) {                     // wave-uniform: one of the wave's four channels runs
            const uint64_t floor = tdet_floor(thr.min_amp, n);
            igdsp_tdet_state *st = a.state + c;
            {
                const uint32_t *h32 = reinterpret_cast<const uint32_t *>(st->hist);     // 2-byte aligned by type, 4 by the argument rule
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) reinterpret_cast<uint32_t *>(buf)[k + 16u * q] = h32[k + 16u * q];
            }
            const uint32_t s0 = reinterpret_cast<const uint32_t *>(st)[64], s1 = reinterpret_cast<const uint32_t *>(st)[65];
            TdetDeb d{s0 & 0xFFu, (s0 >> 8) & 0xFFu, (s0 >> 16) & 0xFFu, s0 >> 24, s1 & 0xFFFFu};
            wave_lds_fence();

            uint32_t nxt[8];
            tdet_row_load(a, c, k, nxt);
            for (uint32_t f = 0; f < a.F; ++f) {
                const uint32_t o = f * a.C + c;                            // < 2^32 - 32: the argument rule
                uint32_t cur[8];
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q) cur[q] = nxt[q];
                if (f + 1u < a.F) tdet_row_load(a, o + a.C, k, nxt);       // in flight during the sums
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q) {
                    const uint32_t m = k + 16u * q;
                    if (m < h) reinterpret_cast<uint32_t *>(buf)[64u + m] = tdet_unit(cur[q], g711, alaw);
                }
                wave_lds_fence();
                uint32_t w0 = 0u, w1 = 0u;
                if (!COPY) {
                    uint32_t code = 0u;
                    const TdetSums sm = tdet_sums<E0>(L, buf, h, k, kb, jb, je, split);
                    const uint32_t h0 = tdet_hit_dev(sm.I0, sm.Q0, sm.E0, n, lane, valid, thr, nhi, floor);
                    uint32_t fl = tdet_debounce(d, h0, thr.min_on, thr.min_off, code);
                    const uint32_t h1 = tdet_hit_dev(sm.I1, sm.Q1, sm.E1, n, lane, valid, thr, nhi, floor);
                    fl |= tdet_debounce(d, h1, thr.min_on, thr.min_off, code) << 2;
                    w0 = tdet_rec_w0(h0, h1, d.cur, fl);
                    w1 = tdet_rec_w1(d.len, code);
                }
                if (a.rec && mine && k == 0u) *reinterpret_cast<uint2 *>(a.rec + o) = make_uint2(w0, w1);
                // the history moves up by n: the last 128 values of (history, frame)
                uint32_t mv[4];
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) mv[q] = reinterpret_cast<const uint32_t *>(buf)[h + k + 16u * q];
                wave_lds_fence();
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) reinterpret_cast<uint32_t *>(buf)[k + 16u * q] = mv[q];
                wave_lds_fence();
            }
            if (mine) {
                uint32_t *h32 = reinterpret_cast<uint32_t *>(st->hist);
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) h32[k + 16u * q] = reinterpret_cast<const uint32_t *>(buf)[k + 16u * q];
                if (k == 0u) {
                    reinterpret_cast<uint32_t *>(st)[64] = d.cur | d.cand << 8 | d.run << 16 | d.off << 24;
                    reinterpret_cast<uint32_t *>(st)[65] = d.len;
                }
            }
        }
        __syncthreads();                                                   // the table is rebuilt next
    }
}

// the list's two passes over the dense records (event_list_pass): an event is a record whose flags meet the mask
struct TdetListRule {
    using Vec = uint2;
    static __device__ __forceinline__ bool is_event(const uint2 &r, uint32_t mask) { return ((r.x >> 24) & mask) != 0u; }
    static __device__ __forceinline__ uint4 make_event(uint32_t c, uint32_t f, const uint2 &r) { return make_uint4(c, f, r.x, r.y); }
};
template <bool WRITE>
__global__ __launch_bounds__(kListWaves * 64) void k_tdet_list(const igdsp_tdet_rec *rec, uint32_t C, uint32_t F, uint32_t W, uint32_t mask,
                                                               uint32_t *counts, igdsp_tdet_event *events, uint32_t cap)
{
    event_list_pass<WRITE, TdetListRule>(rec, C, F, W, mask, counts, events, cap);
}

hipError_t launch_tone_detect(const LaunchCfg &, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, const igdsp_tdet_plan *plans,
                              uint32_t n_plans, const uint16_t *plan_of, uint32_t C, uint32_t F, uint32_t n, uint32_t event_mask,
                              igdsp_tdet_state *state, igdsp_tdet_rec *rec, igdsp_tdet_event *events, uint32_t event_cap, uint32_t *event_count,
                              void *work, bool yardstick, hipStream_t s)
{
    const bool list = event_count != nullptr;
    const TdetRoute r = tdet_route(C, F, n, list, rec != nullptr);
    if (r.grid != 0) {
        rec = list_records(rec, list, work, r);
        const TdetArgs a{g711, codec, pcm, plans, plan_of, n_plans, C, F, n, state, rec};
        with_bool(yardstick, [&](auto Y) { with_key(Keys<0, 1, 2>{}, (int)r.e0, [&](auto O) {
            hipLaunchKernelGGL((k_tdet<Y, O>), dim3(r.grid), dim3(r.threads), 0, s, a); }); });
    }
    const uint32_t mask = event_mask ? event_mask : (uint32_t)IGDSP_TDET_EVENT_DEFAULT;
    return launch_event_list(k_tdet_list<false>, k_tdet_list<true>, r, r.grid == 0, rec, C, F, mask, events, event_cap, event_count, work, s);
}

}  // namespace igdsp
