// igdsp_k_agc.hip — the level control (igdsp_agc_run): per channel a slow gain toward a target peak level and a limiter whose cap ramps
// down one block ahead of a loud block.  Semantics: include/igdsp.h, section "Level control"; the rule's arithmetic: igdsp_agc.h
// (igdsp_agc_frame runs the same functions on the host); independent restatement: tests/agc_model.py.
//
// Shape (route: agc_route).  Half a wave, 32 lanes, owns one channel for the launch's frames, because the envelope, the gain and the
// cap run through time; lane b owns block b of the frame (8 samples: one 16-byte load of PCM or one 8-byte load of codes, one 16-byte
// store) and knot b + 1.  A frame of n samples keeps n / 8 lanes of the 32 busy; the others carry p = 0, which is r = CAP, the value the
// rule gives a term outside the frame.  A wave is two channels, a block kAgcChans.  No LDS.  Per frame:
//   p_b is the lane's own maximum, pk a maximum over the half (row_ror inside a DPP row, one ds_bpermute across the two rows);
//   r_b one exact 32-bit division per lane; the envelope, Gt (one division) and Gn the same in every lane of the half;
//   m_(b+1) = min(r_b, r_(b+1)) with the neighbour's r by a shuffle; knot 0 is every lane's: m_0 = r_0 by a shuffle from lane 0;
//   the knot recurrence runs in EVERY lane at once over k = 1 .. B, m_k read from lane k - 1 of either half by v_readlane (the loop
//   counter is wave-uniform); lane k - 1 keeps c_k, every lane ends with cap' = c_B: no lane waits for another, no scan is needed
//   (two per-half chains of uniform values were tried: the compiler keeps them in vector registers and the loop grows from 8 to 11
//   vector instructions);
//   A_(b+1) one signed division by B per lane; T_b comes from the left neighbour by a shuffle (lane 0: knot 0).
// The next frame's row is loaded before this one's arithmetic.  A bypassed channel runs the same instructions and selects the row.
// COPY (the compute-free yardstick, tools/agc_bench.py): the same row loads, decode, state load and store, row, record and PCM-record
// stores and their reductions; no block peak, division, recurrence or gain; d_ctl is not read.
// The DPP steps, the pack and the G.711 magnitude and sign are igdsp_lanes.h's.
// Everything is written with vector stores in plain C++: a block of the row, the record and the state as 16 bytes each.
#include "igdsp_lanes.h"
#include "igdsp_agc.h"

namespace igdsp {

struct AgcArgs {
    const uint8_t *g711, *codec;
    const int16_t *pcm;
    const uint8_t *ctl;
    AgcK k;
    uint32_t C, F, n;
    igdsp_agc_state *state;
    int16_t *out;
    igdsp_agc_rec *rec;
    igdsp_frame_stats *stats;
};

// op over the 32 lanes of a half, in each of them: row_ror 8, 4, 2, 1 inside a row of 16, then the other row of the half
template <typename Op>
__device__ __forceinline__ uint32_t agc_half_all(uint32_t v, Op op)
{
    v = op(v, dpp<0x128>(v));
    v = op(v, dpp<0x124>(v));
    v = op(v, dpp<0x122>(v));
    v = op(v, dpp<0x121>(v));
    return op(v, (uint32_t)__shfl_xor((int)v, 16, 64));
}
struct OpMin { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return min(a, b); } };
__device__ __forceinline__ uint64_t agc_half_sum64(uint64_t v)             // exact while the half's total is below 2^56
{
    return (uint64_t)agc_half_all((uint32_t)v & 0xFFFFFFu, OpAdd{}) + ((uint64_t)agc_half_all((uint32_t)(v >> 24), OpAdd{}) << 24);
}

// block `blk` of row o as it lies in memory: 16 bytes of PCM, or 8 bytes of codes in .x, .y
template <bool G711>
__device__ __forceinline__ uint4 agc_load(const AgcArgs &a, uint32_t o, uint32_t blk, bool busy)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (busy) {                                                            // d_pcm 16-byte, d_g711 8-byte aligned, n a multiple of 8: the argument rule
        if constexpr (G711) {
            const uint2 u = reinterpret_cast<const uint2 *>(a.g711 + (uint64_t)o * a.n)[blk];
            v.x = u.x; v.y = u.y;
        } else {
            v = reinterpret_cast<const uint4 *>(a.pcm + (uint64_t)o * a.n)[blk];
        }
    }
    return v;
}
template <bool G711>
__device__ __forceinline__ void agc_samples(const uint4 v, bool alaw, bool busy, int32_t (&x)[8])
{
    if constexpr (G711) {
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) {
            const uint32_t code = ((i < 4u ? v.x : v.y) >> (8u * (i & 3u))) & 0xFFu;
            const int32_t m = busy ? (int32_t)g711_abs(code, alaw) : 0;                          // no code of either law decodes to an idle lane's zero
            x[i] = g711_signed(code, m);
        }
    } else {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) { x[2u * i] = (int16_t)(w[i] & 0xFFFFu); x[2u * i + 1u] = (int16_t)(w[i] >> 16); }
    }
}

template <bool G711, bool COPY>
__global__ __launch_bounds__(kAgcWaves * 64, kAgcWaves * kAgcResident / 4) void k_agc(const AgcArgs a)
{
    const uint32_t tid = threadIdx.x, b = tid & (kAgcLanes - 1u), wl = tid & 63u, n = a.n, B = n >> 3;
    const uint64_t c64 = (uint64_t)blockIdx.x * kAgcChans + (tid >> 5);
    const bool chan = c64 < a.C, busy = b < B, first = b == 0u;
    const uint32_t c = chan ? (uint32_t)c64 : a.C - 1u;                    // halves past the end load the last channel and store nothing
    const bool alaw = G711 && a.codec[c] == IGDSP_PT_PCMA;
    const AgcK k = a.k;
    uint32_t ctl = COPY ? (uint32_t)IGDSP_AGC_BYPASS : (a.ctl ? agc_ctl(a.ctl[c]) : (uint32_t)IGDSP_AGC_RUN);

    // ---- the state: 16 bytes, the same in every lane of the half
    igdsp_agc_state *st = a.state + c;
    const uint4 sv = *reinterpret_cast<const uint4 *>(st);                 // d_state 16-byte aligned: the argument rule
    AgcRun r = agc_read(sv.x, sv.y & 0xFFFFu, sv.y >> 16, sv.z & 0xFFFFu, ctl == IGDSP_AGC_RESET, k);
    if (ctl == IGDSP_AGC_RESET) ctl = IGDSP_AGC_RUN;
    const bool bypass = ctl == IGDSP_AGC_BYPASS, frozen = ctl == IGDSP_AGC_FREEZE;
    uint32_t flags = 0u;

    uint4 nxt = agc_load<G711>(a, c, b, busy);
    for (uint32_t f = 0; f < a.F; ++f) {
        const uint32_t o = f * a.C + c;                                    // < 2^32 - 32: the argument rule
        const uint4 cur = nxt;
        if (f + 1u < a.F) nxt = agc_load<G711>(a, o + a.C, b, busy);       // in flight during the frame
        int32_t x[8];
        agc_samples<G711>(cur, alaw, busy, x);                             // an idle lane: eight zeros

        uint32_t Gn = r.G, tmin = kAgcUnity, n_limited = 0u, Tl = kAgcUnity, Tr = kAgcUnity, pk = 0u;
        flags = (uint32_t)IGDSP_AGC_BYPASSED;
        if constexpr (!COPY) {
            uint32_t p = 0u;
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) p = max(p, agc_abs(x[i]));
            pk = agc_half_all(p, OpMax{});
            flags = (pk >= k.gate ? (uint32_t)IGDSP_AGC_ACTIVE : 0u) | (frozen ? (uint32_t)IGDSP_AGC_FROZEN : 0u);
            const AgcRun was = r;
            if (pk >= k.gate && !frozen) Gn = agc_slow(r, pk, k, flags);
            // the limiter: the lane's ratio, the neighbour's, knot 0's
            const uint32_t rb = agc_ratio(p, k.ceil);
            const uint32_t rn = (uint32_t)__shfl_down((int)rb, 1, 32);
            const uint32_t mo = min(rb, b == kAgcLanes - 1u ? kAgcCap : rn);   // m_(b+1)
            const uint32_t m0 = (uint32_t)__shfl((int)rb, 0, 32);
            if (m0 < was.cap) flags |= IGDSP_AGC_ATTACKED;
            uint32_t cc = min(m0, was.cap), co = kAgcCap;
            const uint32_t c0 = cc;
#pragma unroll 1
            for (uint32_t q = 1; q <= B; ++q) {                            // wave-uniform: both halves walk the same knots
                const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)mo, (int)(q - 1u));
                const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)mo, (int)(q + 31u));
                cc = min(wl < 32u ? lo : hi, agc_release(cc, k.lrel));
                co = b == q - 1u ? cc : co;
            }
            r.cap = cc;
            // the knots: the lane's right one, knot 0, the left one from the neighbour
            const uint32_t Ao = agc_knot(was.G, Gn, b + 1u, B), T0 = min(was.G, c0);
            Tr = min(Ao, co);
            const uint32_t up = (uint32_t)__shfl_up((int)Tr, 1, 32);
            Tl = first ? T0 : up;
            const uint64_t lim = __builtin_amdgcn_ballot_w64(busy && co < Ao);
            n_limited = (uint32_t)__builtin_popcount((uint32_t)(lim >> (wl & 32u))) + (c0 < was.G ? 1u : 0u);
            tmin = min(agc_half_all(busy ? Tr : kAgcCap, OpMin{}), T0);
            if (n_limited) flags |= IGDSP_AGC_LIMITED;
            if (bypass) { r = was; Gn = was.G; tmin = kAgcUnity; n_limited = 0u; flags = (uint32_t)IGDSP_AGC_BYPASSED; }
        }

        // ---- the block's eight outputs, the row's sums
        uint32_t ow[4];
        uint64_t sq = 0;
        v2u16_t pko = (v2u16_t)(0);
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            int32_t e0 = x[2u * i], e1 = x[2u * i + 1u];
            if constexpr (!COPY) {
                if (!bypass) {
                    e0 = agc_out(e0, agc_gain_at(Tl, Tr, 2u * i));
                    e1 = agc_out(e1, agc_gain_at(Tl, Tr, 2u * i + 1u));
                }
            }
            ow[i] = pack2(e0, e1);
            pcm_acc2(ow[i], sq, pko);
        }
        if (a.out && chan && busy) reinterpret_cast<uint4 *>(a.out + (uint64_t)o * n)[b] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        const uint32_t opk = agc_half_all(max((uint32_t)pko.x, (uint32_t)pko.y), OpMax{});
        if (COPY || bypass) pk = opk;                                      // out = x
        if (a.stats) {                                                     // wave-uniform
            const uint64_t tot = agc_half_sum64(sq);
            if (chan && first) a.stats[o] = as_stats(pcm_record(tot, opk, n, 0u));
        }
        if (a.rec && chan && first)
            *reinterpret_cast<uint4 *>(a.rec + o) = make_uint4(Gn | tmin << 16, pk | opk << 16, r.env | flags << 16 | n_limited << 24, 0u);
        r.G = Gn;
    }

    // ---- the state goes back once; a bypassed channel's bytes are not touched (the yardstick writes the state as it was read)
    if (chan && first && (COPY || !bypass)) *reinterpret_cast<uint4 *>(st) = make_uint4((uint32_t)IGDSP_AGC_TAG, r.env | r.G << 16, r.cap | flags << 16, 0u);
}

hipError_t launch_agc(const LaunchCfg &, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, const uint8_t *ctl, const igdsp_agc_cfg &agc,
                      uint32_t C, uint32_t F, uint32_t n, igdsp_agc_state *state, int16_t *out, igdsp_agc_rec *rec, igdsp_frame_stats *stats,
                      bool yardstick, hipStream_t s)
{
    const AgcRoute r = agc_route(C, F, n, g711 != nullptr, yardstick);
    if (r.grid == 0) return hipSuccess;
    const AgcArgs a{g711, codec, pcm, ctl, agc_k(agc), C, F, n, state, out, rec, stats};
    with_bool(r.g711, [&](auto G) { with_bool(r.copy, [&](auto Y) { hipLaunchKernelGGL((k_agc<G, Y>), dim3(r.grid), dim3(r.threads), 0, s, a); }); });
    return hipGetLastError();
}

}  // namespace igdsp
