// igdsp_k_filt.hip — the filter (igdsp_filt_run): per channel a chain of up to four second-order IIR sections over the leg's rows.
// Semantics: include/igdsp.h, section "Filter"; the rule's arithmetic: igdsp_filt.h (igdsp_filt_frame runs the same functions on the
// host); independent restatement: tests/filt_model.py.
//
// Shape (route: filt_route).  The recurrence is serial in the sample and independent across channels: a lane owns a channel for the
// launch's frames, with its S sections' coefficients and histories in registers (the loops over the sections have constant bounds and
// unroll: no register array is indexed at run time, no scratch).  A block is one wave.  S is the launch's, 1, 2 or 4: a channel whose
// plan has fewer sections, a bypassed one and one without a plan run identity sections, which return their input bit for bit, so the
// lanes of a wave never diverge in the sample loop.  Per frame:
//   - the NEXT frame's pieces are loaded into registers, wave-wide: 16 bytes of PCM or 8 of codes per lane and turn, consecutive in
//     memory, the first kFiltAhead = 16 turns (a row's first 128 samples) in flight through the sample loop (the turns are a
//     constant-bound loop, so the registers are named at compile time, and branch-free: a turn past the row's last piece loads the
//     last piece again; all 32 turns held ahead took the PCM form to 400 VGPRs);
//   - the lane walks its row of the tile a dword (two samples) at a time: unpack, in-peak, the sections, out-peak, pack, store in place;
//   - the wave stores the tile as 16-byte pieces, consecutive in memory (a lane-per-channel store of the rows would be uncoalesced);
//   - with d_stats the lane folds its row from the tile (pcm_acc2, the PCM record of igdsp_pcmrec.h); record and stats are one store
//     per lane, consecutive across the wave;
//   - the next frame's pieces go from the registers to the tile, G.711 decoded on the way; the turns past kFiltAhead are loaded then.
// The plan (12 dwords, gathered by the lane's plan index) and the state (three 16-byte loads) are read once; the state is stored once.
// COPY (the compute-free yardstick, tools/filt_bench.py): every channel as under BYPASS, so the same loads, decode, tile stores, the
// lane's read and write of every dword of its row with the peak fold a bypassed row's record needs, tile reads, state load and store
// and output stores; no section runs; d_ctl is not read, of a plan only its first dword.
// The tile's addressing (tile_item, tile_piece) and the G.711 piece (g711_decode8) are igdsp_lanes.h's.
// Everything is written with vector stores in plain C++.
#include "igdsp_filt.h"
#include "igdsp_lanes.h"

namespace igdsp {

struct FiltArgs {
    const uint8_t *g711, *codec;
    const int16_t *pcm;
    const uint8_t *ctl;
    const igdsp_filt_plan *plans;
    const uint16_t *plan_of;
    uint32_t n_plans, max_s, C, F, n, inv;
    igdsp_filt_state *state;
    int16_t *out;
    igdsp_filt_rec *rec;
    igdsp_frame_stats *stats;
};

template <int IN> struct FiltPiece { using type = uint4; };
template <> struct FiltPiece<kFiltG711> { using type = uint2; };

// turns u0 .. u0 + kFiltAhead - 1 of the tile whose first row is frame-row t0, into registers: turn u is item u * 64 + lane of `items`
template <int IN, uint32_t U0>
__device__ __forceinline__ void filt_fetch(const FiltArgs &a, uint64_t t0, uint32_t items, uint32_t P, uint32_t lane,
                                           typename FiltPiece<IN>::type (&nx)[kFiltAhead])
{
#pragma unroll
    for (uint32_t u = 0; u < kFiltAhead; ++u) {                            // no branch: a turn past the last item loads the last item again
        const uint32_t i = min((U0 + u) * 64u + lane, items - 1u);         // items >= P >= 1
        if constexpr (IN == kFiltG711) nx[u] = reinterpret_cast<const uint2 *>(a.g711 + t0 * a.n)[i];   // 8-byte aligned: the argument rule
        else nx[u] = reinterpret_cast<const uint4 *>(a.pcm + t0 * a.n)[i];                             // 16-byte aligned
    }
}
// and from the registers into the tile: item i is piece i % P of row i / P
template <int IN, uint32_t U0>
__device__ __forceinline__ void filt_fill(const FiltArgs &a, uint32_t *tile, const uint8_t *law, uint32_t stride, uint32_t items, uint32_t P,
                                          uint32_t lane, const typename FiltPiece<IN>::type (&nx)[kFiltAhead])
{
#pragma unroll
    for (uint32_t u = 0; u < kFiltAhead; ++u) {
        const uint32_t i = (U0 + u) * 64u + lane;                          // i < 2^11
        if (i < items) {                                                   // row < 64, piece < P: the piece lies in its row, the row in the tile
            const TileItem t = tile_item(i, a.inv, P);
            uint4 x;
            if constexpr (IN == kFiltG711) x = g711_decode8(nx[u].x, nx[u].y, law[t.row] != 0u);
            else x = nx[u];
            uint32_t *d = tile_piece(tile, stride, t);
            d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
        }
    }
}
// the turns past the first kFiltAhead (rows of more than 128 samples): loaded and written behind the others, not ahead of the frame
template <int IN>
__device__ __forceinline__ void filt_late(const FiltArgs &a, uint64_t t0, uint32_t *tile, const uint8_t *law, uint32_t stride, uint32_t items, uint32_t P,
                                          uint32_t lane, typename FiltPiece<IN>::type (&nx)[kFiltAhead])
{
    if (P > kFiltAhead) {
        filt_fetch<IN, kFiltAhead>(a, t0, items, P, lane, nx);
        filt_fill<IN, kFiltAhead>(a, tile, law, stride, items, P, lane, nx);
    }
}
// |x| of two samples in one dword, folded into two running unsigned maxima (-32768 stays 0x8000 = 32768 unsigned)
__device__ __forceinline__ void filt_peak2(uint32_t w, v2u16_t &pk)
{
    const v2i16 x = __builtin_bit_cast(v2i16, w);
    const v2u16_t neg = (v2u16_t)(0) - __builtin_bit_cast(v2u16_t, w);
    pk = __builtin_elementwise_max(pk, __builtin_bit_cast(v2u16_t, __builtin_elementwise_max(x, __builtin_bit_cast(v2i16, neg))));
}

template <int IN, int S, bool COPY>
__global__ __launch_bounds__(64) void k_filt(const FiltArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t filt_lds[];
    const uint32_t lane = threadIdx.x, n = a.n, P = n >> 3, stride = tile_row_dwords(n);
    uint32_t *tile = filt_lds;                                             // [kFiltChans][stride]
    uint8_t *law = reinterpret_cast<uint8_t *>(filt_lds + kFiltChans * stride);   // [kFiltChans]
    const uint64_t c0 = (uint64_t)blockIdx.x * kFiltChans;                 // < C: the grid
    const uint32_t rows = (uint32_t)((uint64_t)a.C - c0 < kFiltChans ? (uint64_t)a.C - c0 : kFiltChans), items = rows * P;
    const bool chan = lane < rows;
    const uint32_t c = chan ? (uint32_t)c0 + lane : a.C - 1u;              // lanes past the end load the last channel and store nothing
    law[lane] = (uint8_t)(IN == kFiltG711 && a.codec[c] == IGDSP_PT_PCMA ? 1u : 0u);   // lane < kFiltChans = 64: the block is one wave
    const uint32_t ctl = COPY ? (uint32_t)IGDSP_FILT_BYPASS : (a.ctl ? filt_ctl(a.ctl[c]) : (uint32_t)IGDSP_FILT_RUN);

    // ---- the plan: the lane's index, the plan's dwords that S sections reach (d_plans 4-byte aligned, n_plans >= 1: the argument rule)
    const uint32_t pi = a.plan_of ? a.plan_of[c] : 0u;
    const bool have = pi < a.n_plans;
    uint32_t pw[kFiltPlanWords];
    {
        const uint32_t *pp = reinterpret_cast<const uint32_t *>(a.plans + (have ? pi : 0u));
        constexpr uint32_t kWords = COPY ? 1u : (4u + 5u * (uint32_t)S + 1u) / 2u;
#pragma unroll
        for (uint32_t i = 0; i < kFiltPlanWords; ++i) pw[i] = i < kWords && i != 1u ? pp[i] : 0u;
    }
    uint32_t ns = 0u;
    const uint32_t pflags = filt_plan_flags(pw[0], have, a.max_s, ns);
    const bool pass = COPY || ctl == IGDSP_FILT_BYPASS || (pflags & IGDSP_FILT_NO_PLAN) != 0u;

    // ---- the state: three 16-byte loads per lane (d_state 16-byte aligned: the argument rule)
    uint32_t sw[kFiltStateWords];
    {
        const uint4 *sp = reinterpret_cast<const uint4 *>(a.state + c);
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) {
            const uint4 v = sp[i];
            sw[4u * i] = v.x; sw[4u * i + 1u] = v.y; sw[4u * i + 2u] = v.z; sw[4u * i + 3u] = v.w;
        }
    }
    const bool zero = filt_zeroed(sw[0], ctl == IGDSP_FILT_RESET);
    const uint32_t flags_read = zero ? 0u : sw[11] & 0xFFFFu;             // the yardstick writes them back as read
    filt_read_state(sw, zero);                                            // (a lane that passes does not write it)
    uint32_t flags0 = COPY || ctl == IGDSP_FILT_BYPASS ? (uint32_t)IGDSP_FILT_BYPASSED : pflags;
    if (!pass && zero) flags0 |= (uint32_t)IGDSP_FILT_WAS_RESET;          // the first frame's
    FiltSec q[S];
    bool ran[S];
#pragma unroll
    for (uint32_t s = 0; s < (uint32_t)S; ++s) {                           // ns <= max_s <= S when the lane does not pass
        ran[s] = filt_load_section(pw, s, !pass && s < ns, q[s]);
        if (!pass && s < ns && !ran[s]) flags0 |= (uint32_t)IGDSP_FILT_BAD_PLAN;
        filt_read_section(sw, s, q[s]);
    }
    uint32_t *row = tile + lane * stride;
    uint32_t flags = flags0;

    typename FiltPiece<IN>::type nx[kFiltAhead];
    filt_fetch<IN, 0u>(a, c0, items, P, lane, nx);
    wave_lds_fence();                                                      // the laws
    filt_fill<IN, 0u>(a, tile, law, stride, items, P, lane, nx);
    filt_late<IN>(a, c0, tile, law, stride, items, P, lane, nx);
    wave_lds_fence();

    for (uint32_t f = 0; f < a.F; ++f) {
        const uint32_t o = f * a.C + c;                                    // < 2^32 - 32: the argument rule
        const uint64_t t0 = (uint64_t)f * a.C + c0;                        // the tile's first row
        if (f + 1u < a.F) filt_fetch<IN, 0u>(a, t0 + a.C, items, P, lane, nx);   // in flight during the frame

        // ---- the sample loop, lane per channel, in place
        uint32_t clipped = 0u;
        v2u16_t pin = (v2u16_t)(0), pout = (v2u16_t)(0);
        if (chan) {
            for (uint32_t j = 0; j < n / 2u; ++j) {
                const uint32_t w = row[j];
                filt_peak2(w, pin);
                if constexpr (COPY) {
                    row[j] = w;
                } else {
                    int32_t v0 = (int32_t)(int16_t)w, v1 = (int32_t)w >> 16;
#pragma unroll
                    for (uint32_t s = 0; s < (uint32_t)S; ++s) v0 = filt_step(q[s], v0, clipped);
#pragma unroll
                    for (uint32_t s = 0; s < (uint32_t)S; ++s) v1 = filt_step(q[s], v1, clipped);
                    const uint32_t wo = ((uint32_t)v0 & 0xFFFFu) | ((uint32_t)v1 << 16);
                    filt_peak2(wo, pout);
                    row[j] = wo;
                }
            }
        }
        if constexpr (COPY) pout = pin;
        flags = (f == 0u ? flags0 : flags0 & ~(uint32_t)IGDSP_FILT_WAS_RESET) | (clipped ? (uint32_t)IGDSP_FILT_CLIPPED : 0u);
        wave_lds_fence();

        // ---- the tile goes out, wave-wide
        if (a.out) {
            uint4 *dst = reinterpret_cast<uint4 *>(a.out + t0 * n);       // d_out 16-byte aligned, n a multiple of 8: the argument rule
            for (uint32_t it = 0; it < P; ++it) {
                const uint32_t i = it * 64u + lane;
                if (i < items) {
                    const uint32_t *s = tile_piece(tile, stride, tile_item(i, a.inv, P));
                    dst[i] = make_uint4(s[0], s[1], s[2], s[3]);
                }
            }
        }
        // ---- record, stats: one store per lane
        if (chan) {
            if (a.rec) {
                uint32_t w[4];
                filt_pack_rec(max((uint32_t)pin.x, (uint32_t)pin.y), max((uint32_t)pout.x, (uint32_t)pout.y), clipped, pi, flags, ns, w);
                *reinterpret_cast<uint4 *>(a.rec + o) = make_uint4(w[0], w[1], w[2], w[3]);
            }
            if (a.stats) {
                uint64_t sq = 0u;
                v2u16_t pk2 = (v2u16_t)(0);
                for (uint32_t j = 0; j < n / 2u; ++j) pcm_acc2(row[j], sq, pk2);
                *reinterpret_cast<uint4 *>(a.stats + o) = pcm_record(sq, max((uint32_t)pk2.x, (uint32_t)pk2.y), n, 0u);
            }
        }
        wave_lds_fence();                                                  // the next frame overwrites the tile
        if (f + 1u < a.F) {
            filt_fill<IN, 0u>(a, tile, law, stride, items, P, lane, nx);
            filt_late<IN>(a, t0 + a.C, tile, law, stride, items, P, lane, nx);
            wave_lds_fence();
        }
    }

    // ---- the state goes back once; a channel that passes keeps its bytes (the yardstick writes the state as it was read)
    if (chan && (COPY || !pass)) {
        if constexpr (!COPY) {
#pragma unroll
            for (uint32_t s = 0; s < (uint32_t)S; ++s) filt_write_section(sw, s, ran[s], q[s]);
        }
        filt_close_state(sw, COPY ? flags_read : flags);
        uint4 *sp = reinterpret_cast<uint4 *>(a.state + c);
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) sp[i] = make_uint4(sw[4u * i], sw[4u * i + 1u], sw[4u * i + 2u], sw[4u * i + 3u]);
    }
}

hipError_t launch_filt(const LaunchCfg &, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, const uint8_t *ctl, const igdsp_filt_plan *plans,
                       uint32_t n_plans, const uint16_t *plan_of, uint32_t max_sections, uint32_t C, uint32_t F, uint32_t n, igdsp_filt_state *state,
                       int16_t *out, igdsp_filt_rec *rec, igdsp_frame_stats *stats, bool yardstick, hipStream_t s)
{
    const FiltRoute r = filt_route(C, F, n, g711 != nullptr, max_sections, yardstick);
    if (r.grid == 0) return hipSuccess;
    const FiltArgs a{g711, codec, pcm, ctl, plans, plan_of, n_plans, r.max_sections, C, F, n, r.inv, state, out, rec, stats};
    with_key(Keys<kFiltG711, kFiltPcm>{}, r.in, [&](auto IN) {
        if (r.copy) {
            hipLaunchKernelGGL((k_filt<IN, 1, true>), dim3(r.grid), dim3(r.threads), r.lds, s, a);
        } else {
            with_key(Keys<1, 2, 4>{}, r.sections, [&](auto S) { hipLaunchKernelGGL((k_filt<IN, S, false>), dim3(r.grid), dim3(r.threads), r.lds, s, a); });
        }
    });
    return hipGetLastError();
}

}  // namespace igdsp
