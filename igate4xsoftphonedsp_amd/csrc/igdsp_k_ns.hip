// igdsp_k_ns.hip — noise suppression (igdsp_ns_run): per channel and hop of 80 samples a 256-point integer transform forward and back,
// 32 band gains from a tracked noise estimate between them.  Semantics: include/igdsp.h, section "Noise suppression"; the rule's
// arithmetic, phase by phase: igdsp_ns.h (igdsp_ns_frame runs the same functions on the host with one lane); independent restatement:
// tests/ns_model.py.
//
// Shape (route: ns_route).  kNsLanes = 16 lanes own a channel for the launch's frames, four channels a wave, a block is one wave.  The
// channel's state lives in LDS from the first frame to the last (67 16-byte pieces in, 67 out), beside the transform's 128 complex
// points, the band gains and the frame's row, which is worked in place.  Every phase of a hop is divided over the 16 lanes by item
// (ns_hop: item lane, lane + 16, ...: four butterflies of a pass, two bands, five samples of the window); between two phases stands
// wave_lds_fence, never a barrier: the lanes of a channel are lanes of one wave.  Channels of a wave that differ in d_ctl diverge at
// the hop (BYPASS) and join behind it; a wave's lanes past the last channel work a copy of the last channel in their own LDS and store
// nothing.  Per frame:
//   - the NEXT frame's pieces are loaded into registers (16 bytes of PCM or 8 of codes per lane and turn, up to kNsTurns = 3 turns),
//     in flight through the frame's hops;
//   - the hops (ns_frame_core), the record's sums folded over the 16 lanes through LDS;
//   - the row goes out as 16-byte pieces, record and PCM record as one 16-byte store each by the channel's first lane;
//   - the next frame's pieces go from the registers to the row, G.711 decoded on the way (g711_decode8, igdsp_lanes.h).
// COPY (the compute-free yardstick, tools/ns_bench.py): every channel as under BYPASS, so the same loads, decode, row stores and
// reads, state load and store, folds and output stores, and the delay's pass over the row; no transform, no band runs; d_ctl is not read.
// Everything is written with vector stores in plain C++.
#include "igdsp_ns.h"
#include "igdsp_lanes.h"

namespace igdsp {

static_assert(sizeof(igdsp_ns_state) == kNsStateBytes && sizeof(NsWork) == kNsWorkBytes && kNsLanes == kNsMaxLanes && kNsMaxN == kNsMaxFrame, "ns_chan_bytes");

__device__ const int16_t d_ns_win[kNsWinLen] = {IGDSP_NS_WIN_VALUES};
__device__ const int32_t d_ns_tw[2 * kNsPoints] = {IGDSP_NS_TW_VALUES};

struct NsArgs {
    const uint8_t *g711, *codec;
    const int16_t *pcm;
    const uint8_t *ctl;
    igdsp_ns_cfg cfg;
    uint32_t C, F, n;
    igdsp_ns_state *state;
    int16_t *out;
    igdsp_ns_rec *rec;
    igdsp_frame_stats *stats;
};

struct NsFence {
    __device__ __forceinline__ void operator()() const { wave_lds_fence(); }
};

// a piece in registers: native vectors, so that the turns' array stays registers
typedef uint32_t ns_u32x2_t __attribute__((ext_vector_type(2)));
template <int IN> struct NsPiece { using type = u32x4_t; };
template <> struct NsPiece<kNsG711> { using type = ns_u32x2_t; };

// the pieces lane, lane + 16, lane + 32 of frame-row t (= f * C + c) into registers; no branch: a turn past the row's last piece loads
// the last piece again
template <int IN>
__device__ __forceinline__ void ns_fetch(const NsArgs &a, uint64_t t, uint32_t P, uint32_t lane, typename NsPiece<IN>::type (&nx)[kNsTurns])
{
#pragma unroll
    for (uint32_t u = 0; u < kNsTurns; ++u) {
        const uint32_t p = min(u * kNsLanes + lane, P - 1u);               // p < n / 8: inside row t, t < C * F
        if constexpr (IN == kNsG711) nx[u] = reinterpret_cast<const ns_u32x2_t *>(a.g711 + t * a.n)[p];   // 8-byte aligned: the argument rule, n a multiple of 8
        else nx[u] = reinterpret_cast<const u32x4_t *>(a.pcm + t * a.n)[p];                           // 16-byte aligned
    }
}
// and from the registers into the channel's row
template <int IN>
__device__ __forceinline__ void ns_fill(uint4 *row, bool alaw, uint32_t P, uint32_t lane, const typename NsPiece<IN>::type (&nx)[kNsTurns])
{
#pragma unroll
    for (uint32_t u = 0; u < kNsTurns; ++u) {
        const uint32_t p = u * kNsLanes + lane;
        if (p < P) {                                                       // 16 p + 16 <= 2 n: inside the row
            if constexpr (IN == kNsG711) row[p] = g711_decode8(nx[u].x, nx[u].y, alaw);
            else row[p] = make_uint4(nx[u].x, nx[u].y, nx[u].z, nx[u].w);
        }
    }
}

template <int IN, bool COPY>
__global__ __launch_bounds__(64) void k_ns(const NsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t ns_lds[];
    const uint32_t lane = threadIdx.x & (kNsLanes - 1u), g = threadIdx.x / kNsLanes, n = a.n, P = n >> 3;   // g < kNsChans: the block is one wave
    uint8_t *base = ns_lds + g * ns_chan_bytes(n);                         // (g + 1) * ns_chan_bytes(n) <= ns_lds_bytes(n): the route's LDS
    igdsp_ns_state &st = *reinterpret_cast<igdsp_ns_state *>(base);
    NsWork &ws = *reinterpret_cast<NsWork *>(base + kNsStateBytes);
    int16_t *row = reinterpret_cast<int16_t *>(base + kNsStateBytes + kNsWorkBytes);
    uint4 *row4 = reinterpret_cast<uint4 *>(row);
    const uint64_t c64 = (uint64_t)blockIdx.x * kNsChans + g;
    const bool chan = c64 < (uint64_t)a.C;
    const uint32_t c = chan ? (uint32_t)c64 : a.C - 1u;                    // lanes past the end work the last channel again and store nothing
    const bool alaw = IN == kNsG711 && a.codec[c] == IGDSP_PT_PCMA;
    const uint32_t ctl = COPY ? (uint32_t)IGDSP_NS_BYPASS : (a.ctl ? ns_ctl(a.ctl[c]) : (uint32_t)IGDSP_NS_RUN);
    constexpr uint32_t kStatePieces = kNsStateBytes / 16u;

    // ---- the state into LDS: 67 16-byte pieces over the 16 lanes (d_state 16-byte aligned: the argument rule)
    uint4 *sg = reinterpret_cast<uint4 *>(a.state + c), *sl = reinterpret_cast<uint4 *>(base);
    for (uint32_t p = lane; p < kStatePieces; p += kNsLanes) sl[p] = sg[p];
    typename NsPiece<IN>::type nx[kNsTurns];
    ns_fetch<IN>(a, (uint64_t)c, P, lane, nx);
    wave_lds_fence();
    const bool fresh = ns_fresh(st.tag, ctl == (uint32_t)IGDSP_NS_RESET);
    ns_open_state(st, fresh, lane, kNsLanes, NsFence{});
    ns_fill<IN>(row4, alaw, P, lane, nx);
    wave_lds_fence();

    uint32_t flags = 0u;
    for (uint32_t f = 0; f < a.F; ++f) {
        const uint64_t t = (uint64_t)f * a.C + c;                          // < 2^32 - 32: the argument rule
        if (f + 1u < a.F) ns_fetch<IN>(a, t + a.C, P, lane, nx);           // in flight during the frame
        uint32_t w[4], peak = 0u;
        uint64_t sq = 0u;
        ns_frame_core(a.cfg, st, ws, d_ns_win, d_ns_tw, row, n, ctl, (f == 0u && fresh) ? (uint32_t)IGDSP_NS_WAS_RESET : 0u, lane, kNsLanes, NsFence{}, w, sq,
                      peak);
        flags = w[3] >> 8;
        if (chan) {
            if (a.out) {
                uint4 *dst = reinterpret_cast<uint4 *>(a.out + t * n);    // d_out 16-byte aligned, 2 n a multiple of 16
#pragma unroll
                for (uint32_t u = 0; u < kNsTurns; ++u) {
                    const uint32_t p = u * kNsLanes + lane;
                    if (p < P) dst[p] = row4[p];
                }
            }
            if (lane == 0u) {
                if (a.rec) *reinterpret_cast<uint4 *>(a.rec + t) = make_uint4(w[0], w[1], w[2], w[3]);
                if (a.stats) *reinterpret_cast<uint4 *>(a.stats + t) = pcm_record(sq, peak, n, 0u);
            }
        }
        wave_lds_fence();                                                  // the next frame overwrites the row
        if (f + 1u < a.F) {
            ns_fill<IN>(row4, alaw, P, lane, nx);
            wave_lds_fence();
        }
    }

    // ---- the state goes back once
    if (lane == 0u) ns_close_state(st, flags);
    wave_lds_fence();
    if (chan)
        for (uint32_t p = lane; p < kStatePieces; p += kNsLanes) sg[p] = sl[p];
}

hipError_t launch_ns(const LaunchCfg &, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, const uint8_t *ctl, const igdsp_ns_cfg &ns, uint32_t C,
                     uint32_t F, uint32_t n, igdsp_ns_state *state, int16_t *out, igdsp_ns_rec *rec, igdsp_frame_stats *stats, bool yardstick, hipStream_t s)
{
    const NsRoute r = ns_route(C, F, n, g711 != nullptr, yardstick);
    if (r.grid == 0) return hipSuccess;
    const NsArgs a{g711, codec, pcm, ctl, ns, C, F, n, state, out, rec, stats};
    with_key(Keys<kNsG711, kNsPcm>{}, r.in, [&](auto IN) {
        if (r.copy) hipLaunchKernelGGL((k_ns<IN, true>), dim3(r.grid), dim3(r.threads), r.lds, s, a);
        else hipLaunchKernelGGL((k_ns<IN, false>), dim3(r.grid), dim3(r.threads), r.lds, s, a);
    });
    return hipGetLastError();
}

}  // namespace igdsp
