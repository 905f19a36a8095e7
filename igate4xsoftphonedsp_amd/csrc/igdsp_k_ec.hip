// igdsp_k_ec.hip — the echo canceller (igdsp_echo_cancel): per channel a block-normalised LMS filter of L = 128 or 256 taps over blocks
// of 8 samples.  Semantics: include/igdsp.h, section "Echo canceller"; the rule's arithmetic: igdsp_ec.h (igdsp_ec_frame runs the same
// functions on the host); independent restatement: tests/ec_model.py.
//
// Shape (route: ec_route).  A DPP row of 16 lanes owns one channel for the launch's frames, because the adaptation is sequential in
// time; lane k keeps the T = L / 16 weights of taps k T .. k T + T - 1 as int32 and, packed in pairs, as the 14-bit wh in registers
// across all frames.  A wave is four channels, a block kEcChans.  LDS per channel: x = the shifted far history of L values with the
// frame's xs = far >> 2 behind it, nr = the near row, which the output overwrites in place.  The rows of the next frame are loaded into
// registers a frame ahead.
// Per block of b <= 8 samples ending at value E of the frame: the lane reads the T + 8 values x[E - 8 - k T - T .. E - k T) as dwords D
// (even-packed) and makes the odd-packed O by v_alignbit; the window is anchored at the block's END, so a short last block uses the
// same register indices as a full one: its samples are j' = 8 - b .. 7, the positions below are masked (no output, es = 0).
//   outputs: acc[j'] = sum over the lane's tap pairs of v_dot2_i32_i16(D or O, wh pair): the pair (x[p - 1], x[p]) is aligned when j' is odd.
//   One batched row reduction: the eight partial sums (|.| <= 2^30) go as their low 12 bits, two to a dword, and their high parts
//   (row_ror 8, 4, 2, 1: twelve sums instead of sixteen); the total is 2 hs + ((ls + 1024) >> 11) in 32 bits.  This is why the rule
//   updates per block and not per sample.
//   P, xmax: D[4 ..) holds the lane's T most recent values at the block's end (lane 15's D[0 .. 4) the b values before them): dot2 of a
//   dword with itself, a packed |x| maximum, two row reductions.  dmax: every lane reads the block's near samples.
//   gradient: g[u] = four v_dot2 of (es pairs) with D (u even) or O (u odd); ec_update shifts and saturates in 64 bits.
// A wave whose four channels are all bypassed (or COPY) skips the block loop: the output is the near row as it lies in nr.
// COPY (the compute-free yardstick, tools/ec_bench.py): every channel as IGDSP_EC_BYPASS, d_ctl not read: the same row loads, buffer
// stores, history moves, records, row and state stores; no window read, dot product, reduction or update.
// The row's reductions, the packed dot product, the pack and the G.711 pair are igdsp_lanes.h's.
// Everything is written with vector stores: rows as dwords of a lane's two samples, the weights and the record as 16 bytes.
#include "igdsp_lanes.h"
#include "igdsp_ec.h"

namespace igdsp {

struct EcArgs {
    const uint8_t *g711, *codec;
    const int16_t *pcm, *far;
    const uint32_t *far_of;
    const uint8_t *ctl;
    uint32_t n_far, C, F, n;
    uint32_t mu_shift, pmin, hang, dmin;
    igdsp_ec_state *state;
    int16_t *out;
    igdsp_ec_rec *rec;
    igdsp_frame_stats *stats;
};

struct EcLds {
    __attribute__((aligned(16))) int16_t x[kEcChans][kEcXBuf];
    __attribute__((aligned(16))) int16_t nr[kEcChans][kEcNBuf];
};
static_assert(sizeof(EcLds) == kEcLdsBytes, "ec_route's LDS");

// two near samples as they lie in memory (two codes, or two PCM samples) -> two int16
template <bool G711>
__device__ __forceinline__ uint32_t ec_near_unit(uint32_t u, bool alaw)
{
    if constexpr (!G711) return u;
    return g711_pair(u, alaw);
}
__device__ __forceinline__ uint32_t ec_far_unit(uint32_t u) { return pack2(ec_xs((int16_t)(u & 0xFFFFu)), ec_xs((int16_t)(u >> 16))); }
__device__ __forceinline__ uint32_t ec_hist_unit(uint32_t u) { return pack2(ec_hist((int16_t)(u & 0xFFFFu)), ec_hist((int16_t)(u >> 16))); }

// units k, k + 16, .. of row o: near (codes: 2-byte units, PCM: dwords) and far (row fo; far absent: zeros)
template <bool G711>
__device__ __forceinline__ void ec_row_load(const EcArgs &a, uint32_t o, uint32_t fo, bool has_far, uint32_t k, uint32_t (&un)[8], uint32_t (&uf)[8])
{
    const uint32_t h = a.n >> 1;
#pragma unroll
    for (uint32_t q = 0; q < 8u; ++q) {
        const uint32_t m = k + 16u * q;
        un[q] = 0u;
        uf[q] = 0u;
        if (m < h) {                                                       // d_near_g711 2-byte, d_near_pcm and d_far_pcm 4-byte aligned, n even: the argument rule
            un[q] = G711 ? (uint32_t)reinterpret_cast<const uint16_t *>(a.g711 + (uint64_t)o * a.n)[m]
                         : reinterpret_cast<const uint32_t *>(a.pcm + (uint64_t)o * a.n)[m];
            if (has_far) uf[q] = reinterpret_cast<const uint32_t *>(a.far + (uint64_t)fo * a.n)[m];
        }
    }
}

template <bool G711, int L, bool COPY>
__global__ __launch_bounds__(kEcWaves * 64, kEcWaves * kEcResident / 4) void k_ec(const EcArgs a)
{
    constexpr uint32_t T = L / 16, ND = (T + 8u) / 2u, HQ = L / 32u;       // taps per lane, dwords of a window, history dwords per lane
    __shared__ EcLds S;
    const uint32_t tid = threadIdx.x, k = tid & 15u, slot = tid >> 4, n = a.n, h = n >> 1;
    const uint64_t c64 = (uint64_t)blockIdx.x * kEcChans + slot;
    const bool chan = c64 < a.C;
    const uint32_t c = chan ? (uint32_t)c64 : a.C - 1u;                    // rows past the end load the last channel and store nothing
    int16_t *xb = S.x[slot], *nb = S.nr[slot];
    uint32_t *x32 = reinterpret_cast<uint32_t *>(xb), *n32 = reinterpret_cast<uint32_t *>(nb);
    const bool alaw = G711 && a.codec[c] == IGDSP_PT_PCMA;
    const uint32_t fr = a.far_of ? a.far_of[c] : c;
    const bool has_far = fr < a.n_far;
    uint32_t ctl = COPY ? (uint32_t)IGDSP_EC_BYPASS : (a.ctl ? ec_ctl(a.ctl[c]) : (uint32_t)IGDSP_EC_RUN);

    // ---- the state: weights into registers, the history (read clamped) into LDS; another tag or RESET: the reset state
    igdsp_ec_state *st = a.state + c;
    const uint4 sc = *reinterpret_cast<const uint4 *>(&st->hang);          // d_state 16-byte aligned: the argument rule
    const bool keep = ec_tag_ok(sc.z, (uint32_t)L) && ctl != IGDSP_EC_RESET;
    if (ctl == IGDSP_EC_RESET) ctl = IGDSP_EC_RUN;
    if (!has_far) ctl = IGDSP_EC_BYPASS;
    const bool bypass = ctl == IGDSP_EC_BYPASS, frozen = ctl == IGDSP_EC_FREEZE;
    uint32_t hang = keep ? sc.x : 0u, sflags = keep ? sc.y & (uint32_t)IGDSP_EC_W_SATURATED : 0u;
    int32_t w[T];
    uint32_t wp[T / 2];
#pragma unroll
    for (uint32_t q = 0; q < T / 4u; ++q) {
        const uint4 v = reinterpret_cast<const uint4 *>(st->w)[k * (T / 4u) + q];
        w[4u * q] = keep ? (int32_t)v.x : 0; w[4u * q + 1u] = keep ? (int32_t)v.y : 0;
        w[4u * q + 2u] = keep ? (int32_t)v.z : 0; w[4u * q + 3u] = keep ? (int32_t)v.w : 0;
    }
#pragma unroll
    for (uint32_t m = 0; m < T / 2u; ++m) wp[m] = pack2(ec_wh(w[2u * m + 1u]), ec_wh(w[2u * m]));
    if (k < kEcPad / 2u) {                                                 // the pads: read only into masked positions; zero all the same
        x32[k] = 0u;
        x32[(kEcXBuf - kEcPad) / 2u + k] = 0u;
        n32[k] = 0u;
    }
#pragma unroll
    for (uint32_t q = 0; q < HQ; ++q) {
        const uint32_t v = reinterpret_cast<const uint32_t *>(st->hist)[k + 16u * q];
        x32[kEcPad / 2u + k + 16u * q] = keep ? ec_hist_unit(v) : 0u;
    }
    wave_lds_fence();

    const uint32_t t0 = k * T;
    const bool all_bypass = COPY || __builtin_amdgcn_ballot_w64(!bypass) == 0u;   // wave-uniform
    uint32_t nn[8], nf[8];
    ec_row_load<G711>(a, c, fr, has_far, k, nn, nf);
    for (uint32_t f = 0; f < a.F; ++f) {
        const uint32_t o = f * a.C + c;                                    // < 2^32 - 32: the argument rule (f * n_far + fr likewise)
        uint32_t cn[8], cf[8];
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) { cn[q] = nn[q]; cf[q] = nf[q]; }
        if (f + 1u < a.F) ec_row_load<G711>(a, o + a.C, (f + 1u) * a.n_far + fr, has_far, k, nn, nf);   // in flight during the blocks
        uint64_t sq_near = 0;
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) {
            const uint32_t m = k + 16u * q;
            if (m < h) {
                const uint32_t u = ec_near_unit<G711>(cn[q], alaw);
                sq_near += dot2(u, u, 0u);
                n32[kEcPad / 2u + m] = u;
                x32[(kEcPad + (uint32_t)L) / 2u + m] = ec_far_unit(cf[q]);
            }
        }
        wave_lds_fence();

        uint32_t flags = bypass ? (uint32_t)IGDSP_EC_BYPASSED : 0u, n_adapt = 0u, n_dt = 0u;
        if (!all_bypass) {
#pragma unroll 1
            for (uint32_t s = 0; s < n; s += 8u) {
                const uint32_t b = min(8u, n - s), E = s + b, j0 = 8u - b; // the block's samples are window positions j0 .. 7
                // the window: T + 8 values that end at the block's end, the lane's taps behind them
                const uint32_t *xw = x32 + (kEcPad + (uint32_t)L + E - 8u - t0 - T) / 2u;
                uint32_t D[ND], O[ND - 1u];
#pragma unroll
                for (uint32_t i = 0; i < ND; ++i) D[i] = xw[i];
#pragma unroll
                for (uint32_t i = 0; i + 1u < ND; ++i) O[i] = __builtin_amdgcn_alignbit(D[i + 1u], D[i], 16u);
                const uint32_t *nw = n32 + (kEcPad + E - 8u) / 2u;
                uint32_t nr4[4];
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) nr4[i] = nw[i];
                // the lane's part of the eight sums
                uint32_t acc[8];
#pragma unroll
                for (uint32_t j = 0; j < 8u; ++j) {
                    acc[j] = 0u;
#pragma unroll
                    for (uint32_t m = 0; m < T / 2u; ++m)
                        acc[j] = (j & 1u) ? dot2(D[(T + j - 2u * m - 1u) / 2u], wp[m], acc[j]) : dot2(O[(T + j - 2u * m - 2u) / 2u], wp[m], acc[j]);
                }
                // the batched row reduction, the outputs, dmax
                int32_t e[8];
                uint32_t dmax = 0u;
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) {
                    const uint32_t ls = row16_sum((acc[2u * i] & 0xFFFu) | (acc[2u * i + 1u] & 0xFFFu) << 16);
                    const int32_t hs0 = (int32_t)row16_sum((uint32_t)((int32_t)acc[2u * i] >> 12));
                    const int32_t hs1 = (int32_t)row16_sum((uint32_t)((int32_t)acc[2u * i + 1u] >> 12));
                    const int32_t y0 = ec_clamp16(2 * hs0 + (int32_t)(((ls & 0xFFFFu) + 1024u) >> 11));    // (4096 hs + ls + 1024) >> 11
                    const int32_t y1 = ec_clamp16(2 * hs1 + (int32_t)(((ls >> 16) + 1024u) >> 11));
                    const int32_t d0 = (int16_t)(nr4[i] & 0xFFFFu), d1 = (int16_t)(nr4[i] >> 16);
                    const bool v = 2u * i >= j0;                           // b is even: a pair is in the block or not
                    e[2u * i] = bypass ? d0 : ec_clamp16(d0 - y0);
                    e[2u * i + 1u] = bypass ? d1 : ec_clamp16(d1 - y1);
                    if (v) dmax = max(dmax, max((uint32_t)(d0 < 0 ? -d0 : d0), (uint32_t)(d1 < 0 ? -d1 : d1)));
                }
                // P and xmax over the lane's T most recent values (lane 15: and the b values before them)
                uint32_t ps = 0u;
                v2u16_t pk = (v2u16_t)(0);
                auto fold = [&](uint32_t d) {
                    const v2i16 xv = __builtin_bit_cast(v2i16, d);
                    const v2u16_t neg = (v2u16_t)(0) - __builtin_bit_cast(v2u16_t, d);
                    pk = __builtin_elementwise_max(pk, __builtin_bit_cast(v2u16_t, __builtin_elementwise_max(xv, __builtin_bit_cast(v2i16, neg))));
                };
#pragma unroll
                for (uint32_t i = 4u; i < ND; ++i) { ps = dot2(D[i], D[i], ps); fold(D[i]); }
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) if (k == 15u && 2u * i >= j0) fold(D[i]);
                const uint64_t P = row16_sum64(ps);
                const uint32_t xm = row16_max(max((uint32_t)pk.x, (uint32_t)pk.y));
                if (!bypass) {
                    hang = ec_hang(hang, xm, dmax, a.hang, a.dmin);
                    if (hang > 0u) { ++n_dt; flags |= IGDSP_EC_DOUBLETALK; }
                    if (P >= a.pmin) flags |= IGDSP_EC_FAR_ACTIVE;
                }
                const bool adapt = !bypass && !frozen && hang == 0u && P >= a.pmin;
                if (__builtin_amdgcn_ballot_w64(adapt) != 0u) {            // wave-uniform: one of the wave's four channels adapts
                    uint32_t ep[4];
#pragma unroll
                    for (uint32_t i = 0; i < 4u; ++i) ep[i] = 2u * i >= j0 ? pack2(ec_es(e[2u * i]), ec_es(e[2u * i + 1u])) : 0u;
                    const int32_t sh = 31 - (int32_t)a.mu_shift - ec_bit_length(P);
                    bool sat = false;
#pragma unroll
                    for (uint32_t u = 0; u < T; ++u) {
                        uint32_t g = 0u;
#pragma unroll
                        for (uint32_t i = 0; i < 4u; ++i)
                            g = (u & 1u) ? dot2(O[(T + 2u * i - u - 1u) / 2u], ep[i], g) : dot2(D[(T + 2u * i - u) / 2u], ep[i], g);
                        const int32_t nw32 = ec_update(w[u], (int32_t)g, sh, sat);
                        w[u] = adapt ? nw32 : w[u];
                    }
#pragma unroll
                    for (uint32_t m = 0; m < T / 2u; ++m) wp[m] = pack2(ec_wh(w[2u * m + 1u]), ec_wh(w[2u * m]));
                    const uint64_t sb = __builtin_amdgcn_ballot_w64(sat && adapt);     // a lane clipped one of its taps: the row's 16 bits
                    if (adapt) {
                        ++n_adapt;
                        flags |= IGDSP_EC_ADAPTED;
                        if (((sb >> (tid & 48u)) & 0xFFFFu) != 0u) { flags |= IGDSP_EC_W_SATURATED; sflags |= IGDSP_EC_W_SATURATED; }
                    }
                }
                // the outputs over the near samples, in place: lane i < 4 stores pair i of the block
                {
                    const uint32_t p0 = pack2(e[0], e[1]), p1 = pack2(e[2], e[3]), p2 = pack2(e[4], e[5]), p3 = pack2(e[6], e[7]);
                    const uint32_t mine = k == 0u ? p0 : (k == 1u ? p1 : (k == 2u ? p2 : p3));
                    if (k < 4u && 2u * k >= j0) n32[(kEcPad + E - 8u) / 2u + k] = mine;
                }
                wave_lds_fence();
            }
        }

        // ---- the frame's stores: the row, its records
        uint32_t wm = 0u;
#pragma unroll
        for (uint32_t u = 0; u < T; ++u) { const int32_t v = ec_wh(w[u]); wm = max(wm, (uint32_t)(v < 0 ? -v : v)); }
        wm = row16_max(wm);
        uint64_t sq_out = 0;
        v2u16_t pko = (v2u16_t)(0);
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) {
            const uint32_t m = k + 16u * q;
            if (m < h) {
                const uint32_t u = n32[kEcPad / 2u + m];
                pcm_acc2(u, sq_out, pko);
                if (a.out && chan) reinterpret_cast<uint32_t *>(a.out + (uint64_t)o * n)[m] = u;
            }
        }
        const uint64_t tn = row16_sum64(sq_near), to = row16_sum64(sq_out);
        const uint32_t peak = row16_max(max((uint32_t)pko.x, (uint32_t)pko.y));
        if (chan && k == 0u) {
            if (a.rec) *reinterpret_cast<uint4 *>(a.rec + o) = make_uint4((uint32_t)(tn >> 8), (uint32_t)(to >> 8), flags | n_adapt << 8 | n_dt << 16, wm);
            if (a.stats) a.stats[o] = as_stats(pcm_record(to, peak, n, 0u));
        }
        // the history moves up by n: the last L values of (history, frame)
        uint32_t mv[HQ];
#pragma unroll
        for (uint32_t q = 0; q < HQ; ++q) mv[q] = x32[kEcPad / 2u + h + k + 16u * q];
        wave_lds_fence();
#pragma unroll
        for (uint32_t q = 0; q < HQ; ++q) x32[kEcPad / 2u + k + 16u * q] = mv[q];
        wave_lds_fence();
    }

    // ---- the state goes back once: weights, history, the scalars; at L = 128 the upper halves are written 0
    if (chan) {
#pragma unroll
        for (uint32_t q = 0; q < T / 4u; ++q)
            reinterpret_cast<uint4 *>(st->w)[k * (T / 4u) + q] = make_uint4((uint32_t)w[4u * q], (uint32_t)w[4u * q + 1u], (uint32_t)w[4u * q + 2u], (uint32_t)w[4u * q + 3u]);
#pragma unroll
        for (uint32_t q = 0; q < HQ; ++q) reinterpret_cast<uint32_t *>(st->hist)[k + 16u * q] = x32[kEcPad / 2u + k + 16u * q];
        if constexpr (L == 128) {
#pragma unroll
            for (uint32_t q = 0; q < 2u; ++q) reinterpret_cast<uint4 *>(st->w)[32u + k * 2u + q] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) reinterpret_cast<uint32_t *>(st->hist)[64u + k + 16u * q] = 0u;
        }
        if (k == 0u) *reinterpret_cast<uint4 *>(&st->hang) = make_uint4(hang, sflags, (uint32_t)IGDSP_EC_TAG | (uint32_t)L, 0u);
    }
}

hipError_t launch_echo_cancel(const LaunchCfg &, const uint8_t *near_g711, const uint8_t *codec, const int16_t *near_pcm, const int16_t *far_pcm,
                              uint32_t n_far, const uint32_t *far_of, const uint8_t *ctl, const igdsp_ec_cfg &ec, uint32_t C, uint32_t F, uint32_t n,
                              igdsp_ec_state *state, int16_t *out, igdsp_ec_rec *rec, igdsp_frame_stats *stats, bool yardstick, hipStream_t s)
{
    const EcRoute r = ec_route(C, F, n, ec.tail);
    if (r.grid == 0) return hipSuccess;
    const EcArgs a{near_g711, codec, near_pcm, far_pcm, far_of, ctl, n_far, C, F, n, ec.mu_shift, ec.pmin, ec.hang, ec.dmin, state, out, rec, stats};
    with_bool(near_g711 != nullptr, [&](auto G) { with_key(Keys<128, 256>{}, (int)r.tail, [&](auto T) { with_bool(yardstick, [&](auto Y) {
        hipLaunchKernelGGL((k_ec<G, T, Y>), dim3(r.grid), dim3(r.threads), 0, s, a); }); }); });
    return hipGetLastError();
}

}  // namespace igdsp
