// igdsp_k_vad.hip — voice activity, DTX and the comfort-noise payload (igdsp_vad_run): per channel and frame the exact autocorrelation of
// the row over 11 lags, the decision against an adaptive floor, the hangover, the noise model and, on the rare frame that sends one, the
// RFC 3389 payload.  Semantics: include/igdsp.h, section "Voice activity"; the rule's arithmetic: igdsp_vad.h (igdsp_vad_frame runs the
// same functions on the host); independent restatement: tests/vad_model.py.
//
// Shape (route: vad_route), the transposed one.  A DPP row of 16 lanes owns one channel for the launch's frames; a wave is four
// channels, a block kVadChans.  Per frame the row (loaded a frame ahead: lane p takes pieces p and p + 16 of 8 samples, 8 bytes of codes
// or 16 of PCM each) is decoded, shifted to v = x >> 2 and stored to LDS behind kVadPad zeros, zeros behind it too.  An odd lag's
// pairs straddle dwords, so the row is kept a second time one sample ahead (the lanes pack it with v_alignbit from the first copy, once
// per frame and piece, not once per lag and pair): an even lane reads the pairs (v[j], v[j+1]) and an odd lane the pairs (v[j+1],
// v[j+2]), j even, and both then find their partners k samples earlier on a dword boundary.  Lane k sums lag k over the whole row: per
// 8 samples one 16-byte read of its copy (two addresses in a row), four dwords of the first copy k samples earlier, four
// v_dot2_i32_i16 into a 32-bit partial (16 products of at most 2^26) that is widened to 64 bits every other step.  Lanes 11..15 sum
// lags nobody reads.  No reduction exists: lane 0 holds E = r[0] and hands it to the row, lane k keeps A[k] in registers.  The
// decision, the floor, the hangover and the DTX step run in every lane of the row on the same values.  The two levels of a frame
// (skipped, by a wave-uniform test, where neither is read: no records and every row of the wave in VOICE or without DTX) come
// from one pass over the table in LDS, which holds n * T8[d]: lane k compares both energies with entries 8 k .. 8 k + 7 and the row adds
// the counts of entries still above them, which is vad_level's least d because T8 never rises.  A frame that sends a SID (wave-uniform
// test: most frames skip the block) gathers A in LDS and lane 0 of the row runs the recursion there with 64-bit arithmetic: vad_sid
// indexes LDS, never a register array.  Lanes 0..3 of the row store the record, the payload, the kind and the control byte.
// COPY (the compute-free yardstick, tools/vad_bench.py): the same row loads, decode, LDS stores, state load and store and output stores;
// no lag sum, level, decision, model or recursion; d_ctl is not read.
// The list (launch_vad, launch_event_list): k_vad_list is event_list_pass over the records whose flags meet the mask.
// The row's sum, the packed dot product and the G.711 magnitude and sign are igdsp_lanes.h's.  Everything is written with vector stores in plain C++.
#include "igdsp_lanes.h"
#include "igdsp_vad.h"

namespace igdsp {

__device__ const uint64_t d_vad_t8[128] = {IGDSP_VAD_T8_VALUES};

struct VadArgs {
    const uint8_t *g711, *codec;
    const int16_t *pcm;
    const uint8_t *ctl;
    VadK k;
    uint32_t C, F, n;
    igdsp_vad_state *state;
    uint8_t *kind;
    igdsp_vad_rec *rec;
    uint8_t *sid, *txctl;
};

struct VadLds {
    uint64_t tab[128];                                                     // n * T8[d]
    __attribute__((aligned(16))) int16_t buf[kVadChans][kVadBuf];         // kVadPad zeros, the row, zeros
    __attribute__((aligned(16))) int16_t odd[kVadChans][256];             // the row one sample ahead: dword i = (v[2 i + 1], v[2 i + 2])
    int64_t A[kVadChans][12], R[kVadChans][12], a[kVadChans][12];         // the rare path's arrays
    __attribute__((aligned(16))) uint8_t sid[kVadChans][16];
};
static_assert(sizeof(VadLds) == kVadLdsBytes, "vad_route's LDS");

// level(e0) and level(e1) in every lane of the row: lane k counts the entries 8 k .. 8 k + 7 of tab = n * T8 that lie above e << 8, the
// row adds the counts (row16_sum).  T8 never rises and T8[127] is 0, so the count is the least d with (e << 8) >= n * T8[d],
// 127 if there is none in 0..126: vad_level's value
__device__ __forceinline__ void vad_levels(int64_t e0, int64_t e1, const uint64_t *tab, uint32_t k, uint32_t &l0, uint32_t &l1)
{
    const uint64_t a = e0 > 0 ? (uint64_t)e0 << 8 : 0u, b = e1 > 0 ? (uint64_t)e1 << 8 : 0u;          // e <= 2^40
    uint32_t c = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 8u; ++i) {
        const uint64_t t = tab[8u * k + i];
        c += (a < t ? 1u : 0u) + (b < t ? 0x10000u : 0u);
    }
    c = row16_sum(c);
    l0 = e0 > 0 ? c & 0xFFFFu : 127u;
    l1 = e1 > 0 ? c >> 16 : 127u;
}

// a value of lane 0 of the row, in each of its lanes
__device__ __forceinline__ uint64_t vad_row0(uint64_t v)
{
    return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, 0, 16) | (uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), 0, 16) << 32;
}
// piece `p` of row o as it lies in memory: 16 bytes of PCM, or 8 bytes of codes in .x, .y
template <bool G711>
__device__ __forceinline__ uint4 vad_load(const VadArgs &a, uint32_t o, uint32_t p, bool busy)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (busy) {                                                            // d_pcm 16-byte, d_g711 8-byte aligned, n a multiple of 8: the argument rule
        if constexpr (G711) {
            const uint2 u = reinterpret_cast<const uint2 *>(a.g711 + (uint64_t)o * a.n)[p];
            v.x = u.x; v.y = u.y;
        } else {
            v = reinterpret_cast<const uint4 *>(a.pcm + (uint64_t)o * a.n)[p];
        }
    }
    return v;
}
// the piece's eight values v = x >> 2 as four dwords of two int16; codes: the shift on the MAGNITUDE (a multiple of 4), then the sign
// (g711_abs, g711_signed: igdsp_lanes.h), which is why g711_decode8 does not serve here
template <bool G711>
__device__ __forceinline__ uint4 vad_values(const uint4 v, bool alaw)
{
    uint32_t w[4];
    if constexpr (G711) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            const uint32_t d = i < 2u ? v.x : v.y, c0 = (d >> (16u * (i & 1u))) & 0xFFu, c1 = (d >> (16u * (i & 1u) + 8u)) & 0xFFu;
            const int32_t m0 = (int32_t)g711_abs(c0, alaw) >> 2, m1 = (int32_t)g711_abs(c1, alaw) >> 2;   // multiples of 4
            w[i] = ((uint32_t)g711_signed(c0, m0) & 0xFFFFu) | ((uint32_t)g711_signed(c1, m1) << 16);
        }
    } else {
        const uint32_t s[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) w[i] = pack2((int32_t)(int16_t)(s[i] & 0xFFFFu) >> 2, (int32_t)(int16_t)(s[i] >> 16) >> 2);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <bool G711, bool COPY>
__global__ __launch_bounds__(kVadWaves * 64, kVadWaves * kVadResident / 4) void k_vad(const VadArgs a)
{
    __shared__ VadLds L;
    const uint32_t tid = threadIdx.x, k = tid & (kVadLanes - 1u), slot = tid >> 4, n = a.n, P = n >> 3;
    const uint64_t c64 = (uint64_t)blockIdx.x * kVadChans + slot;
    const bool chan = c64 < a.C;
    const uint32_t c = chan ? (uint32_t)c64 : a.C - 1u;                    // rows past the end load the last channel and store nothing
    const bool alaw = G711 && a.codec[c] == IGDSP_PT_PCMA;
    const VadK K = a.k;
    uint32_t ctl = COPY ? (uint32_t)IGDSP_VAD_BYPASS : (a.ctl ? vad_ctl(a.ctl[c]) : (uint32_t)IGDSP_VAD_RUN);
    const bool p0 = k < P, p1 = k + 16u < P;

    if (!COPY && tid < 128u) L.tab[tid] = d_vad_t8[tid] * n;
    int16_t *buf = L.buf[slot];
    if (k < kVadPad / 2u) reinterpret_cast<uint32_t *>(buf)[k] = 0u;
    if (k < 4u) reinterpret_cast<uint32_t *>(buf)[kVadPad / 2u + n / 2u + k] = 0u;         // v[n .. n + 7]: no row store reaches them
    __syncthreads();

    // ---- the state: the scalars the same in every lane of the row, A[k] in lane k
    igdsp_vad_state *st = a.state + c;
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(st);          // d_state 16-byte aligned: the argument rule
    const bool reset = ctl == IGDSP_VAD_RESET, is_reset = vad_is_reset(sw[0], reset);
    VadRun r = vad_read(sw[0], sw[1], sw[24], sw[25], sw[26], reset, K);
    int64_t A = vad_read_a(k < kVadLags ? st->A[k] : 0, is_reset);
    if (reset) ctl = IGDSP_VAD_RUN;
    const bool bypass = ctl == IGDSP_VAD_BYPASS, frozen = ctl == IGDSP_VAD_FREEZE;
    uint32_t flags = 0u;

    const uint32_t *vb = reinterpret_cast<const uint32_t *>(buf) + kVadPad / 2u;   // the dword of sample 0
    uint32_t *ob = reinterpret_cast<uint32_t *>(L.odd[slot]);
    const uint4 *xb = reinterpret_cast<const uint4 *>((k & 1u) ? ob : vb);         // the lane's own pairs
    const uint32_t *lb = vb - (k >> 1);                                            // their partners k samples earlier: >= the pad's first dword

    uint4 n0 = vad_load<G711>(a, c, k, p0), n1 = vad_load<G711>(a, c, k + 16u, p1);
    for (uint32_t f = 0; f < a.F; ++f) {
        const uint32_t o = f * a.C + c;                                    // < 2^32 - 32: the argument rule
        const uint4 c0 = n0, c1 = n1;
        if (f + 1u < a.F) { n0 = vad_load<G711>(a, o + a.C, k, p0); n1 = vad_load<G711>(a, o + a.C, k + 16u, p1); }   // in flight during the frame
        if (p0) reinterpret_cast<uint4 *>(buf + kVadPad)[k] = vad_values<G711>(c0, alaw);
        if (p1) reinterpret_cast<uint4 *>(buf + kVadPad)[k + 16u] = vad_values<G711>(c1, alaw);
        wave_lds_fence();
        // the second copy, one sample ahead; the dword behind the row's last piece is zero
        uint32_t d0[5], d1[5];
#pragma unroll
        for (uint32_t i = 0; i < 5u; ++i) { d0[i] = p0 ? vb[4u * k + i] : 0u; d1[i] = p1 ? vb[4u * (k + 16u) + i] : 0u; }
        if (p0) reinterpret_cast<uint4 *>(ob)[k] = make_uint4(__builtin_amdgcn_alignbit(d0[1], d0[0], 16), __builtin_amdgcn_alignbit(d0[2], d0[1], 16),
                                                              __builtin_amdgcn_alignbit(d0[3], d0[2], 16), __builtin_amdgcn_alignbit(d0[4], d0[3], 16));
        if (p1) reinterpret_cast<uint4 *>(ob)[k + 16u] = make_uint4(__builtin_amdgcn_alignbit(d1[1], d1[0], 16), __builtin_amdgcn_alignbit(d1[2], d1[1], 16),
                                                                    __builtin_amdgcn_alignbit(d1[3], d1[2], 16), __builtin_amdgcn_alignbit(d1[4], d1[3], 16));
        wave_lds_fence();

        uint32_t ms = 0u, lvl_e = 127u, kind = IGDSP_VAD_VOICE, sid_len = 0u;
        uint4 pay = make_uint4(0u, 0u, 0u, 0u);
        flags = (uint32_t)IGDSP_VAD_F_BYPASSED;
        if constexpr (!COPY) {
            int64_t rk = 0;
            auto step = [&](uint32_t j, uint32_t acc) -> uint32_t {        // 8 samples of the lane's lag
                const uint4 x = xb[j];
                const uint32_t *lp = lb + 4u * j;
                return dot2(x.w, lp[3], dot2(x.z, lp[2], dot2(x.y, lp[1], dot2(x.x, lp[0], acc))));
            };
            uint32_t j = 0;
            for (; j + 2u <= P; j += 2u) rk += (int32_t)step(j + 1u, step(j, 0u));   // wave-uniform; 16 products of at most 2^26 fit 32 bits
            if (j < P) rk += (int32_t)step(j, 0u);
            const uint64_t E = vad_row0((uint64_t)rk);
            uint32_t lvl = 0u;
            ms = vad_ms(E, n);
            if (!bypass) {
                flags = vad_decide(r, ms, frozen, K);
                if (!frozen && !(flags & IGDSP_VAD_F_RAW)) {
                    A = vad_model(A, rk, r.avalid, K.asm_shift);
                    r.avalid = 1u;
                }
            }
            // the levels, where somebody reads one: level(E) goes into the record (the list's records included), vad_dtx reads level(A[0])
            // on a non-VOICE frame with dtx only.  Wave-uniform: a launch without records skips the pass on its VOICE frames
            const bool reads_a = !bypass && K.dtx && !(flags & IGDSP_VAD_F_VOICE);
            if (a.rec != nullptr || __builtin_amdgcn_ballot_w64(reads_a) != 0u) {
                const int64_t A0 = (int64_t)vad_row0((uint64_t)A);         // every lane of the wave is here
                vad_levels((int64_t)E, reads_a ? A0 : 0, L.tab, k, lvl_e, lvl);
            }
            if (!bypass) {
                kind = vad_dtx(r, flags, lvl, K);
                const bool sid = kind == IGDSP_VAD_SID;
                if (__builtin_amdgcn_ballot_w64(sid) != 0u) {              // wave-uniform: the rare path
                    if (sid && k < kVadLags) L.A[slot][k] = A;
                    wave_lds_fence();
                    if (sid && k == 0u) vad_sid(L.A[slot], lvl, K.order, L.R[slot], L.a[slot], L.sid[slot]);
                    wave_lds_fence();
                    if (sid) {
                        pay = *reinterpret_cast<const uint4 *>(L.sid[slot]);
                        sid_len = 1u + K.order;
                        flags |= IGDSP_VAD_F_SID;
                    }
                }
            }
        }
        // ---- the frame's outputs: the row's lanes 0..3 take one each
        if (chan) {
            if (a.rec && k == 0u) {
                uint32_t w[4];
                vad_pack_rec(ms, r.nf, r.run, flags, kind, lvl_e, r.hang, sid_len, w);
                *reinterpret_cast<uint4 *>(a.rec + o) = make_uint4(w[0], w[1], w[2], w[3]);
            }
            if (a.sid && k == 1u) reinterpret_cast<uint4 *>(a.sid)[o] = pay;
            if (a.kind && k == 2u) a.kind[o] = (uint8_t)kind;
            if (a.txctl && k == 3u) a.txctl[o] = (uint8_t)((flags & (IGDSP_VAD_F_VOICE | IGDSP_VAD_F_BYPASSED)) ? K.vox_on : K.vox_off);
        }
        wave_lds_fence();                                                  // the next row overwrites this one
    }

    // ---- the state goes back once; a bypassed channel's bytes are not touched (the yardstick writes the state as it was read)
    if (chan && (COPY || !bypass)) {
        uint32_t *so = reinterpret_cast<uint32_t *>(st);
        if (k < kVadLags) st->A[k] = A;
        else if (k == kVadLags) *reinterpret_cast<uint2 *>(so) = make_uint2((uint32_t)IGDSP_VAD_TAG, r.nf);
        if (k < 8u) so[24u + k] = k == 0u ? vad_w24(r) : (k == 1u ? vad_w25(r) : (k == 2u ? vad_w26(r, flags) : 0u));
    }
}

// the list's two passes over the dense records (event_list_pass): an event is a record whose flags meet the mask
struct VadListRule {
    using Vec = uint4;
    static __device__ __forceinline__ bool is_event(const uint4 &r, uint32_t mask) { return ((r.z >> 16) & 0xFFu & mask) != 0u; }
    static __device__ __forceinline__ uint4 make_event(uint32_t c, uint32_t f, const uint4 &r) { return make_uint4(c, f, r.x, (r.z & 0x00FFFFFFu) | (r.w & 0xFFu) << 24); }
};
template <bool WRITE>
__global__ __launch_bounds__(kListWaves * 64) void k_vad_list(const igdsp_vad_rec *rec, uint32_t C, uint32_t F, uint32_t W, uint32_t mask,
                                                              uint32_t *counts, igdsp_vad_event *events, uint32_t cap)
{
    event_list_pass<WRITE, VadListRule>(rec, C, F, W, mask, counts, events, cap);
}

hipError_t launch_vad(const LaunchCfg &, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, const uint8_t *ctl, const igdsp_vad_cfg &vad,
                      uint32_t C, uint32_t F, uint32_t n, uint32_t event_mask, igdsp_vad_state *state, uint8_t *kind, igdsp_vad_rec *rec, uint8_t *sid,
                      uint8_t *txctl, igdsp_vad_event *events, uint32_t event_cap, uint32_t *event_count, void *work, bool yardstick, hipStream_t s)
{
    const bool list = event_count != nullptr;
    const VadRoute r = vad_route(C, F, n, g711 != nullptr, yardstick, list, rec != nullptr);
    if (r.grid != 0) {
        rec = list_records(rec, list, work, r);
        const VadArgs a{g711, codec, pcm, ctl, vad_k(vad), C, F, n, state, kind, rec, sid, txctl};
        with_bool(r.g711, [&](auto G) { with_bool(r.copy, [&](auto Y) { hipLaunchKernelGGL((k_vad<G, Y>), dim3(r.grid), dim3(r.threads), 0, s, a); }); });
    }
    const uint32_t mask = event_mask ? event_mask : (uint32_t)IGDSP_VAD_EVENT_DEFAULT;
    return launch_event_list(k_vad_list<false>, k_vad_list<true>, r, r.grid == 0, rec, C, F, mask, events, event_cap, event_count, work, s);
}

}  // namespace igdsp
