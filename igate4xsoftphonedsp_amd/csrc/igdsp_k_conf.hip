// igdsp_k_conf.hip — the conference mix (igdsp_conf_mix): pjmedia's bridge step behind pjsua_conf_connect / pjsua_conf_adjust_rx_level
// (roip_ed137.cpp:4907-4917, 5190-5233), batched over frames and output ports.  Semantics: include/igdsp.h, section "Conference mix";
// independent restatement: tests/conf_model.py.
//
// Shape.  An item is one (frame, port) pair, items frame-major (item = f * P + p), so neighbouring items are neighbouring ports of one
// frame: a gateway that numbers its calls by console reads one contiguous run of frame rows per group of items.  A block of kConfWaves
// waves takes groups of kConfWaves consecutive items (static, grid-stride).  A lane owns samples 4 lane .. 4 lane + 3 of the frame.
//   narrow ports (<= kConfWideMin members; the console case): wave w of the block mixes item w of the group by itself, member after
//             member, kConfU frame loads in flight, and writes the port-frame's PCM and record.
//   wide ports (more members): flagged in LDS; after one barrier the whole block takes each flagged item in turn, wave w sums a
//             contiguous 1 / kConfWaves slice of the member list into int64 partials in LDS, and wave 0 combines the partials and
//             writes.  One wave per destination would run as long as its longest list; the integer sums are exact, so any
//             split gives the same bits.
// Member metadata (channel, gain, length, law) are read 64 members at a time, one per lane, and handed to the member loop with
// v_readlane, so the frame loads of a batch do not wait behind a chain of dependent scalar loads.  Members at or past C and members
// whose gain or length is 0 are never read.
#include "igdsp_q7.h"

namespace igdsp {

static_assert(kConfWaves * 64 * 4 * 8 <= 32 * 1024, "the wide form's partials fit next to the 64 KiB LUT");

struct ConfArgs {
    const uint8_t *g711;
    const uint8_t *codec;
    const int16_t *pcm;
    const uint16_t *len;
    const uint16_t *gain;
    const uint32_t *port_ptr;
    const uint32_t *members;
    uint32_t n_members, C, P, F, n;
    int16_t *out;
    igdsp_frame_stats *stats;
    uint32_t vec_in, vec_out;   // n % 4 == 0 and the input (4-byte G.711 / 8-byte PCM) / output (8-byte) rows aligned
};

// running sums of one wave over a member range: samples 4 lane + k
struct ConfAcc {
    int64_t s[4];
    uint32_t sat;       // a per-member clamp fired (lane-local)
    uint32_t live;      // a member < C with len > 0 was seen (wave-uniform)
};

// the lane's four input samples of frame row `row` as magnitudes + sign bits (bit k = sample k negative)
template <int IN>
__device__ __forceinline__ uint2 conf_load(const ConfArgs &a, uint64_t row, uint32_t lane)
{
    const uint32_t b0 = 4u * lane;
    if (b0 >= a.n) return make_uint2(0u, 0u);
    if (IN == kConfG711) {
        const uint8_t *p = a.g711 + row * a.n + b0;
        if (a.vec_in) return make_uint2(*reinterpret_cast<const uint32_t *>(p), 0u);
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4u && b0 + k < a.n; ++k) w |= (uint32_t)p[k] << (8u * k);
        return make_uint2(w, 0u);
    } else {
        const int16_t *p = a.pcm + row * a.n + b0;
        if (a.vec_in) return *reinterpret_cast<const uint2 *>(p);
        uint32_t x = 0, y = 0;
        for (uint32_t k = 0; k < 4u && b0 + k < a.n; ++k) {
            const uint32_t v = (uint16_t)p[k];
            if (k < 2u) x |= v << (16u * k); else y |= v << (16u * (k - 2u));
        }
        return make_uint2(x, y);
    }
}

// Mix members [b, e) of frame f into acc.  COPY: the yardstick — the same loads, folded by xor instead of decoded and scaled.
template <int IN, bool COPY>
__device__ __forceinline__ void conf_range(const ConfArgs &a, const uint2 *lut, uint32_t f, uint32_t b, uint32_t e, uint32_t lane, ConfAcc &acc)
{
    const uint32_t off = (lane & 31u) * 8u;
    for (uint32_t j0 = b; j0 < e; j0 += 64u) {
        const uint32_t cnt = min(e - j0, 64u);
        // metadata, one member per lane: channel, and meta = gain | len << 16 | A-law << 25 (0 = contributes nothing)
        uint32_t cv = 0, meta = 0;
        if (lane < cnt) {
            const uint32_t c = a.members[j0 + lane];
            if (c < a.C) {
                const uint32_t l = a.len ? min((uint32_t)a.len[(uint64_t)f * a.C + c], a.n) : a.n;
                const uint32_t g = a.gain[c];
                const uint32_t law = (IN == kConfG711 && a.codec[c] == IGDSP_PT_PCMA) ? 1u : 0u;
                cv = c;
                meta = l ? (g | l << 16 | law << 25) : 0u;
                if (g == 0u) meta &= 0xFFFF0000u;
            }
        }
        if (__builtin_amdgcn_ballot_w64(meta != 0u)) acc.live = 1u;       // a muted member still makes the frame live
        int32_t s32[4] = {0, 0, 0, 0};                                     // <= 64 members x 32 768: no overflow
#pragma nounroll
        for (uint32_t k0 = 0; k0 < cnt; k0 += kConfU) {                    // (kConfU loads in flight, not more: the register budget)
            uint2 v[kConfU];
            uint32_t m[kConfU];
#pragma unroll
            for (int u = 0; u < kConfU; ++u) {
                const uint32_t idx = k0 + (uint32_t)u;                     // < 64: kConfU divides 64
                m[u] = (uint32_t)__builtin_amdgcn_readlane((int)meta, (int)idx);
                const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cv, (int)idx);
                if (idx >= cnt || (m[u] & 0xFFFFu) == 0u) m[u] = 0u;
                v[u] = m[u] ? conf_load<IN>(a, (uint64_t)f * a.C + c, lane) : make_uint2(0u, 0u);
            }
#pragma unroll
            for (int u = 0; u < kConfU; ++u) {
                const uint32_t mm = m[u];
                if (mm == 0u) continue;                                    // wave-uniform
                if (COPY) { s32[u & 3] ^= (int32_t)(v[u].x ^ v[u].y); continue; }
                const uint32_t g = mm & 0xFFFFu, l = (mm >> 16) & 0x1FFu, law80 = (mm >> 25) ? 0x80808080u : 0u;
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    uint32_t ax, neg;
                    q7_sample<IN>(lut, v[u], law80, off, k, ax, neg);
                    IGDSP_Q7_LEVEL(q, ax, neg, g, 4u * lane + k, l, acc.sat);   // 0 past this member's len (and past n)
                    s32[k] += neg ? -(int32_t)q : (int32_t)q;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc.s[k] += s32[k];
    }
}

// The port-frame's PCM and record from the wave's final sums (every lane of the wave active).
template <bool COPY>
__device__ __forceinline__ void conf_finish(const ConfArgs &a, uint64_t item, uint32_t lane, const ConfAcc &acc)
{
    const uint32_t n = a.n, b0 = 4u * lane;
    const bool empty = acc.live == 0u;
    int32_t o[4];
    uint32_t sat = acc.sat, peak = 0;
    uint64_t sq = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int64_t s = acc.s[k];
        if (COPY) { o[k] = (int32_t)s; continue; }
        const int64_t cl = s < -32768 ? -32768 : (s > 32767 ? 32767 : s);
        sat |= cl != s ? 1u : 0u;
        o[k] = (b0 + (uint32_t)k < n && !empty) ? (int32_t)cl : 0;
        const uint32_t ax = (uint32_t)(o[k] < 0 ? -o[k] : o[k]);
        sq += (uint64_t)ax * ax;
        peak = max(peak, ax);
    }
    q7_store(a.out, a.stats, item, n, a.vec_out, lane, o, empty, sat, sq, peak);
}

template <int IN, bool COPY>
__global__ __launch_bounds__(kConfWaves * 64) void k_conf_mix(const ConfArgs a)
{
    __shared__ __attribute__((aligned(16))) uint2 lut[IN == kConfG711 && !COPY ? kLutEntries : 1];
    __shared__ int64_t part[kConfWaves][4][64];                            // wide form: [wave][sample k][lane]
    __shared__ uint32_t part_sat[kConfWaves], part_live[kConfWaves];
    __shared__ uint32_t wide[2][kConfWaves];                               // wide items of the group (wave + 1, or 0), by group parity
    if (IN == kConfG711 && !COPY) fill_lut(lut);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t n_items = (uint64_t)a.F * a.P;
    const uint64_t n_groups = (n_items + kConfWaves - 1u) / kConfWaves;
    __syncthreads();
    uint32_t par = 0;
    for (uint64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x, par ^= 1u) {
        // (wide[] is double-buffered: a wave that leaves the wide loop early writes the next group's flags while the others
        // still read this group's, and cannot get two groups ahead without passing the next group's barrier)
        const uint64_t item = grp * kConfWaves + w;
        uint32_t f = 0, b = 0, e = 0;
        if (item < n_items) {
            const uint32_t p = (uint32_t)(item % a.P);
            f = (uint32_t)(item / a.P);
            b = min(a.port_ptr[p], a.n_members);
            e = min(a.port_ptr[p + 1u], a.n_members);
            if (e < b) e = b;                                               // a descending port_ptr: empty port
        }
        const bool is_wide = item < n_items && e - b > (uint32_t)kConfWideMin;
        if (item < n_items && !is_wide) {
            ConfAcc acc{{0, 0, 0, 0}, 0u, 0u};
            conf_range<IN, COPY>(a, lut, f, b, e, lane, acc);
            conf_finish<COPY>(a, item, lane, acc);
        }
        if (lane == 0u) wide[par][w] = is_wide ? (uint32_t)(w + 1u) : 0u;
        __syncthreads();
        for (uint32_t i = 0; i < (uint32_t)kConfWaves; ++i) {
            if (wide[par][i] == 0u) continue;                                    // block-uniform
            const uint64_t it = grp * kConfWaves + i;
            const uint32_t p = (uint32_t)(it % a.P), fi = (uint32_t)(it / a.P);
            const uint32_t wb = min(a.port_ptr[p], a.n_members), we = min(a.port_ptr[p + 1u], a.n_members);
            const uint32_t sl = (we - wb + kConfWaves - 1u) / kConfWaves;
            const uint32_t sb = min(wb + w * sl, we), se = min(sb + sl, we);
            ConfAcc acc{{0, 0, 0, 0}, 0u, 0u};
            conf_range<IN, COPY>(a, lut, fi, sb, se, lane, acc);
#pragma unroll
            for (int k = 0; k < 4; ++k) part[w][k][lane] = acc.s[k];
            const uint32_t s = __builtin_amdgcn_ballot_w64(acc.sat != 0u) != 0u ? 1u : 0u;
            if (lane == 0u) { part_sat[w] = s; part_live[w] = acc.live; }
            __syncthreads();
            if (w == 0u) {
                ConfAcc t{{0, 0, 0, 0}, 0u, 0u};
#pragma nounroll
                for (uint32_t q = 0; q < (uint32_t)kConfWaves; ++q) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) t.s[k] = COPY ? (t.s[k] ^ part[q][k][lane]) : t.s[k] + part[q][k][lane];
                    t.sat |= part_sat[q];
                    t.live |= part_live[q];
                }
                conf_finish<COPY>(a, it, lane, t);
            }
            __syncthreads();
        }
    }
}

static ConfArgs conf_args(const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, const uint16_t *len, const uint16_t *gain,
                          const uint32_t *port_ptr, const uint32_t *members, uint32_t n_members, uint32_t C, uint32_t P, uint32_t F, uint32_t n,
                          int16_t *out, igdsp_frame_stats *stats, const ConfRoute &r)
{
    return ConfArgs{g711, codec, pcm, len, gain, port_ptr, members, n_members, C, P, F, n, out, stats, r.vec_in, r.vec_out};
}

hipError_t launch_conf_mix(const LaunchCfg &cfg, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm, const uint16_t *len,
                           const uint16_t *gain, const uint32_t *port_ptr, const uint32_t *members, uint32_t n_members, uint32_t C, uint32_t P,
                           uint32_t F, uint32_t n, int16_t *out, igdsp_frame_stats *stats, bool yardstick, hipStream_t s)
{
    const ConfRoute r = conf_route(P, F, n, pcm != nullptr, reinterpret_cast<uintptr_t>(pcm ? (const void *)pcm : (const void *)g711),
                                   reinterpret_cast<uintptr_t>(out), (uint32_t)cfg.compute_units);
    if (r.grid == 0) return hipSuccess;
    const ConfArgs a = conf_args(g711, codec, pcm, len, gain, port_ptr, members, n_members, C, P, F, n, out, stats, r);
    with_key(Keys<kConfG711, kConfPcm>{}, r.form, [&](auto IN) { with_bool(yardstick, [&](auto Y) {
        hipLaunchKernelGGL((k_conf_mix<IN, Y>), dim3(r.grid), dim3(r.threads), 0, s, a); }); });
    return hipGetLastError();
}

}  // namespace igdsp
