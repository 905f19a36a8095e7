// igdsp_group.h — what the kernels that walk a CSR of groups over igdsp_depayload's info records share (igdsp_bss_select in
// igdsp_k_bss.hip, igdsp_ptt_arbitrate in igdsp_k_ptt.hip): an info record as two words and the stored-word rule, a wave's group
// ranges, the slot -> (group, position) map of the gather, the gather's frame loop, and the emit of the selected frames at their Q7
// level.  A wave owns up to kGrpGroups consecutive groups; its LDS selection table is [frames][kGrpGroups] (channel + 1, 0 = none).
#pragma once
#include "igdsp_q7.h"

namespace igdsp {

constexpr uint32_t kGrpGroups = 16;                       // groups per wave at most (decision lanes), the selection table's row
constexpr uint32_t kGrpU = 8;                             // loads of a lane in flight together
constexpr uint32_t kGrpNoChan = 0xFFFFFFFFu;
static_assert(kGrpGroups == kBssGroups && kGrpGroups == kPttGroups && kGrpU == kBssU && kGrpU == kPttU, "one geometry for both stages");

// info[f][c] as two words: x = ed137, y = payload_len | pt << 16 | flags << 24 (igdsp_rtp_info is 4-byte aligned)
__device__ __forceinline__ uint2 grp_info(const igdsp_rtp_info *info, uint32_t C, uint32_t f, uint32_t c)
{
    const uint32_t *p = reinterpret_cast<const uint32_t *>(info + ((uint64_t)f * C + c));
    return make_uint2(p[0], p[1]);
}

// the frame stores its word on the channel (transport_rtp_cb: PT 0, 8, 18, 123 and not a runt)
__device__ __forceinline__ bool grp_stores(uint2 r)
{
    const uint32_t pt = (r.y >> 16) & 0xFFu;
    return ((r.y >> 24) & IGDSP_RTP_RUNT) == 0u && (pt == 0u || pt == 8u || pt == 18u || pt == 123u);
}

// The slot ranges of the wave's ng groups g0 .. g0 + ng - 1, clamped: lane i < ng gets its group's [b, e) and the group's first slot
// in the wave's concatenation (myoff); every lane gets V, the wave's slot count.  gbeg / goff (per wave, [kGrpGroups]) receive b and
// myoff for grp_locate; the caller fences before reading them.
__device__ __forceinline__ void grp_ranges(const uint32_t *group_ptr, uint32_t n_members, uint64_t g0, uint32_t ng, uint32_t lane,
                                           uint32_t *gbeg, uint32_t *goff, uint32_t &b, uint32_t &e, uint32_t &myoff, uint32_t &V)
{
    b = 0; e = 0;
    if (lane < ng) {
        b = min(group_ptr[g0 + lane], n_members);
        e = min(group_ptr[g0 + lane + 1u], n_members);
        if (e < b) e = b;                                                  // a descending group_ptr: empty group
    }
    V = 0; myoff = 0;
    for (uint32_t i = 0; i < ng; ++i) {
        if (lane == i) myoff = V;
        V += (uint32_t)__builtin_amdgcn_readlane((int)(e - b), (int)i);
    }
    if (lane < ng) { gbeg[lane] = b; goff[lane] = myoff; }
}

// slot v of the wave's concatenation: its group (local index) and position; returns the member slot k
__device__ __forceinline__ uint32_t grp_locate(const uint32_t *gbeg, const uint32_t *goff, uint32_t ng, uint32_t v, uint32_t &gl, uint32_t &pos)
{
    gl = 0;
    for (uint32_t i = 1; i < ng; ++i) if (goff[i] <= v) gl = i;           // the last group starting at or before v (empty ones skipped)
    pos = v - goff[gl];
    return gbeg[gl] + pos;
}

// The gather's frame loop: channel c's info records of frames f0 + ta .. f0 + tb - 1, kGrpU loads in flight, body(t, r) in frame
// order.  A lane without a channel (c == kGrpNoChan) and the frames past tb get the missing-frame record.
template <class Body>
__device__ __forceinline__ void grp_frames(const igdsp_rtp_info *info, uint32_t C, uint32_t f0, uint32_t ta, uint32_t tb, uint32_t c, Body &&body)
{
    for (uint32_t t0 = ta; t0 < tb; t0 += kGrpU) {
        uint2 r[kGrpU];
#pragma unroll
        for (uint32_t u = 0; u < kGrpU; ++u)
            r[u] = (c != kGrpNoChan && t0 + u < tb) ? grp_info(info, C, f0 + t0 + u, c) : make_uint2(0u, (uint32_t)IGDSP_RTP_RUNT << 24);
#pragma unroll
        for (uint32_t u = 0; u < kGrpU; ++u) body(t0 + u, r[u]);
    }
}

// The emit: the whole wave takes the (frame, group) items of the part in turn: metadata one item per lane, handed over with
// v_readlane; kGrpU frame loads in flight; decode, the Q7 level and the record as igdsp_conf_mix does them for a one-member port
// (igdsp_q7.h).  selw: the wave's selection table [pf][kGrpGroups].  a: the stage's argument block (info-free fields: g711, codec, pcm,
// len, gain, C, G, n, f0, sel, out, stats, vec_in, vec_out).  IN: kConfG711, kConfPcm, or kBssNone (sel only).  COPY: the same bytes,
// undecoded.
template <int IN, bool COPY, class Args>
__device__ __forceinline__ void grp_emit(const Args &a, const uint2 *lut, const uint32_t *selw, uint32_t pf, uint32_t ng, uint64_t g0, uint32_t lane)
{
    const uint32_t n_items = pf * ng, off = (lane & 31u) * 8u, n = a.n;
    for (uint32_t j0 = 0; j0 < n_items; j0 += 64u) {
        const uint32_t cnt = min(n_items - j0, 64u);
        // one item per lane: tg = t << 16 | group, cs = the selection (channel + 1, 0 = none), meta = gain | len << 16 | A-law << 25
        uint32_t tg = 0, cs = 0, meta = 0;
        if (lane < cnt) {
            const uint32_t j = j0 + lane, t = j / ng, gl = j - t * ng;
            tg = t << 16 | gl;
            cs = selw[t * kGrpGroups + gl];
            if (a.sel != nullptr) a.sel[(uint64_t)(a.f0 + t) * a.G + g0 + gl] = (int32_t)(cs - 1u);
            if (IN != kBssNone && cs != 0u) {
                const uint32_t c = cs - 1u;
                const uint32_t l = a.len ? min((uint32_t)a.len[(uint64_t)(a.f0 + t) * a.C + c], n) : n;
                const uint32_t g = a.gain ? (uint32_t)a.gain[c] : 256u;
                const uint32_t law = (IN == kConfG711 && a.codec[c] == IGDSP_PT_PCMA) ? 1u : 0u;
                meta = g | l << 16 | law << 25;
            }
        }
        if (IN == kBssNone) continue;
#pragma nounroll
        for (uint32_t k0 = 0; k0 < cnt; k0 += kGrpU) {
            uint2 v[kGrpU];
#pragma unroll
            for (uint32_t u = 0; u < kGrpU; ++u) {
                const uint32_t idx = min(k0 + u, 63u);
                const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)meta, (int)idx);
                const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)cs, (int)idx);
                const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)tg, (int)idx) >> 16;
                const bool load = k0 + u < cnt && s != 0u && (m & 0xFFFFu) != 0u && ((m >> 16) & 0x1FFu) != 0u;
                v[u] = load ? q7_load<IN>(a.g711, a.pcm, n, a.vec_in, (uint64_t)(a.f0 + t) * a.C + (s - 1u), lane) : make_uint2(0u, 0u);
            }
#pragma unroll
            for (uint32_t u = 0; u < kGrpU; ++u) {
                if (k0 + u >= cnt) break;                                  // wave-uniform
                const uint32_t idx = k0 + u;
                const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)meta, (int)idx);
                const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)cs, (int)idx);
                const uint32_t tgi = (uint32_t)__builtin_amdgcn_readlane((int)tg, (int)idx);
                const uint64_t item = (uint64_t)(a.f0 + (tgi >> 16)) * a.G + g0 + (tgi & 0xFFFFu);
                if (COPY) {                                                // the same bytes, undecoded
                    const uint32_t b0 = 4u * lane;
                    if (a.out != nullptr && b0 < n) {
                        int16_t *dst = a.out + item * n + b0;
                        const uint2 x = IN == kConfG711 ? make_uint2(v[u].x, v[u].x) : v[u];
                        if (a.vec_out) *reinterpret_cast<uint2 *>(dst) = x;
                        else for (uint32_t k = 0; k < 4u && b0 + k < n; ++k) dst[k] = (int16_t)((k < 2u ? x.x : x.y) >> (16u * (k & 1u)));
                    }
                    if (a.stats != nullptr && lane == 0u) {
                        igdsp_frame_stats st;
                        st.sumsq = ((uint64_t)v[u].y << 32) | v[u].x; st.rms = 0.f; st.peak = (uint16_t)m; st.byte_mean = 0; st.flags = (uint8_t)s;
                        a.stats[item] = st;
                    }
                    continue;
                }
                const uint32_t g = m & 0xFFFFu, l = (m >> 16) & 0x1FFu, law80 = (m >> 25) ? 0x80808080u : 0u;
                int32_t o[4];
                uint32_t sat = 0, peak = 0;
                uint64_t sq = 0;
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    uint32_t ax, neg;
                    q7_sample<IN>(lut, v[u], law80, off, k, ax, neg);
                    IGDSP_Q7_LEVEL(q, ax, neg, g, 4u * lane + k, l, sat);        // 0 past len (and past n)
                    if (s == 0u) q = 0u;                                           // nothing selected
                    o[k] = neg ? -(int32_t)q : (int32_t)q;
                    sq += (uint64_t)q * q;
                    peak = max(peak, q);
                }
                q7_store(a.out, a.stats, item, n, a.vec_out, lane, o, s == 0u || l == 0u, sat, sq, peak);
            }
        }
    }
}

}  // namespace igdsp
