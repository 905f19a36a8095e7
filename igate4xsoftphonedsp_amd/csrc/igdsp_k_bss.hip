// igdsp_k_bss.hip — best signal selection (igdsp_bss_select): the ED-137 receiver vote of the reference's checkEvents
// (roip_ed137.cpp:5985-6119), batched over frames and groups.  Semantics: include/igdsp.h, section "Best signal selection";
// independent restatements: tests/bss_model.py (any group size) and BssVoter in host/igdsp_host.cpp (the reference's four radios).
//
// Shape (route: bss_route).  A wave owns gpw consecutive groups for the frames of one part (<= kBssPart frames), in three phases:
//   A. gather: the groups' member slots, concatenated, one slot per lane (64-slot chunks), each lane reading its channel's info
//      records of the part's frames, kBssU at a time.  The lane replays the slot's stored word over the frames and folds every frame
//      where it is open into that frame's vote key of its group with an LDS max: key = (BSS + 1) << 24 | (0xFFFFFF - position), so
//      the maximum is the first member (in member order) of the highest BSS, and 0 means no member is open.
//   B. decide: lanes 0 .. gpw - 1, one group each, step the state machine over the part's frames from the keys.  Whether the voted
//      member is still open is read from its own info records (kBssU prefetched, reloaded after a vote changes the channel).  The
//      keys are replaced by the selection (channel + 1, 0 = none).
//   C. emit: the whole wave takes the (frame, group) items in turn: metadata one item per lane, handed over with v_readlane; kBssU
//      frame loads in flight; decode, the Q7 level and the record as igdsp_conf_mix does them for a one-member port (igdsp_q7.h).
// The stored words are only read here.  After each part k_bss_words writes every slot's last stored word (a thread per slot, a
// backward scan that usually stops at the part's last frame), so slots shared by two groups of a bad table never race.
#include "igdsp_group.h"

namespace igdsp {

static_assert(kBssWaves * kBssPart * kBssGroups * 4 <= 32 * 1024, "the vote keys fit next to the 64 KiB LUT");
static_assert(kBssPart <= 0x8000u && kBssGroups <= 0x10000u, "item packing of the emit phase");

struct BssArgs {
    const igdsp_rtp_info *info;
    const uint8_t *g711;
    const uint8_t *codec;
    const int16_t *pcm;
    const uint16_t *len;
    const uint16_t *gain;                  // nullptr: 256
    const uint32_t *group_ptr;
    const uint32_t *members;
    const uint8_t *mute;
    uint32_t n_members, C, G, n, vote_frames, gpw;
    uint32_t f0, pf;                       // this part: frames f0 .. f0 + pf - 1
    igdsp_bss_state *state;
    const uint32_t *words;
    int32_t *sel;
    int16_t *out;
    igdsp_frame_stats *stats;
    uint32_t vec_in, vec_out;
};

constexpr uint32_t kBssNoChan = kGrpNoChan;

__device__ __forceinline__ uint2 bss_info(const igdsp_rtp_info *info, uint32_t C, uint32_t f, uint32_t c) { return grp_info(info, C, f, c); }
__device__ __forceinline__ bool bss_stores(uint2 r) { return grp_stores(r); }
__device__ __forceinline__ uint32_t bss_squ(uint32_t w) { return IGDSP_ED137_SQU(w); }

template <int IN, bool COPY>
__global__ __launch_bounds__(kBssWaves * 64) void k_bss_select(const BssArgs a)
{
    constexpr bool kLut = IN == kConfG711 && !COPY;
    __shared__ __attribute__((aligned(16))) uint2 lut[kLut ? kLutEntries : 1];
    __shared__ uint32_t key[kBssWaves][kBssPart][kBssGroups];             // vote keys, then the selection (channel + 1, 0 = none)
    __shared__ uint32_t gbeg[kBssWaves][kBssGroups], goff[kBssWaves][kBssGroups], gmut[kBssWaves][kBssGroups];
    if (kLut) fill_lut(lut);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t g0 = ((uint64_t)blockIdx.x * kBssWaves + w) * a.gpw;
    __syncthreads();                                                       // the LUT; from here on each wave works alone
    if (g0 >= a.G) return;
    const uint32_t ng = (uint32_t)min((uint64_t)a.gpw, (uint64_t)a.G - g0);
    const uint32_t pf = a.pf;
    uint32_t *kw = &key[w][0][0];
    for (uint32_t i = lane; i < kBssPart * kBssGroups; i += 64u) kw[i] = 0u;

    // the groups' slot ranges, clamped; lane i < ng holds group g0 + i
    uint32_t b, e, V, myoff;                                               // V: slots of the wave; myoff: the lane's group's first one
    grp_ranges(a.group_ptr, a.n_members, g0, ng, lane, gbeg[w], goff[w], b, e, myoff, V);
    const uint32_t muted = (lane < ng && a.mute != nullptr && a.mute[g0 + lane] != 0u) ? 1u : 0u;
    if (lane < ng) gmut[w][lane] = muted;

    // the groups' state; the voted member's channel and the SQU bit of its stored word
    uint32_t count = 0, voted = 0, on = 0, votes = 0, cv = kBssNoChan, vw = 0;
    if (lane < ng && !COPY) {
        const igdsp_bss_state st = a.state[g0 + lane];
        count = st.count; voted = st.voted; on = st.on != 0u ? 1u : 0u; votes = st.votes;
        if (voted != 0u && voted <= e - b) {
            cv = a.members[b + voted - 1u];
            if (cv < a.C) vw = bss_squ(a.words[b + voted - 1u]);
        }
    }
    wave_lds_fence();

    // A. gather and fold
    uint32_t fold = 0;
    for (uint32_t v0 = 0; v0 < V; v0 += 64u) {
        const uint32_t v = v0 + lane;
        uint32_t c = kBssNoChan, word = 0, gl = 0, pos = 0;
        if (v < V) {
            const uint32_t k = grp_locate(gbeg[w], goff[w], ng, v, gl, pos);
            c = a.members[k];
            word = a.words[k];
            if (c >= a.C || gmut[w][gl] != 0u) c = kBssNoChan;             // never open: nothing to read
        }
        if (__builtin_amdgcn_ballot_w64(c != kBssNoChan) == 0u) continue;
        grp_frames(a.info, a.C, a.f0, 0u, pf, c, [&](uint32_t t, uint2 r) {
            if (COPY) { fold ^= r.x ^ r.y; return; }
            if (bss_stores(r)) word = r.x;
            if (c != kBssNoChan && t < pf && bss_squ(word))
                atomicMax(&key[w][t][gl], ((IGDSP_ED137_BSS(word) + 1u) << 24) | (0xFFFFFFu - pos));
        });
    }
    if (COPY && fold == 0x9E3779B9u) kw[0] = 0u;                           // keeps the yardstick's loads
    wave_lds_fence();

    // B. decide
    if (lane < ng) {
        if (COPY) {
            const uint32_t c0 = e > b ? a.members[b] : kBssNoChan;
            for (uint32_t t = 0; t < pf; ++t) key[w][t][lane] = c0 < a.C ? c0 + 1u : 0u;
        } else {
            const uint32_t vf = a.vote_frames;
            for (uint32_t t0 = 0; t0 < pf; t0 += kBssU) {
                const uint32_t pc = (voted != 0u && cv < a.C && muted == 0u) ? cv : kBssNoChan;
                uint2 pv[kBssU];
#pragma unroll
                for (uint32_t u = 0; u < kBssU; ++u)
                    pv[u] = (pc != kBssNoChan && t0 + u < pf) ? bss_info(a.info, a.C, a.f0 + t0 + u, pc) : make_uint2(0u, 0u);
#pragma unroll
                for (uint32_t u = 0; u < kBssU; ++u) {
                    const uint32_t t = t0 + u;
                    if (t >= pf) break;
                    if (voted != 0u) {                                     // step 1: the voted member closed (or names no member)
                        uint32_t rxv = 0;
                        if (cv < a.C && muted == 0u) {
                            const uint2 r = cv == pc ? pv[u] : bss_info(a.info, a.C, a.f0 + t, cv);
                            if (bss_stores(r)) vw = bss_squ(r.x);
                            rxv = vw;
                        }
                        if (rxv == 0u) { count = 0; on = 0; voted = 0; }
                    }
                    const uint32_t kk = key[w][t][lane];
                    if (kk != 0u) {                                        // step 2
                        if (count != 0xFFFFFFFFu) ++count;
                        if (count >= vf && on == 0u) {
                            const uint32_t pos = 0xFFFFFFu - (kk & 0xFFFFFFu);
                            on = 1; voted = pos + 1u; ++votes;
                            cv = a.members[b + pos];
                            vw = 1;
                        }
                    } else {                                               // step 3
                        count = 0; on = 0; voted = 0;
                    }
                    key[w][t][lane] = voted != 0u ? cv + 1u : 0u;
                }
            }
            igdsp_bss_state st;
            st.count = count; st.voted = voted; st.on = on; st.votes = votes;
            a.state[g0 + lane] = st;
        }
    }
    wave_lds_fence();

    // C. emit
    grp_emit<IN, COPY>(a, lut, kw, pf, ng, g0, lane);
}

// every member slot's last stored word of frames f0 .. f0 + pf - 1 (unchanged when no frame stores one, or the member is >= C)
__global__ __launch_bounds__(kBssWordsThreads) void k_bss_words(const igdsp_rtp_info *info, const uint32_t *members, uint32_t n_members,
                                                               uint32_t C, uint32_t f0, uint32_t pf, uint32_t *words)
{
    const uint32_t k = blockIdx.x * kBssWordsThreads + threadIdx.x;
    if (k >= n_members) return;
    const uint32_t c = members[k];
    if (c >= C) return;
    for (uint32_t t1 = pf; t1 > 0u; t1 = t1 > 4u ? t1 - 4u : 0u) {         // frames t1 - 1 down to t1 - 4
        uint2 r[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) r[u] = t1 > u ? bss_info(info, C, f0 + t1 - 1u - u, c) : make_uint2(0u, (uint32_t)IGDSP_RTP_RUNT << 24);
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u)
            if (bss_stores(r[u])) { words[k] = r[u].x; return; }
    }
}

hipError_t launch_bss_select(const LaunchCfg &, const igdsp_rtp_info *info, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm,
                             const uint16_t *len, const uint16_t *gain, const uint32_t *group_ptr, const uint32_t *members, uint32_t n_members,
                             const uint8_t *mute, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t vote_frames, igdsp_bss_state *state,
                             uint32_t *words, int32_t *sel, int16_t *out, igdsp_frame_stats *stats, bool yardstick, hipStream_t s)
{
    const int form = g711 ? kConfG711 : (pcm ? kConfPcm : kBssNone);
    const BssRoute r = bss_route(G, F, n, n_members, form, reinterpret_cast<uintptr_t>(pcm ? (const void *)pcm : (const void *)g711),
                                 reinterpret_cast<uintptr_t>(out));
    if (r.grid == 0) return hipSuccess;
    BssArgs a{info, g711, codec, pcm, len, gain, group_ptr, members, mute, n_members, C, G, n,
              vote_frames ? vote_frames : (uint32_t)IGDSP_BSS_VOTE_FRAMES, r.gpw, 0u, 0u, state, words, sel, out, stats, r.vec_in, r.vec_out};
    for (uint32_t p = 0; p < r.parts; ++p) {
        a.f0 = p * kBssPart;
        a.pf = std::min(kBssPart, F - a.f0);
        with_key(Keys<kConfG711, kConfPcm, kBssNone>{}, r.form, [&](auto IN) { with_bool(yardstick, [&](auto Y) {
            hipLaunchKernelGGL((k_bss_select<IN, Y>), dim3(r.grid), dim3(r.threads), 0, s, a); }); });
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        if (r.words_grid) {
            hipLaunchKernelGGL(k_bss_words, dim3(r.words_grid), dim3(kBssWordsThreads), 0, s, info, members, n_members, C, a.f0, a.pf, words);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace igdsp
