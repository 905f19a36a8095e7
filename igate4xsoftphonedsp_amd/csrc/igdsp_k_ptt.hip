// igdsp_k_ptt.hip — PTT priority arbitration (igdsp_ptt_arbitrate): the CLIENT-mode block of the reference's checkEvents
// (roip_ed137.cpp:6124-6231), batched over frames and groups.  Semantics: include/igdsp.h, section "PTT priority arbitration";
// independent restatements: tests/ptt_model.py (holder form and the literal per-leg volumes) and PttArbiter in host/igdsp_host.cpp.
//
// Shape (route: ptt_route; the gather, the group ranges and the emit are igdsp_group.h's, shared with igdsp_k_bss.hip).  A wave owns
// gpw consecutive groups for the frames of one part (<= kPttPart frames).  Unlike the receiver vote the arbitration depends on member
// order within a tick, so the two halves are split by what they depend on:
//   A. step: a member slot per lane (64-slot chunks), sequential over frames: the stored word, the debounce and the press state
//      depend on the slot alone.  The lane leaves an op per (frame, slot) in LDS: the effective PTT type, a press or release event,
//      and the PTT id of the stored word.  Every member is one of "raise to p", "reset to 0" or identity.
//   B. decide: lanes 0 .. gpw - 1, one group each, walk their members in order, frame by frame, over the ops (four LDS reads in
//      flight), write the tick records and leave the selection (channel + 1, 0 = none) in LDS.
//   C. emit: grp_emit, as igdsp_bss_select.
// The ops of a wave are kPttOps entries: a window of W slots x kPttOps / W frames, so A and B alternate in passes; every pass steps
// its slots again from the part's first frame (the info records are 8 bytes a frame and sit in L2).  The slots are only read here.
// After each part k_ptt_slots steps every slot through the part once more and stores it (a thread per slot), so slots shared by two
// groups of a bad table never race.
#include "igdsp_group.h"

namespace igdsp {

static_assert(kPttWaves * (kPttPart * kPttGroups * 4 + kPttOps * 2) <= 64 * 1024, "selections and ops fit next to the 64 KiB LUT");
static_assert(kPttPart <= 0x8000u && kPttOps % 64u == 0u && kPttOps >= 64u, "item packing of the emit; windows are whole chunks");

struct PttArgs {
    const igdsp_rtp_info *info;
    const uint8_t *g711;
    const uint8_t *codec;
    const int16_t *pcm;
    const uint16_t *len;
    const uint16_t *gain;                  // nullptr: 256
    const uint32_t *group_ptr;
    const uint32_t *members;
    const uint8_t *rxonly;
    uint32_t n_members, C, G, n, release_frames, gpw;
    uint32_t f0, pf;                       // this part: frames f0 .. f0 + pf - 1
    igdsp_ptt_state *state;
    const igdsp_ptt_slot *slots;
    int32_t *sel;
    igdsp_ptt_tick *tick;
    uint8_t *ctl_out;
    int16_t *out;
    igdsp_frame_stats *stats;
    uint32_t vec_in, vec_out;
};

// an op: bits 0-2 the effective PTT type, then the events, bits 8-13 the PTT id of the slot's stored word
constexpr uint32_t kPttOpRelease = 8u, kPttOpPress = 16u;

struct PttSlot { uint32_t word, last_tx, cnt, pressed, reserved; };

__device__ __forceinline__ PttSlot ptt_slot_load(const igdsp_ptt_slot *p)
{
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
    const uint32_t x = q[1];
    return PttSlot{q[0], x & 0xFFu, (x >> 8) & 0xFFu, (x >> 16) & 0xFFu, x >> 24};
}

// one tick of a slot with a call (steps 1, 3, 4 and the slot's half of step 6): returns the op without the id
__device__ __forceinline__ uint32_t ptt_step(PttSlot &s, uint2 r, uint32_t rxonly, uint32_t rf)
{
    if (grp_stores(r)) s.word = r.x;
    uint32_t p = rxonly != 0u ? 0u : IGDSP_ED137_PTT_TYPE(s.word);
    if (p != s.last_tx) {
        if (p == 0u) {
            s.cnt = min(s.cnt + 1u, 255u);
            if (s.cnt < rf) p = 1u;                                        // the release is bridged: with type 1, not the old type
        }
    } else {
        s.cnt = 0u;
    }
    s.last_tx = p;
    uint32_t op = p;
    if (p != 0u && s.pressed == 0u) { s.pressed = 1u; op |= kPttOpPress; }
    else if (p == 0u && s.pressed != 0u) { s.pressed = 0u; op |= kPttOpRelease; }
    return op;
}

template <int IN, bool COPY>
__global__ __launch_bounds__(kPttWaves * 64) void k_ptt_arbitrate(const PttArgs a)
{
    constexpr bool kLut = IN == kConfG711 && !COPY;
    __shared__ __attribute__((aligned(16))) uint2 lut[kLut ? kLutEntries : 1];
    __shared__ uint32_t selt[kPttWaves][kPttPart][kPttGroups];            // the selection (channel + 1, 0 = none)
    __shared__ uint16_t ops[kPttWaves][kPttOps];                          // [frames of the pass][W]
    __shared__ uint32_t gbeg[kPttWaves][kPttGroups], goff[kPttWaves][kPttGroups];
    if (kLut) fill_lut(lut);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t g0 = ((uint64_t)blockIdx.x * kPttWaves + w) * a.gpw;
    __syncthreads();                                                       // the LUT; from here on each wave works alone
    if (g0 >= a.G) return;
    const uint32_t ng = (uint32_t)min((uint64_t)a.gpw, (uint64_t)a.G - g0);
    const uint32_t pf = a.pf;
    uint32_t *sw = &selt[w][0][0];
    uint16_t *ow = &ops[w][0];

    // the groups' slot ranges, clamped; lane i < ng holds group g0 + i
    uint32_t b, e, V, myoff;
    grp_ranges(a.group_ptr, a.n_members, g0, ng, lane, gbeg[w], goff[w], b, e, myoff, V);
    const uint32_t m = e - b, end = myoff + m;

    // the groups' state, read defensively; hc: the holder's channel
    uint32_t level = 0, holder = 0, takeovers = 0, reserved = 0, hc = kGrpNoChan, pid = 0, fl = 0;
    if (lane < ng && !COPY) {
        const igdsp_ptt_state st = a.state[g0 + lane];
        level = st.level & 7u; holder = st.holder <= m ? st.holder : 0u; takeovers = st.takeovers; reserved = st.reserved;
        if (holder != 0u) hc = a.members[b + holder - 1u];
    }
    wave_lds_fence();

    const uint32_t W = min((max(V, 1u) + 63u) & ~63u, kPttOps);            // slots per window
    const uint32_t sub = min(pf, kPttOps / W);                             // frames per pass
    const uint32_t rf = a.release_frames;
    uint32_t fold = 0;
    for (uint32_t t0 = 0; t0 < pf; t0 += sub) {
        const uint32_t ns = min(sub, pf - t0);
        uint32_t s0 = 0;
        do {                                                               // the windows of a wave of more than kPttOps slots (ns == 1)
            const uint32_t s1 = min(V, s0 + W);
            // A. step the window's slots from the part's first frame; ops of frames t0 .. t0 + ns - 1
            for (uint32_t v0 = s0; v0 < s1; v0 += 64u) {
                const uint32_t v = v0 + lane, idx = v - s0;
                uint32_t c = kGrpNoChan, rx = 0;
                PttSlot s{0u, 0u, 0u, 0u, 0u};
                if (v < s1) {
                    uint32_t gl, pos;
                    const uint32_t k = grp_locate(gbeg[w], goff[w], ng, v, gl, pos);
                    c = a.members[k];
                    s = ptt_slot_load(a.slots + k);
                    if (c >= a.C) {                                        // no call: identity, with the untouched word's id
                        c = kGrpNoChan;
                        if (!COPY) for (uint32_t t = 0; t < ns; ++t) ow[t * W + idx] = (uint16_t)(IGDSP_ED137_PTT_ID(s.word) << 8);
                    } else if (a.rxonly != nullptr) {
                        rx = a.rxonly[c];
                    }
                }
                if (__builtin_amdgcn_ballot_w64(c != kGrpNoChan) == 0u) continue;
                const uint32_t t1 = t0 + ns;
                grp_frames(a.info, a.C, a.f0, 0u, t1, c, [&](uint32_t t, uint2 r) {
                    if (COPY) { fold ^= r.x ^ r.y; return; }
                    if (c == kGrpNoChan || t >= t1) return;
                    const uint32_t op = ptt_step(s, r, rx, rf);
                    if (t >= t0) ow[(t - t0) * W + idx] = (uint16_t)(op | IGDSP_ED137_PTT_ID(s.word) << 8);
                });
            }
            wave_lds_fence();

            // B. decide: the lane's group's members of this window, in order
            if (lane < ng) {
                if (COPY) {
                    const uint32_t c0 = e > b ? a.members[b] : kGrpNoChan;
                    if (s0 == 0u) for (uint32_t t = 0; t < ns; ++t) sw[(t0 + t) * kPttGroups + lane] = c0 < a.C ? c0 + 1u : 0u;
                } else {
                    const uint32_t lo = max(myoff, s0), hi = min(end, s1);
                    const bool last = end <= s0 + W && (s0 == 0u || end > s0);   // the group ends in this window: the tick is complete
                    for (uint32_t t = 0; t < ns; ++t) {
                        const uint16_t *row = ow + t * W;
                        for (uint32_t v = lo; v < hi; v += 4u) {
                            uint32_t o4[4];
#pragma unroll
                            for (uint32_t u = 0; u < 4u; ++u) o4[u] = row[min(v + u, hi - 1u) - s0];
#pragma unroll
                            for (uint32_t u = 0; u < 4u; ++u) {
                                if (v + u >= hi) break;
                                const uint32_t pos = v + u - myoff, op = o4[u], p = op & 7u;
                                if (p > level) {                           // step 5
                                    level = p; holder = pos + 1u; ++takeovers; fl |= IGDSP_PTT_TAKEOVER;
                                    hc = a.members[b + pos];
                                }
                                if (p != 0u) fl |= IGDSP_PTT_ON;
                                if (op & kPttOpPress) fl |= IGDSP_PTT_PRESS;
                                if (op & kPttOpRelease) {                  // step 6: any pressed leg's release zeroes the level
                                    fl |= IGDSP_PTT_RELEASE;
                                    if (holder == pos + 1u) holder = 0u;
                                    level = 0u;
                                }
                                if (holder == pos + 1u) pid = op >> 8;
                            }
                        }
                        if (!last) continue;
                        const uint32_t tt = t0 + t;
                        const uint32_t cs = (holder != 0u && hc < a.C) ? hc + 1u : 0u;
                        const uint32_t ctl = IGDSP_TX_CTL_SET | ((fl & IGDSP_PTT_ON) ? IGDSP_TX_CTL_PTT : 0u);
                        const uint64_t item = (uint64_t)(a.f0 + tt) * a.G + g0 + lane;
                        sw[tt * kPttGroups + lane] = cs;
                        if (a.tick != nullptr) {
                            uint32_t *q = reinterpret_cast<uint32_t *>(a.tick + item);
                            q[0] = cs - 1u;
                            q[1] = level | (holder != 0u ? pid : 0u) << 8 | fl << 16 | ctl << 24;
                        }
                        if (a.ctl_out != nullptr) a.ctl_out[item] = (uint8_t)ctl;
                        fl = 0u;
                    }
                }
            }
            wave_lds_fence();
            s0 += W;
        } while (s0 < V);
    }
    if (COPY && fold == 0x9E3779B9u) sw[0] = 0u;                           // keeps the yardstick's loads
    if (lane < ng && !COPY) {
        igdsp_ptt_state st;
        st.level = level; st.holder = holder; st.takeovers = takeovers; st.reserved = reserved;
        a.state[g0 + lane] = st;
    }
    wave_lds_fence();

    // C. emit
    grp_emit<IN, COPY>(a, lut, sw, pf, ng, g0, lane);
}

// every member slot with a call, stepped through frames f0 .. f0 + pf - 1 and stored (a slot whose member is >= C is left untouched)
__global__ __launch_bounds__(kPttSlotsThreads) void k_ptt_slots(const igdsp_rtp_info *info, const uint32_t *members, const uint8_t *rxonly,
                                                               uint32_t n_members, uint32_t C, uint32_t f0, uint32_t pf, uint32_t rf,
                                                               igdsp_ptt_slot *slots)
{
    const uint32_t k = blockIdx.x * kPttSlotsThreads + threadIdx.x;
    if (k >= n_members) return;
    const uint32_t c = members[k];
    if (c >= C) return;
    PttSlot s = ptt_slot_load(slots + k);
    const uint32_t rx = rxonly != nullptr ? rxonly[c] : 0u;
    grp_frames(info, C, f0, 0u, pf, c, [&](uint32_t t, uint2 r) {
        if (t < pf) ptt_step(s, r, rx, rf);
    });
    uint32_t *q = reinterpret_cast<uint32_t *>(slots + k);
    q[0] = s.word;
    q[1] = s.last_tx | s.cnt << 8 | s.pressed << 16 | s.reserved << 24;
}

hipError_t launch_ptt_arbitrate(const LaunchCfg &, const igdsp_rtp_info *info, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm,
                                const uint16_t *len, const uint16_t *gain, const uint32_t *group_ptr, const uint32_t *members,
                                uint32_t n_members, const uint8_t *rxonly, uint32_t C, uint32_t G, uint32_t F, uint32_t n,
                                uint32_t release_frames, igdsp_ptt_state *state, igdsp_ptt_slot *slots, int32_t *sel, igdsp_ptt_tick *tick,
                                uint8_t *ctl_out, int16_t *out, igdsp_frame_stats *stats, bool yardstick, hipStream_t s)
{
    const int form = g711 ? kConfG711 : (pcm ? kConfPcm : kBssNone);
    const PttRoute r = ptt_route(G, F, n, n_members, form, reinterpret_cast<uintptr_t>(pcm ? (const void *)pcm : (const void *)g711),
                                 reinterpret_cast<uintptr_t>(out));
    if (r.grid == 0) return hipSuccess;
    const uint32_t rf = release_frames ? release_frames : (uint32_t)IGDSP_PTT_RELEASE_FRAMES;
    PttArgs a{info, g711, codec, pcm, len, gain, group_ptr, members, rxonly, n_members, C, G, n, rf, r.gpw, 0u, 0u, state, slots, sel, tick,
              ctl_out, out, stats, r.vec_in, r.vec_out};
    for (uint32_t p = 0; p < r.parts; ++p) {
        a.f0 = p * kPttPart;
        a.pf = std::min(kPttPart, F - a.f0);
        with_key(Keys<kConfG711, kConfPcm, kBssNone>{}, r.form, [&](auto IN) { with_bool(yardstick, [&](auto Y) {
            hipLaunchKernelGGL((k_ptt_arbitrate<IN, Y>), dim3(r.grid), dim3(r.threads), 0, s, a); }); });
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        if (r.slots_grid) {
            hipLaunchKernelGGL(k_ptt_slots, dim3(r.slots_grid), dim3(kPttSlotsThreads), 0, s, info, members, rxonly, n_members, C, a.f0, a.pf, rf, slots);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace igdsp
