// igdsp_k_link.hip — R2S link supervision and the device event list (igdsp_link_watch): the body of the reference's 40 ms timer
// (detectR2SPacketAndReconn, roip_ed137.cpp:1764-1780, :2009-2040) and the rtpAudio edge of transport_rtp_cb (TransportAdapter.cpp:
// 286-315), batched over ticks and channels.  Semantics: include/igdsp.h, section "R2S link supervision"; independent restatements:
// tests/link_model.py (a scalar walk and a numpy form) and LinkWatch in host/igdsp_host.cpp.
//
// Shape (route: link_route).  The state machine is sequential per channel and the list is tick-major, so a lane owns a channel and
// walks the arrival slots of one part (<= kLinkPart ticks) in order, kLinkU record loads in flight (8 bytes a lane, coalesced over the
// wave's 64 consecutive channels).  Without a list one pass (kLinkSingle) stores the state and the kind bytes.  With a list:
//   A. count (kLinkCount): the walk; per tick the wave's event lanes are a ballot, lane 0 leaves its popcount at counts[t][wave];
//   B. k_link_scan: one block turns the counts into exclusive offsets in place, in tick-major order, on top of the offset the earlier
//      parts of the launch reached (d_work's header), and after the last part writes the two totals;
//   C. write (kLinkWrite): the walk again from the same state, now storing the state, the kind bytes and each event at its wave's
//      offset plus the lane's rank among the wave's event lanes (events past event_cap are dropped).
// Replaying avoids a dense per-(tick, channel) stash; its cost is reading the inputs twice.  The hand-offs are kernel boundaries on the
// stream, nothing is read back within a kernel, and everything is written with vector stores.
#include "igdsp_device.h"

namespace igdsp {

static_assert(kLinkPart * IGDSP_STAGE_DEPTH <= 0x10000u, "arrival slots of a part are counted in 32 bits with room to spare");
static_assert(kLinkScanThreads == 1024u, "k_link_scan's block scan is written for 16 waves");

struct LinkArgs {
    const igdsp_rtp_info *info;
    const uint16_t *sizes;                 // nullptr: every slot holds a packet
    const uint8_t *up;                     // nullptr: every call is up
    const uint16_t *period;                // nullptr: IGDSP_LINK_R2S_PERIOD_MS
    uint32_t C, S, W;                      // channels, slots per tick, waves (the counts' row)
    uint32_t f0, pf;                       // this part: ticks f0 .. f0 + pf - 1
    uint64_t now0;                         // now(f0)
    uint32_t tick_ms, miss, mask;
    igdsp_link_state *state;
    uint8_t *kind;
    igdsp_link_event *events;
    uint32_t cap;
    const uint32_t *offs;                  // kLinkWrite: the scanned offsets [pf][W]
    uint32_t *counts;                      // kLinkCount: [pf][W]
};

// info[a][c] as two words: x = ed137, y = payload_len | pt << 16 | flags << 24; igdsp_rtp_info is 4-byte aligned, and one 8-byte load
// serves a record at that alignment
struct __attribute__((aligned(4))) LinkRec { uint32_t x, y; };
static_assert(sizeof(LinkRec) == sizeof(igdsp_rtp_info), "a record is two words");

// the tick's end: step 3, then the outputs
template <bool COPY, int PASS>
__device__ __forceinline__ void link_tick_end(const LinkArgs &a, bool valid, bool down, uint32_t lane, uint32_t w, uint32_t c, uint32_t t, uint64_t now,
                                              int64_t late, uint32_t fold, uint64_t last, uint32_t &alarms, uint32_t &count, uint32_t &flags,
                                              uint32_t &kind, uint32_t word)
{
    if (COPY) {
        kind = fold == 0x9E3779B9u ? 1u : 0u;                              // keeps the yardstick's loads; no event in practice
    } else if (down) {
        flags &= ~(uint32_t)IGDSP_LINK_UP;
    } else {
        const int64_t diff = (int64_t)(now - last);
        if (diff > late) {
            kind |= IGDSP_LINK_LATE;
            if (count == a.miss - 1u) { kind |= IGDSP_LINK_MISSING; flags |= IGDSP_LINK_ALARMED; ++alarms; }
            count = min(count + 1u, 65535u);
        } else {
            if (count > 0u) kind |= IGDSP_LINK_RECOVERED;
            count = 0u;
            flags &= ~(uint32_t)IGDSP_LINK_ALARMED;
        }
    }
    if (PASS != kLinkCount && a.kind != nullptr && valid) a.kind[(uint64_t)(a.f0 + t) * a.C + c] = (uint8_t)kind;
    if (PASS == kLinkSingle) return;
    const bool ev = valid && (kind & a.mask) != 0u;
    const uint64_t bal = __builtin_amdgcn_ballot_w64(ev);
    if (PASS == kLinkCount) {
        if (lane == 0u) a.counts[(uint64_t)t * a.W + w] = (uint32_t)__popcll(bal);
    } else if (bal != 0u) {                                                // wave-uniform, and rare in a healthy system
        const uint32_t off = a.offs[(uint64_t)t * a.W + w];
        const uint32_t idx = off + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (ev && idx < a.cap) {
            uint32_t *q = reinterpret_cast<uint32_t *>(a.events + idx);
            q[0] = c; q[1] = a.f0 + t; q[2] = word; q[3] = count | kind << 16;
        }
    }
}

template <bool COPY, int PASS, bool SIZES>
__global__ __launch_bounds__(kLinkWaves * 64) void k_link_watch(const LinkArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t c64 = (uint64_t)blockIdx.x * (kLinkWaves * 64) + threadIdx.x;
    const uint32_t w = (uint32_t)(c64 >> 6);
    if (w >= a.W) return;                                                  // wave-uniform: the block's waves past the last channel
    const bool valid = c64 < a.C;
    const uint32_t c = valid ? (uint32_t)c64 : a.C - 1u;                   // lanes past the end load the last channel and store nothing

    // the channel's state as four words: last_ms, alarms, count | flags << 16 | reserved << 24
    const uint2 *sp = reinterpret_cast<const uint2 *>(a.state + c);
    const uint2 s0 = sp[0], s1 = sp[1];
    uint64_t last = (uint64_t)s0.y << 32 | s0.x;
    uint32_t alarms = s1.x, count = s1.y & 0xFFFFu, flags = (s1.y >> 16) & 0xFFu;
    const uint32_t reserved = s1.y >> 24;
    const bool down = a.up != nullptr && a.up[c] == 0u;
    const int64_t late = 3 * (int64_t)(a.period != nullptr ? (uint32_t)a.period[c] : (uint32_t)IGDSP_LINK_R2S_PERIOD_MS);

    const uint32_t A = a.pf * a.S;
    const uint64_t row0 = (uint64_t)a.f0 * a.S;
    uint64_t now = a.now0;
    uint32_t t = 0, k = 0, kind = 0, word = 0, fold = 0;
    for (uint32_t a0 = 0; a0 < A; a0 += kLinkU) {
        uint2 r[kLinkU];
        uint32_t sz[kLinkU];
#pragma unroll
        for (uint32_t u = 0; u < kLinkU; ++u) {
            const uint64_t i = (row0 + min(a0 + u, A - 1u)) * a.C + c;
            const LinkRec x = reinterpret_cast<const LinkRec *>(a.info)[i];
            r[u] = make_uint2(x.x, x.y);
            sz[u] = SIZES ? (uint32_t)a.sizes[i] : 1u;
        }
#pragma unroll
        for (uint32_t u = 0; u < kLinkU; ++u) {
            const bool live = a0 + u < A;                                  // wave-uniform
            if (COPY) {
                if (live) fold ^= r[u].x ^ r[u].y ^ sz[u];
            } else if (live && !down) {
                if (k == 0u && (flags & IGDSP_LINK_UP) == 0u) {            // step 1: the call came up
                    last = now; count = 0u;
                    flags = (flags & ~(uint32_t)(IGDSP_LINK_AUDIO | IGDSP_LINK_ALARMED)) | IGDSP_LINK_UP;
                    kind |= IGDSP_LINK_CAME_UP;
                }
                if (sz[u] != 0u) {                                         // step 2: a packet
                    last = now;
                    const uint32_t pt = (r[u].y >> 16) & 0xFFu;
                    if (((r[u].y >> 24) & IGDSP_RTP_RUNT) == 0u) {
                        if (pt == IGDSP_PT_R2S) {
                            if (flags & IGDSP_LINK_AUDIO) { flags &= ~(uint32_t)IGDSP_LINK_AUDIO; kind |= IGDSP_LINK_AUDIO_OFF; word = r[u].x; }
                        } else if ((r[u].y & 0xFFFFu) < 1024u) {
                            if ((flags & IGDSP_LINK_AUDIO) == 0u) { flags |= IGDSP_LINK_AUDIO; kind |= IGDSP_LINK_AUDIO_ON; word = r[u].x; }
                        }
                    }
                }
            }
            if (live && ++k == a.S) {                                      // wave-uniform: the tick's end
                link_tick_end<COPY, PASS>(a, valid, down, lane, w, c, t, now, late, fold, last, alarms, count, flags, kind, word);
                k = 0u; ++t; now += a.tick_ms; kind = 0u; word = 0u;
            }
        }
    }
    if (PASS != kLinkCount && valid) {
        uint2 *dp = reinterpret_cast<uint2 *>(a.state + c);
        dp[0] = make_uint2((uint32_t)last, (uint32_t)(last >> 32));
        dp[1] = make_uint2(alarms, count | flags << 16 | reserved << 24);
    }
}

// counts[0 .. N) -> exclusive offsets in place, starting at head[0] (0 for the launch's first part); head[0] = the offset reached.
// After the last part: event_count = {total, min(total, cap)}.  One block; a thread scans a contiguous run of `per` counts.
__global__ __launch_bounds__(kLinkScanThreads) void k_link_scan(uint32_t *head, uint64_t N, uint32_t first, uint32_t last, uint32_t cap,
                                                               uint32_t *event_count)
{
    __shared__ uint32_t wsum[kLinkScanThreads / 64];
    uint32_t *cnt = head + kLinkWorkHead / 4;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t base = first ? 0u : head[0];
    const uint64_t per = (((N + kLinkScanThreads - 1) / kLinkScanThreads) + 3u) & ~3ull;      // whole uint4s: cnt is 16-byte aligned
    const uint64_t b = min((uint64_t)tid * per, N), e = min(b + per, N);
    uint32_t sum = 0;
    uint64_t i = b;
    for (; i + 4u <= e; i += 4u) { const uint4 v = *reinterpret_cast<const uint4 *>(cnt + i); sum += v.x + v.y + v.z + v.w; }
    for (; i < e; ++i) sum += cnt[i];
    // the block's exclusive scan of the threads' sums: within the wave by shuffles, across the 16 waves through LDS
    uint32_t inc = sum;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63u) wsum[w] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t j = 0; j < kLinkScanThreads / 64; ++j) { const uint32_t x = wsum[j]; if (j < w) before += x; total += x; }
    uint32_t run = base + before + inc - sum;
    i = b;
    for (; i + 4u <= e; i += 4u) {
        uint4 *p = reinterpret_cast<uint4 *>(cnt + i);
        const uint4 v = *p;
        uint4 o;
        o.x = run; o.y = o.x + v.x; o.z = o.y + v.y; o.w = o.z + v.z; run = o.w + v.w;
        *p = o;
    }
    for (; i < e; ++i) { const uint32_t x = cnt[i]; cnt[i] = run; run += x; }
    __syncthreads();                                                       // every thread has read head[0]
    if (tid == 0u) {
        total += base;
        head[0] = total;
        if (last && event_count != nullptr) { event_count[0] = total; event_count[1] = min(total, cap); }
    }
}

hipError_t launch_link_watch(const LaunchCfg &, const igdsp_rtp_info *info, const uint16_t *sizes, const uint8_t *up, const uint16_t *period,
                             uint32_t C, uint32_t T, uint32_t S, uint64_t t0_ms, uint32_t tick_ms, uint32_t miss_ticks, uint32_t event_mask,
                             igdsp_link_state *state, uint8_t *kind, igdsp_link_event *events, uint32_t event_cap, uint32_t *event_count,
                             void *work, bool yardstick, hipStream_t s)
{
    const bool list = event_count != nullptr;
    const LinkRoute r = link_route(C, T, list);
    uint32_t *head = static_cast<uint32_t *>(work);
    if (r.grid == 0) {                                                     // nothing to do: the counts are 0
        if (list) hipLaunchKernelGGL(k_link_scan, dim3(1), dim3(kLinkScanThreads), 0, s, head, (uint64_t)0, 1u, 1u, event_cap, event_count);
        return hipGetLastError();
    }
    LinkArgs a{info, sizes, up, period, C, S, r.waves, 0u, 0u, 0ull, tick_ms, miss_ticks ? miss_ticks : (uint32_t)IGDSP_LINK_MISS_TICKS,
               event_mask ? event_mask : (uint32_t)IGDSP_LINK_EVENT_DEFAULT, state, kind, events, event_cap,
               list ? head + kLinkWorkHead / 4 : nullptr, list ? head + kLinkWorkHead / 4 : nullptr};
    auto walk = [&](int pass) {
        with_key(Keys<kLinkSingle, kLinkCount, kLinkWrite>{}, pass, [&](auto P) { with_bool(yardstick, [&](auto Y) { with_bool(sizes != nullptr, [&](auto Z) {
            hipLaunchKernelGGL((k_link_watch<Y, P, Z>), dim3(r.grid), dim3(r.threads), 0, s, a); }); }); });
        return hipGetLastError();
    };
    for (uint32_t p = 0; p < r.parts; ++p) {
        a.f0 = p * kLinkPart;
        a.pf = std::min(kLinkPart, T - a.f0);
        a.now0 = t0_ms + (uint64_t)a.f0 * tick_ms;
        if (!list) {
            if (hipError_t e = walk(kLinkSingle); e != hipSuccess) return e;
            continue;
        }
        if (hipError_t e = walk(kLinkCount); e != hipSuccess) return e;
        hipLaunchKernelGGL(k_link_scan, dim3(1), dim3(r.scan_threads), 0, s, head, (uint64_t)a.pf * r.waves, p == 0u ? 1u : 0u,
                           p + 1u == r.parts ? 1u : 0u, event_cap, event_count);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        if (hipError_t e = walk(kLinkWrite); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the event list behind a stage's dense records: count -> k_link_scan -> store (igdsp_internal.h)
template <class Rec, class Event>
hipError_t launch_event_list(ListPass<Rec, Event> count, ListPass<Rec, Event> store, const ListRoute &r, bool empty, const Rec *rec, uint32_t C,
                             uint32_t F, uint32_t mask, Event *events, uint32_t event_cap, uint32_t *event_count, void *work, hipStream_t s)
{
    const bool list = event_count != nullptr;
    uint32_t *head = static_cast<uint32_t *>(work), *counts = head + kLinkWorkHead / 4;
    if (empty) {                                                           // nothing to do: the counts are 0
        if (list) hipLaunchKernelGGL(k_link_scan, dim3(1), dim3(kLinkScanThreads), 0, s, head, (uint64_t)0, 1u, 1u, event_cap, event_count);
        return hipGetLastError();
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess || !list) return e;          // the stage's own kernel
    hipLaunchKernelGGL(count, dim3(r.list_grid), dim3(kListWaves * 64), 0, s, rec, C, F, r.waves, mask, counts, events, event_cap);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_link_scan, dim3(1), dim3(kLinkScanThreads), 0, s, head, (uint64_t)F * r.waves, 1u, 1u, event_cap, event_count);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(store, dim3(r.list_grid), dim3(kListWaves * 64), 0, s, rec, C, F, r.waves, mask, counts, events, event_cap);
    return hipGetLastError();
}
template hipError_t launch_event_list(ListPass<igdsp_tdet_rec, igdsp_tdet_event>, ListPass<igdsp_tdet_rec, igdsp_tdet_event>, const ListRoute &, bool,
                                      const igdsp_tdet_rec *, uint32_t, uint32_t, uint32_t, igdsp_tdet_event *, uint32_t, uint32_t *, void *, hipStream_t);
template hipError_t launch_event_list(ListPass<igdsp_vad_rec, igdsp_vad_event>, ListPass<igdsp_vad_rec, igdsp_vad_event>, const ListRoute &, bool,
                                      const igdsp_vad_rec *, uint32_t, uint32_t, uint32_t, igdsp_vad_event *, uint32_t, uint32_t *, void *, hipStream_t);

}  // namespace igdsp
