// igdsp_k_jb.hip — the jitter buffer (igdsp_jb_receive): RTP sequence validation (RFC 3550 A.1), interarrival jitter (A.8) and a fixed-
// delay playout ring per channel, between igdsp_depayload's packet arrays and one playout frame per channel and tick.  Semantics:
// include/igdsp.h, section "Jitter buffer"; independent restatement: tests/jb_model.py.
//
// Shape (route: jb_route).  A wave owns kJbCh consecutive channels for the ticks of one part (<= kJbPart), in four phases:
//   A. decide: lane ch < kJbCh walks channel c0 + ch's arrivals of the part in order (kJbU headers in flight: size, bytes 0-11, arrival
//      time), steps the state machine with the ring's tags in LDS (rtag, and rsrc: which arrival of this part a slot's packet is, or
//      kJbOld for a packet the ring already holds) and writes a descriptor per (tick, channel) into LDS: PLAYED from an arrival of the
//      part or from a ring slot, or IDLE / LOST with the tick's last keep-alive or nothing.
//   B. records: an item (tick, channel) per lane: the header is parsed again from the packet (parse_rtp_words, as igdsp_depayload does)
//      or read from the ring slot's record head; len / info / tick flag are written, len goes back into the descriptor.
//   C. rows: 16-byte pieces of the payload rows, a piece per lane: from the packet (masked past len), from the ring slot, or zeros.
//   D. ring: the packets of this part still in the ring are written into their slots (record head + masked payload), then every tag.
// A packet that arrives and is played within one part never touches the ring.  The state is read once and written once per part.
#include "igdsp_rtp.h"

namespace igdsp {

static_assert(IGDSP_JB_DEPTH == 16, "slot = seq & 15");
static_assert(kJbPart * IGDSP_STAGE_DEPTH <= 1024u, "arrival indices of a part are 10-bit in the descriptors");
static_assert(sizeof(igdsp_jb_state) == 80 && alignof(igdsp_jb_state) == 4, "igdsp_jb_state layout (capi.JB_STATE mirrors it)");

struct JbArgs {
    const uint8_t *packets;
    const uint16_t *sizes;                 // nullptr: every packet fills its slot
    const uint8_t *radio;
    const uint32_t *arrival;               // nullptr: no jitter
    uint32_t C, S, stride, n, delay, pieces, vec;
    uint32_t t0, pt;                       // this part: ticks t0 .. t0 + pt - 1
    igdsp_jb_state *state;
    uint8_t *ring;
    uint8_t *payload;
    uint16_t *len;
    igdsp_rtp_info *info;
    uint8_t *tick;
    uint8_t *pkt;
    uint64_t slot_bytes;
};

// descriptor: kind | arrival or slot << 2 | flag << 12 | radio << 14 | len << 16
enum : uint32_t { kJdNone = 0, kJdKa = 1, kJdArr = 2, kJdRing = 3 };
constexpr uint16_t kJbOld = 0xFFFFu;       // rsrc: the slot's packet is in the ring already
constexpr uint32_t kJbTag = 0x10000u;      // tag = kJbTag | seq, 0 = empty

__device__ __forceinline__ uint32_t jb_desc(uint32_t kind, uint32_t idx, uint32_t flag) { return kind | idx << 2 | flag << 12; }

__device__ __forceinline__ const uint8_t *jb_pkt(const JbArgs &a, uint32_t al, uint32_t c)
{
    return a.packets + ((uint64_t)(a.t0 * a.S + al) * a.C + c) * a.stride;
}
__device__ __forceinline__ uint32_t jb_size(const JbArgs &a, uint32_t al, uint32_t c)
{
    return a.sizes ? min((uint32_t)a.sizes[(uint64_t)(a.t0 * a.S + al) * a.C + c], a.stride) : a.stride;
}
__device__ __forceinline__ uint8_t *jb_slot(const JbArgs &a, uint32_t c, uint32_t s)
{
    return a.ring + (uint64_t)a.C * IGDSP_JB_DEPTH * 4u + ((uint64_t)c * IGDSP_JB_DEPTH + s) * a.slot_bytes;
}
// depayload of arrival al: the header parse
__device__ __forceinline__ FrameHdr jb_parse(const JbArgs &a, uint32_t al, uint32_t c, bool radio)
{
    return parse_rtp(jb_pkt(a, al, c), jb_size(a, al, c), radio ? 20u : 12u, radio, a.n);
}
// bytes [b0, b0 + 16) of arrival al's payload, zero past len; never reads past the packet's slot (as k_depayload16)
__device__ __forceinline__ uint4 jb_piece(const JbArgs &a, uint32_t al, uint32_t c, uint32_t hdr, uint32_t len, uint32_t b0)
{
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (len > b0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(jb_pkt(a, al, c) + hdr + b0);
        const uint32_t nb = min(len - b0, 16u);
        if (hdr + b0 + 16u <= a.stride) {
            struct __attribute__((packed, aligned(4))) Q { uint32_t a, b, c, d; };
            const Q qv = *reinterpret_cast<const Q *>(src);
            const uint32_t x[4] = {qv.a, qv.b, qv.c, qv.d};
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t keep = nb > 4u * k ? min(nb - 4u * k, 4u) : 0u;
                v[k] = keep == 4u ? x[k] : (keep == 0u ? 0u : (x[k] & ((1u << (8u * keep)) - 1u)));
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k)
                if (nb > 4u * k) {
                    uint32_t x = (hdr + b0 + 4u * k + 4u <= a.stride) ? src[k] : 0u;
                    const uint32_t keep = nb - 4u * k;
                    if (keep < 4u) x &= (1u << (8u * keep)) - 1u;
                    v[k] = x;
                }
        }
    }
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// one channel's state in registers, and its ring tags in LDS
struct JbLane {
    igdsp_jb_state s;
    uint32_t *tag;                         // [IGDSP_JB_DEPTH]
    uint16_t *src;                         // [IGDSP_JB_DEPTH]

    __device__ __forceinline__ void drop_ring()      // discarded += frames in the ring; the ring is emptied
    {
#pragma unroll
        for (uint32_t i = 0; i < IGDSP_JB_DEPTH; ++i) {
            if (tag[i] != 0u) ++s.discarded;
            tag[i] = 0u;
            src[i] = kJbOld;
        }
    }
    __device__ __forceinline__ void stop()
    {
        drop_ring();
        s.flags &= (uint8_t)~IGDSP_JB_PLAYING;
        s.wait = 0; s.lost_run = 0;
    }
    __device__ __forceinline__ void init_seq(uint32_t seq)
    {
        s.base_seq = seq; s.max_seq = (uint16_t)seq; s.bad_seq = 0x10001u; s.cycles = 0; s.received = 0;
        ++s.epoch;                                   // received_prior = expected_prior = 0
    }
    // RFC 3550 A.1 update_seq; *did_init: it ran init_seq
    __device__ __forceinline__ bool update_seq(uint32_t seq, bool *did_init)
    {
        const uint32_t udelta = (seq - s.max_seq) & 0xFFFFu;
        *did_init = false;
        if (s.probation) {
            if (seq == (uint32_t)s.max_seq + 1u) {   // an int comparison in A.1: 0 does not follow 65535
                --s.probation;
                s.max_seq = (uint16_t)seq;
                if (s.probation == 0u) {
                    init_seq(seq);
                    ++s.received;
                    *did_init = true;
                    return true;
                }
            } else {
                s.probation = 1u;                    // MIN_SEQUENTIAL - 1
                s.max_seq = (uint16_t)seq;
            }
            return false;
        } else if (udelta < 3000u) {                 // MAX_DROPOUT
            if (seq < s.max_seq) s.cycles += 0x10000u;
            s.max_seq = (uint16_t)seq;
        } else if (udelta <= 0x10000u - 100u) {      // RTP_SEQ_MOD - MAX_MISORDER
            if (seq == s.bad_seq) {
                init_seq(seq);
                *did_init = true;
            } else {
                s.bad_seq = (seq + 1u) & 0xFFFFu;
                return false;
            }
        }
        ++s.received;
        return true;
    }
    // a packet that is neither missing nor a runt; returns its IGDSP_JB_PKT_* status.  *ka: keep-alive of this tick (arrival al)
    __device__ __forceinline__ uint32_t packet(uint32_t al, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t arr, bool has_arr, uint32_t delay,
                                               uint32_t *ka)
    {
        if (((w0 >> 6) & 3u) != 2u) { ++s.invalid; return IGDSP_JB_PKT_INVALID; }
        if (((w0 >> 8) & 0x7Fu) == 123u) { ++s.keepalives; *ka = al; return IGDSP_JB_PKT_KEEPALIVE; }
        const uint32_t seq = ((w0 >> 8) & 0xFF00u) | (w0 >> 24);
        const uint32_t ts = __builtin_bswap32(w1), ssrc = __builtin_bswap32(w2);
        const bool heard = (s.flags & IGDSP_JB_HEARD) != 0u;
        if (heard && ssrc != s.ssrc) { stop(); ++s.restarts; }
        if (!heard || ssrc != s.ssrc) {              // a new source: A.1's initialisation, A.8's state cleared
            s.flags = (uint8_t)((s.flags | IGDSP_JB_HEARD) & ~IGDSP_JB_TRANSIT);
            s.ssrc = ssrc;
            init_seq(seq);
            s.max_seq = (uint16_t)(seq - 1u);
            s.probation = 2u;                        // MIN_SEQUENTIAL
            s.transit = 0; s.jitter = 0;
        }
        bool did_init;
        if (!update_seq(seq, &did_init)) { ++s.invalid; return IGDSP_JB_PKT_INVALID; }
        if (has_arr) {                               // A.8
            const uint32_t transit = arr - ts;
            if (s.flags & IGDSP_JB_TRANSIT) {
                const int32_t d = (int32_t)(transit - s.transit);
                const uint32_t ad = d < 0 ? 0u - (uint32_t)d : (uint32_t)d;
                s.jitter += ad - ((s.jitter + 8u) >> 4);
            }
            s.transit = transit;
            s.flags |= IGDSP_JB_TRANSIT;
        }
        const uint32_t slot = seq & (IGDSP_JB_DEPTH - 1u);
        const bool playing = (s.flags & IGDSP_JB_PLAYING) != 0u;
        const int32_t d = (int16_t)(uint16_t)(seq - s.head);
        if (playing && !did_init && d < 0) { ++s.late; return IGDSP_JB_PKT_LATE; }
        if (!playing || did_init || d >= IGDSP_JB_DEPTH) {      // Start
            drop_ring();
            if (playing) ++s.restarts;
            s.flags |= IGDSP_JB_PLAYING;
            s.head = (uint16_t)seq; s.wait = (uint8_t)delay; s.lost_run = 0;
            tag[slot] = kJbTag | seq; src[slot] = (uint16_t)al;
            return IGDSP_JB_PKT_RESTART;
        }
        if (tag[slot] == (kJbTag | seq)) { ++s.duplicate; return IGDSP_JB_PKT_DUPLICATE; }
        tag[slot] = kJbTag | seq; src[slot] = (uint16_t)al;
        return IGDSP_JB_PKT_PLACED;
    }
    // the tick's playout decision, as a descriptor (len and radio filled in later)
    __device__ __forceinline__ uint32_t tick(uint32_t ka)
    {
        const uint32_t idle = ka != kJbOld ? jb_desc(kJdKa, ka, IGDSP_JB_IDLE) : jb_desc(kJdNone, 0u, IGDSP_JB_IDLE);
        if (!(s.flags & IGDSP_JB_PLAYING)) return idle;
        if (s.wait > 0u) { --s.wait; return idle; }
        const uint32_t slot = s.head & (IGDSP_JB_DEPTH - 1u);
        uint32_t r;
        if (tag[slot] == (kJbTag | s.head)) {
            r = src[slot] == kJbOld ? jb_desc(kJdRing, slot, IGDSP_JB_PLAYED) : jb_desc(kJdArr, src[slot], IGDSP_JB_PLAYED);
            tag[slot] = 0u; src[slot] = kJbOld;
            ++s.played; s.lost_run = 0;
        } else {
            r = ka != kJbOld ? jb_desc(kJdKa, ka, IGDSP_JB_LOST) : jb_desc(kJdNone, 0u, IGDSP_JB_LOST);
            ++s.lost; ++s.lost_run;
        }
        s.head = (uint16_t)(s.head + 1u);
        if (s.lost_run >= IGDSP_JB_DEPTH) stop();
        return r;
    }
};

template <bool COPY>
__global__ __launch_bounds__(kJbWaves * 64) void k_jb_receive(const JbArgs a)
{
    __shared__ uint32_t desc[kJbWaves][kJbPart][kJbCh];
    __shared__ uint32_t rtag[kJbWaves][kJbCh][IGDSP_JB_DEPTH];
    __shared__ uint16_t rsrc[kJbWaves][kJbCh][IGDSP_JB_DEPTH];
    __shared__ uint32_t todo[kJbWaves][kJbCh * IGDSP_JB_DEPTH];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t c0l = ((uint64_t)blockIdx.x * kJbWaves + w) * kJbCh;
    if (c0l >= a.C) return;                                                // waves are independent: no block barrier below
    const uint32_t c0 = (uint32_t)c0l, nch = min(kJbCh, a.C - c0), pt = a.pt, ntag = nch * IGDSP_JB_DEPTH;
    uint32_t *tags = reinterpret_cast<uint32_t *>(a.ring) + (uint64_t)c0 * IGDSP_JB_DEPTH;   // the wave's tags: contiguous
    uint32_t *rt = &rtag[w][0][0];
    uint16_t *rs = &rsrc[w][0][0];
    for (uint32_t i = lane; i < ntag; i += 64u) { rt[i] = tags[i]; rs[i] = kJbOld; }
    wave_lds_fence();

    // A. decide
    if (lane < nch) {
        const uint32_t c = c0 + lane;
        const bool radio = a.radio[c] != 0u;
        if (COPY) {
            for (uint32_t t = 0; t < pt; ++t) desc[w][t][lane] = jb_desc(kJdArr, t * a.S, IGDSP_JB_PLAYED) | (radio ? 1u << 14 : 0u);
        } else {
            JbLane L;
            L.s = a.state[c];
            L.tag = rt + lane * IGDSP_JB_DEPTH;
            L.src = rs + lane * IGDSP_JB_DEPTH;
            const uint32_t hdr = radio ? 20u : 12u, na = pt * a.S;
            uint32_t ka = kJbOld, k = 0, t = 0;
            for (uint32_t a0 = 0; a0 < na; a0 += kJbU) {
                uint32_t sz[kJbU], w0[kJbU], w1[kJbU], w2[kJbU], ar[kJbU];
#pragma unroll
                for (uint32_t u = 0; u < kJbU; ++u) {                      // the headers of kJbU arrivals in flight
                    const uint32_t al = min(a0 + u, na - 1u);
                    const uint32_t *p = reinterpret_cast<const uint32_t *>(jb_pkt(a, al, c));
                    sz[u] = jb_size(a, al, c);
                    w0[u] = p[0]; w1[u] = p[1]; w2[u] = p[2];
                    ar[u] = a.arrival ? a.arrival[(uint64_t)(a.t0 * a.S + al) * a.C + c] : 0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < kJbU; ++u) {
                    const uint32_t al = a0 + u;
                    if (al >= na) break;
                    uint32_t st = IGDSP_JB_PKT_NONE;
                    if (sz[u] != 0u) {
                        if (sz[u] < hdr) { ++L.s.invalid; st = IGDSP_JB_PKT_INVALID; }
                        else st = L.packet(al, w0[u], w1[u], w2[u], ar[u], a.arrival != nullptr, a.delay, &ka);
                    }
                    if (a.pkt) a.pkt[(uint64_t)(a.t0 * a.S + al) * a.C + c] = (uint8_t)st;
                    if (++k == a.S) {                                      // the tick's last arrival: playout
                        desc[w][t][lane] = L.tick(ka) | (radio ? 1u << 14 : 0u);
                        k = 0; ++t; ka = kJbOld;
                    }
                }
            }
            a.state[c] = L.s;
        }
    }
    wave_lds_fence();

    // B. records
    const uint32_t items = pt * nch;
    for (uint32_t j = lane; j < items; j += 64u) {
        const uint32_t t = j / nch, ch = j - t * nch, c = c0 + ch;
        const uint32_t d = desc[w][t][ch], kind = d & 3u, idx = (d >> 2) & 0x3FFu, flag = (d >> 12) & 3u;
        uint2 inf = make_uint2(0u, (uint32_t)IGDSP_RTP_RUNT << 24);
        uint32_t l = 0;
        if (kind == kJdRing) {
            const uint4 h = *reinterpret_cast<const uint4 *>(jb_slot(a, c, idx));
            inf = make_uint2(h.x, h.y); l = h.z;
        } else if (kind != kJdNone) {
            const FrameHdr h = jb_parse(a, idx, c, (d >> 14) & 1u);
            inf = make_uint2(h.info.ed137, (uint32_t)h.info.payload_len | (uint32_t)h.info.pt << 16 | (uint32_t)h.info.flags << 24);
            l = kind == kJdArr ? h.len : 0u;
        }
        const uint64_t o = (uint64_t)(a.t0 + t) * a.C + c;
        a.len[o] = (uint16_t)l;
        *reinterpret_cast<uint2 *>(a.info + o) = inf;
        if (a.tick) a.tick[o] = (uint8_t)flag;
        desc[w][t][ch] = d | l << 16;
    }
    wave_lds_fence();

    // C. rows: piece q of frame (t, ch), kJbU pieces of a lane in flight
    const uint32_t P = a.pieces, n = a.n, total = items * P;
    for (uint32_t j0 = 0; j0 < total; j0 += 64u * kJbU) {
        uint4 v[kJbU];
        uint64_t dst[kJbU];
        uint32_t b0s[kJbU];
#pragma unroll
        for (uint32_t u = 0; u < kJbU; ++u) {
            const uint32_t j = j0 + u * 64u + lane;
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            dst[u] = ~0ull;
            if (j < total) {
                const uint32_t row = j / P, q = j - row * P, t = row / nch, ch = row - t * nch, c = c0 + ch;
                const uint32_t d = desc[w][t][ch], kind = d & 3u, idx = (d >> 2) & 0x3FFu, l = d >> 16;
                if (kind == kJdArr) v[u] = jb_piece(a, idx, c, (d >> 14) & 1u ? 20u : 12u, l, 16u * q);
                else if (kind == kJdRing) v[u] = *reinterpret_cast<const uint4 *>(jb_slot(a, c, idx) + kJbSlotHead + 16u * q);
                dst[u] = ((uint64_t)(a.t0 + t) * a.C + c) * n;
                b0s[u] = 16u * q;
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kJbU; ++u) {
            if (dst[u] == ~0ull) continue;
            uint8_t *o = a.payload + dst[u] + b0s[u];
            if (a.vec) {
                *reinterpret_cast<uint4 *>(o) = v[u];
            } else {
                const uint32_t x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                for (uint32_t b = 0; b < 16u && b0s[u] + b < n; ++b) o[b] = (uint8_t)(x[b >> 2] >> (8u * (b & 3u)));
            }
        }
    }

    // D. ring: this part's unplayed packets into their slots, then the tags
    if (!COPY) {
        uint32_t cnt = 0;
        for (uint32_t i0 = 0; i0 < ntag; i0 += 64u) {
            const uint32_t i = i0 + lane;
            const bool st = i < ntag && rt[i] != 0u && rs[i] != kJbOld;
            const uint64_t m = __builtin_amdgcn_ballot_w64(st);
            if (st) todo[w][cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = i | (uint32_t)rs[i] << 16;
            cnt += (uint32_t)__builtin_popcountll(m);
        }
        wave_lds_fence();
        const uint32_t per = P + 1u;                                       // the record head, then P payload pieces
        for (uint32_t j = lane; j < cnt * per; j += 64u) {
            const uint32_t e = j / per, q = j - e * per, ent = todo[w][e];
            const uint32_t ch = (ent & 0xFFFFu) / IGDSP_JB_DEPTH, s = ent & (IGDSP_JB_DEPTH - 1u), al = ent >> 16, c = c0 + ch;
            const bool radio = a.radio[c] != 0u;
            const FrameHdr h = jb_parse(a, al, c, radio);
            uint8_t *slot = jb_slot(a, c, s);
            if (q == 0u)
                *reinterpret_cast<uint4 *>(slot) = make_uint4(h.info.ed137, (uint32_t)h.info.payload_len | (uint32_t)h.info.pt << 16 |
                                                                                (uint32_t)h.info.flags << 24, h.len, 0u);
            else
                *reinterpret_cast<uint4 *>(slot + kJbSlotHead + 16u * (q - 1u)) = jb_piece(a, al, c, radio ? 20u : 12u, h.len, 16u * (q - 1u));
        }
        for (uint32_t i = lane; i < ntag; i += 64u) tags[i] = rt[i];
    }
}

hipError_t launch_jb_receive(const LaunchCfg &, const uint8_t *packets, const uint16_t *sizes, const uint8_t *radio, const uint32_t *arrival,
                             uint32_t C, uint32_t T, uint32_t S, uint32_t stride, uint32_t n, uint32_t delay, igdsp_jb_state *state, void *ring,
                             uint8_t *payload, uint16_t *len, igdsp_rtp_info *info, uint8_t *tick, uint8_t *pkt, bool yardstick, hipStream_t s)
{
    const JbRoute r = jb_route(C, T, n, reinterpret_cast<uintptr_t>(payload));
    if (r.grid == 0) return hipSuccess;
    JbArgs a{packets, sizes, radio, arrival, C, S, stride, n, delay, r.pieces, r.vec, 0u, 0u, state, static_cast<uint8_t *>(ring), payload,
             len, info, tick, pkt, jb_slot_bytes(n)};
    const auto kernel = yardstick ? k_jb_receive<true> : k_jb_receive<false>;
    for (uint32_t p = 0; p < r.parts; ++p) {
        a.t0 = p * kJbPart;
        a.pt = std::min(kJbPart, T - a.t0);
        hipLaunchKernelGGL(kernel, dim3(r.grid), dim3(r.threads), 0, s, a);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace igdsp
