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
//
// igdsp_jb_receive_adaptive (k_jb_adaptive) is the same body with ADAPT: phase A also carries the channel's igdsp_jb_adapt (8 bytes, read
// and written once per part beside the state), takes the pre-roll of a Start from jb_adapt_start (igdsp_route.h) where the fixed entry
// takes delay_frames, and lets the late_restart-th consecutive LATE packet start playout again; the delay after a tick's arrivals rides
// in bits 28-31 of the tick's descriptor to phase B, which writes d_delay_out.  Independent restatement: tests/jb_adapt_model.py.
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

// igdsp_jb_receive_adaptive: the fixed entry's arguments (delay unused), then its own
struct JbAdaptArgs {
    JbArgs a;
    igdsp_jb_adapt *adapt;
    uint8_t *delay_out;                    // nullptr: not wanted
    igdsp_jb_adapt_cfg cfg;
};

// descriptor: kind | arrival or slot << 2 | flag << 12 | radio << 14 | len << 16 (9 bits) | ADAPT: delay << 28
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

// one channel's igdsp_jb_adapt in registers, with what its rules need
struct JbAdaptLane {
    igdsp_jb_adapt a;
    igdsp_jb_adapt_cfg cfg;
    uint32_t n;

    // a LATE packet, behind = -d frames behind the head; true: it is the late_restart-th in a row and starts playout again
    __device__ __forceinline__ bool late(uint32_t behind)
    {
        a.need = (uint8_t)max((uint32_t)a.need, min((uint32_t)a.delay + behind, (uint32_t)cfg.max_frames));
        a.late_run = (uint8_t)min((uint32_t)a.late_run + 1u, 255u);
        return cfg.late_restart > 0u && a.late_run >= cfg.late_restart;
    }
};

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
    // a packet that is neither missing nor a runt; returns its IGDSP_JB_PKT_* status.  *ka: keep-alive of this tick (arrival al).
    // ADAPT: ad holds the channel's igdsp_jb_adapt and delay is not used
    template <bool ADAPT>
    __device__ __forceinline__ uint32_t packet(uint32_t al, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t arr, bool has_arr, uint32_t delay,
                                               uint32_t *ka, JbAdaptLane *ad)
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
        if (playing && !did_init && d < 0) {
            ++s.late;
            if (!ADAPT || !ad->late((uint32_t)-d)) return IGDSP_JB_PKT_LATE;
        }
        if (!playing || did_init || d >= IGDSP_JB_DEPTH || (ADAPT && d < 0)) {      // Start (ADAPT, d < 0: the late re-sync)
            drop_ring();
            if (playing) ++s.restarts;
            if (ADAPT) delay = jb_adapt_start(ad->cfg, s.jitter, ad->n, ad->a);
            s.flags |= IGDSP_JB_PLAYING;
            s.head = (uint16_t)seq; s.wait = (uint8_t)delay; s.lost_run = 0;
            tag[slot] = kJbTag | seq; src[slot] = (uint16_t)al;
            return IGDSP_JB_PKT_RESTART;
        }
        if (ADAPT) ad->a.late_run = 0;
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
    constexpr bool ADAPT = false;
    constexpr JbAdaptArgs x{};                                             // the body reads x only where ADAPT
#include "igdsp_k_jb_body.h"
}

__global__ __launch_bounds__(kJbWaves * 64) void k_jb_adaptive(const JbAdaptArgs x)
{
    constexpr bool COPY = false, ADAPT = true;
    const JbArgs &a = x.a;
#include "igdsp_k_jb_body.h"
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

hipError_t launch_jb_adaptive(const LaunchCfg &, const uint8_t *packets, const uint16_t *sizes, const uint8_t *radio, const uint32_t *arrival,
                              uint32_t C, uint32_t T, uint32_t S, uint32_t stride, uint32_t n, const igdsp_jb_adapt_cfg &cfg, igdsp_jb_state *state,
                              void *ring, igdsp_jb_adapt *adapt, uint8_t *payload, uint16_t *len, igdsp_rtp_info *info, uint8_t *tick, uint8_t *pkt,
                              uint8_t *delay_out, hipStream_t s)
{
    const JbRoute r = jb_route(C, T, n, reinterpret_cast<uintptr_t>(payload));
    if (r.grid == 0) return hipSuccess;
    JbAdaptArgs x{{packets, sizes, radio, arrival, C, S, stride, n, 0u, r.pieces, r.vec, 0u, 0u, state, static_cast<uint8_t *>(ring), payload, len,
                   info, tick, pkt, jb_slot_bytes(n)}, adapt, delay_out, cfg};
    for (uint32_t p = 0; p < r.parts; ++p) {
        x.a.t0 = p * kJbPart;
        x.a.pt = std::min(kJbPart, T - x.a.t0);
        hipLaunchKernelGGL(k_jb_adaptive, dim3(r.grid), dim3(r.threads), 0, s, x);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace igdsp
