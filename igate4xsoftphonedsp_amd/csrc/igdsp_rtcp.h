// igdsp_rtcp.h — the RTCP and SRTCP rules (include/igdsp.h, "RTCP / SRTCP"; independent restatement: tests/rtcp_model.py) in plain C++17,
// so that the host entries igdsp_rtcp_build_packet / igdsp_rtcp_parse_packet / igdsp_srtcp_*_packet and the kernels k_rtcp_build,
// k_rtcp_parse and k_srtcp run the same code.
//   Build: what a report holds is decided in rtcp_plan (RFC 3550 6.4: SR or RR, the A.3 block of igdsp_jb_report's arithmetic, LSR and
//   DLSR); the packet is then a list of big-endian words handed to a sink one after the other (rtcp_emit), the host's sink a buffer,
//   the kernel's a row of LDS.  The CNAME's 64 bytes come as 16 words whose bytes past L are masked, shifted by the item's two bytes.
//   Parse: a compound packet is walked a word at a time (rtcp_walk_word) in increasing order, which is how a lane meets it in 64-byte
//   pieces of an LDS tile: the word at `next` is a sub-packet's header (RFC 3550 A.2's checks on it), the words behind it are taken by
//   their distance from it.  Nothing is read by an offset taken from the packet: a length only moves `next`, and a word past the
//   packet's size is never handed in.  What a valid packet changes is applied at its end (rtcp_seen_commit).
//   SRTCP (RFC 3711 3.4) reuses igdsp_srtp.h's AES, SHA-1, keystream and hash pieces as they are: the header is 8 bytes, the 31-bit
//   index and E travel in a word behind the packet, which the tag covers in the place of SRTP's rollover counter.
// Nothing here indexes a private array by a run-time value.  Little-endian hosts only.
#pragma once
#include "igdsp_srtp.h"

namespace igdsp {

static_assert(sizeof(igdsp_rtcp_state) == 80 && sizeof(igdsp_rtcp_src) == 16 && sizeof(igdsp_rtcp_built) == 8 && sizeof(igdsp_rtcp_seen) == 32 &&
              sizeof(igdsp_jb_state) == 80 && sizeof(igdsp_jb_prior) == 16, "capi.RTCP_STATE, RTCP_SRC, RTCP_BUILT, RTCP_SEEN");
static_assert(offsetof(igdsp_rtcp_state, sent_prior) == 16 && offsetof(igdsp_rtcp_state, lsr) == 24 && offsetof(igdsp_rtcp_state, flags) == 32 &&
              offsetof(igdsp_rtcp_state, rtt_last) == 44 && offsetof(igdsp_rtcp_state, peer_fraction_lost) == 52 && offsetof(igdsp_rtcp_state, reserved) == 68 &&
              offsetof(igdsp_jb_state, ssrc) == 0 && offsetof(igdsp_jb_state, cycles) == 4 && offsetof(igdsp_jb_state, base_seq) == 8 &&
              offsetof(igdsp_jb_state, received) == 20 && offsetof(igdsp_jb_state, jitter) == 28 && offsetof(igdsp_jb_state, epoch) == 32 &&
              offsetof(igdsp_jb_state, max_seq) == 36 && offsetof(igdsp_jb_state, flags) == 42, "both states go as 20 dwords");
static_assert(IGDSP_RTCP_MAX_BUILT == 52 + 76 + 8 && IGDSP_RTCP_CNAME_MAX == 64, "SR with one block, SDES with a 64-byte CNAME, BYE");

constexpr uint32_t kRtcpStateWords = 20, kRtcpMaxWords = IGDSP_RTCP_MAX_BUILT / 4u, kRtcpCnameWords = IGDSP_RTCP_CNAME_MAX / 4u;
constexpr uint32_t kRtcpSr = 200, kRtcpRr = 201, kRtcpSdes = 202, kRtcpByePt = 203;

// ---- what a leg carries through its ticks: igdsp_rtcp_state's first seventeen words
struct RtcpLane {
    uint32_t exp_prior, rec_prior, epoch, prior_rsv, sent_prior, n_built, lsr, lsr_arrival, flags, n_parsed, n_malformed, rtt_last, rtt_count, peer_fl, peer_cum,
        peer_ext, peer_jit;
};
IGDSP_SRTP_HD RtcpLane rtcp_lane_read(const uint32_t (&w)[kRtcpStateWords])
{
    return RtcpLane{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12], w[13], w[14], w[15], w[16]};
}
IGDSP_SRTP_HD void rtcp_lane_write(const RtcpLane &l, uint32_t (&w)[kRtcpStateWords])    // the reserved words stay as they were read
{
    w[0] = l.exp_prior; w[1] = l.rec_prior; w[2] = l.epoch; w[3] = l.prior_rsv; w[4] = l.sent_prior; w[5] = l.n_built; w[6] = l.lsr; w[7] = l.lsr_arrival;
    w[8] = l.flags; w[9] = l.n_parsed; w[10] = l.n_malformed; w[11] = l.rtt_last; w[12] = l.rtt_count; w[13] = l.peer_fl; w[14] = l.peer_cum; w[15] = l.peer_ext;
    w[16] = l.peer_jit;
}

// ---- build ---------------------------------------------------------------------------------------------------------------------------
// the words of igdsp_jb_state a report needs (jw: the state as dwords; heard false for a NULL d_jb)
struct RtcpJb {
    bool heard;
    uint32_t ssrc, cycles, base_seq, received, jitter, epoch, max_seq;
};
IGDSP_SRTP_HD RtcpJb rtcp_jb_of(const uint32_t (&jw)[kRtcpStateWords], bool present)
{
    return RtcpJb{present && ((jw[10] >> 16) & IGDSP_JB_HEARD) != 0u, jw[0], jw[1], jw[2], jw[5], jw[7], jw[8], jw[9] & 0xFFFFu};
}
struct RtcpPlan {
    uint32_t ctl, pt, rc, L, size, flags;
    uint32_t blk[6];                                                       // the report block, host order
};
IGDSP_SRTP_HD uint32_t rtcp_ctl(uint32_t v) { return (v == IGDSP_RTCP_REPORT || v == IGDSP_RTCP_BYE) ? v : (uint32_t)IGDSP_RTCP_NONE; }
IGDSP_SRTP_HD uint32_t rtcp_sdes_words(uint32_t L) { return 1u + (7u + L + 3u) / 4u; }   // the header and the chunk
IGDSP_SRTP_HD uint32_t rtcp_size_of(bool sr, uint32_t rc, uint32_t L, uint32_t ctl)   // L <= 64
{
    return 4u * ((sr ? 7u : 2u) + 6u * rc + rtcp_sdes_words(L) + (ctl == IGDSP_RTCP_BYE ? 2u : 0u));
}
// What the packet of this tick holds; advances the lane as the packet will have been written (ctl REPORT or BYE).  The block is RFC 3550
// A.3 in igdsp_jb_report's arithmetic: 64-bit differences, the clamp to 24 bits, the priors of another epoch counted as zero.
IGDSP_SRTP_HD RtcpPlan rtcp_plan(RtcpLane &l, uint32_t ctl, const RtcpJb &jb, const igdsp_rtcp_src &src, uint64_t now, uint32_t cname_len)
{
    RtcpPlan p{};
    p.ctl = ctl;
    p.pt = src.packets != l.sent_prior ? kRtcpSr : kRtcpRr;
    p.rc = jb.heard ? 1u : 0u;
    p.L = cname_len < (uint32_t)IGDSP_RTCP_CNAME_MAX ? cname_len : (uint32_t)IGDSP_RTCP_CNAME_MAX;
    p.flags = (p.pt == kRtcpSr ? IGDSP_RTCP_SR : IGDSP_RTCP_RR) | (p.rc ? IGDSP_RTCP_HAS_BLOCK : 0u) | (ctl == IGDSP_RTCP_BYE ? IGDSP_RTCP_BYE_SENT : 0u);
    p.size = rtcp_size_of(p.pt == kRtcpSr, p.rc, p.L, ctl);
    if (p.rc) {
        const uint32_t ext = jb.cycles + jb.max_seq, expected = ext - jb.base_seq + 1u;
        const int64_t lost = (int64_t)expected - (int64_t)jb.received;
        const bool same = l.epoch == jb.epoch;
        const uint32_t exp_int = expected - (same ? l.exp_prior : 0u), rec_int = jb.received - (same ? l.rec_prior : 0u);
        const int64_t lost_int = (int64_t)exp_int - (int64_t)rec_int;
        const int64_t cum = lost < -0x800000 ? -0x800000 : (lost > 0x7FFFFF ? 0x7FFFFF : lost);
        uint32_t frac = 0u;
        if (exp_int != 0u && lost_int > 0) {
            const uint64_t q = ((uint64_t)lost_int << 8) / exp_int;
            frac = q > 255u ? 255u : (uint32_t)q;
        }
        const bool sr = (l.flags & IGDSP_RTCP_HAVE_SR) != 0u;
        p.blk[0] = jb.ssrc;
        p.blk[1] = (frac << 24) | ((uint32_t)cum & 0xFFFFFFu);
        p.blk[2] = ext;
        p.blk[3] = jb.jitter >> 4;
        p.blk[4] = sr ? l.lsr : 0u;
        p.blk[5] = sr ? (uint32_t)(now >> 16) - l.lsr_arrival : 0u;
        l.exp_prior = expected; l.rec_prior = jb.received; l.epoch = jb.epoch;
    }
    l.sent_prior = src.packets;
    ++l.n_built;
    return p;
}
// The packet's p.size / 4 words in order, each as the memory word (the big-endian field byte-swapped): put(k, word) with k counting up
// from 0.  cn: the CNAME's 64 bytes as 16 words in memory order (what lies past L is masked here, so any bytes may stand there).
template <class PUT>
IGDSP_SRTP_HD void rtcp_emit(const RtcpPlan &p, const igdsp_rtcp_src &src, uint64_t now, const uint32_t (&cn)[kRtcpCnameWords], const PUT &put)
{
    uint32_t k = 0;
    const uint32_t words0 = (p.pt == kRtcpSr ? 7u : 2u) + 6u * p.rc;
    put(k++, srtp_bswap(((0x80u | p.rc) << 24) | (p.pt << 16) | (words0 - 1u)));
    put(k++, srtp_bswap(src.ssrc));
    if (p.pt == kRtcpSr) {
        put(k++, srtp_bswap((uint32_t)(now >> 32)));
        put(k++, srtp_bswap((uint32_t)now));
        put(k++, srtp_bswap(src.rtp_ts));
        put(k++, srtp_bswap(src.packets));
        put(k++, srtp_bswap(src.octets));
    }
    if (p.rc) {
        IGDSP_SRTP_UNROLL
        for (uint32_t i = 0; i < 6u; ++i) put(k++, srtp_bswap(p.blk[i]));
    }
    const uint32_t sw = rtcp_sdes_words(p.L);
    put(k++, srtp_bswap((0x81u << 24) | (kRtcpSdes << 16) | (sw - 1u)));
    put(k++, srtp_bswap(src.ssrc));
    // the item: 01, L, the text, nulls.  Item word i holds the text's bytes 4 i - 2 .. 4 i + 1
    uint32_t prev = 0x01u | (p.L << 8);                                    // the low half of item word 0
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 0; i <= kRtcpCnameWords; ++i) {
        uint32_t t = 0u;
        if (i < kRtcpCnameWords) {
            const uint32_t nb = p.L > 4u * i ? (p.L - 4u * i < 4u ? p.L - 4u * i : 4u) : 0u;
            t = cn[i & (kRtcpCnameWords - 1u)] & (nb >= 4u ? 0xFFFFFFFFu : ((1u << (8u * nb)) - 1u));
        }
        if (i + 2u < sw) put(k++, (prev & 0xFFFFu) | (t << 16));
        prev = t >> 16;
    }
    if (p.ctl == IGDSP_RTCP_BYE) {
        put(k++, srtp_bswap((0x81u << 24) | (kRtcpByePt << 16) | 1u));
        put(k++, srtp_bswap(src.ssrc));
    }
}

// ---- parse ---------------------------------------------------------------------------------------------------------------------------
struct RtcpWalk {
    uint32_t nwords, next, start, pt, blk0, blk1, nsub;
    bool bad, last_p, match, found, have_sr, bye;
    uint32_t sender, msw, lsw, sr_ts, sr_packets, sr_octets, b_lost, b_ext, b_jit, b_lsr, b_dlsr;
};
// the size's own checks: 0, IGDSP_RTCP_EMPTY or IGDSP_RTCP_MALFORMED
IGDSP_SRTP_HD uint32_t rtcp_size_check(uint32_t size, uint32_t slot)
{
    if (size == 0u) return IGDSP_RTCP_EMPTY;
    return (size < 8u || (size & 3u) || size > slot) ? (uint32_t)IGDSP_RTCP_MALFORMED : 0u;
}
IGDSP_SRTP_HD RtcpWalk rtcp_walk_begin(uint32_t size)
{
    RtcpWalk w{};
    w.nwords = size >> 2;
    return w;
}
// word g of the packet (memory order), g = 0, 1, .. nwords - 1 in order
IGDSP_SRTP_HD void rtcp_walk_word(RtcpWalk &w, uint32_t g, uint32_t mem, uint32_t local_ssrc)
{
    if (w.bad || g >= w.nwords) return;
    const uint32_t be = srtp_bswap(mem);
    if (g == w.next) {                                                     // a sub-packet's header
        const uint32_t v = be >> 30, pad = (be >> 29) & 1u, rc = (be >> 24) & 31u, pt = (be >> 16) & 255u, len = be & 0xFFFFu;
        const uint32_t bytes = 4u * (len + 1u), end = g + len + 1u;        // < 2^17
        const uint32_t least = pt == kRtcpSr ? 28u + 24u * rc : (pt == kRtcpRr ? 8u + 24u * rc : (pt == kRtcpByePt ? 4u + 4u * rc : 4u));
        if (v != 2u || w.last_p || end > w.nwords || bytes < least || (w.nsub == 0u && (pad != 0u || (pt != kRtcpSr && pt != kRtcpRr)))) {
            w.bad = true;
            return;
        }
        const bool report = pt == kRtcpSr || pt == kRtcpRr;
        w.last_p = pad != 0u;
        w.next = end; w.start = g; w.pt = pt;
        w.blk0 = report ? g + (pt == kRtcpSr ? 7u : 2u) : 0u;
        w.blk1 = report ? w.blk0 + 6u * rc : 0u;
        w.match = false;
        if (pt == kRtcpByePt) w.bye = true;
        if (pt == kRtcpSr) w.have_sr = true;
        ++w.nsub;
        return;
    }
    if (w.pt != kRtcpSr && w.pt != kRtcpRr) return;                       // stepped over by its length
    const uint32_t o = g - w.start;
    if (o == 1u && w.nsub == 1u) w.sender = be;
    if (w.pt == kRtcpSr && o >= 2u && o <= 6u) {                          // the sender info's five words, shifted in as the block's are below
        w.msw = w.lsw; w.lsw = w.sr_ts; w.sr_ts = w.sr_packets; w.sr_packets = w.sr_octets; w.sr_octets = be;
    }
    if (g >= w.blk0 && g < w.blk1) {
        const uint32_t k = (g - w.blk0) % 6u;
        if (k == 0u) {
            w.match = !w.found && be == local_ssrc;
            if (w.match) w.found = true;
        } else if (w.match) {
            // the block's five words behind its SSRC are shifted in (all five are there: the header's length check), so that after the
            // last b_lost .. b_dlsr hold them in order.  (Five ifs on k are turned into a store indexed by k: a private array.)
            w.b_lost = w.b_ext; w.b_ext = w.b_jit; w.b_jit = w.b_lsr; w.b_lsr = w.b_dlsr; w.b_dlsr = be;
        }
    }
}
// the packet's end: the record, and what it changes in the lane.  pre: rtcp_size_check's verdict (the walk is not looked at if non-zero)
IGDSP_SRTP_HD igdsp_rtcp_seen rtcp_seen_commit(RtcpLane &l, uint32_t pre, const RtcpWalk &w, uint32_t arrival)
{
    igdsp_rtcp_seen r{};
    if (pre == IGDSP_RTCP_EMPTY) {
        r.flags = IGDSP_RTCP_EMPTY;
        return r;
    }
    if (pre != 0u || w.bad || w.next != w.nwords) {
        ++l.n_malformed;
        r.flags = IGDSP_RTCP_MALFORMED;
        return r;
    }
    uint32_t flags = IGDSP_RTCP_PARSED;
    r.n_sub = (uint8_t)(w.nsub < 255u ? w.nsub : 255u);
    r.sender_ssrc = w.sender;
    if (w.have_sr) {
        l.lsr = (w.msw << 16) | (w.lsw >> 16);
        l.lsr_arrival = arrival;
        l.flags |= IGDSP_RTCP_HAVE_SR;
        r.sr_packets = w.sr_packets; r.sr_octets = w.sr_octets;
        flags |= IGDSP_RTCP_GOT_SR;
    }
    if (w.found) {
        const uint32_t cum = (w.b_lost & 0xFFFFFFu) | ((w.b_lost & 0x800000u) ? 0xFF000000u : 0u);
        l.peer_fl = w.b_lost >> 24; l.peer_cum = cum; l.peer_ext = w.b_ext; l.peer_jit = w.b_jit;
        l.flags |= IGDSP_RTCP_PEER_VALID;
        r.peer_fraction_lost = (uint8_t)(w.b_lost >> 24); r.peer_cum_lost = (int32_t)cum; r.peer_ext_seq = w.b_ext; r.peer_jitter = w.b_jit;
        flags |= IGDSP_RTCP_GOT_BLOCK;
        if (w.b_lsr != 0u) {
            const uint32_t rtt = arrival - w.b_lsr - w.b_dlsr;
            r.rtt = rtt;
            if (rtt < 0x80000000u) {
                l.rtt_last = rtt;
                ++l.rtt_count;
                l.flags |= IGDSP_RTCP_RTT_VALID;
                flags |= IGDSP_RTCP_GOT_RTT;
            } else {
                flags |= IGDSP_RTCP_RTT_NEGATIVE;
            }
        }
    }
    if (w.bye) {
        l.flags |= IGDSP_RTCP_BYE_SEEN;
        flags |= IGDSP_RTCP_GOT_BYE;
    }
    ++l.n_parsed;
    r.flags = (uint8_t)flags;
    return r;
}

// ---- SRTCP -----------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kSrtcpTrailer = IGDSP_SRTCP_TRAILER, kSrtcpTagLen = 10, kSrtcpHeader = 8, kSrtcpIndexMask = 0x7FFFFFFFu, kSrtcpE = 0x80000000u;
struct SrtcpPkt {
    uint32_t end, size_out, idxw, dist;                                    // end: the bytes in front of the index word; idxw: E << 31 | index
    bool ahead;
};
IGDSP_SRTP_HD uint32_t srtcp_tag_len(uint32_t tagw) { return tagw == (IGDSP_SRTCP_TAG | kSrtcpTagLen) ? kSrtcpTagLen : 0u; }   // 0: no key
template <int DIR>
IGDSP_SRTP_HD uint32_t srtcp_sizes(uint32_t size, uint32_t out_cap, SrtcpPkt &p)
{
    if (DIR == kSrtpUnprotect) {
        if (size < kSrtcpHeader + kSrtcpTrailer || ((size - kSrtcpTrailer) & 3u)) return IGDSP_SRTP_MALFORMED;
        p.end = size - kSrtcpTrailer;
        p.size_out = p.end;
    } else {
        if (size < kSrtcpHeader || (size & 3u)) return IGDSP_SRTP_MALFORMED;
        p.end = size;
        p.size_out = size + kSrtcpTrailer;
    }
    return p.size_out > out_cap ? (uint32_t)IGDSP_SRTP_MALFORMED : 0u;
}
// w0: the packet's first word (memory order); idxw_in: the received index word (unprotect).  0 to go on, else the refusal
template <int DIR>
IGDSP_SRTP_HD uint32_t srtcp_admit(const SrtpLane &l, uint32_t w0, uint32_t idxw_in, SrtcpPkt &p)
{
    const uint32_t top = l.roc & kSrtcpIndexMask;
    if (DIR == kSrtpProtect) {
        if ((w0 & 0xC0u) != 0x80u) return IGDSP_SRTP_MALFORMED;
        p.idxw = kSrtcpE | top;
        p.ahead = true;
        p.dist = 0u;
        return 0u;
    }
    p.idxw = idxw_in;
    const uint32_t index = idxw_in & kSrtcpIndexMask;
    p.ahead = !l.have || index > top;
    const uint32_t d = p.ahead ? index - top : top - index;
    p.dist = d < kSrtpWindow ? d : kSrtpWindow;
    if (!p.ahead) {
        if (p.dist >= kSrtpWindow) return IGDSP_SRTP_OLD;
        if ((l.win >> p.dist) & 1u) return IGDSP_SRTP_REPLAY;
    }
    return 0u;
}
template <int DIR>
IGDSP_SRTP_HD uint32_t srtcp_commit(SrtpLane &l, const SrtcpPkt &p)
{
    ++l.n_ok;
    if (DIR == kSrtpProtect) {
        l.roc = ((p.idxw & kSrtcpIndexMask) + 1u) & kSrtcpIndexMask;
        return IGDSP_SRTP_OK;
    }
    if (p.ahead) {
        l.win = ((!l.have || p.dist >= kSrtpWindow) ? 0ull : l.win << p.dist) | 1ull;
        l.roc = p.idxw & kSrtcpIndexMask;
        l.have = 1u;
    } else {
        l.win |= 1ull << p.dist;                                           // dist < 64: srtcp_admit
    }
    return IGDSP_SRTP_OK | ((p.idxw & kSrtcpE) ? 0u : (uint32_t)IGDSP_SRTCP_CLEAR);
}
// The packet as SRTP's pieces see it, and its IV: the header is 8 bytes (with E = 0 the whole packet, so no keystream is laid on it),
// the 48-bit index is the SRTCP index, and the word the tag covers behind the packet is the index word
IGDSP_SRTP_HD SrtpPkt srtcp_view(const uint32_t (&ksw)[4], uint32_t ssrc, const SrtcpPkt &p, uint32_t (&iv)[4])
{
    SrtpPkt q{};
    const uint32_t index = p.idxw & kSrtcpIndexMask;
    q.h = (p.idxw & kSrtcpE) ? kSrtcpHeader : p.end;
    q.end = p.end;
    q.ssrc = ssrc;
    q.v = index >> 16;
    q.seq = index & 0xFFFFu;
    srtp_iv(ksw, q, iv);
    q.v = p.idxw;
    return q;
}
// the trailer's words in memory order: the tag's ten bytes from the digest, and the other way round
IGDSP_SRTP_HD uint32_t srtcp_tag_half(const uint32_t (&d)[5]) { return ((d[2] >> 24) & 0xFFu) | ((d[2] >> 8) & 0xFF00u); }   // bytes 8 and 9 as a 16-bit word
IGDSP_SRTP_HD void srtcp_tag_words(uint32_t m1, uint32_t m2, uint32_t half, uint32_t (&rt)[3])
{
    rt[0] = srtp_bswap(m1); rt[1] = srtp_bswap(m2); rt[2] = ((half & 0xFFu) << 24) | ((half & 0xFF00u) << 8);
}

// ---- host only from here ---------------------------------------------------------------------------------------------------------------
inline void srtcp_derive(const uint8_t key_salt[30], uint32_t index0, igdsp_srtp_state &st)
{
    srtp_derive_keys(key_salt, 3, st);
    st.tag = IGDSP_SRTCP_TAG | kSrtcpTagLen;
    st.roc = index0 & kSrtcpIndexMask;
}

// One SRTCP packet; the arguments are srtp_packet_run's
template <int DIR>
inline void srtcp_packet_run(igdsp_srtp_state &st, uint32_t ctl, const uint8_t *in, uint32_t size, uint32_t in_cap, uint8_t *out, uint32_t out_cap,
                             uint32_t &size_out, igdsp_srtp_rec &rec)
{
    size_out = 0u;
    rec = igdsp_srtp_rec{0u, 0u, IGDSP_SRTP_NO_KEY, 0u};
    ctl = srtp_ctl(ctl);
    const bool fits = size <= kSrtpMaxPacket && size <= in_cap;
    if (ctl == IGDSP_SRTP_BYPASS) {
        if (size == 0u) rec.flags = IGDSP_SRTP_EMPTY;
        else if (!fits || size > out_cap) rec.flags = IGDSP_SRTP_MALFORMED;
        else {
            if (out != in) std::memmove(out, in, size);
            size_out = size; rec.size_out = (uint16_t)size; rec.flags = IGDSP_SRTP_BYPASSED;
        }
        return;
    }
    uint32_t sw[10];
    std::memcpy(sw, &st, sizeof(sw));
    if (!srtcp_tag_len(sw[0])) return;                                     // NO_KEY
    SrtpLane l = srtp_lane_read(sw);
    if (ctl == IGDSP_SRTP_RESET) srtp_lane_reset(l);
    auto close = [&](uint32_t flags, uint32_t v) {
        srtp_lane_write(l, sw);
        std::memcpy(&st, sw, sizeof(sw));
        rec.roc_used = v; rec.size_out = (uint16_t)size_out; rec.flags = (uint8_t)flags;
    };
    if (size == 0u) return close(IGDSP_SRTP_EMPTY, 0u);
    SrtcpPkt p{};
    uint32_t pw[16], ssrc = 0u, rt[3] = {0u, 0u, 0u};
    uint32_t flags = fits ? srtcp_sizes<DIR>(size, out_cap, p) : (uint32_t)IGDSP_SRTP_MALFORMED;
    if (!flags) {
        srtp_load_piece(in, size, 0, pw);
        ssrc = srtp_bswap(pw[1]);
        uint32_t t[3] = {0u, 0u, 0u};
        uint16_t half = 0;
        if (DIR == kSrtpUnprotect) {                                       // p.end + 14 == size
            std::memcpy(t, in + p.end, 12);
            std::memcpy(&half, in + p.end + 12u, 2);
            srtcp_tag_words(t[1], t[2], half, rt);
        }
        flags = srtcp_admit<DIR>(l, pw[0], srtp_bswap(t[0]), p);
    }
    if (flags) {
        srtp_refuse(l, flags);
        return close(flags, (flags & (IGDSP_SRTP_OLD | IGDSP_SRTP_REPLAY)) ? p.idxw : 0u);
    }
    uint32_t ksw[4], iv[4], hs[5], d[5], carry[4] = {0u, 0u, 0u, 0u}, x[16];
    for (int i = 0; i < 4; ++i) ksw[i] = srtp_be32(st.ks + 4 * i);
    const SrtpPkt q = srtcp_view(ksw, ssrc, p, iv);
    std::memcpy(hs, st.mid_i, 20);
    const uint32_t nblk = srtp_hash_blocks(q.end);
    if (DIR == kSrtpProtect) {
        for (uint32_t j = 0; j < nblk; ++j) {
            srtp_load_piece(in, q.end, j, pw);
            srtp_ks_piece(SrtpRkArray{st.rk}, SrtpHostTe{}, SrtpHostAny{}, iv, q.h, q.end, j, carry, x);
            for (int i = 0; i < 16; ++i) pw[i] ^= x[i];
            srtp_hash_piece(hs, pw, j, q.end, q.v);
            srtp_store_piece(out, q.end, j, pw);
        }
        srtp_hmac_finish(hs, st.mid_o, d);
        const uint32_t t[3] = {srtp_bswap(p.idxw), srtp_bswap(d[0]), srtp_bswap(d[1])};
        const uint16_t half = (uint16_t)srtcp_tag_half(d);
        std::memcpy(out + p.end, t, 12);
        std::memcpy(out + p.end + 12u, &half, 2);
    } else {
        for (uint32_t j = 0; j < nblk; ++j) {
            srtp_load_piece(in, q.end, j, pw);
            srtp_hash_piece(hs, pw, j, q.end, q.v);
        }
        srtp_hmac_finish(hs, st.mid_o, d);
        if (!srtp_tag_equal(d, rt, kSrtcpTagLen)) {
            srtp_refuse(l, IGDSP_SRTP_AUTH_FAIL);
            return close(IGDSP_SRTP_AUTH_FAIL, p.idxw);
        }
        for (uint32_t j = 0; 64u * j < q.end; ++j) {
            srtp_load_piece(in, q.end, j, pw);
            srtp_ks_piece(SrtpRkArray{st.rk}, SrtpHostTe{}, SrtpHostAny{}, iv, q.h, q.end, j, carry, x);
            for (int i = 0; i < 16; ++i) pw[i] ^= x[i];
            srtp_store_piece(out, q.end, j, pw);
        }
    }
    size_out = p.size_out;
    close(srtcp_commit<DIR>(l, p), p.idxw);
}

// One report into out (capacity >= IGDSP_RTCP_MAX_BUILT: the caller's rule).  jb and cname may be null
inline void rtcp_build_run(igdsp_rtcp_state &st, uint32_t ctl, const igdsp_jb_state *jb, const igdsp_rtcp_src &src, uint64_t now, const uint8_t *cname,
                           uint32_t cname_len, uint8_t *out, uint32_t &size_out, igdsp_rtcp_built &rec)
{
    size_out = 0u;
    rec = igdsp_rtcp_built{};
    ctl = rtcp_ctl(ctl);
    if (ctl == IGDSP_RTCP_NONE) return;
    uint32_t sw[kRtcpStateWords], jw[kRtcpStateWords] = {}, cn[kRtcpCnameWords] = {};
    std::memcpy(sw, &st, sizeof(sw));
    if (jb) std::memcpy(jw, jb, sizeof(jw));
    const uint32_t L = cname ? (cname_len < (uint32_t)IGDSP_RTCP_CNAME_MAX ? cname_len : (uint32_t)IGDSP_RTCP_CNAME_MAX) : 0u;
    if (L) std::memcpy(cn, cname, L);
    RtcpLane l = rtcp_lane_read(sw);
    const RtcpPlan p = rtcp_plan(l, ctl, rtcp_jb_of(jw, jb != nullptr), src, now, L);
    rtcp_emit(p, src, now, cn, [&](uint32_t k, uint32_t word) { std::memcpy(out + 4u * k, &word, 4); });
    rtcp_lane_write(l, sw);
    std::memcpy(&st, sw, sizeof(sw));
    size_out = p.size;
    rec.size = (uint16_t)p.size;
    rec.flags = (uint8_t)p.flags;
}

inline void rtcp_parse_run(igdsp_rtcp_state &st, const uint8_t *in, uint32_t size, uint32_t slot, uint32_t arrival, uint32_t local_ssrc, igdsp_rtcp_seen &rec)
{
    uint32_t sw[kRtcpStateWords];
    std::memcpy(sw, &st, sizeof(sw));
    RtcpLane l = rtcp_lane_read(sw);
    const uint32_t pre = rtcp_size_check(size, slot);
    RtcpWalk w = rtcp_walk_begin(pre ? 0u : size);
    for (uint32_t g = 0; g < w.nwords; ++g) {
        uint32_t mem;
        std::memcpy(&mem, in + 4u * g, 4);
        rtcp_walk_word(w, g, mem, local_ssrc);
    }
    rec = rtcp_seen_commit(l, pre, w, arrival);
    rtcp_lane_write(l, sw);
    std::memcpy(&st, sw, sizeof(sw));
}

}  // namespace igdsp
