// igdsp_srtp.h — the SRTP rule (include/igdsp.h, "SRTP"; independent restatement: tests/srtp_model.py) in plain C++17, so that the host
// entries igdsp_srtp_protect_packet / igdsp_srtp_unprotect_packet and the kernel k_srtp run the same code: the header's length, the
// index estimate of RFC 3711 Appendix A, the replay window, AES-128 in counter mode (FIPS-197), HMAC-SHA1 (FIPS 180, RFC 2104) from two
// stored midstates, and the key derivation of RFC 3711 4.3.1 (host only).  A packet is walked in pieces of 64 bytes, one SHA-1 block and
// four AES blocks: the host walks a local copy of a piece, a lane of the kernel its row of an LDS tile.  What the two sides do
// differently is only who loads a piece, how a table word is read (`te`) and how "does anybody need this AES block" is asked (`any`:
// a wave-uniform vote on the device).  Nothing here indexes a private array by a run-time value: every loop over rk[], w[] or a piece's
// words has constant bounds and unrolls, so they stay registers in the kernel.  Every number read from a packet is compared against the
// packet's size before it moves an offset.  Little-endian hosts only (a piece's words are the packet's bytes in memory order).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "igdsp.h"

#if defined(__HIPCC__)
#define IGDSP_SRTP_HD __host__ __device__ inline __attribute__((always_inline))   // (no HIP header need come first)
#define IGDSP_SRTP_UNROLL _Pragma("unroll")
#else
#define IGDSP_SRTP_HD inline
#define IGDSP_SRTP_UNROLL
#endif

namespace igdsp {

static_assert(sizeof(igdsp_srtp_state) == 288 && sizeof(igdsp_srtp_rec) == 8, "capi.SRTP_STATE, SRTP_REC");
static_assert(offsetof(igdsp_srtp_state, window) == 16 && offsetof(igdsp_srtp_state, n_ok) == 24 && offsetof(igdsp_srtp_state, rk) == 40 &&
              offsetof(igdsp_srtp_state, ks) == 216 && offsetof(igdsp_srtp_state, mid_i) == 232 && offsetof(igdsp_srtp_state, mid_o) == 252 &&
              offsetof(igdsp_srtp_rec, size_out) == 4 && offsetof(igdsp_srtp_rec, flags) == 6, "the state goes as 72 dwords, the record as one 8-byte store");

constexpr int kSrtpProtect = 0, kSrtpUnprotect = 1;
constexpr uint32_t kSrtpMaxPacket = IGDSP_SRTP_MAX_PACKET, kSrtpStateWords = 72, kSrtpWindow = 64, kSrtpPiece = 64, kSrtpPieceWords = 16;

// ---- AES-128: one table Te0[x] = S[x] . (02, 01, 01, 03), built at compile time from the field's arithmetic; Te1..Te3 are its rotations
struct SrtpTe0 {
    uint32_t t[256];
};
constexpr uint32_t srtp_rotl8(uint32_t x, int s) { return ((x << s) | (x >> (8 - s))) & 0xFFu; }
constexpr SrtpTe0 srtp_make_te0()
{
    SrtpTe0 r{};
    uint32_t sb[256] = {};
    uint32_t p = 1, q = 1;
    do {                                                                   // p runs through the field's units as powers of 3, q through their inverses
        p = (p ^ (p << 1) ^ ((p & 0x80u) ? 0x1Bu : 0u)) & 0xFFu;
        q ^= q << 1; q ^= q << 2; q ^= q << 4; q &= 0xFFu;
        if (q & 0x80u) q ^= 0x09u;
        sb[p] = (q ^ srtp_rotl8(q, 1) ^ srtp_rotl8(q, 2) ^ srtp_rotl8(q, 3) ^ srtp_rotl8(q, 4) ^ 0x63u) & 0xFFu;
    } while (p != 1);
    sb[0] = 0x63u;
    for (int i = 0; i < 256; ++i) {
        const uint32_t s = sb[i], s2 = ((s << 1) ^ ((s & 0x80u) ? 0x11Bu : 0u)) & 0xFFu, s3 = s2 ^ s;
        r.t[i] = (s2 << 24) | (s << 16) | (s << 8) | s3;
    }
    return r;
}
inline constexpr SrtpTe0 kSrtpTe0 = srtp_make_te0();
static_assert(kSrtpTe0.t[0] == 0xc66363a5u && kSrtpTe0.t[1] == 0xf87c7c84u && kSrtpTe0.t[255] == 0x2c16163au && kSrtpTe0.t[0x53] == 0xc1eded2cu,
              "FIPS-197 figure 7: S[00] = 63, S[01] = 7c, S[ff] = 16, S[53] = ed");
struct SrtpHostTe {
    uint32_t operator()(uint32_t i) const { return kSrtpTe0.t[i & 255u]; }
};
struct SrtpRkArray {                                                       // the round keys where they lie: the state's array, a lane's registers
    const uint32_t (&r)[44];
    IGDSP_SRTP_HD uint32_t operator()(uint32_t i) const { return r[i]; }   // i a constant below 44
};
struct SrtpHostAny {
    bool operator()(bool b) const { return b; }
};

IGDSP_SRTP_HD uint32_t srtp_ror(uint32_t x, uint32_t n) { return (x >> n) | (x << (32u - n)); }   // n 8, 16, 24: one v_alignbit_b32
IGDSP_SRTP_HD uint32_t srtp_rol(uint32_t x, uint32_t n) { return (x << n) | (x >> (32u - n)); }
IGDSP_SRTP_HD uint32_t srtp_bswap(uint32_t x) { return __builtin_bswap32(x); }                     // one v_perm_b32

// one block: s0..s3 the input as big-endian words, out the same.  Nine table rounds, the last from the table's S byte
template <class RK, class TE>
IGDSP_SRTP_HD void srtp_aes(const RK &rk, const TE &te, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t *out)
{
    s0 ^= rk(0u); s1 ^= rk(1u); s2 ^= rk(2u); s3 ^= rk(3u);
    IGDSP_SRTP_UNROLL
    for (uint32_t r = 1; r < 10u; ++r) {
        const uint32_t t0 = te(s0 >> 24) ^ srtp_ror(te((s1 >> 16) & 255u), 8) ^ srtp_ror(te((s2 >> 8) & 255u), 16) ^ srtp_ror(te(s3 & 255u), 24) ^ rk(4u * r);
        const uint32_t t1 = te(s1 >> 24) ^ srtp_ror(te((s2 >> 16) & 255u), 8) ^ srtp_ror(te((s3 >> 8) & 255u), 16) ^ srtp_ror(te(s0 & 255u), 24) ^ rk(4u * r + 1u);
        const uint32_t t2 = te(s2 >> 24) ^ srtp_ror(te((s3 >> 16) & 255u), 8) ^ srtp_ror(te((s0 >> 8) & 255u), 16) ^ srtp_ror(te(s1 & 255u), 24) ^ rk(4u * r + 2u);
        const uint32_t t3 = te(s3 >> 24) ^ srtp_ror(te((s0 >> 16) & 255u), 8) ^ srtp_ror(te((s1 >> 8) & 255u), 16) ^ srtp_ror(te(s2 & 255u), 24) ^ rk(4u * r + 3u);
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    auto sb = [&](uint32_t x) { return (te(x & 255u) >> 8) & 255u; };
    out[0] = ((sb(s0 >> 24) << 24) | (sb(s1 >> 16) << 16) | (sb(s2 >> 8) << 8) | sb(s3)) ^ rk(40u);
    out[1] = ((sb(s1 >> 24) << 24) | (sb(s2 >> 16) << 16) | (sb(s3 >> 8) << 8) | sb(s0)) ^ rk(41u);
    out[2] = ((sb(s2 >> 24) << 24) | (sb(s3 >> 16) << 16) | (sb(s0 >> 8) << 8) | sb(s1)) ^ rk(42u);
    out[3] = ((sb(s3 >> 24) << 24) | (sb(s0 >> 16) << 16) | (sb(s1 >> 8) << 8) | sb(s2)) ^ rk(43u);
}

// ---- SHA-1: one compression; the 16-word schedule is circular and stays in w
IGDSP_SRTP_HD void srtp_sha1(uint32_t (&h)[5], uint32_t (&w)[16])
{
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
    IGDSP_SRTP_UNROLL
    for (uint32_t t = 0; t < 80u; ++t) {
        if (t >= 16u) w[t & 15u] = srtp_rol(w[(t + 13u) & 15u] ^ w[(t + 8u) & 15u] ^ w[(t + 2u) & 15u] ^ w[t & 15u], 1);
        const uint32_t f = t < 20u ? (d ^ (b & (c ^ d))) : t < 40u ? (b ^ c ^ d) : t < 60u ? ((b & c) | (d & (b | c))) : (b ^ c ^ d);
        const uint32_t k = t < 20u ? 0x5A827999u : t < 40u ? 0x6ED9EBA1u : t < 60u ? 0x8F1BBCDCu : 0xCA62C1D6u;
        const uint32_t tmp = srtp_rol(a, 5) + f + e + k + w[t & 15u];
        e = d; d = c; c = srtp_rol(b, 30); b = a; a = tmp;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e;
}

// ---- what runs through a channel's frames, and what is known of one packet
struct SrtpLane {
    uint32_t tagw, roc, s_l, have;
    uint64_t win;
    uint32_t n_ok, n_auth, n_replay, n_mal;
};
struct SrtpPkt {
    uint32_t h, end, size_out, v, seq, ssrc, dist;    // end: the bytes under the tag (header and payload); dist: how far ahead of / behind top
    bool ahead;
};

IGDSP_SRTP_HD uint32_t srtp_tag_len(uint32_t tagw)                         // 0: no key
{
    const uint32_t n = tagw & 0xFFu;
    return ((tagw & 0xFFFFFF00u) == IGDSP_SRTP_TAG && (n == 4u || n == 10u)) ? n : 0u;
}
IGDSP_SRTP_HD uint32_t srtp_ctl(uint32_t v) { return v <= (uint32_t)IGDSP_SRTP_RESET ? v : (uint32_t)IGDSP_SRTP_RUN; }

IGDSP_SRTP_HD SrtpLane srtp_lane_read(const uint32_t (&w)[10])
{
    return SrtpLane{w[0], w[1], w[2] & 0xFFFFu, (w[2] >> 16) != 0u ? 1u : 0u, (uint64_t)w[4] | ((uint64_t)w[5] << 32), w[6], w[7], w[8], w[9]};
}
// the ten words back; w[3] (reserved) stays as it was read
IGDSP_SRTP_HD void srtp_lane_write(const SrtpLane &l, uint32_t (&w)[10])
{
    w[0] = l.tagw; w[1] = l.roc; w[2] = (l.s_l & 0xFFFFu) | (l.have << 16); w[4] = (uint32_t)l.win; w[5] = (uint32_t)(l.win >> 32);
    w[6] = l.n_ok; w[7] = l.n_auth; w[8] = l.n_replay; w[9] = l.n_mal;
}
IGDSP_SRTP_HD void srtp_lane_reset(SrtpLane &l) { l.roc = 0u; l.have = 0u; l.win = 0u; }

// the fixed header from the packet's first word (memory order): 0, or MALFORMED.  h = 12 + 4 CC; x: the extension's length is to be
// read at h + 2 (inside the packet: h + 4 <= size)
IGDSP_SRTP_HD uint32_t srtp_hdr_fixed(uint32_t w0, uint32_t size, uint32_t &h, bool &x)
{
    const uint32_t b0 = w0 & 0xFFu;
    h = 12u + 4u * (b0 & 15u);
    x = ((b0 >> 4) & 1u) != 0u;
    if ((b0 >> 6) != 2u || h > size || (x && h + 4u > size)) return IGDSP_SRTP_MALFORMED;
    return 0u;
}
IGDSP_SRTP_HD uint32_t srtp_hdr_ext(uint32_t ext_len, uint32_t size, uint32_t &h)
{
    h += 4u + 4u * (ext_len & 0xFFFFu);                                    // <= 72 + 4 + 262 140
    return h > size ? (uint32_t)IGDSP_SRTP_MALFORMED : 0u;
}
IGDSP_SRTP_HD uint32_t srtp_seq_of(uint32_t w0) { return ((w0 >> 8) & 0xFF00u) | (w0 >> 24); }

// RFC 3711 Appendix A, as written: integer comparisons, v mod 2^32
IGDSP_SRTP_HD uint32_t srtp_estimate(uint32_t roc, uint32_t s_l, uint32_t seq)
{
    if (s_l < 32768u) return ((int32_t)seq - (int32_t)s_l > 32768) ? roc - 1u : roc;
    return ((int32_t)s_l - 32768 > (int32_t)seq) ? roc + 1u : roc;
}

// sizes, index and (unprotect) the replay window: 0 to go on, else the refusal
template <int DIR>
IGDSP_SRTP_HD uint32_t srtp_admit(const SrtpLane &l, uint32_t tag_len, uint32_t size, uint32_t out_cap, SrtpPkt &p)
{
    if (DIR == kSrtpUnprotect) {
        if (size < p.h + tag_len) return IGDSP_SRTP_MALFORMED;
        p.end = size - tag_len;
        p.size_out = p.end;
    } else {
        p.end = size;
        p.size_out = size + tag_len;
    }
    if (p.size_out > out_cap) return IGDSP_SRTP_MALFORMED;
    const uint32_t s_l = l.have ? l.s_l : p.seq;
    p.v = srtp_estimate(l.roc, s_l, p.seq);
    const uint64_t index = ((uint64_t)p.v << 16) | p.seq, top = ((uint64_t)l.roc << 16) | s_l;
    p.ahead = !l.have || index > top;
    const uint64_t d = p.ahead ? index - top : top - index;
    p.dist = d < kSrtpWindow ? (uint32_t)d : kSrtpWindow;
    if (DIR == kSrtpUnprotect && !p.ahead) {
        if (p.dist >= kSrtpWindow) return IGDSP_SRTP_OLD;
        if ((l.win >> p.dist) & 1u) return IGDSP_SRTP_REPLAY;
    }
    return 0u;
}
IGDSP_SRTP_HD void srtp_refuse(SrtpLane &l, uint32_t flags)
{
    if (flags & IGDSP_SRTP_AUTH_FAIL) ++l.n_auth;
    else if (flags & (IGDSP_SRTP_REPLAY | IGDSP_SRTP_OLD)) ++l.n_replay;
    else if (flags & IGDSP_SRTP_MALFORMED) ++l.n_mal;
}
// an accepted packet: the record's flags
template <int DIR>
IGDSP_SRTP_HD uint32_t srtp_commit(SrtpLane &l, const SrtpPkt &p)
{
    uint32_t flags = IGDSP_SRTP_OK;
    ++l.n_ok;
    if (p.ahead) {
        if (DIR == kSrtpUnprotect) l.win = ((!l.have || p.dist >= kSrtpWindow) ? 0ull : l.win << p.dist) | 1ull;
        if (p.v != l.roc) flags |= IGDSP_SRTP_ROLLED;
        l.roc = p.v; l.s_l = p.seq; l.have = 1u;
    } else if (DIR == kSrtpUnprotect) {
        l.win |= 1ull << p.dist;                                           // dist < 64: srtp_admit
    }
    return flags;
}

// IV = (k_s 2^16) xor (SSRC 2^64) xor (index 2^16) as four big-endian words; ksw: the state's ks bytes as big-endian words
IGDSP_SRTP_HD void srtp_iv(const uint32_t (&ksw)[4], const SrtpPkt &p, uint32_t (&iv)[4])
{
    iv[0] = ksw[0]; iv[1] = ksw[1] ^ p.ssrc; iv[2] = ksw[2] ^ p.v; iv[3] = ksw[3] ^ (p.seq << 16);
}

// The keystream under piece j's 16 words, in memory order and masked to the bytes [h, end): x[i] is what packet word 16 j + i takes.
// h is a multiple of 4, so keystream word k = 16 j + i - h / 4 lies under packet word 16 j + i: with d = (h / 4) & 3 the piece takes
// the last d words of the AES block in front (carry, from the piece before) and then the blocks 4 j + t - (h / 16), t = 0..3, which
// are computed where anybody needs them.  carry: in and out, zero at piece 0.
template <class RK, class TE, class ANY>
IGDSP_SRTP_HD void srtp_ks_piece(const RK &rk, const TE &te, const ANY &any, const uint32_t (&iv)[4], uint32_t h, uint32_t end, uint32_t j,
                                 uint32_t (&carry)[4], uint32_t (&x)[16])
{
    const uint32_t hw = h >> 2, hq = hw >> 2, d = hw & 3u, pay = end - h;   // end >= h: srtp_admit
    uint32_t cat[20];
    cat[0] = carry[0]; cat[1] = carry[1]; cat[2] = carry[2]; cat[3] = carry[3];
    IGDSP_SRTP_UNROLL
    for (uint32_t t = 0; t < 4u; ++t) {
        const int32_t idx = (int32_t)(4u * j + t) - (int32_t)hq;           // < 2^7
        const bool need = idx >= 0 && (uint32_t)idx * 16u < pay;
        if (any(need)) {
            srtp_aes(rk, te, iv[0], iv[1], iv[2], iv[3] + ((uint32_t)idx & 0xFFFFu), &cat[4u + 4u * t]);
        } else {
            cat[4u + 4u * t] = 0u; cat[5u + 4u * t] = 0u; cat[6u + 4u * t] = 0u; cat[7u + 4u * t] = 0u;
        }
    }
    carry[0] = cat[16]; carry[1] = cat[17]; carry[2] = cat[18]; carry[3] = cat[19];
    // cat[4 + i - d] by two masked steps (written with masks: a select between neighbours is turned into an indexed read of cat[])
    const uint32_t m1 = 0u - (d & 1u), m2 = 0u - ((d >> 1) & 1u);
    uint32_t b[19];                                                        // b[i] = cat[i + 1 - (d & 1)]
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 0; i < 19u; ++i) b[i] = cat[i + 1u] ^ ((cat[i] ^ cat[i + 1u]) & m1);
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t k = b[i + 3u] ^ ((b[i + 1u] ^ b[i + 3u]) & m2);
        const uint32_t at = 4u * (16u * j + i);                            // the word's first byte
        const uint32_t nb = (at < h || at >= end) ? 0u : (end - at < 4u ? end - at : 4u);
        const uint32_t mask = nb >= 4u ? 0xFFFFFFFFu : ((1u << (8u * nb)) - 1u);
        x[i] = srtp_bswap(k) & mask;
    }
}

// SHA-1 blocks of the inner hash behind the key's: header || ciphertext || v, the padding and the length
IGDSP_SRTP_HD uint32_t srtp_hash_blocks(uint32_t end) { return (end + 4u + 9u + 63u) >> 6; }
// piece j of the message: c the packet's (ciphertext) words in memory order, bytes from `end` on ignored
IGDSP_SRTP_HD void srtp_hash_piece(uint32_t (&hs)[5], const uint32_t (&c)[16], uint32_t j, uint32_t end, uint32_t v)
{
    const uint32_t nblk = srtp_hash_blocks(end);
    if (j >= nblk) return;
    const uint32_t E = end >> 2, e = end & 3u;
    const uint64_t tail = (((uint64_t)v << 32) | 0x80000000ull) >> (8u * e);   // v, then the padding's first byte, from byte `end` on
    const uint32_t keep = e ? 0xFFFFFFFFu << (32u - 8u * e) : 0u;
    uint32_t w[16];
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t g = 16u * j + i, m = srtp_bswap(c[i]);
        w[i] = g < E ? m : (g == E ? ((m & keep) | (uint32_t)(tail >> 32)) : (g == E + 1u ? (uint32_t)tail : 0u));
    }
    if (j == nblk - 1u) w[15] = (64u + end + 4u) * 8u;                     // words 14 and 15 of the last block lie behind word E + 1
    srtp_sha1(hs, w);
}
// the outer hash: d = SHA-1(k_a xor opad || inner digest)
IGDSP_SRTP_HD void srtp_hmac_finish(const uint32_t (&hs)[5], const uint32_t (&mo)[5], uint32_t (&d)[5])
{
    uint32_t w[16];
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 0; i < 16u; ++i) w[i] = i < 5u ? hs[i] : 0u;
    w[5] = 0x80000000u;
    w[15] = (64u + 20u) * 8u;
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 0; i < 5u; ++i) d[i] = mo[i];
    srtp_sha1(d, w);
}
IGDSP_SRTP_HD uint32_t srtp_tag_byte(const uint32_t (&d)[5], uint32_t i)   // i a constant below 10
{
    return (d[i >> 2] >> (24u - 8u * (i & 3u))) & 0xFFu;
}
// the received tag's bytes that lie in piece j (pb: the piece's 64 bytes), gathered as the digest's words hold them
IGDSP_SRTP_HD void srtp_grab_tag(const uint8_t *pb, uint32_t j, uint32_t end, uint32_t tag_len, uint32_t (&rt)[3])
{
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 0; i < 10u; ++i) {
        const uint32_t at = end + i;
        if (i < tag_len && (at >> 6) == j) rt[i >> 2] |= (uint32_t)pb[at & 63u] << (24u - 8u * (i & 3u));
    }
}
IGDSP_SRTP_HD bool srtp_tag_equal(const uint32_t (&d)[5], const uint32_t (&rt)[3], uint32_t tag_len)
{
    const uint32_t diff = (d[0] ^ rt[0]) | (tag_len == 10u ? ((d[1] ^ rt[1]) | ((d[2] ^ rt[2]) & 0xFFFF0000u)) : 0u);
    return diff == 0u;
}

// ---- host only from here: key schedule, key derivation, one packet ------------------------------------------------------------------
inline uint32_t srtp_be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline void srtp_put_be32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

inline void srtp_aes_expand(const uint8_t key[16], uint32_t (&rk)[44])
{
    static const uint8_t rcon[10] = {0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1B, 0x36};
    auto sb = [](uint32_t x) { return (kSrtpTe0.t[x & 255u] >> 8) & 255u; };
    for (int i = 0; i < 4; ++i) rk[i] = srtp_be32(key + 4 * i);
    for (int i = 4; i < 44; ++i) {
        uint32_t t = rk[i - 1];
        if (i % 4 == 0) {
            t = srtp_rol(t, 8);
            t = ((sb(t >> 24) << 24) | (sb(t >> 16) << 16) | (sb(t >> 8) << 8) | sb(t)) ^ ((uint32_t)rcon[i / 4 - 1] << 24);
        }
        rk[i] = rk[i - 4] ^ t;
    }
}

// RFC 3711 4.3.1 at key derivation rate 0: n bytes of AES-CM_master((salt xor label 2^48) 2^16)
inline void srtp_kdf(const uint32_t (&mrk)[44], const uint8_t salt[14], uint8_t label, uint8_t *out, uint32_t n)
{
    uint8_t x[16] = {0};
    std::memcpy(x, salt, 14);
    x[7] ^= label;
    const uint32_t iv[4] = {srtp_be32(x), srtp_be32(x + 4), srtp_be32(x + 8), srtp_be32(x + 12)};
    for (uint32_t blk = 0; blk * 16u < n; ++blk) {
        uint32_t o[4];
        uint8_t b[16];
        srtp_aes(SrtpRkArray{mrk}, SrtpHostTe{}, iv[0], iv[1], iv[2], iv[3] + blk, o);
        for (int i = 0; i < 4; ++i) srtp_put_be32(b + 4 * i, o[i]);
        std::memcpy(out + blk * 16u, b, n - blk * 16u < 16u ? n - blk * 16u : 16u);
    }
}

// the session keys of the labels label0, label0 + 1, label0 + 2 (k_e, k_a, k_s) into a zeroed state: k_e's key schedule, k_s, the two midstates
inline void srtp_derive_keys(const uint8_t key_salt[30], uint8_t label0, igdsp_srtp_state &st)
{
    std::memset(&st, 0, sizeof(st));
    uint32_t mrk[44];
    uint8_t ke[16], ka[20];
    srtp_aes_expand(key_salt, mrk);
    srtp_kdf(mrk, key_salt + 16, label0, ke, 16);
    srtp_kdf(mrk, key_salt + 16, (uint8_t)(label0 + 1u), ka, 20);
    srtp_kdf(mrk, key_salt + 16, (uint8_t)(label0 + 2u), st.ks, 14);        // ks[14], ks[15] stay 0
    srtp_aes_expand(ke, st.rk);
    for (int side = 0; side < 2; ++side) {
        uint8_t blk[64];
        std::memset(blk, side ? 0x5C : 0x36, 64);
        for (int i = 0; i < 20; ++i) blk[i] ^= ka[i];
        uint32_t w[16], hs[5] = {0x67452301u, 0xEFCDAB89u, 0x98BADCFEu, 0x10325476u, 0xC3D2E1F0u};
        for (int i = 0; i < 16; ++i) w[i] = srtp_be32(blk + 4 * i);
        srtp_sha1(hs, w);
        std::memcpy(side ? st.mid_o : st.mid_i, hs, 20);
    }
}

inline bool srtp_derive(const uint8_t key_salt[30], uint32_t tag_len, uint32_t roc0, igdsp_srtp_state &st)
{
    if (tag_len != 4u && tag_len != 10u) return false;
    srtp_derive_keys(key_salt, 0, st);
    st.tag = IGDSP_SRTP_TAG | tag_len;
    st.roc = roc0;
    return true;
}

// piece j of a packet of `size` bytes as 16 words, zero behind the packet's end
inline void srtp_load_piece(const uint8_t *in, uint32_t size, uint32_t j, uint32_t (&pw)[16])
{
    std::memset(pw, 0, 64);
    if (64u * j < size) std::memcpy(pw, in + 64u * j, size - 64u * j < 64u ? size - 64u * j : 64u);
}
inline void srtp_store_piece(uint8_t *out, uint32_t len, uint32_t j, const uint32_t (&pw)[16])
{
    if (64u * j < len) std::memcpy(out + 64u * j, pw, len - 64u * j < 64u ? len - 64u * j : 64u);
}

// One packet.  in_cap: the input slot (a packet longer than it is MALFORMED); out_cap: the output's.  in == out is allowed.
template <int DIR>
inline void srtp_packet_run(igdsp_srtp_state &st, uint32_t ctl, const uint8_t *in, uint32_t size, uint32_t in_cap, uint8_t *out, uint32_t out_cap,
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
    const uint32_t tag_len = srtp_tag_len(sw[0]);
    if (!tag_len) return;                                                  // NO_KEY
    SrtpLane l = srtp_lane_read(sw);
    if (ctl == IGDSP_SRTP_RESET) srtp_lane_reset(l);
    auto close = [&](uint32_t flags, uint32_t v) {
        srtp_lane_write(l, sw);
        std::memcpy(&st, sw, sizeof(sw));
        rec.roc_used = v; rec.size_out = (uint16_t)size_out; rec.flags = (uint8_t)flags;
    };
    if (size == 0u) return close(IGDSP_SRTP_EMPTY, 0u);
    SrtpPkt p{};
    uint32_t pw[16], flags = 0u;
    if (size < 12u || !fits) {
        flags = IGDSP_SRTP_MALFORMED;
    } else {
        bool x = false;
        srtp_load_piece(in, size, 0, pw);
        flags = srtp_hdr_fixed(pw[0], size, p.h, x);
        if (!flags && x) flags = srtp_hdr_ext(((uint32_t)in[p.h + 2u] << 8) | in[p.h + 3u], size, p.h);   // p.h + 4 <= size: srtp_hdr_fixed
        p.seq = srtp_seq_of(pw[0]);
        p.ssrc = srtp_bswap(pw[2]);
    }
    if (!flags) flags = srtp_admit<DIR>(l, tag_len, size, out_cap, p);
    if (flags) {
        srtp_refuse(l, flags);
        return close(flags, (flags & (IGDSP_SRTP_OLD | IGDSP_SRTP_REPLAY)) ? p.v : 0u);
    }
    uint32_t ksw[4], iv[4], hs[5], d[5], carry[4] = {0u, 0u, 0u, 0u}, x[16];
    for (int i = 0; i < 4; ++i) ksw[i] = srtp_be32(st.ks + 4 * i);
    srtp_iv(ksw, p, iv);
    std::memcpy(hs, st.mid_i, 20);
    const uint32_t nblk = srtp_hash_blocks(p.end);
    if (DIR == kSrtpProtect) {
        for (uint32_t j = 0; j < nblk; ++j) {
            srtp_load_piece(in, size, j, pw);
            srtp_ks_piece(SrtpRkArray{st.rk}, SrtpHostTe{}, SrtpHostAny{}, iv, p.h, p.end, j, carry, x);
            for (int i = 0; i < 16; ++i) pw[i] ^= x[i];
            srtp_hash_piece(hs, pw, j, p.end, p.v);
            srtp_store_piece(out, p.end, j, pw);
        }
        srtp_hmac_finish(hs, st.mid_o, d);
        for (uint32_t i = 0; i < tag_len; ++i) out[p.end + i] = (uint8_t)((d[i >> 2] >> (24u - 8u * (i & 3u))) & 0xFFu);
    } else {
        uint32_t rt[3] = {0u, 0u, 0u};
        for (uint32_t j = 0; j < nblk; ++j) {
            srtp_load_piece(in, size, j, pw);
            srtp_grab_tag(reinterpret_cast<const uint8_t *>(pw), j, p.end, tag_len, rt);
            srtp_hash_piece(hs, pw, j, p.end, p.v);
        }
        srtp_hmac_finish(hs, st.mid_o, d);
        if (!srtp_tag_equal(d, rt, tag_len)) {
            srtp_refuse(l, IGDSP_SRTP_AUTH_FAIL);
            return close(IGDSP_SRTP_AUTH_FAIL, p.v);
        }
        for (uint32_t j = 0; 64u * j < p.end; ++j) {
            srtp_load_piece(in, size, j, pw);
            srtp_ks_piece(SrtpRkArray{st.rk}, SrtpHostTe{}, SrtpHostAny{}, iv, p.h, p.end, j, carry, x);
            for (int i = 0; i < 16; ++i) pw[i] ^= x[i];
            srtp_store_piece(out, p.end, j, pw);
        }
    }
    size_out = p.size_out;
    close(srtp_commit<DIR>(l, p), p.v);
}

}  // namespace igdsp
