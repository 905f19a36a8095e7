// igdsp_srtp_gcm.h — the AES-GCM SRTP rule (include/igdsp.h, "SRTP with AES-GCM"; independent restatement: tests/srtp_gcm_model.py) in
// plain C++17, so that the host entries igdsp_srtp_gcm_protect_packet / igdsp_srtp_gcm_unprotect_packet and the kernel k_srtp_gcm run the
// same code.  The header's length, the index estimate, the replay window, admit / commit / refuse, the table Te0 and the piece loads are
// igdsp_srtp.h's, used as they are (the first ten words of igdsp_srtp_gcm_state are igdsp_srtp_state's).  New here: an AES encrypt of 10
// or 14 rounds, the GHASH multiply, the keystream and the GHASH of one 64-byte piece, the per-packet function and the derive.
// A packet is walked in pieces of 64 bytes as in igdsp_srtp.h.  The keystream's blocks start at the header's end h (a multiple of 4, not
// of 16), so a piece takes up to three words of the block in front (carry), as SRTP's does.  GHASH's blocks are of two kinds: the AAD
// blocks cover [0, h) and lie on the piece's own 16-byte items; the ciphertext blocks start at h and straddle items and pieces.  A piece
// has four GHASH slots t = 0..3, slot number b = 4 j + t.  Slot b is an AAD block when 16 b < h.  Otherwise it is ciphertext block
// b - 1 - (h / 16): the 16 bytes that END in item t, taken from the last four words of the piece in front (carry) and this piece's words.
// Every ciphertext block is so hashed one slot late, which keeps the two kinds from ever sharing a slot and the order A, then C.  The
// last ciphertext block may therefore need one piece behind the data's last (srtp_gcm_pieces), as SHA-1's padding does in SRTP.
// The round count is a leg's own (legs of both key sizes stand side by side in a launch): rounds 1..9 always, rounds 10..13 where `any`
// lane holds a 256-bit key, the last round's keys at 4 nr.  NR != 0 fixes it at compile time (the derive).  Nothing indexes a private
// array by a run-time value except rk through its functor (LDS on the device, the state's array on the host).
#pragma once
#include "igdsp_srtp.h"

#if defined(__HIPCC__)
#define IGDSP_GCM_NOUNROLL _Pragma("nounroll")
#else
#define IGDSP_GCM_NOUNROLL
#endif

namespace igdsp {

static_assert(sizeof(igdsp_srtp_gcm_state) == 320 && offsetof(igdsp_srtp_gcm_state, window) == offsetof(igdsp_srtp_state, window) &&
              offsetof(igdsp_srtp_gcm_state, roc) == offsetof(igdsp_srtp_state, roc) && offsetof(igdsp_srtp_gcm_state, s_l) == offsetof(igdsp_srtp_state, s_l) &&
              offsetof(igdsp_srtp_gcm_state, n_ok) == offsetof(igdsp_srtp_state, n_ok) && offsetof(igdsp_srtp_gcm_state, n_malformed) == offsetof(igdsp_srtp_state, n_malformed) &&
              offsetof(igdsp_srtp_gcm_state, rk) == 40 && offsetof(igdsp_srtp_gcm_state, salt) == 280 && offsetof(igdsp_srtp_gcm_state, h) == 296,
              "capi.SRTP_GCM_STATE; the ten words that move are igdsp_srtp_state's; the state goes as 80 dwords");
static_assert((IGDSP_SRTP_GCM_TAG & 0xFFFFFF00u) != IGDSP_SRTP_TAG && (IGDSP_SRTP_GCM_TAG & 0xFFFFFF00u) != IGDSP_SRTCP_TAG && (IGDSP_SRTP_GCM_TAG & 0xFFu) == 0u,
              "a state of one suite is NO_KEY to the others' entries");

constexpr uint32_t kSrtpGcmStateWords = 80, kSrtpGcmTagLen = IGDSP_SRTP_GCM_TAG_LEN;

struct SrtpGcmRkArray {                                                    // the host's round keys: the state's array
    const uint32_t (&r)[60];
    uint32_t operator()(uint32_t i) const { return r[i]; }               // i <= 4 nr + 3 <= 59
};

// the key's bytes, 0: no key
IGDSP_SRTP_HD uint32_t srtp_gcm_key_bytes(uint32_t tagw)
{
    const uint32_t n = tagw & 0xFFu;
    return ((tagw & 0xFFFFFF00u) == IGDSP_SRTP_GCM_TAG && (n == 16u || n == 32u)) ? n : 0u;
}

template <class TE>
IGDSP_SRTP_HD void srtp_gcm_round(const TE &te, uint32_t (&s)[4], uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3)
{
    const uint32_t t0 = te(s[0] >> 24) ^ srtp_ror(te((s[1] >> 16) & 255u), 8) ^ srtp_ror(te((s[2] >> 8) & 255u), 16) ^ srtp_ror(te(s[3] & 255u), 24) ^ k0;
    const uint32_t t1 = te(s[1] >> 24) ^ srtp_ror(te((s[2] >> 16) & 255u), 8) ^ srtp_ror(te((s[3] >> 8) & 255u), 16) ^ srtp_ror(te(s[0] & 255u), 24) ^ k1;
    const uint32_t t2 = te(s[2] >> 24) ^ srtp_ror(te((s[3] >> 16) & 255u), 8) ^ srtp_ror(te((s[0] >> 8) & 255u), 16) ^ srtp_ror(te(s[1] & 255u), 24) ^ k2;
    const uint32_t t3 = te(s[3] >> 24) ^ srtp_ror(te((s[0] >> 16) & 255u), 8) ^ srtp_ror(te((s[1] >> 8) & 255u), 16) ^ srtp_ror(te(s[2] & 255u), 24) ^ k3;
    s[0] = t0; s[1] = t1; s[2] = t2; s[3] = t3;
}

// one block: s0..s3 the input as big-endian words, out the same.  NR 10 or 14: the round count at compile time; NR 0: nr (10 or 14) is
// the lane's own and rounds 10..13 run where any lane has 14
template <uint32_t NR, class RK, class TE, class ANY>
IGDSP_SRTP_HD void srtp_gcm_aes(const RK &rk, const TE &te, const ANY &any, uint32_t nr, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t *out)
{
    static_assert(NR == 0u || NR == 10u || NR == 14u, "AES-128 or AES-256");
    uint32_t s[4] = {s0 ^ rk(0u), s1 ^ rk(1u), s2 ^ rk(2u), s3 ^ rk(3u)};
    IGDSP_SRTP_UNROLL
    for (uint32_t r = 1; r < 10u; ++r) srtp_gcm_round(te, s, rk(4u * r), rk(4u * r + 1u), rk(4u * r + 2u), rk(4u * r + 3u));
    const bool longer = NR == 14u || (NR == 0u && nr == 14u);
    if (NR == 14u || (NR == 0u && any(longer))) {
        uint32_t t[4] = {s[0], s[1], s[2], s[3]};
        IGDSP_SRTP_UNROLL
        for (uint32_t r = 10; r < 14u; ++r) srtp_gcm_round(te, t, rk(4u * r), rk(4u * r + 1u), rk(4u * r + 2u), rk(4u * r + 3u));
        IGDSP_SRTP_UNROLL
        for (uint32_t i = 0; i < 4u; ++i) s[i] = longer ? t[i] : s[i];
    }
    const uint32_t last = NR ? 4u * NR : (longer ? 56u : 40u);
    auto sb = [&](uint32_t x) { return (te(x & 255u) >> 8) & 255u; };
    out[0] = ((sb(s[0] >> 24) << 24) | (sb(s[1] >> 16) << 16) | (sb(s[2] >> 8) << 8) | sb(s[3])) ^ rk(last);
    out[1] = ((sb(s[1] >> 24) << 24) | (sb(s[2] >> 16) << 16) | (sb(s[3] >> 8) << 8) | sb(s[0])) ^ rk(last + 1u);
    out[2] = ((sb(s[2] >> 24) << 24) | (sb(s[3] >> 16) << 16) | (sb(s[0] >> 8) << 8) | sb(s[1])) ^ rk(last + 2u);
    out[3] = ((sb(s[3] >> 24) << 24) | (sb(s[0] >> 16) << 16) | (sb(s[1] >> 8) << 8) | sb(s[2])) ^ rk(last + 3u);
}

// ---- GHASH: y = y . H in GF(2^128), GCM's convention (word 0 holds bits 0..31, bit 0 the most significant of word 0; the reduction is
// 0xE1 || 0^120).  Shoup's 4-bit tables: m[n] = n . H for the sixteen nibbles n (a nibble's top bit is its lowest power of x, so
// m[8] = H, m[4] = H x, m[2] = H x^2, m[1] = H x^3 and the others their XORs), built once per leg from H.  A multiply walks y's 32
// nibbles from the last (the highest powers) to the first by Horner's rule: Z = Z x^4 xor m[nibble], where Z x^4 is a shift right by
// four bits and the four bits that fall out come back as red[bits] = bits . x^128 into the top word.  A loop over y's four words with
// the eight nibbles of a word unrolled, so the body is one basic block (tools/srtp_gcm_bench.py's VALU_PER_GHASH_WORD counts it).
// TAB: how a table word is read (LDS on the device, a local array on the host)
struct SrtpGcmRed {
    uint32_t t[16];
};
constexpr SrtpGcmRed srtp_gcm_make_red()
{
    SrtpGcmRed r{};
    for (uint32_t i = 0; i < 16u; ++i)
        for (uint32_t b = 0; b < 4u; ++b)
            if ((i >> b) & 1u) r.t[i] ^= 0xE1000000u >> (3u - b);         // bit b of what falls out is x^(124 + 3 - b) x^4 = x^128 x^(3 - b)
    return r;
}
inline constexpr SrtpGcmRed kSrtpGcmRed = srtp_gcm_make_red();
static_assert(kSrtpGcmRed.t[1] == 0x1C200000u && kSrtpGcmRed.t[8] == 0xE1000000u && kSrtpGcmRed.t[15] == 0xB5E00000u, "the 4-bit reduction table of the GCM specification's 4.1");

IGDSP_SRTP_HD void srtp_gcm_table(const uint32_t (&hh)[4], uint32_t (&m)[16][4])
{
    IGDSP_SRTP_UNROLL
    for (uint32_t w = 0; w < 4u; ++w) { m[0][w] = 0u; m[8][w] = hh[w]; }
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 4; i >= 1u; i >>= 1) {                               // m[i] = m[2 i] x
        const uint32_t red = (0u - (m[2u * i][3] & 1u)) & 0xE1000000u;
        m[i][3] = (m[2u * i][3] >> 1) | (m[2u * i][2] << 31); m[i][2] = (m[2u * i][2] >> 1) | (m[2u * i][1] << 31);
        m[i][1] = (m[2u * i][1] >> 1) | (m[2u * i][0] << 31); m[i][0] = (m[2u * i][0] >> 1) ^ red;
    }
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 2; i <= 8u; i <<= 1) {
        IGDSP_SRTP_UNROLL
        for (uint32_t j = 1; j < i; ++j) {
            IGDSP_SRTP_UNROLL
            for (uint32_t w = 0; w < 4u; ++w) m[i + j][w] = m[i][w] ^ m[j][w];
        }
    }
}
struct SrtpGcmHostTab {
    const uint32_t (&m)[16][4];
    uint32_t h(uint32_t n, uint32_t w) const { return m[n & 15u][w]; }
    uint32_t r(uint32_t bits) const { return kSrtpGcmRed.t[bits & 15u]; }
};

template <class TAB>
IGDSP_SRTP_HD void srtp_gcm_mul(uint32_t (&y)[4], const TAB &tab)
{
    uint32_t z0 = 0u, z1 = 0u, z2 = 0u, z3 = 0u, xw = y[3], x2 = y[2], x1 = y[1], x0 = y[0];
    IGDSP_GCM_NOUNROLL
    for (uint32_t w = 0; w < 4u; ++w) {
        IGDSP_SRTP_UNROLL
        for (uint32_t k = 0; k < 8u; ++k) {
            const uint32_t n = (xw >> (4u * k)) & 15u, red = tab.r(z3 & 15u);
            z3 = (z3 >> 4) | (z2 << 28); z2 = (z2 >> 4) | (z1 << 28); z1 = (z1 >> 4) | (z0 << 28); z0 = (z0 >> 4) ^ red;
            z0 ^= tab.h(n, 0u); z1 ^= tab.h(n, 1u); z2 ^= tab.h(n, 2u); z3 ^= tab.h(n, 3u);
        }
        xw = x2; x2 = x1; x1 = x0;
    }
    y[0] = z0; y[1] = z1; y[2] = z2; y[3] = z3;
}

// pieces a pass over [0, end) walks: the data's, and the slot of the last ciphertext block, which lies one item behind the block's end
IGDSP_SRTP_HD uint32_t srtp_gcm_pieces(uint32_t h, uint32_t end)
{
    const uint32_t hw = h >> 2, nct = (end - h + 15u) >> 4;               // end >= h >= 12: srtp_admit
    const uint32_t last = nct ? (hw >> 2) + nct : ((hw + 3u) >> 2) - 1u;
    return (last >> 2) + 1u;
}

// the 12-byte IV as three big-endian words: k_s xor (00 00 || SSRC || v || SEQ); iv[3] is the counter of payload block 0
IGDSP_SRTP_HD void srtp_gcm_iv(const uint32_t (&ksw)[3], const SrtpPkt &p, uint32_t (&iv)[4])
{
    iv[0] = ksw[0] ^ (p.ssrc >> 16); iv[1] = ksw[1] ^ (p.ssrc << 16) ^ (p.v >> 16); iv[2] = ksw[2] ^ (p.v << 16) ^ (p.seq & 0xFFFFu); iv[3] = 2u;
}

// The keystream under piece j's 16 words, in memory order and masked to the bytes [h, end): srtp_ks_piece's alignment (which see) with
// this file's AES and GCM's 32-bit block counter
template <class RK, class TE, class ANY>
IGDSP_SRTP_HD void srtp_gcm_ks_piece(const RK &rk, const TE &te, const ANY &any, uint32_t nr, const uint32_t (&iv)[4], uint32_t h, uint32_t end, uint32_t j,
                                     uint32_t (&carry)[4], uint32_t (&x)[16])
{
    const uint32_t hw = h >> 2, hq = hw >> 2, d = hw & 3u, pay = end - h;
    uint32_t cat[20];
    cat[0] = carry[0]; cat[1] = carry[1]; cat[2] = carry[2]; cat[3] = carry[3];
    IGDSP_SRTP_UNROLL
    for (uint32_t t = 0; t < 4u; ++t) {
        const int32_t idx = (int32_t)(4u * j + t) - (int32_t)hq;           // < 2^7
        const bool need = idx >= 0 && (uint32_t)idx * 16u < pay;
        if (any(need)) {
            srtp_gcm_aes<0u>(rk, te, any, nr, iv[0], iv[1], iv[2], iv[3] + ((uint32_t)idx & 0xFFFFu), &cat[4u + 4u * t]);
        } else {
            cat[4u + 4u * t] = 0u; cat[5u + 4u * t] = 0u; cat[6u + 4u * t] = 0u; cat[7u + 4u * t] = 0u;
        }
    }
    carry[0] = cat[16]; carry[1] = cat[17]; carry[2] = cat[18]; carry[3] = cat[19];
    const uint32_t m1 = 0u - (d & 1u), m2 = 0u - ((d >> 1) & 1u);
    uint32_t b[19];                                                        // b[i] = cat[i + 1 - (d & 1)]
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 0; i < 19u; ++i) b[i] = cat[i + 1u] ^ ((cat[i] ^ cat[i + 1u]) & m1);
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t k = b[i + 3u] ^ ((b[i + 1u] ^ b[i + 3u]) & m2);     // cat[4 + i - d]
        const uint32_t at = 4u * (16u * j + i);
        const uint32_t nb = (at < h || at >= end) ? 0u : (end - at < 4u ? end - at : 4u);
        const uint32_t mask = nb >= 4u ? 0xFFFFFFFFu : ((1u << (8u * nb)) - 1u);
        x[i] = srtp_bswap(k) & mask;
    }
}

// GHASH over piece j: c the packet's words in memory order (the header in the clear, the payload as ciphertext), bytes from `end` on
// ignored.  carry: the last four ciphertext words of the piece in front, masked and as big-endian numbers; zero at piece 0
template <class ANY, class TAB>
IGDSP_SRTP_HD void srtp_gcm_ghash_piece(const ANY &any, const TAB &tab, const uint32_t (&c)[16], uint32_t j, uint32_t h, uint32_t end,
                                        uint32_t (&carry)[4], uint32_t (&y)[4])
{
    const uint32_t hw = h >> 2, hq = hw >> 2, d = hw & 3u, nct = (end - h + 15u) >> 4;
    uint32_t cat[20];
    cat[0] = carry[0]; cat[1] = carry[1]; cat[2] = carry[2]; cat[3] = carry[3];
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t at = 4u * (16u * j + i);
        const uint32_t nb = (at < h || at >= end) ? 0u : (end - at < 4u ? end - at : 4u);
        const uint32_t mask = nb >= 4u ? 0xFFFFFFFFu : ((1u << (8u * nb)) - 1u);
        cat[4u + i] = srtp_bswap(c[i] & mask);
    }
    carry[0] = cat[16]; carry[1] = cat[17]; carry[2] = cat[18]; carry[3] = cat[19];
    const uint32_t m1 = 0u - (d & 1u), m2 = 0u - ((d >> 1) & 1u);
    uint32_t s1[18];                                                       // s1[i] = cat[i + (d & 1)]
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 0; i < 18u; ++i) s1[i] = cat[i] ^ ((cat[i] ^ cat[i + 1u]) & m1);
    IGDSP_SRTP_UNROLL
    for (uint32_t t = 0; t < 4u; ++t) {
        const uint32_t slot = 4u * j + t;                                  // < 2^8
        const bool aad = 4u * slot < hw;
        const int32_t idx = (int32_t)slot - 1 - (int32_t)hq;
        const bool ct = !aad && idx >= 0 && (uint32_t)idx < nct;
        if (any(aad || ct)) {
            uint32_t x[4];
            IGDSP_SRTP_UNROLL
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t cw = s1[4u * t + k] ^ ((s1[4u * t + k] ^ s1[4u * t + k + 2u]) & m2);   // cat[4 t + d + k]: packet word hw + 4 idx + k
                const uint32_t aw = 4u * slot + k < hw ? srtp_bswap(c[4u * t + k]) : 0u;
                x[k] = y[k] ^ (aad ? aw : cw);
            }
            srtp_gcm_mul(x, tab);
            if (aad || ct) { y[0] = x[0]; y[1] = x[1]; y[2] = x[2]; y[3] = x[3]; }
        }
    }
}

// the length block, then the tag's four big-endian words: GHASH xor AES(J0)
template <class RK, class TE, class ANY, class TAB>
IGDSP_SRTP_HD void srtp_gcm_finish(const RK &rk, const TE &te, const ANY &any, uint32_t nr, const uint32_t (&iv)[4], const TAB &tab, uint32_t h, uint32_t end,
                                   uint32_t (&y)[4], uint32_t (&tag)[4])
{
    y[1] ^= 8u * h;                                                        // < 2^15 bits each: the upper words are zero
    y[3] ^= 8u * (end - h);
    srtp_gcm_mul(y, tab);
    uint32_t e[4];
    srtp_gcm_aes<0u>(rk, te, any, nr, iv[0], iv[1], iv[2], 1u, e);
    tag[0] = y[0] ^ e[0]; tag[1] = y[1] ^ e[1]; tag[2] = y[2] ^ e[2]; tag[3] = y[3] ^ e[3];
}

// the received tag's bytes that lie in piece j (pb: the piece's 64 bytes), gathered as big-endian words
IGDSP_SRTP_HD void srtp_gcm_grab_tag(const uint8_t *pb, uint32_t j, uint32_t end, uint32_t (&rt)[4])
{
    IGDSP_SRTP_UNROLL
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t at = end + i;
        if ((at >> 6) == j) rt[i >> 2] |= (uint32_t)pb[at & 63u] << (24u - 8u * (i & 3u));
    }
}
IGDSP_SRTP_HD bool srtp_gcm_tag_equal(const uint32_t (&a)[4], const uint32_t (&b)[4])
{
    return ((a[0] ^ b[0]) | (a[1] ^ b[1]) | (a[2] ^ b[2]) | (a[3] ^ b[3])) == 0u;
}

// ---- host only from here: key schedule, key derivation, one packet ------------------------------------------------------------------
// FIPS-197 5.2 for Nk = 4 (44 words) and Nk = 8 (60 words); the words behind the schedule stay zero
inline void srtp_gcm_aes_expand(const uint8_t *key, uint32_t key_bytes, uint32_t (&rk)[60])
{
    static const uint8_t rcon[10] = {0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1B, 0x36};
    auto sb = [](uint32_t x) { return (kSrtpTe0.t[x & 255u] >> 8) & 255u; };
    auto sub = [&](uint32_t t) { return (sb(t >> 24) << 24) | (sb(t >> 16) << 16) | (sb(t >> 8) << 8) | sb(t); };
    const uint32_t nk = key_bytes / 4u, total = 4u * (nk + 7u);           // 4 (Nr + 1)
    for (uint32_t i = 0; i < 60u; ++i) rk[i] = 0u;
    for (uint32_t i = 0; i < nk; ++i) rk[i] = srtp_be32(key + 4u * i);
    for (uint32_t i = nk; i < total; ++i) {
        uint32_t t = rk[i - 1u];
        if (i % nk == 0u) t = sub(srtp_rol(t, 8)) ^ ((uint32_t)rcon[i / nk - 1u] << 24);
        else if (nk > 6u && i % nk == 4u) t = sub(t);
        rk[i] = rk[i - nk] ^ t;
    }
}

template <uint32_t NR>
inline void srtp_gcm_aes_host(const uint32_t (&rk)[60], const uint32_t (&in)[4], uint32_t (&out)[4])
{
    srtp_gcm_aes<NR>(SrtpGcmRkArray{rk}, SrtpHostTe{}, SrtpHostAny{}, NR, in[0], in[1], in[2], in[3], out);
}

// RFC 3711 4.3.1 at key derivation rate 0 with AES of the master key's size: n bytes of AES-CM_master((salt14 xor label 2^48) 2^16)
template <uint32_t NR>
inline void srtp_gcm_kdf(const uint32_t (&mrk)[60], const uint8_t salt14[14], uint8_t label, uint8_t *out, uint32_t n)
{
    uint8_t x[16] = {0};
    std::memcpy(x, salt14, 14);
    x[7] ^= label;
    const uint32_t iv[4] = {srtp_be32(x), srtp_be32(x + 4), srtp_be32(x + 8), srtp_be32(x + 12)};
    for (uint32_t blk = 0; blk * 16u < n; ++blk) {
        const uint32_t ctr[4] = {iv[0], iv[1], iv[2], iv[3] + blk};
        uint32_t o[4];
        uint8_t b[16];
        srtp_gcm_aes_host<NR>(mrk, ctr, o);
        for (int i = 0; i < 4; ++i) srtp_put_be32(b + 4 * i, o[i]);
        std::memcpy(out + blk * 16u, b, n - blk * 16u < 16u ? n - blk * 16u : 16u);
    }
}

template <uint32_t NR>
inline void srtp_gcm_derive_keys(const uint8_t *key_salt, uint32_t key_bytes, igdsp_srtp_gcm_state &st)
{
    uint32_t mrk[60];
    uint8_t ke[32], salt14[14] = {0};
    std::memcpy(salt14, key_salt + key_bytes, 12);                         // the 96-bit master salt times 2^16: RFC 7714 11
    srtp_gcm_aes_expand(key_salt, key_bytes, mrk);
    srtp_gcm_kdf<NR>(mrk, salt14, 0, ke, key_bytes);
    srtp_gcm_kdf<NR>(mrk, salt14, 2, st.salt, 12);
    srtp_gcm_aes_expand(ke, key_bytes, st.rk);
    const uint32_t zero[4] = {0u, 0u, 0u, 0u};
    uint32_t hh[4];
    srtp_gcm_aes_host<NR>(st.rk, zero, hh);
    for (int i = 0; i < 4; ++i) srtp_put_be32(st.h + 4 * i, hh[i]);
}

// key_salt: key_bytes of master key, then 12 of master salt
inline bool srtp_gcm_derive(const uint8_t *key_salt, uint32_t key_bytes, uint32_t roc0, igdsp_srtp_gcm_state &st)
{
    if (key_bytes != 16u && key_bytes != 32u) return false;
    std::memset(&st, 0, sizeof(st));
    if (key_bytes == 16u) srtp_gcm_derive_keys<10u>(key_salt, key_bytes, st);
    else srtp_gcm_derive_keys<14u>(key_salt, key_bytes, st);
    st.tag = IGDSP_SRTP_GCM_TAG | key_bytes;
    st.roc = roc0;
    return true;
}

// One packet.  in_cap: the input slot (a packet longer than it is MALFORMED); out_cap: the output's.  in == out is allowed.
template <int DIR>
inline void srtp_gcm_packet_run(igdsp_srtp_gcm_state &st, uint32_t ctl, const uint8_t *in, uint32_t size, uint32_t in_cap, uint8_t *out, uint32_t out_cap,
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
    const uint32_t key_bytes = srtp_gcm_key_bytes(sw[0]);
    if (!key_bytes) return;                                                // NO_KEY
    const uint32_t nr = key_bytes == 32u ? 14u : 10u;
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
    if (!flags) flags = srtp_admit<DIR>(l, kSrtpGcmTagLen, size, out_cap, p);
    if (flags) {
        srtp_refuse(l, flags);
        return close(flags, (flags & (IGDSP_SRTP_OLD | IGDSP_SRTP_REPLAY)) ? p.v : 0u);
    }
    const SrtpGcmRkArray rk{st.rk};
    uint32_t ksw[3], hh[4], iv[4], y[4] = {0u, 0u, 0u, 0u}, tag[4], kc[4] = {0u, 0u, 0u, 0u}, gc[4] = {0u, 0u, 0u, 0u}, x[16];
    for (int i = 0; i < 3; ++i) ksw[i] = srtp_be32(st.salt + 4 * i);
    for (int i = 0; i < 4; ++i) hh[i] = srtp_be32(st.h + 4 * i);
    uint32_t gm[16][4];
    srtp_gcm_table(hh, gm);
    const SrtpGcmHostTab tab{gm};
    srtp_gcm_iv(ksw, p, iv);
    const uint32_t nb = srtp_gcm_pieces(p.h, p.end);
    if (DIR == kSrtpProtect) {
        for (uint32_t j = 0; j < nb; ++j) {
            srtp_load_piece(in, size, j, pw);
            srtp_gcm_ks_piece(rk, SrtpHostTe{}, SrtpHostAny{}, nr, iv, p.h, p.end, j, kc, x);
            for (int i = 0; i < 16; ++i) pw[i] ^= x[i];
            srtp_gcm_ghash_piece(SrtpHostAny{}, tab, pw, j, p.h, p.end, gc, y);
            srtp_store_piece(out, p.end, j, pw);
        }
        srtp_gcm_finish(rk, SrtpHostTe{}, SrtpHostAny{}, nr, iv, tab, p.h, p.end, y, tag);
        for (uint32_t i = 0; i < kSrtpGcmTagLen; ++i) out[p.end + i] = (uint8_t)(tag[i >> 2] >> (24u - 8u * (i & 3u)));
    } else {
        uint32_t rt[4] = {0u, 0u, 0u, 0u};
        const uint32_t nb1 = nb > ((size + 63u) >> 6) ? nb : ((size + 63u) >> 6);
        for (uint32_t j = 0; j < nb1; ++j) {
            srtp_load_piece(in, size, j, pw);
            srtp_gcm_grab_tag(reinterpret_cast<const uint8_t *>(pw), j, p.end, rt);
            if (j < nb) srtp_gcm_ghash_piece(SrtpHostAny{}, tab, pw, j, p.h, p.end, gc, y);
        }
        srtp_gcm_finish(rk, SrtpHostTe{}, SrtpHostAny{}, nr, iv, tab, p.h, p.end, y, tag);
        if (!srtp_gcm_tag_equal(tag, rt)) {
            srtp_refuse(l, IGDSP_SRTP_AUTH_FAIL);
            return close(IGDSP_SRTP_AUTH_FAIL, p.v);
        }
        for (uint32_t j = 0; 64u * j < p.end; ++j) {
            srtp_load_piece(in, size, j, pw);
            srtp_gcm_ks_piece(rk, SrtpHostTe{}, SrtpHostAny{}, nr, iv, p.h, p.end, j, kc, x);
            for (int i = 0; i < 16; ++i) pw[i] ^= x[i];
            srtp_store_piece(out, p.end, j, pw);
        }
    }
    size_out = p.size_out;
    close(srtp_commit<DIR>(l, p), p.v);
}

}  // namespace igdsp
