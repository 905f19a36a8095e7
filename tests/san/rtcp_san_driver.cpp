// A stand-alone program for tests/test_rtcp_san_cpu.py, compiled with -fsanitize=address,undefined against csrc/igdsp_rtcp.h and
// csrc/igdsp_srtp.h only: the per-packet rules (rtcp_parse_run, rtcp_build_run, srtcp_packet_run: what igdsp_rtcp_parse_packet,
// igdsp_rtcp_build_packet and igdsp_srtcp_*_packet call) over packets from the network's point of view: every malformed form, a few
// thousand seeded random byte strings through parse and unprotect, compounds with one field pushed out of bounds, a real stream with
// packets tampered on the way, and states of random bytes.  Every input and output buffer is a heap block of exactly the size passed,
// so a read or write one byte outside it is reported.  Exit code 0 and "ok <counts>" when nothing is; 2 when an outcome contradicts
// the rule's own promise (a refused packet with a size, bytes behind a size written, a refusal that moved more than its counter).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "igdsp_rtcp.h"

using namespace igdsp;

static uint64_t g_seed = 0x3550u;
static uint32_t rnd()
{
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_seed >> 33);
}

static int g_bad = 0;
static unsigned long g_srtcp[256], g_seen[256], g_built[16];

static uint32_t srtcp(int dir, igdsp_srtp_state &st, uint32_t ctl, const std::vector<uint8_t> &pkt, uint32_t out_cap, bool in_place, std::vector<uint8_t> *result = nullptr)
{
    const uint32_t size = (uint32_t)pkt.size();
    if (in_place && out_cap < size) out_cap = size;                        // in place the packet's buffer is the output's: one block of out_cap bytes
    const uint32_t in_bytes = in_place ? out_cap : size;
    uint8_t *in = static_cast<uint8_t *>(std::malloc(in_bytes ? in_bytes : 1));
    uint8_t *out = in;
    if (in_bytes) std::memset(in, 0xA5, in_bytes);
    if (size) std::memcpy(in, pkt.data(), size);
    if (!in_place) {
        out = static_cast<uint8_t *>(std::malloc(out_cap ? out_cap : 1));
        std::memset(out, 0xA5, out_cap ? out_cap : 1);
    }
    uint32_t n = 0xFFFFFFFFu;
    igdsp_srtp_rec rec;
    if (dir == kSrtpProtect) srtcp_packet_run<kSrtpProtect>(st, ctl, in, size, kSrtpMaxPacket, out, out_cap, n, rec);
    else srtcp_packet_run<kSrtpUnprotect>(st, ctl, in, size, kSrtpMaxPacket, out, out_cap, n, rec);
    const bool done = (rec.flags & (IGDSP_SRTP_OK | IGDSP_SRTP_BYPASSED)) != 0;
    if (n != rec.size_out || n > out_cap || (!done && n != 0) || (done && n == 0)) g_bad = 1;
    for (uint32_t i = in_place ? (n > size ? n : size) : n; i < out_cap; ++i)
        if (out[i] != 0xA5) g_bad = 1;                                     // nothing at or behind size_out is written
    if (in_place && !done && size && std::memcmp(in, pkt.data(), size) != 0) g_bad = 1;   // a refused packet's slot stays as it was
    if (result) result->assign(out, out + n);
    ++g_srtcp[rec.flags];
    if (!in_place) std::free(out);
    std::free(in);
    return rec.flags;
}

static igdsp_rtcp_seen parse(igdsp_rtcp_state &st, const std::vector<uint8_t> &pkt, uint32_t arrival, uint32_t local)
{
    const uint32_t size = (uint32_t)pkt.size();
    uint8_t *in = static_cast<uint8_t *>(std::malloc(size ? size : 1));
    if (size) std::memcpy(in, pkt.data(), size);
    igdsp_rtcp_state before = st;
    igdsp_rtcp_seen rec;
    rtcp_parse_run(st, in, size, kSrtpMaxPacket, arrival, local, rec);
    std::free(in);
    if (rec.flags == IGDSP_RTCP_MALFORMED) before.n_malformed += 1u;
    if (!(rec.flags & IGDSP_RTCP_PARSED) && std::memcmp(&before, &st, sizeof(st)) != 0) g_bad = 1;   // a refusal moves its counter and nothing else
    if (!(rec.flags & IGDSP_RTCP_PARSED) && rec.flags != IGDSP_RTCP_MALFORMED && rec.flags != IGDSP_RTCP_EMPTY) g_bad = 1;
    ++g_seen[rec.flags];
    return rec;
}

static std::vector<uint8_t> build(igdsp_rtcp_state &st, uint32_t ctl, const igdsp_jb_state *jb, uint32_t ssrc, uint32_t packets, uint64_t now, uint32_t L)
{
    uint8_t *out = static_cast<uint8_t *>(std::malloc(IGDSP_RTCP_MAX_BUILT));
    uint8_t *cname = static_cast<uint8_t *>(std::malloc(L ? L : 1));
    std::memset(out, 0xA5, IGDSP_RTCP_MAX_BUILT);
    for (uint32_t i = 0; i < L; ++i) cname[i] = (uint8_t)(1u + rnd() % 255u);
    const igdsp_rtcp_src src{ssrc, rnd(), packets, packets * 160u};
    uint32_t n = 0xFFFFFFFFu;
    igdsp_rtcp_built rec;
    rtcp_build_run(st, ctl, jb, src, now, L ? cname : nullptr, L, out, n, rec);      // (L above 64: the rule reads 64 bytes; the block holds L)
    if (n != rec.size || n > (uint32_t)IGDSP_RTCP_MAX_BUILT || (n & 3u) || (rtcp_ctl(ctl) == IGDSP_RTCP_NONE) != (n == 0u)) g_bad = 1;
    for (uint32_t i = n; i < (uint32_t)IGDSP_RTCP_MAX_BUILT; ++i)
        if (out[i] != 0xA5) g_bad = 1;
    ++g_built[rec.flags & 15u];
    std::vector<uint8_t> r(out, out + n);
    std::free(cname);
    std::free(out);
    return r;
}

static void put32(std::vector<uint8_t> &p, uint32_t v) { for (int s = 24; s >= 0; s -= 8) p.push_back((uint8_t)(v >> s)); }

int main()
{
    uint8_t key[30];
    for (auto &b : key) b = (uint8_t)rnd();
    igdsp_srtp_state tx, rx, rtp;
    srtcp_derive(key, 0, tx);
    srtcp_derive(key, 0, rx);
    if (!srtp_derive(key, 10, 0, rtp)) return 2;

    // ---- parse: every size around the rule's bounds, the first word's every version / padding / count and the types around 200..204
    for (uint32_t size : {0u, 1u, 3u, 4u, 7u, 8u, 9u, 12u, 28u, 31u, 32u, 52u, 2044u, 2048u, 2049u, 2052u, 4000u})
        for (uint32_t b0 = 0; b0 < 256u; b0 += 5u)
            for (uint32_t pt : {0u, 199u, 200u, 201u, 202u, 203u, 204u, 255u})
                for (uint32_t len : {0u, 1u, 6u, 7u, 12u, 510u, 511u, 65535u}) {
                    std::vector<uint8_t> p(size);
                    for (auto &b : p) b = (uint8_t)rnd();
                    if (size >= 4u) { p[0] = (uint8_t)b0; p[1] = (uint8_t)pt; p[2] = (uint8_t)(len >> 8); p[3] = (uint8_t)len; }
                    igdsp_rtcp_state st{};
                    parse(st, p, rnd(), rnd());
                }
    // ---- parse: seeded random byte strings behind a sound first header, and compounds of random sub-packets that fit exactly
    igdsp_rtcp_state wild{};
    for (int i = 0; i < 6000; ++i) {
        std::vector<uint8_t> p;
        const uint32_t local = 0x77u;
        const uint32_t subs = 1u + rnd() % 5u;
        for (uint32_t s = 0; s < subs; ++s) {
            const uint32_t pt = s == 0 ? 200u + (rnd() & 1u) : 200u + rnd() % 6u, rc = rnd() % 4u;
            uint32_t words = (pt == 200u ? 7u : 2u) + 6u * rc + rnd() % 3u;
            if (pt >= 202u) words = 1u + rc + rnd() % 6u;
            if (i % 9 == 0) words = rnd() % 12u + 1u;                       // often too short for its count
            put32(p, ((0x80u | rc | ((s + 1u == subs && (rnd() & 7u) == 0u) ? 0x20u : 0u)) << 24) | (pt << 16) | ((words - 1u) & 0xFFFFu));
            for (uint32_t k = 1; k < words; ++k) put32(p, (rnd() & 3u) ? rnd() : local);
            if (i % 7 == 0 && s == 0 && words > 8u) { p[8 + 16] = 0; p[8 + 17] = 0; p[8 + 18] = 0; p[8 + 19] = 0; }
        }
        if (i % 5 == 0) p[4u * (rnd() % (uint32_t)(p.size() / 4u))] ^= (uint8_t)(0x40u << (rnd() & 1u));   // a version bit somewhere
        if (i % 11 == 0) p.resize(p.size() - 1u - rnd() % 4u);
        if (i % 13 == 0 && p.size() > 8u) { p[2] = (uint8_t)rnd(); p[3] = (uint8_t)rnd(); }                 // the first length anywhere
        parse(wild, p, rnd(), local);
    }
    for (int i = 0; i < 3000; ++i) {
        std::vector<uint8_t> p(4u * (rnd() % 80u) + (i % 3 == 0 ? rnd() % 4u : 0u));
        for (auto &b : p) b = (uint8_t)rnd();
        if (p.size() >= 2u && (i & 1)) { p[0] = (uint8_t)(0x80u | (rnd() & 31u)); p[1] = (uint8_t)(200u + (rnd() & 1u)); }
        parse(wild, p, rnd(), rnd());
    }

    // ---- build -> protect -> (tamper) -> unprotect -> parse: a real exchange, every CNAME length, with and without a block
    igdsp_rtcp_state a{}, b{};
    igdsp_srtp_state sa, sb;
    srtcp_derive(key, 1, sa);
    srtcp_derive(key, 0, sb);
    igdsp_jb_state jb{};
    uint64_t now = 0x83AA7E8000000000ull;
    for (int i = 0; i < 1500; ++i, now += 0x500000000ull + rnd()) {
        jb.flags = (i % 5) ? IGDSP_JB_HEARD : 0;
        jb.ssrc = 0x77u; jb.base_seq = 100; jb.max_seq = (uint16_t)(100 + 50 * i); jb.cycles = ((100u + 50u * (uint32_t)i) >> 16) << 16;
        jb.received = 40u * (uint32_t)i + rnd() % 20u; jb.jitter = rnd() & 0xFFFFFu; jb.epoch = (uint32_t)(i / 400);
        const uint32_t ctl = i % 17 == 0 ? 0u : (i % 19 == 0 ? 77u : 1u + (uint32_t)(i % 7 == 0));
        const std::vector<uint8_t> clear = build(a, ctl, i % 3 ? &jb : nullptr, 0xA0A0u, (uint32_t)(i / 2), now, (uint32_t)(i % 80));
        if (clear.empty()) continue;
        std::vector<uint8_t> prot, back;
        if (srtcp(kSrtpProtect, sa, IGDSP_SRTP_RUN, clear, (uint32_t)clear.size() + 14u, (i & 1) != 0, &prot) != IGDSP_SRTP_OK || prot.size() != clear.size() + 14u) { g_bad = 1; continue; }
        if (i % 11 == 0) {
            std::vector<uint8_t> t = prot;
            t[rnd() % t.size()] ^= (uint8_t)(1u << (rnd() & 7u));
            igdsp_srtp_state before = sb;
            const uint32_t fl = srtcp(kSrtpUnprotect, sb, IGDSP_SRTP_RUN, t, (uint32_t)clear.size(), (i & 1) != 0);
            if (fl & IGDSP_SRTP_OK) g_bad = 1;
            before.n_auth_fail = sb.n_auth_fail; before.n_malformed = sb.n_malformed; before.n_replay = sb.n_replay;
            if (std::memcmp(&before, &sb, sizeof(sb)) != 0) g_bad = 1;      // a refusal moves a counter and nothing else
        }
        if (srtcp(kSrtpUnprotect, sb, IGDSP_SRTP_RUN, prot, (uint32_t)clear.size(), (i & 1) != 0, &back) != IGDSP_SRTP_OK || back != clear) g_bad = 1;
        if (i % 13 == 0 && srtcp(kSrtpUnprotect, sb, IGDSP_SRTP_RUN, prot, 2048, false) != IGDSP_SRTP_REPLAY) g_bad = 1;
        const igdsp_rtcp_seen seen = parse(b, back, (uint32_t)(now >> 16) + 100u, 0x77u);
        if (!(seen.flags & IGDSP_RTCP_PARSED) || ((seen.flags & IGDSP_RTCP_GOT_BLOCK) != 0) != ((i % 3) && (i % 5))) g_bad = 1;
    }
    // an old packet, a cleartext one (E = 0 under a sound tag cannot be made without the key: the flag is reached through protect's own output
    // with the E bit cleared and the tag recomputed by a second protect of the index word's state), BYPASS, RESET, EMPTY
    {
        std::vector<uint8_t> first, p(28, 0);
        p[0] = 0x80; p[1] = 201;
        igdsp_srtp_state s1, s2;
        srtcp_derive(key, 0, s1);
        srtcp_derive(key, 0, s2);
        srtcp(kSrtpProtect, s1, IGDSP_SRTP_RUN, p, 64, false, &first);
        for (int i = 0; i < 70; ++i) {
            std::vector<uint8_t> q;
            srtcp(kSrtpProtect, s1, IGDSP_SRTP_RUN, p, 64, false, &q);
            srtcp(kSrtpUnprotect, s2, IGDSP_SRTP_RUN, q, 64, false);
        }
        if (srtcp(kSrtpUnprotect, s2, IGDSP_SRTP_RUN, first, 64, false) != IGDSP_SRTP_OLD) g_bad = 1;
        if (srtcp(kSrtpUnprotect, s2, IGDSP_SRTP_RESET, first, 64, true) != IGDSP_SRTP_OK) g_bad = 1;
        srtcp(kSrtpProtect, s1, IGDSP_SRTP_BYPASS, p, 28, false);
        srtcp(kSrtpProtect, s1, IGDSP_SRTP_RUN, std::vector<uint8_t>(), 0, false);
        // E = 0: the sender's keys are ours, so the tag over the clear packet and a clear index word is made with the rule's own hash
        igdsp_srtp_state s3;
        srtcp_derive(key, 0, s3);
        std::vector<uint8_t> c = p;
        put32(c, 500u);
        uint32_t hs[5], d[5], pw[16];
        std::memcpy(hs, s3.mid_i, 20);
        for (uint32_t j = 0; j < srtp_hash_blocks(28); ++j) { srtp_load_piece(p.data(), 28, j, pw); srtp_hash_piece(hs, pw, j, 28, 500u); }
        srtp_hmac_finish(hs, s3.mid_o, d);
        for (uint32_t i = 0; i < 10u; ++i) c.push_back((uint8_t)srtp_tag_byte(d, i));
        std::vector<uint8_t> back;
        if (srtcp(kSrtpUnprotect, s3, IGDSP_SRTP_RUN, c, 28, false, &back) != (IGDSP_SRTP_OK | IGDSP_SRTCP_CLEAR) || back != p) g_bad = 1;
    }

    // ---- unprotect and protect: random byte strings, any control value, any capacity; every size around the rule's bounds
    for (int i = 0; i < 6000; ++i) {
        const uint32_t size = (i % 7 == 0) ? rnd() % 2100u : rnd() % 260u;
        std::vector<uint8_t> p(size);
        for (auto &b : p) b = (uint8_t)rnd();
        if (size && (i & 1)) p[0] = (uint8_t)((p[0] & 0x3Fu) | 0x80u);
        srtcp(i % 3 ? kSrtpUnprotect : kSrtpProtect, (i & 2) ? tx : rx, rnd() % 5u, p, rnd() % 2200u, (i % 5) == 0);
    }
    for (uint32_t size : {1u, 7u, 8u, 9u, 12u, 21u, 22u, 23u, 24u, 26u, 2032u, 2034u, 2036u, 2046u, 2048u, 2049u, 4000u})
        for (int dir = 0; dir < 2; ++dir)
            for (int ip = 0; ip < 2; ++ip)
                for (uint32_t cap : {0u, 7u, 8u, size - 14u, size, size + 13u, size + 14u, 2048u}) {
                    std::vector<uint8_t> p(size, 0x80);
                    igdsp_srtp_state st = dir ? rx : tx;
                    srtcp(dir, st, IGDSP_SRTP_RUN, p, cap > 5000u ? 0u : cap, ip != 0);
                }

    // ---- states of random bytes: NO_KEY for SRTCP unless the tag word is SRTCP's (an SRTP state is no key here); any RTCP state is tolerated
    for (int i = 0; i < 400; ++i) {
        igdsp_srtp_state st, copy;
        uint8_t *raw = reinterpret_cast<uint8_t *>(&st);
        for (size_t k = 0; k < sizeof(st); ++k) raw[k] = (uint8_t)rnd();
        if (i % 4 == 1) st.tag = IGDSP_SRTP_TAG | 10u;
        if (i % 4 == 2) st.tag = IGDSP_SRTCP_TAG | 10u;
        if (i % 8 == 3) st.tag = IGDSP_SRTCP_TAG | 4u;
        const bool keyed = srtcp_tag_len(st.tag) != 0u;
        copy = st;
        std::vector<uint8_t> p(8u + 4u * (rnd() % 60u) + (i & 1 ? 14u : 0u), 0x80);
        const uint32_t fl = srtcp(i & 1, st, IGDSP_SRTP_RUN, p, 2048, false);
        if (!keyed && (fl != IGDSP_SRTP_NO_KEY || std::memcmp(&st, &copy, sizeof(st)) != 0)) g_bad = 1;
        if (keyed && fl == IGDSP_SRTP_NO_KEY) g_bad = 1;
        igdsp_rtcp_state rs;
        raw = reinterpret_cast<uint8_t *>(&rs);
        for (size_t k = 0; k < sizeof(rs); ++k) raw[k] = (uint8_t)rnd();
        const std::vector<uint8_t> built = build(rs, 1u + (uint32_t)(i & 1), &jb, rnd(), rnd(), now, rnd() % 70u);
        const igdsp_rtcp_seen seen = parse(rs, built, rnd(), 0x77u);
        if (!(seen.flags & IGDSP_RTCP_PARSED)) g_bad = 1;
    }
    if (srtcp(kSrtpProtect, rtp, IGDSP_SRTP_RUN, std::vector<uint8_t>(28, 0x80), 64, false) != IGDSP_SRTP_NO_KEY) g_bad = 1;

    unsigned long parsed = 0, rtt = 0, neg = 0, bye = 0, sr = 0, blk = 0, clear = 0;
    for (int f = 0; f < 256; ++f) {
        if (f & IGDSP_RTCP_PARSED) parsed += g_seen[f];
        if (f & IGDSP_RTCP_GOT_RTT) rtt += g_seen[f];
        if (f & IGDSP_RTCP_RTT_NEGATIVE) neg += g_seen[f];
        if (f & IGDSP_RTCP_GOT_BYE) bye += g_seen[f];
        if (f & IGDSP_RTCP_GOT_SR) sr += g_seen[f];
        if (f & IGDSP_RTCP_GOT_BLOCK) blk += g_seen[f];
    }
    clear = g_srtcp[IGDSP_SRTP_OK | IGDSP_SRTCP_CLEAR];
    std::printf("%s no_key=%lu ok=%lu auth_fail=%lu replay=%lu old=%lu srtcp_malformed=%lu srtcp_empty=%lu clear=%lu bypassed=%lu parsed=%lu malformed=%lu empty=%lu "
                "got_sr=%lu got_block=%lu got_rtt=%lu rtt_negative=%lu got_bye=%lu built_sr=%lu built_rr=%lu built_sr_block=%lu built_rr_block_bye=%lu\n",
                g_bad ? "BAD" : "ok", g_srtcp[0], g_srtcp[1], g_srtcp[2], g_srtcp[4], g_srtcp[8], g_srtcp[16], g_srtcp[32], clear, g_srtcp[128], parsed,
                g_seen[IGDSP_RTCP_MALFORMED], g_seen[IGDSP_RTCP_EMPTY], sr, blk, rtt, neg, bye, g_built[1], g_built[2], g_built[5], g_built[14]);
    return g_bad ? 2 : 0;
}
