// A stand-alone program for tests/test_srtp_gcm_san_cpu.py, compiled with -fsanitize=address,undefined against csrc/igdsp_srtp_gcm.h only:
// both per-packet rules (srtp_gcm_packet_run, what igdsp_srtp_gcm_protect_packet / igdsp_srtp_gcm_unprotect_packet call) over packets
// from the network's point of view: the malformed ones, a few thousand seeded random byte strings, well-formed packets with one field
// pushed out of bounds, a tampered stream across the sequence wrap under both key sizes, and states of random bytes and of the other
// suites.  Every input and output buffer is a heap block of exactly the size passed, so a read or write one byte outside it is reported.
// Exit code 0 and "ok <counts>" when nothing is; 2 when an outcome contradicts the rule's own promise (a refused packet with a size,
// bytes behind size_out written, a state without this suite's tag word that did anything).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "igdsp_srtp_gcm.h"

using namespace igdsp;

static uint64_t g_seed = 0x7714u;
static uint32_t rnd()
{
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_seed >> 33);
}

static int g_bad = 0;
static unsigned long g_counts[256];

// one call with exactly sized heap buffers; returns the record's flags
static uint32_t call(int dir, igdsp_srtp_gcm_state &st, uint32_t ctl, const std::vector<uint8_t> &pkt, uint32_t out_cap, bool in_place,
                     std::vector<uint8_t> *result = nullptr)
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
    if (dir == kSrtpProtect) srtp_gcm_packet_run<kSrtpProtect>(st, ctl, in, size, kSrtpMaxPacket, out, out_cap, n, rec);
    else srtp_gcm_packet_run<kSrtpUnprotect>(st, ctl, in, size, kSrtpMaxPacket, out, out_cap, n, rec);
    const bool done = (rec.flags & (IGDSP_SRTP_OK | IGDSP_SRTP_BYPASSED)) != 0;
    if (n != rec.size_out || n > out_cap || (!done && n != 0) || (done && n == 0)) g_bad = 1;
    for (uint32_t i = in_place ? (n > size ? n : size) : n; i < out_cap; ++i)
        if (out[i] != 0xA5) g_bad = 1;                                     // nothing at or behind size_out is written
    if (in_place && !done && size && std::memcmp(in, pkt.data(), size) != 0) g_bad = 1;   // a refused packet's slot stays as it was
    if (result) result->assign(out, out + n);
    ++g_counts[rec.flags];
    if (!in_place) std::free(out);
    std::free(in);
    return rec.flags;
}

static std::vector<uint8_t> well_formed(uint32_t size, uint32_t cc, int ext_len, uint32_t seq)
{
    std::vector<uint8_t> p(size);
    for (auto &b : p) b = (uint8_t)rnd();
    if (size >= 1u) p[0] = (uint8_t)(0x80u | (ext_len >= 0 ? 0x10u : 0u) | cc);
    if (size >= 4u) { p[2] = (uint8_t)(seq >> 8); p[3] = (uint8_t)seq; }
    if (ext_len >= 0 && 12u + 4u * cc + 4u <= size) { p[12 + 4 * cc + 2] = (uint8_t)(ext_len >> 8); p[12 + 4 * cc + 3] = (uint8_t)ext_len; }
    return p;
}

int main()
{
    uint8_t key[44];
    for (auto &b : key) b = (uint8_t)rnd();
    igdsp_srtp_gcm_state tx, rx;
    if (!srtp_gcm_derive(key, 16, 0, tx) || !srtp_gcm_derive(key, 32, 0, rx) || srtp_gcm_derive(key, 24, 0, rx) || srtp_gcm_derive(key, 0, 0, rx)) return 2;
    srtp_gcm_derive(key, 16, 0, rx);

    // ---- the malformed cases, in both directions, out of place and in place
    const uint32_t sizes[] = {0, 1, 11, 12, 13, 15, 16, 19, 20, 21, 27, 28, 29, 40, 71, 72, 75, 76, 87, 88, 2031, 2032, 2033, 2047, 2048, 2049, 4000};
    for (uint32_t size : sizes)
        for (uint32_t cc : {0u, 1u, 3u, 15u})
            for (int ext : {-1, 0, 1, 5, 200, 65535})
                for (int dir = 0; dir < 2; ++dir)
                    for (int ip = 0; ip < 2; ++ip) {
                        std::vector<uint8_t> p = well_formed(size, cc, ext, 100);
                        if (size && (rnd() & 7u) == 0u) p[0] = (uint8_t)((p[0] & 0x3Fu) | 0x40u);   // version 1
                        igdsp_srtp_gcm_state st = dir ? rx : tx;
                        call(dir, st, IGDSP_SRTP_RUN, p, size + (rnd() % 24u), ip != 0);
                    }

    // ---- seeded random byte strings as packets, any control value, any capacity
    for (int i = 0; i < 6000; ++i) {
        const uint32_t size = (i % 7 == 0) ? rnd() % 2100u : rnd() % 260u;
        std::vector<uint8_t> p(size);
        for (auto &b : p) b = (uint8_t)rnd();
        if (size && (i & 1)) p[0] = (uint8_t)((p[0] & 0x3Fu) | 0x80u);      // half of them pass the version test
        call(i & 1 ? kSrtpProtect : kSrtpUnprotect, (i & 2) ? tx : rx, rnd() % 5u, p, rnd() % 2200u, (i % 5) == 0);
    }

    // ---- a real stream through both rules under each key size, with packets tampered on the way: payloads around GHASH's block and the
    // pieces' boundaries, the wrap
    for (uint32_t kb : {16u, 32u}) {
        igdsp_srtp_gcm_state a, b;
        srtp_gcm_derive(key, kb, 0, a);
        srtp_gcm_derive(key, kb, 0, b);
        uint32_t seq = 65500;
        for (int i = 0; i < 900; ++i, ++seq) {
            const uint32_t cc = (uint32_t)(i % 4 == 3 ? 15 : i % 4), hdr = 12u + 4u * cc + (i % 3 == 0 ? 4u + 4u * (uint32_t)(i % 6) : 0u);
            const uint32_t size = hdr + rnd() % 200u + (i % 97 == 0 ? 1700u : 0u);
            std::vector<uint8_t> clear = well_formed(size, cc, i % 3 == 0 ? i % 6 : -1, seq & 0xFFFFu), prot, back;
            if (!(call(kSrtpProtect, a, IGDSP_SRTP_RUN, clear, size + 16u, false, &prot) & IGDSP_SRTP_OK) || prot.size() != size + 16u) { g_bad = 1; continue; }
            if (i % 11 == 0) {
                std::vector<uint8_t> t = prot;
                t[rnd() % t.size()] ^= (uint8_t)(1u << (rnd() & 7u));
                igdsp_srtp_gcm_state before = b;
                const uint32_t fl = call(kSrtpUnprotect, b, IGDSP_SRTP_RUN, t, size, (i & 1) != 0);
                if (fl & IGDSP_SRTP_OK) g_bad = 1;
                before.n_auth_fail = b.n_auth_fail; before.n_malformed = b.n_malformed; before.n_replay = b.n_replay;
                if (std::memcmp(&before, &b, sizeof(b)) != 0) g_bad = 1;    // a refusal moves a counter and nothing else
            }
            if (!(call(kSrtpUnprotect, b, IGDSP_SRTP_RUN, prot, size, (i & 1) != 0, &back) & IGDSP_SRTP_OK) || back != clear) g_bad = 1;
            if (i % 13 == 0 && call(kSrtpUnprotect, b, IGDSP_SRTP_RUN, prot, size, false) != IGDSP_SRTP_REPLAY) g_bad = 1;
        }
        if (a.roc != 1u || b.roc != 1u) g_bad = 1;
    }

    // ---- states of random bytes and the other suites' tag words: NO_KEY, nothing written, the state as it was (this suite's tag word over
    // random keys must work like any key)
    for (int i = 0; i < 400; ++i) {
        igdsp_srtp_gcm_state st, copy;
        uint8_t *raw = reinterpret_cast<uint8_t *>(&st);
        for (size_t k = 0; k < sizeof(st); ++k) raw[k] = (uint8_t)rnd();
        if (i % 6 == 1) st.tag = IGDSP_SRTP_GCM_TAG | 24u;
        if (i % 6 == 2) st.tag = IGDSP_SRTP_GCM_TAG | (i & 8 ? 16u : 32u);
        if (i % 6 == 3) st.tag = IGDSP_SRTP_TAG | 10u;
        if (i % 6 == 4) st.tag = IGDSP_SRTCP_TAG | 10u;
        const bool keyed = srtp_gcm_key_bytes(st.tag) != 0u;
        copy = st;
        std::vector<uint8_t> p = well_formed(12u + rnd() % 300u, 0, -1, rnd());
        const uint32_t fl = call(i & 1, st, IGDSP_SRTP_RUN, p, 2048, false);
        if (!keyed && (fl != IGDSP_SRTP_NO_KEY || std::memcmp(&st, &copy, sizeof(st)) != 0)) g_bad = 1;
    }

    std::printf("%s no_key=%lu ok=%lu auth_fail=%lu replay=%lu old=%lu malformed=%lu empty=%lu rolled=%lu bypassed=%lu\n", g_bad ? "BAD" : "ok", g_counts[0], g_counts[1],
                g_counts[2], g_counts[4], g_counts[8], g_counts[16], g_counts[32], g_counts[0x41], g_counts[128]);
    return g_bad ? 2 : 0;
}
