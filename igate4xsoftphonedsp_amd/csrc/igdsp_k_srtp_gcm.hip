// igdsp_k_srtp_gcm.hip — AES-GCM SRTP on the packets of a batch (igdsp_srtp_gcm_protect / igdsp_srtp_gcm_unprotect): AES-128 or AES-256
// counter mode over the payload, GHASH over header and ciphertext, the index estimate and the replay window per leg.  Semantics:
// include/igdsp.h, section "SRTP with AES-GCM"; the rule's arithmetic: igdsp_srtp_gcm.h (the host entries run the same functions on one
// packet) on top of igdsp_srtp.h; independent restatement: tests/srtp_gcm_model.py.
//
// Shape (route: srtp_gcm_route): k_srtp's, which see.  A lane owns a leg for the launch and walks f; 64 legs a wave, a block is one wave.
// A frame's packets pass through the 64 x 17-word LDS tile in pieces of 64 bytes (igdsp_k_srtp_tile.h's loads and stores): every load is
// bounded by the packet's size (s_lim) and its slot, whole 16-byte items go out wave-wide below s_full, the owner stores its odd tail,
// lanes past C store nothing, sizes and controls are loaded a frame ahead.  Loops are wave-uniform; what a lane needs is asked by ballot.
// Per lane in registers: the ten state words that move, k_s, the running GHASH, two carries of four words, a piece's 16 words.
// Protect is one pass: keystream, XOR, GHASH of the ciphertext just made, store; then the length block, AES(J0) and the tag's sixteen byte
// stores.  Unprotect must not write before the tag is known, so pass 1 runs GHASH only and stores nothing (no AES but J0's block), and
// pass 2 decrypts and stores what passed the compare.  GHASH's blocks do not lie on the tile's items: igdsp_srtp_gcm.h says how the
// slots of a piece are dealt (AAD blocks on their items, ciphertext blocks one slot late from a four-word carry).  The header's length
// is read from piece 0; only with X and CC >= 13 does it need piece 1 first.
// AES: the table Te0 in LDS, the other three by v_alignbit_b32; the round keys as [60][64] words in LDS; a leg's round count is its own
// (legs of both key sizes share a wave): rounds 10..13 run where a lane of the wave holds a 256-bit key.  The multiply is Shoup's with
// 4-bit tables: the sixteen multiples of a leg's H, built in the prologue from the state's 16 bytes of H by doubling and XOR, lie as
// [entry][word][lane] in LDS (16 KiB a block; the bank depends on the lane alone, so the lanes' own entries do not conflict), beside
// sixteen reduction words.  DESIGN 3.31 holds the bit-serial form's count from the saved ISA, which decided against it.
// MOVE (the compute-free yardstick, tools/srtp_gcm_bench.py): protect's loads, tile traffic, state load and store and stores, the header
// parse and the size rules; no AES round, no multiply: the packet goes out as it came, the tag's bytes as zeros, the state as read.
// Everything is written with vector stores in plain C++.
#include "igdsp_k_srtp_tile.h"
#include "igdsp_srtp_gcm.h"

namespace igdsp {

struct SrtpGcmArgs {
    const uint8_t *ctl, *pkts;
    const uint16_t *sizes;
    uint32_t C, F, stride;
    igdsp_srtp_gcm_state *state;
    uint8_t *out;
    uint32_t ostride;
    uint16_t *sizes_out;
    igdsp_srtp_rec *rec;
};

__device__ const SrtpTe0 d_srtp_gcm_te0 = srtp_make_te0();
__device__ const SrtpGcmRed d_srtp_gcm_red = srtp_gcm_make_red();

struct SrtpGcmLdsTab {                                                     // p: the lane's column of s_gh[16][4][64]; red: the sixteen reduction words
    const uint32_t *p, *red;
    __device__ __forceinline__ uint32_t h(uint32_t n, uint32_t w) const { return p[(n * 4u + w) * kSrtpChans]; }   // n < 16, w a constant below 4
    __device__ __forceinline__ uint32_t r(uint32_t bits) const { return red[bits]; }                              // bits < 16
};

// One pass over the pieces 0 .. maxb - 1 (wave-uniform).  go: the lane works its packet, nb its number of pieces in this pass.
// GRAB: gather the received tag; CRYPT: XOR the keystream into the row; GHASH: hash the row's ciphertext; STORE: the tile goes out
template <bool NT, bool GRAB, bool CRYPT, bool GHASH, bool STORE>
__device__ __forceinline__ void srtp_gcm_pass(const uint8_t *in_base, uint32_t stride, uint8_t *out_base, uint32_t ostride, uint32_t lane, bool go, uint32_t nb,
                                              uint32_t maxb, bool have0, uint32_t out_len, const SrtpPkt &p, uint32_t nr, const SrtpRkLds &rk,
                                              const uint32_t (&iv)[4], const SrtpGcmLdsTab &tab, uint32_t (&y)[4], uint32_t (&rt)[4], const uint32_t *s_te,
                                              uint32_t *s_tile, const uint32_t *s_lim, const uint32_t *s_full)
{
    uint32_t kc[4] = {0u, 0u, 0u, 0u}, gc[4] = {0u, 0u, 0u, 0u};
    uint32_t *row = s_tile + lane * kSrtpPitch;
    for (uint32_t j = 0; j < maxb; ++j) {
        if (!(j == 0u && have0)) srtp_load_tile<NT>(in_base, stride, j, s_lim, s_tile, lane);
        wave_lds_fence();
        if (go && j < nb) {
            uint32_t pw[16];
            if constexpr (GRAB) srtp_gcm_grab_tag(reinterpret_cast<const uint8_t *>(row), j, p.end, rt);
            if constexpr (CRYPT) {                                         // the keystream first: the row's words are not live through the AES rounds
                uint32_t x[16];
                srtp_gcm_ks_piece(rk, SrtpLdsTe{s_te}, SrtpWaveAny{}, nr, iv, p.h, p.end, j, kc, x);
#pragma unroll
                for (uint32_t i = 0; i < 16u; ++i) {
                    pw[i] = row[i] ^ x[i];
                    row[i] = pw[i];
                }
            } else {
#pragma unroll
                for (uint32_t i = 0; i < 16u; ++i) pw[i] = row[i];
            }
            if constexpr (!CRYPT && STORE) {                               // the yardstick: the row is read and written back as it is
#pragma unroll
                for (uint32_t i = 0; i < 16u; ++i) {
                    asm volatile("" : "+v"(pw[i]));
                    row[i] = pw[i];
                }
            }
            if constexpr (GHASH) srtp_gcm_ghash_piece(SrtpWaveAny{}, tab, pw, j, p.h, p.end, gc, y);
        }
        wave_lds_fence();
        if constexpr (STORE) {
            srtp_store_tile(out_base, ostride, j, s_full, s_tile, lane, out_len);
            wave_lds_fence();                                              // the next piece overwrites the tile
        }
    }
}

template <int DIR, bool MOVE>
__global__ __launch_bounds__(64) void k_srtp_gcm(const SrtpGcmArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_te[256];
    __shared__ uint32_t s_tile[kSrtpChans * kSrtpPitch];
    __shared__ uint32_t s_lim[kSrtpChans], s_full[kSrtpChans];
    __shared__ uint32_t s_rk[kSrtpGcmRkWords * kSrtpChans];
    __shared__ uint32_t s_gh[kSrtpGcmTabWords * kSrtpChans], s_red[16];
    const uint32_t lane = threadIdx.x;                                     // < 64: the block is one wave
    const uint64_t c0 = (uint64_t)blockIdx.x * kSrtpChans;                 // < C: the grid
    const uint32_t rows = (uint32_t)((uint64_t)a.C - c0 < kSrtpChans ? (uint64_t)a.C - c0 : kSrtpChans);
    const bool chan = lane < rows;
    const uint32_t c = chan ? (uint32_t)c0 + lane : a.C - 1u;              // lanes past the end load the last leg's state and store nothing
    if constexpr (!MOVE) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) s_te[i * 64u + lane] = d_srtp_gcm_te0.t[i * 64u + lane];
        if (lane < 16u) s_red[lane] = d_srtp_gcm_red.t[lane];
    }

    // ---- the state: twenty 16-byte loads per lane (d_state 16-byte aligned: the argument rule)
    const SrtpRkLds rk{s_rk + lane};
    const SrtpGcmLdsTab tab{s_gh + lane, s_red};
    uint32_t sw[10], ksw[3];
    {
        uint32_t all[kSrtpGcmStateWords];
        const uint4 *sp = reinterpret_cast<const uint4 *>(a.state + c);
#pragma unroll
        for (uint32_t i = 0; i < kSrtpGcmStateWords / 4u; ++i) {
            const uint4 v = sp[i];
            all[4u * i] = v.x; all[4u * i + 1u] = v.y; all[4u * i + 2u] = v.z; all[4u * i + 3u] = v.w;
        }
#pragma unroll
        for (uint32_t i = 0; i < 10u; ++i) sw[i] = all[i];
#pragma unroll
        for (uint32_t i = 0; i < kSrtpGcmRkWords; ++i)
            if constexpr (!MOVE) s_rk[i * kSrtpChans + lane] = all[10u + i];
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) ksw[i] = srtp_bswap(all[70u + i]);
        if constexpr (!MOVE) {                                             // the sixteen multiples of H, [entry][word][lane]: the bank is the lane's
            uint32_t hh[4], m[16][4];
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) hh[i] = srtp_bswap(all[74u + i]);
            srtp_gcm_table(hh, m);
#pragma unroll
            for (uint32_t i = 0; i < kSrtpGcmTabWords; ++i) s_gh[i * kSrtpChans + lane] = m[i >> 2][i & 3u];
        }
    }
    const uint32_t key_bytes = srtp_gcm_key_bytes(sw[0]), nr = key_bytes == 32u ? 14u : 10u;
    SrtpLane L = srtp_lane_read(sw);
    uint32_t *row = s_tile + lane * kSrtpPitch;
    const uint8_t *rowb = reinterpret_cast<const uint8_t *>(row);

    uint32_t size_n = a.sizes[c], ctl_n = (!MOVE && a.ctl) ? a.ctl[c] : (uint32_t)IGDSP_SRTP_RUN;
    for (uint32_t f = 0; f < a.F; ++f) {
        const uint32_t o = f * a.C + c;                                    // < 2^32 - 32: the argument rule
        const uint64_t t0 = (uint64_t)f * a.C + c0;                        // the frame's first slot of this block
        const uint8_t *in_base = a.pkts + t0 * a.stride;
        uint8_t *out_base = a.out + t0 * a.ostride;
        const uint32_t size = chan ? size_n : 0u, ctl = srtp_ctl(ctl_n);
        if (f + 1u < a.F) {                                                // in flight during the frame
            size_n = a.sizes[o + a.C];
            if (!MOVE && a.ctl) ctl_n = a.ctl[o + a.C];
        }

        // ---- what the lane does with its packet, in the host's order (srtp_gcm_packet_run)
        uint32_t flags = IGDSP_SRTP_NO_KEY, size_out = 0u, roc_used = 0u;
        const bool fits = size <= kSrtpMaxPacket && size <= a.stride;
        const bool bypass = ctl == IGDSP_SRTP_BYPASS, keyed = chan && !bypass && key_bytes != 0u;
        bool copy = false, hdr = false;
        if (chan && bypass) {
            if (size == 0u) flags = IGDSP_SRTP_EMPTY;
            else if (!fits || size > a.ostride) flags = IGDSP_SRTP_MALFORMED;
            else copy = true;
        } else if (keyed) {
            if (ctl == IGDSP_SRTP_RESET) srtp_lane_reset(L);
            if (size == 0u) flags = IGDSP_SRTP_EMPTY;
            else if (size < 12u || !fits) flags = IGDSP_SRTP_MALFORMED;
            else hdr = true;
        }
        s_lim[lane] = (hdr || copy) ? size : 0u;
        wave_lds_fence();

        // ---- the header: piece 0, and piece 1 where an extension's length lies behind 15 CSRCs
        SrtpPkt p{};
        bool x = false, have0 = true;
        uint32_t ext = 0u;
        srtp_load_tile<DIR == kSrtpProtect>(in_base, a.stride, 0u, s_lim, s_tile, lane);
        wave_lds_fence();
        if (hdr) {
            const uint32_t w0 = row[0];
            const uint32_t fl = srtp_hdr_fixed(w0, size, p.h, x);
            p.seq = srtp_seq_of(w0);
            p.ssrc = srtp_bswap(row[2]);
            if (fl) { flags = fl; hdr = false; }
        }
        const bool far = hdr && x && p.h + 2u >= kSrtpPiece;               // p.h <= 72: in piece 1; p.h + 4 <= size: loaded
        if (hdr && x && !far) ext = ((uint32_t)rowb[p.h + 2u] << 8) | rowb[p.h + 3u];
        if (__builtin_amdgcn_ballot_w64(far) != 0u) {
            wave_lds_fence();
            srtp_load_tile<false>(in_base, a.stride, 1u, s_lim, s_tile, lane);
            wave_lds_fence();
            if (far) ext = ((uint32_t)rowb[(p.h + 2u) & 63u] << 8) | rowb[(p.h + 3u) & 63u];
            wave_lds_fence();
            have0 = false;
        }
        if (hdr && x) {
            const uint32_t fl = srtp_hdr_ext(ext, size, p.h);
            if (fl) { flags = fl; hdr = false; }
        }
        if (hdr) {
            const uint32_t fl = srtp_admit<DIR>(L, kSrtpGcmTagLen, size, a.ostride, p);
            if (fl) { flags = fl; hdr = false; roc_used = (fl & (IGDSP_SRTP_OLD | IGDSP_SRTP_REPLAY)) ? p.v : 0u; }
        }
        if (!MOVE && keyed && flags != 0u) srtp_refuse(L, flags);          // (EMPTY counts nowhere)
        bool go = hdr;

        uint32_t iv[4], y[4] = {0u, 0u, 0u, 0u}, rt[4] = {0u, 0u, 0u, 0u};
        srtp_gcm_iv(ksw, p, iv);

        if constexpr (DIR == kSrtpProtect) {
            const uint32_t len = go ? p.end : (copy ? size : 0u);
            const uint32_t nb = (go && !MOVE) ? srtp_gcm_pieces(p.h, len) : (len + 63u) >> 6;
            wave_lds_fence();
            s_lim[lane] = len;
            s_full[lane] = len & ~15u;
            wave_lds_fence();
            const uint32_t maxb = wave_reduce_dpp(nb, OpMax{});
            srtp_gcm_pass<true, false, !MOVE, !MOVE, true>(in_base, a.stride, out_base, a.ostride, lane, go, nb, maxb, have0, len, p, nr, rk, iv, tab, y, rt, s_te,
                                                           s_tile, s_lim, s_full);
            if (go) {
                uint8_t *tag = out_base + (uint64_t)lane * a.ostride + p.end;   // p.end + 16 <= ostride: srtp_admit
                uint32_t d[4] = {0u, 0u, 0u, 0u};
                if constexpr (!MOVE) srtp_gcm_finish(rk, SrtpLdsTe{s_te}, SrtpWaveAny{}, nr, iv, tab, p.h, p.end, y, d);
#pragma unroll
                for (uint32_t i = 0; i < kSrtpGcmTagLen; ++i) tag[i] = (uint8_t)(d[i >> 2] >> (24u - 8u * (i & 3u)));
                flags = MOVE ? (uint32_t)IGDSP_SRTP_BYPASSED : srtp_commit<DIR>(L, p);
                size_out = p.size_out;
                roc_used = MOVE ? 0u : p.v;
            }
        } else {
            // pass 1: GHASH over header and ciphertext, the received tag gathered; nothing is stored
            const uint32_t np = go ? srtp_gcm_pieces(p.h, p.end) : 0u, ns = go ? (size + 63u) >> 6 : 0u, nb1 = np > ns ? np : ns;
            wave_lds_fence();
            s_lim[lane] = go ? size : 0u;
            wave_lds_fence();
            const uint32_t maxb1 = wave_reduce_dpp(nb1, OpMax{});
            srtp_gcm_pass<false, true, false, true, false>(in_base, a.stride, out_base, a.ostride, lane, go, nb1, maxb1, have0, 0u, p, nr, rk, iv, tab, y, rt, s_te,
                                                           s_tile, s_lim, s_full);
            if (go) {
                uint32_t d[4];
                srtp_gcm_finish(rk, SrtpLdsTe{s_te}, SrtpWaveAny{}, nr, iv, tab, p.h, p.end, y, d);
                if (!srtp_gcm_tag_equal(d, rt)) {
                    flags = IGDSP_SRTP_AUTH_FAIL;
                    srtp_refuse(L, flags);
                    roc_used = p.v;
                    go = false;
                }
            }
            // pass 2: the accepted packets are decrypted and stored, the bypassed ones copied
            const uint32_t len = go ? p.end : (copy ? size : 0u), nb2 = (len + 63u) >> 6;
            wave_lds_fence();
            s_lim[lane] = len;
            s_full[lane] = len & ~15u;
            wave_lds_fence();
            const uint32_t maxb2 = wave_reduce_dpp(nb2, OpMax{});
            srtp_gcm_pass<false, false, true, false, true>(in_base, a.stride, out_base, a.ostride, lane, go, nb2, maxb2, have0 && maxb1 <= 1u, len, p, nr, rk, iv,
                                                           tab, y, rt, s_te, s_tile, s_lim, s_full);
            if (go) {
                flags = srtp_commit<DIR>(L, p);
                size_out = p.size_out;
                roc_used = p.v;
            }
        }
        if (copy) { flags = IGDSP_SRTP_BYPASSED; size_out = size; }

        // ---- length and record: one store per lane, consecutive across the wave
        if (chan) {
            a.sizes_out[o] = (uint16_t)size_out;
            if (a.rec) *reinterpret_cast<uint2 *>(a.rec + o) = make_uint2(roc_used, size_out | (flags << 16));
        }
        wave_lds_fence();
    }

    // ---- the ten words that move go back once; a state without a key is not touched (the yardstick writes them as read)
    if (chan && key_bytes != 0u) {
        srtp_lane_write(L, sw);
        uint32_t *sp = reinterpret_cast<uint32_t *>(a.state + c);
        *reinterpret_cast<uint4 *>(sp) = make_uint4(sw[0], sw[1], sw[2], sw[3]);
        *reinterpret_cast<uint4 *>(sp + 4) = make_uint4(sw[4], sw[5], sw[6], sw[7]);
        *reinterpret_cast<uint2 *>(sp + 8) = make_uint2(sw[8], sw[9]);
    }
}

hipError_t launch_srtp_gcm(const LaunchCfg &, int dir, const uint8_t *ctl, const uint8_t *packets, const uint16_t *sizes, uint32_t C, uint32_t F, uint32_t pkt_stride,
                           igdsp_srtp_gcm_state *state, uint8_t *out, uint32_t out_stride, uint16_t *sizes_out, igdsp_srtp_rec *rec, bool yardstick, hipStream_t s)
{
    const SrtpRoute r = srtp_gcm_route(C, F, pkt_stride, out_stride, dir, yardstick);
    if (r.grid == 0) return hipSuccess;
    const SrtpGcmArgs a{ctl, packets, sizes, C, F, pkt_stride, state, out, out_stride, sizes_out, rec};
    if (r.move) hipLaunchKernelGGL((k_srtp_gcm<kSrtpProtect, true>), dim3(r.grid), dim3(r.threads), 0, s, a);
    else if (r.dir == kSrtpProtect) hipLaunchKernelGGL((k_srtp_gcm<kSrtpProtect, false>), dim3(r.grid), dim3(r.threads), 0, s, a);
    else hipLaunchKernelGGL((k_srtp_gcm<kSrtpUnprotect, false>), dim3(r.grid), dim3(r.threads), 0, s, a);
    return hipGetLastError();
}

}  // namespace igdsp
