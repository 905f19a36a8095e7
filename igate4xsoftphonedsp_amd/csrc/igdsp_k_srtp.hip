// igdsp_k_srtp.hip — SRTP on the packets of a batch (igdsp_srtp_protect / igdsp_srtp_unprotect): AES-128 counter mode over the payload,
// HMAC-SHA1 over header, ciphertext and rollover counter, the index estimate and the replay window per leg.  Semantics: include/igdsp.h,
// section "SRTP"; the rule's arithmetic: igdsp_srtp.h (the host entries run the same functions on one packet); independent
// restatement: tests/srtp_model.py.
//
// Shape (route: srtp_route).  The index and the window are serial in a channel's frames (the next estimate depends on whether this
// packet authenticated), so a lane owns a channel for the launch and walks f; 64 channels a wave, a block is one wave.  Per lane in
// registers: the ten state words that move, k_s, the two SHA-1 midstates, the running hash, a piece's 16 words.
// A frame's 64 packets are one run of 64 x stride bytes.  They pass through an LDS tile piece by piece, a piece being 64 bytes of every
// packet (one SHA-1 block, four AES blocks), so the tile is 64 rows of 16 words whatever the stride (row pitch 17 words: a lane's read
// of word i of its row and the wave's 16-byte writes fall on different banks).  Per piece:
//   - the wave loads it, 16 bytes a lane and turn, four turns, only below each packet's size (s_lim) and never past the packet's slot;
//   - each lane reads its row, XORs the keystream (srtp_ks_piece: AES blocks only where some lane of the wave needs one), writes the
//     row back and runs its SHA-1 block (lanes past their packet's last block are masked);
//   - the wave stores the whole 16-byte items below each packet's length (s_full); the owner stores the odd tail from its row.
// Protect is one such pass, then the outer hash and the tag's byte stores.  Unprotect must not write before the tag is known (a refused
// packet leaves its slot alone, in place too), so it hashes in a first pass that stores nothing and decrypts in a second (the loads of
// the second hit the cache).  The header's length is read from piece 0; only with X and CC >= 13 does it need piece 1 first.
// AES: one 1 KiB table Te0 in LDS, the other three by v_alignbit_b32; the round keys as [word][lane] in LDS (as 44 VGPRs the kernel
// takes 276 to 289 registers and one wave a SIMD; in LDS 236 to 238 and two).  DESIGN 3.29 says what else was costed.
// MOVE (the compute-free yardstick, tools/srtp_bench.py): protect's loads, tile traffic, state load and store and stores, the header
// parse and the size rules; no AES round, no compression: the packet goes out as it came, the tag's bytes as zeros, the state as read.
// Everything is written with vector stores in plain C++.
#include "igdsp_k_srtp_tile.h"

namespace igdsp {

__device__ const SrtpTe0 d_srtp_te0 = srtp_make_te0();

template <int DIR, bool MOVE>
__global__ __launch_bounds__(64) void k_srtp(const SrtpArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_te[256];
    __shared__ uint32_t s_tile[kSrtpChans * kSrtpPitch];
    __shared__ uint32_t s_lim[kSrtpChans], s_full[kSrtpChans];
    const uint32_t lane = threadIdx.x;                                     // < 64: the block is one wave
    const uint64_t c0 = (uint64_t)blockIdx.x * kSrtpChans;                 // < C: the grid
    const uint32_t rows = (uint32_t)((uint64_t)a.C - c0 < kSrtpChans ? (uint64_t)a.C - c0 : kSrtpChans);
    const bool chan = lane < rows;
    const uint32_t c = chan ? (uint32_t)c0 + lane : a.C - 1u;              // lanes past the end load the last channel's state and store nothing
    if constexpr (!MOVE) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) s_te[i * 64u + lane] = d_srtp_te0.t[i * 64u + lane];
    }

    // ---- the state: eighteen 16-byte loads per lane (d_state 16-byte aligned: the argument rule)
#if IGDSP_SRTP_RK_LDS
    __shared__ uint32_t s_rk[44u * kSrtpChans];
    const SrtpRkLds rk{s_rk + lane};
    uint32_t sw[10], ksw[4], mi[5], mo[5];
#else
    uint32_t sw[10], rkv[44], ksw[4], mi[5], mo[5];
    const SrtpRkArray rk{rkv};
#endif
    {
        uint32_t all[kSrtpStateWords];
        const uint4 *sp = reinterpret_cast<const uint4 *>(a.state + c);
#pragma unroll
        for (uint32_t i = 0; i < kSrtpStateWords / 4u; ++i) {
            const uint4 v = sp[i];
            all[4u * i] = v.x; all[4u * i + 1u] = v.y; all[4u * i + 2u] = v.z; all[4u * i + 3u] = v.w;
        }
#pragma unroll
        for (uint32_t i = 0; i < 10u; ++i) sw[i] = all[i];
#pragma unroll
        for (uint32_t i = 0; i < 44u; ++i) {
#if IGDSP_SRTP_RK_LDS
            if constexpr (!MOVE) s_rk[i * kSrtpChans + lane] = all[10u + i];
#else
            rkv[i] = all[10u + i];
#endif
        }
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) ksw[i] = srtp_bswap(all[54u + i]);
#pragma unroll
        for (uint32_t i = 0; i < 5u; ++i) { mi[i] = all[58u + i]; mo[i] = all[63u + i]; }
    }
    const uint32_t tag_len = srtp_tag_len(sw[0]);
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

        // ---- what the lane does with its packet, in the host's order (srtp_packet_run)
        uint32_t flags = IGDSP_SRTP_NO_KEY, size_out = 0u, roc_used = 0u;
        const bool fits = size <= kSrtpMaxPacket && size <= a.stride;
        const bool bypass = ctl == IGDSP_SRTP_BYPASS, keyed = chan && !bypass && tag_len != 0u;
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
            const uint32_t fl = srtp_admit<DIR>(L, tag_len, size, a.ostride, p);
            if (fl) { flags = fl; hdr = false; roc_used = (fl & (IGDSP_SRTP_OLD | IGDSP_SRTP_REPLAY)) ? p.v : 0u; }
        }
        if (!MOVE && keyed && flags != 0u) srtp_refuse(L, flags);          // (EMPTY counts nowhere)
        bool go = hdr;

        uint32_t iv[4], hs[5], rt[3] = {0u, 0u, 0u};
        srtp_iv(ksw, p, iv);
#pragma unroll
        for (uint32_t i = 0; i < 5u; ++i) hs[i] = mi[i];

        if constexpr (DIR == kSrtpProtect) {
            const uint32_t len = go ? p.end : (copy ? size : 0u);
            const uint32_t nb = go ? (MOVE ? (len + 63u) >> 6 : srtp_hash_blocks(len)) : (len + 63u) >> 6;
            wave_lds_fence();
            s_lim[lane] = len;
            s_full[lane] = len & ~15u;
            wave_lds_fence();
            const uint32_t maxb = wave_reduce_dpp(nb, OpMax{});
            srtp_pass<true, false, !MOVE, !MOVE, true>(in_base, a.stride, out_base, a.ostride, lane, go, nb, maxb, have0, len, p, tag_len, rk, iv, hs, rt, s_te,
                                                       s_tile, s_lim, s_full);
            if (go) {
                uint8_t *tag = out_base + (uint64_t)lane * a.ostride + p.end;   // p.end + tag_len <= ostride: srtp_admit
                uint32_t d[5] = {0u, 0u, 0u, 0u, 0u};
                if constexpr (!MOVE) srtp_hmac_finish(hs, mo, d);
#pragma unroll
                for (uint32_t i = 0; i < 10u; ++i)
                    if (i < tag_len) tag[i] = (uint8_t)srtp_tag_byte(d, i);
                flags = MOVE ? (uint32_t)IGDSP_SRTP_BYPASSED : srtp_commit<DIR>(L, p);
                size_out = p.size_out;
                roc_used = MOVE ? 0u : p.v;
            }
        } else {
            // pass 1: the tag over the ciphertext; nothing is stored
            const uint32_t nb1 = go ? srtp_hash_blocks(p.end) : 0u;
            wave_lds_fence();
            s_lim[lane] = go ? size : 0u;
            wave_lds_fence();
            const uint32_t maxb1 = wave_reduce_dpp(nb1, OpMax{});
            srtp_pass<false, true, false, true, false>(in_base, a.stride, out_base, a.ostride, lane, go, nb1, maxb1, have0, 0u, p, tag_len, rk, iv, hs, rt, s_te,
                                                       s_tile, s_lim, s_full);
            if (go) {
                uint32_t d[5];
                srtp_hmac_finish(hs, mo, d);
                if (!srtp_tag_equal(d, rt, tag_len)) {
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
            srtp_pass<false, false, true, false, true>(in_base, a.stride, out_base, a.ostride, lane, go, nb2, maxb2, have0 && maxb1 <= 1u, len, p, tag_len, rk, iv,
                                                       hs, rt, s_te, s_tile, s_lim, s_full);
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
    if (chan && tag_len != 0u) {
        srtp_lane_write(L, sw);
        uint32_t *sp = reinterpret_cast<uint32_t *>(a.state + c);
        *reinterpret_cast<uint4 *>(sp) = make_uint4(sw[0], sw[1], sw[2], sw[3]);
        *reinterpret_cast<uint4 *>(sp + 4) = make_uint4(sw[4], sw[5], sw[6], sw[7]);
        *reinterpret_cast<uint2 *>(sp + 8) = make_uint2(sw[8], sw[9]);
    }
}

hipError_t launch_srtp(const LaunchCfg &, int dir, const uint8_t *ctl, const uint8_t *packets, const uint16_t *sizes, uint32_t C, uint32_t F, uint32_t pkt_stride,
                       igdsp_srtp_state *state, uint8_t *out, uint32_t out_stride, uint16_t *sizes_out, igdsp_srtp_rec *rec, bool yardstick, hipStream_t s)
{
    const SrtpRoute r = srtp_route(C, F, pkt_stride, out_stride, dir, yardstick);
    if (r.grid == 0) return hipSuccess;
    const SrtpArgs a{ctl, packets, sizes, C, F, pkt_stride, state, out, out_stride, sizes_out, rec};
    if (r.move) hipLaunchKernelGGL((k_srtp<kSrtpProtect, true>), dim3(r.grid), dim3(r.threads), 0, s, a);
    else if (r.dir == kSrtpProtect) hipLaunchKernelGGL((k_srtp<kSrtpProtect, false>), dim3(r.grid), dim3(r.threads), 0, s, a);
    else hipLaunchKernelGGL((k_srtp<kSrtpUnprotect, false>), dim3(r.grid), dim3(r.threads), 0, s, a);
    return hipGetLastError();
}

}  // namespace igdsp
