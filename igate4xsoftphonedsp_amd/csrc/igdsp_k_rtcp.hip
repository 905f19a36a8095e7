// igdsp_k_rtcp.hip — RTCP and SRTCP on the packets of a batch: k_rtcp_build (igdsp_rtcp_build), k_rtcp_parse (igdsp_rtcp_parse) and
// k_srtcp<DIR, MOVE> (igdsp_srtcp_protect / igdsp_srtcp_unprotect).  Semantics: include/igdsp.h, section "RTCP / SRTCP"; the rules'
// arithmetic: igdsp_rtcp.h (the host entries run the same functions on one packet); independent restatement: tests/rtcp_model.py.
//
// Shape (routes: rtcp_build_route, rtcp_parse_route, srtcp_route).  The report's prior, the SRTCP index and the replay window are serial
// in a leg's ticks, so in all three a lane owns a leg for the launch and walks f; 64 legs a wave, a block is one wave: k_srtp's shape
// (igdsp_k_srtp.hip's head comment), whose tile loads, tile stores and pass are used as they are (igdsp_k_srtp_tile.h).
//   k_rtcp_build: a lane holds its leg's twenty state words, the jitter buffer's twenty (read only) and the CNAME's 16 words in
//   registers.  Per tick it plans the packet (rtcp_plan) and writes its words into its row of an LDS tile of 64 rows of 34 words
//   (pitch 35: odd), from which the wave stores the whole 16-byte items below each packet's size, item i = turn * 64 + lane being
//   sixteenth i % 9 of row i / 9; the owner stores the 4, 8 or 12 bytes behind them.  Nothing at or behind the size is written.
//   k_rtcp_parse: the tick's packets pass the 64 x 64-byte tile piece by piece, each byte loaded below its packet's size only; a lane
//   hands its row's words to rtcp_walk_word in order, up to the longest packet of the wave (a wave-uniform bound: reports are 20 to
//   34 words, so the second piece is mostly skipped), which takes nothing from the packet as an offset.  Lanes past their packet's
//   last piece are masked.  The record goes out as two 16-byte stores.
//   k_srtcp: k_srtp with an 8-byte header and the 14-byte trailer (index word and tag) behind the packet.  The trailer does not pass
//   the tile: on unprotect the owner reads it from its slot as three dwords and a 16-bit word before anything is stored (the index word
//   decides the replay test and lies under the tag, so it is needed in front of the first pass), on protect it writes it behind the
//   ciphertext the same way.  A packet with E = 0 is laid under no keystream (srtcp_view) and goes out as authenticated.  MOVE (the
//   compute-free yardstick): protect's loads, tile traffic, state load and store and stores and the size rules; no AES round, no
//   compression: the packet goes out as it came, the trailer's 14 bytes as zeros, the state as read.
//   The yardsticks of build and parse (MOVE): build's loads, the size rule, the row filled with one loaded word, the stores; parse's
//   loads, tile traffic and row reads, the size's verdict as the record; no plan, no walk; the state goes back as read.
// Everything is written with vector stores in plain C++.
#include "igdsp_rtcp.h"
#include "igdsp_k_srtp_tile.h"

namespace igdsp {

__device__ const SrtpTe0 d_srtcp_te0 = srtp_make_te0();

// a leg's 80-byte state (igdsp_rtcp_state, igdsp_jb_state) as five 16-byte loads / stores; 16-byte aligned: the argument rule
__device__ __forceinline__ void rtcp_load20(const void *p, uint32_t (&w)[kRtcpStateWords])
{
    const uint4 *sp = reinterpret_cast<const uint4 *>(p);
#pragma unroll
    for (uint32_t i = 0; i < kRtcpStateWords / 4u; ++i) {
        const uint4 v = sp[i];
        w[4u * i] = v.x; w[4u * i + 1u] = v.y; w[4u * i + 2u] = v.z; w[4u * i + 3u] = v.w;
    }
}
__device__ __forceinline__ void rtcp_store20(void *p, const uint32_t (&w)[kRtcpStateWords])
{
    uint4 *sp = reinterpret_cast<uint4 *>(p);
#pragma unroll
    for (uint32_t i = 0; i < kRtcpStateWords / 4u; ++i) sp[i] = make_uint4(w[4u * i], w[4u * i + 1u], w[4u * i + 2u], w[4u * i + 3u]);
}

// ---- igdsp_rtcp_build -----------------------------------------------------------------------------------------------------------------
struct RtcpBuildArgs {
    const uint8_t *ctl;
    const igdsp_jb_state *jb;
    const igdsp_rtcp_src *src;
    const uint64_t *now;
    const uint8_t *cname, *cname_len;
    uint32_t C, F;
    igdsp_rtcp_state *state;
    uint8_t *pkts;
    uint32_t stride;
    uint16_t *sizes;
    igdsp_rtcp_built *rec;
};

template <bool MOVE>
__global__ __launch_bounds__(64) void k_rtcp_build(const RtcpBuildArgs a)
{
    __shared__ uint32_t s_row[kRtcpChans * kRtcpRowPitch];
    __shared__ uint32_t s_size[kRtcpChans];
    const uint32_t lane = threadIdx.x;                                     // < 64: the block is one wave
    const uint64_t c0 = (uint64_t)blockIdx.x * kRtcpChans;                 // < C: the grid
    const uint32_t rows = (uint32_t)((uint64_t)a.C - c0 < kRtcpChans ? (uint64_t)a.C - c0 : kRtcpChans);
    const bool chan = lane < rows;
    const uint32_t c = chan ? (uint32_t)c0 + lane : a.C - 1u;              // lanes past the end load the last leg's state and store nothing

    uint32_t sw[kRtcpStateWords], jw[kRtcpStateWords], cn[kRtcpCnameWords];
    rtcp_load20(a.state + c, sw);
#pragma unroll
    for (uint32_t i = 0; i < kRtcpStateWords; ++i) jw[i] = 0u;
    if (a.jb) rtcp_load20(a.jb + c, jw);
    const RtcpJb jb = rtcp_jb_of(jw, a.jb != nullptr);
    uint32_t L = 0u;
#pragma unroll
    for (uint32_t i = 0; i < kRtcpCnameWords; ++i) cn[i] = 0u;
    if (a.cname) {                                                         // with d_cname_len: the argument rule
        L = a.cname_len[c];
        L = L < (uint32_t)IGDSP_RTCP_CNAME_MAX ? L : (uint32_t)IGDSP_RTCP_CNAME_MAX;
        const uint4 *cp = reinterpret_cast<const uint4 *>(a.cname + (uint64_t)c * IGDSP_RTCP_CNAME_MAX);
#pragma unroll
        for (uint32_t i = 0; i < kRtcpCnameWords / 4u; ++i) {
            const uint4 v = cp[i];
            cn[4u * i] = v.x; cn[4u * i + 1u] = v.y; cn[4u * i + 2u] = v.z; cn[4u * i + 3u] = v.w;
        }
    }
    RtcpLane Ln = rtcp_lane_read(sw);
    uint32_t *row = s_row + lane * kRtcpRowPitch;

    for (uint32_t f = 0; f < a.F; ++f) {
        const uint32_t o = f * a.C + c;                                    // < 2^32 - 32: the argument rule
        uint8_t *out_base = a.pkts + ((uint64_t)f * a.C + c0) * a.stride;
        const uint32_t ctl = chan ? rtcp_ctl(a.ctl[o]) : (uint32_t)IGDSP_RTCP_NONE;
        const uint4 sv = *reinterpret_cast<const uint4 *>(a.src + o);
        const igdsp_rtcp_src src{sv.x, sv.y, sv.z, sv.w};
        const uint64_t now = a.now[f];
        uint32_t size = 0u, flags = 0u;
        if (MOVE && ctl != IGDSP_RTCP_NONE) {                             // the yardstick: the size rule, the row filled with a word that was loaded
            size = rtcp_size_of(src.packets != Ln.sent_prior, jb.heard ? 1u : 0u, L, ctl);
            uint32_t fill = src.ssrc ^ (uint32_t)now;
#pragma unroll
            for (uint32_t i = 0; i < kRtcpCnameWords; ++i) asm volatile("" : "+v"(fill) : "v"(cn[i]));   // the CNAME's loads stay
#pragma unroll
            for (uint32_t k = 0; k < kRtcpRowWords; ++k)
                if (4u * k < size) row[k] = fill;
        } else if (ctl != IGDSP_RTCP_NONE) {
            const RtcpPlan p = rtcp_plan(Ln, ctl, jb, src, now, L);
            rtcp_emit(p, src, now, cn, [&](uint32_t k, uint32_t word) { row[k] = word; });   // k < p.size / 4 <= kRtcpRowWords
            size = p.size;                                                 // <= IGDSP_RTCP_MAX_BUILT <= stride: the argument rule
            flags = p.flags;
        }
        s_size[lane] = size;
        wave_lds_fence();
#pragma unroll
        for (uint32_t u = 0; u < kRtcpRowItems; ++u) {
            const uint32_t i = u * 64u + lane, r = i / kRtcpRowItems, q = i - r * kRtcpRowItems;   // r < 64
            if (16u * q + 16u <= (s_size[r] & ~15u)) {
                const uint32_t *s = s_row + r * kRtcpRowPitch + 4u * q;
                u32x4_a4_t t; t.x = s[0]; t.y = s[1]; t.z = s[2]; t.w = s[3];
                *reinterpret_cast<u32x4_a4_t *>(out_base + (uint64_t)r * a.stride + 16u * q) = t;
            }
        }
        {
            const uint32_t t0 = size & ~15u, nt = size & 15u;              // nt 0, 4, 8 or 12
            uint32_t *op = reinterpret_cast<uint32_t *>(out_base + (uint64_t)lane * a.stride + t0);
#pragma unroll
            for (uint32_t k = 0; k < 3u; ++k)
                if (4u * k + 4u <= nt) op[k] = row[(t0 >> 2) + k];
        }
        if (chan) {
            a.sizes[o] = (uint16_t)size;
            if (a.rec) *reinterpret_cast<uint2 *>(a.rec + o) = make_uint2(size | (flags << 16), 0u);
        }
        wave_lds_fence();                                                  // the next tick overwrites the rows
    }
    if (chan) {
        rtcp_lane_write(Ln, sw);
        rtcp_store20(a.state + c, sw);
    }
}

// ---- igdsp_rtcp_parse -----------------------------------------------------------------------------------------------------------------
struct RtcpParseArgs {
    const uint8_t *pkts;
    const uint16_t *sizes;
    const uint32_t *arrival, *local;
    uint32_t C, F, stride;
    igdsp_rtcp_state *state;
    igdsp_rtcp_seen *rec;
};

template <bool MOVE>
__global__ __launch_bounds__(64) void k_rtcp_parse(const RtcpParseArgs a)
{
    __shared__ uint32_t s_tile[kSrtpChans * kSrtpPitch];
    __shared__ uint32_t s_lim[kSrtpChans];
    const uint32_t lane = threadIdx.x;
    const uint64_t c0 = (uint64_t)blockIdx.x * kRtcpChans;
    const uint32_t rows = (uint32_t)((uint64_t)a.C - c0 < kRtcpChans ? (uint64_t)a.C - c0 : kRtcpChans);
    const bool chan = lane < rows;
    const uint32_t c = chan ? (uint32_t)c0 + lane : a.C - 1u;

    uint32_t sw[kRtcpStateWords];
    rtcp_load20(a.state + c, sw);
    RtcpLane Ln = rtcp_lane_read(sw);
    const uint32_t local = a.local[c];
    const uint32_t *row = s_tile + lane * kSrtpPitch;

    for (uint32_t f = 0; f < a.F; ++f) {
        const uint32_t o = f * a.C + c;
        const uint8_t *in_base = a.pkts + ((uint64_t)f * a.C + c0) * a.stride;
        const uint32_t size = chan ? a.sizes[o] : 0u, arrival = a.arrival[o];
        const uint32_t pre = rtcp_size_check(size, a.stride);
        RtcpWalk w = rtcp_walk_begin(pre ? 0u : size);
        s_lim[lane] = pre ? 0u : size;                                     // <= stride
        wave_lds_fence();
        const uint32_t np = (w.nwords + 15u) >> 4;
        const uint32_t maxw = wave_reduce_dpp(w.nwords, OpMax{});          // wave-uniform: a word no packet of the wave has is skipped by all
        const uint32_t maxp = (maxw + 15u) >> 4;
        for (uint32_t j = 0; j < maxp; ++j) {
            srtp_load_tile<true>(in_base, a.stride, j, s_lim, s_tile, lane);
            wave_lds_fence();
            if (j < np) {
#pragma unroll
                for (uint32_t i = 0; i < 16u; ++i) {
                    if (16u * j + i >= maxw) break;
                    if constexpr (MOVE) {                                  // the yardstick: the row is read and nothing is made of it
                        const uint32_t x = row[i];
                        asm volatile("" : : "v"(x));
                    } else {
                        rtcp_walk_word(w, 16u * j + i, row[i], local);
                    }
                }
            }
            wave_lds_fence();                                              // the next piece overwrites the tile
        }
        igdsp_rtcp_seen r{};
        if constexpr (MOVE) r.flags = (uint8_t)(pre ? pre : (uint32_t)IGDSP_RTCP_PARSED) | (uint8_t)(arrival & local & 0u);   // the size's verdict alone
        else r = rtcp_seen_commit(Ln, pre, w, arrival);                    // lanes past the end: EMPTY, nothing moves
        if (chan && a.rec) {
            uint4 *rp = reinterpret_cast<uint4 *>(a.rec + o);
            rp[0] = make_uint4((uint32_t)r.flags | ((uint32_t)r.n_sub << 8) | ((uint32_t)r.peer_fraction_lost << 16), r.sender_ssrc, r.rtt, (uint32_t)r.peer_cum_lost);
            rp[1] = make_uint4(r.peer_ext_seq, r.peer_jitter, r.sr_packets, r.sr_octets);
        }
    }
    if (chan) {
        rtcp_lane_write(Ln, sw);
        rtcp_store20(a.state + c, sw);
    }
}

// ---- igdsp_srtcp_protect / igdsp_srtcp_unprotect ------------------------------------------------------------------------------------------
template <int DIR, bool MOVE>
__global__ __launch_bounds__(64) void k_srtcp(const SrtpArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_te[256];
    __shared__ uint32_t s_tile[kSrtpChans * kSrtpPitch];
    __shared__ uint32_t s_lim[kSrtpChans], s_full[kSrtpChans];
    __shared__ uint32_t s_rk[44u * kSrtpChans];
    const uint32_t lane = threadIdx.x;                                     // < 64: the block is one wave
    const uint64_t c0 = (uint64_t)blockIdx.x * kSrtpChans;                 // < C: the grid
    const uint32_t rows = (uint32_t)((uint64_t)a.C - c0 < kSrtpChans ? (uint64_t)a.C - c0 : kSrtpChans);
    const bool chan = lane < rows;
    const uint32_t c = chan ? (uint32_t)c0 + lane : a.C - 1u;              // lanes past the end load the last leg's state and store nothing
    if constexpr (!MOVE) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) s_te[i * 64u + lane] = d_srtcp_te0.t[i * 64u + lane];
    }

    // ---- the state: eighteen 16-byte loads per lane; the round keys as [word][lane] in LDS (k_srtp's head comment says why)
    const SrtpRkLds rk{s_rk + lane};
    uint32_t sw[10], ksw[4], mi[5], mo[5];
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
        for (uint32_t i = 0; i < 44u; ++i)
            if constexpr (!MOVE) s_rk[i * kSrtpChans + lane] = all[10u + i];
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) ksw[i] = srtp_bswap(all[54u + i]);
#pragma unroll
        for (uint32_t i = 0; i < 5u; ++i) { mi[i] = all[58u + i]; mo[i] = all[63u + i]; }
    }
    const uint32_t tag_len = srtcp_tag_len(sw[0]);
    SrtpLane L = srtp_lane_read(sw);
    const uint32_t *row = s_tile + lane * kSrtpPitch;

    uint32_t size_n = a.sizes[c], ctl_n = (!MOVE && a.ctl) ? a.ctl[c] : (uint32_t)IGDSP_SRTP_RUN;
    for (uint32_t f = 0; f < a.F; ++f) {
        const uint32_t o = f * a.C + c;                                    // < 2^32 - 32: the argument rule
        const uint64_t t0 = (uint64_t)f * a.C + c0;                        // the tick's first slot of this block
        const uint8_t *in_base = a.pkts + t0 * a.stride;
        uint8_t *out_base = a.out + t0 * a.ostride;
        const uint32_t size = chan ? size_n : 0u, ctl = srtp_ctl(ctl_n);
        if (f + 1u < a.F) {                                                // in flight during the tick
            size_n = a.sizes[o + a.C];
            if (!MOVE && a.ctl) ctl_n = a.ctl[o + a.C];
        }

        // ---- what the lane does with its packet, in the host's order (srtcp_packet_run)
        uint32_t flags = IGDSP_SRTP_NO_KEY, size_out = 0u, idx_used = 0u;
        const bool fits = size <= kSrtpMaxPacket && size <= a.stride;
        const bool bypass = ctl == IGDSP_SRTP_BYPASS, keyed = chan && !bypass && tag_len != 0u;
        bool copy = false, go = false;
        SrtcpPkt p{};
        if (chan && bypass) {
            if (size == 0u) flags = IGDSP_SRTP_EMPTY;
            else if (!fits || size > a.ostride) flags = IGDSP_SRTP_MALFORMED;
            else copy = true;
        } else if (keyed) {
            if (ctl == IGDSP_SRTP_RESET) srtp_lane_reset(L);
            if (size == 0u) flags = IGDSP_SRTP_EMPTY;
            else if (!fits) flags = IGDSP_SRTP_MALFORMED;
            else {
                flags = srtcp_sizes<DIR>(size, a.ostride, p);
                go = flags == 0u;
            }
        }
        // ---- the trailer of a received packet, from the owner's slot: p.end + 14 == size <= stride, p.end a multiple of 4
        uint32_t idxw_in = 0u, rt[3] = {0u, 0u, 0u};
        if (DIR == kSrtpUnprotect && go) {
            const uint8_t *t = in_base + (uint64_t)lane * a.stride + p.end;
            const uint32_t *tw = reinterpret_cast<const uint32_t *>(t);
            idxw_in = srtp_bswap(tw[0]);
            srtcp_tag_words(tw[1], tw[2], *reinterpret_cast<const uint16_t *>(t + 12), rt);
        }
        s_lim[lane] = (go || copy) ? size : 0u;
        wave_lds_fence();
        srtp_load_tile<DIR == kSrtpProtect>(in_base, a.stride, 0u, s_lim, s_tile, lane);
        wave_lds_fence();
        uint32_t ssrc = 0u;
        if (go) {
            ssrc = srtp_bswap(row[1]);                                     // size >= 8
            const uint32_t fl = srtcp_admit<DIR>(L, row[0], idxw_in, p);
            if (fl) { flags = fl; go = false; idx_used = (fl & (IGDSP_SRTP_OLD | IGDSP_SRTP_REPLAY)) ? p.idxw : 0u; }
        }
        if (!MOVE && keyed && flags != 0u) srtp_refuse(L, flags);          // (EMPTY counts nowhere)

        uint32_t iv[4], hs[5];
        const SrtpPkt q = srtcp_view(ksw, ssrc, p, iv);
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
            srtp_pass<true, false, !MOVE, !MOVE, true>(in_base, a.stride, out_base, a.ostride, lane, go, nb, maxb, true, len, q, tag_len, rk, iv, hs, rt, s_te,
                                                       s_tile, s_lim, s_full);
            if (go) {
                uint8_t *t = out_base + (uint64_t)lane * a.ostride + p.end;     // p.end + 14 <= ostride: srtcp_sizes; p.end a multiple of 4
                uint32_t d[5] = {0u, 0u, 0u, 0u, 0u};
                if constexpr (!MOVE) srtp_hmac_finish(hs, mo, d);
                uint32_t *tw = reinterpret_cast<uint32_t *>(t);
                tw[0] = MOVE ? 0u : srtp_bswap(p.idxw);
                tw[1] = srtp_bswap(d[0]);
                tw[2] = srtp_bswap(d[1]);
                *reinterpret_cast<uint16_t *>(t + 12) = (uint16_t)srtcp_tag_half(d);
                flags = MOVE ? (uint32_t)IGDSP_SRTP_BYPASSED : srtcp_commit<DIR>(L, p);
                size_out = p.size_out;
                idx_used = MOVE ? 0u : p.idxw;
            }
        } else {
            // pass 1: the tag over what came; nothing is stored
            const uint32_t nb1 = go ? srtp_hash_blocks(p.end) : 0u;
            wave_lds_fence();
            s_lim[lane] = go ? p.end : 0u;
            wave_lds_fence();
            const uint32_t maxb1 = wave_reduce_dpp(nb1, OpMax{});
            uint32_t none[3] = {0u, 0u, 0u};
            srtp_pass<false, false, false, true, false>(in_base, a.stride, out_base, a.ostride, lane, go, nb1, maxb1, true, 0u, q, tag_len, rk, iv, hs, none, s_te,
                                                        s_tile, s_lim, s_full);
            if (go) {
                uint32_t d[5];
                srtp_hmac_finish(hs, mo, d);
                if (!srtp_tag_equal(d, rt, kSrtcpTagLen)) {
                    flags = IGDSP_SRTP_AUTH_FAIL;
                    srtp_refuse(L, flags);
                    idx_used = p.idxw;
                    go = false;
                }
            }
            // pass 2: the accepted packets are decrypted (E = 1) and stored, the bypassed ones copied
            const uint32_t len = go ? p.end : (copy ? size : 0u), nb2 = (len + 63u) >> 6;
            wave_lds_fence();
            s_lim[lane] = len;
            s_full[lane] = len & ~15u;
            wave_lds_fence();
            const uint32_t maxb2 = wave_reduce_dpp(nb2, OpMax{});
            srtp_pass<false, false, true, false, true>(in_base, a.stride, out_base, a.ostride, lane, go, nb2, maxb2, maxb1 <= 1u, len, q, tag_len, rk, iv, hs, none,
                                                       s_te, s_tile, s_lim, s_full);
            if (go) {
                flags = srtcp_commit<DIR>(L, p);
                size_out = p.size_out;
                idx_used = p.idxw;
            }
        }
        if (copy) { flags = IGDSP_SRTP_BYPASSED; size_out = size; }

        // ---- length and record: one store per lane, consecutive across the wave
        if (chan) {
            a.sizes_out[o] = (uint16_t)size_out;
            if (a.rec) *reinterpret_cast<uint2 *>(a.rec + o) = make_uint2(idx_used, size_out | (flags << 16));
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

hipError_t launch_rtcp_build(const LaunchCfg &, const uint8_t *ctl, const igdsp_jb_state *jb, const igdsp_rtcp_src *src, const uint64_t *now, const uint8_t *cname,
                             const uint8_t *cname_len, uint32_t C, uint32_t F, igdsp_rtcp_state *state, uint8_t *packets, uint32_t pkt_stride, uint16_t *sizes,
                             igdsp_rtcp_built *rec, bool yardstick, hipStream_t s)
{
    const RtcpRoute r = rtcp_build_route(C, F, pkt_stride, yardstick);
    if (r.grid == 0) return hipSuccess;
    const RtcpBuildArgs a{ctl, jb, src, now, cname, cname_len, C, F, state, packets, pkt_stride, sizes, rec};
    if (r.move) hipLaunchKernelGGL(k_rtcp_build<true>, dim3(r.grid), dim3(r.threads), 0, s, a);
    else hipLaunchKernelGGL(k_rtcp_build<false>, dim3(r.grid), dim3(r.threads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_rtcp_parse(const LaunchCfg &, const uint8_t *packets, const uint16_t *sizes, const uint32_t *arrival, const uint32_t *local_ssrc, uint32_t C,
                             uint32_t F, uint32_t pkt_stride, igdsp_rtcp_state *state, igdsp_rtcp_seen *rec, bool yardstick, hipStream_t s)
{
    const RtcpRoute r = rtcp_parse_route(C, F, pkt_stride, yardstick);
    if (r.grid == 0) return hipSuccess;
    const RtcpParseArgs a{packets, sizes, arrival, local_ssrc, C, F, pkt_stride, state, rec};
    if (r.move) hipLaunchKernelGGL(k_rtcp_parse<true>, dim3(r.grid), dim3(r.threads), 0, s, a);
    else hipLaunchKernelGGL(k_rtcp_parse<false>, dim3(r.grid), dim3(r.threads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_srtcp(const LaunchCfg &, int dir, const uint8_t *ctl, const uint8_t *packets, const uint16_t *sizes, uint32_t C, uint32_t F, uint32_t pkt_stride,
                        igdsp_srtp_state *state, uint8_t *out, uint32_t out_stride, uint16_t *sizes_out, igdsp_srtp_rec *rec, bool yardstick, hipStream_t s)
{
    const SrtpRoute r = srtcp_route(C, F, pkt_stride, out_stride, dir, yardstick);
    if (r.grid == 0) return hipSuccess;
    const SrtpArgs a{ctl, packets, sizes, C, F, pkt_stride, state, out, out_stride, sizes_out, rec};
    if (r.move) hipLaunchKernelGGL((k_srtcp<kSrtpProtect, true>), dim3(r.grid), dim3(r.threads), 0, s, a);
    else if (r.dir == kSrtpProtect) hipLaunchKernelGGL((k_srtcp<kSrtpProtect, false>), dim3(r.grid), dim3(r.threads), 0, s, a);
    else hipLaunchKernelGGL((k_srtcp<kSrtpUnprotect, false>), dim3(r.grid), dim3(r.threads), 0, s, a);
    return hipGetLastError();
}

}  // namespace igdsp
