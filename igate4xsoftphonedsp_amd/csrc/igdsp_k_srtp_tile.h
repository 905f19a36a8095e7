// igdsp_k_srtp_tile.h — what the kernels that walk SRTP-shaped packets share (k_srtp in igdsp_k_srtp.hip, k_srtcp in igdsp_k_rtcp.hip):
// the argument block, how a table word, a round key and a wave-wide vote are read on the device, the LDS tile's loads and stores and
// one pass over a frame's pieces.  The shape is described at the head of igdsp_k_srtp.hip; the geometry is igdsp_route.h's.
#pragma once
#include "igdsp_srtp.h"
#include "igdsp_device.h"

namespace igdsp {

struct SrtpArgs {
    const uint8_t *ctl, *pkts;
    const uint16_t *sizes;
    uint32_t C, F, stride;
    igdsp_srtp_state *state;
    uint8_t *out;
    uint32_t ostride;
    uint16_t *sizes_out;
    igdsp_srtp_rec *rec;
};

struct SrtpLdsTe {
    const uint32_t *t;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return t[i & 255u]; }
};
#ifndef IGDSP_SRTP_RK_LDS
#define IGDSP_SRTP_RK_LDS 1      // A/B: the 44 round keys as [word][lane] in LDS (1) or as 44 VGPRs (0)
#endif
struct SrtpRkLds {                                                         // p: the lane's column of s_rk[44][64]
    const uint32_t *p;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return p[i * kSrtpChans]; }   // i a constant below 44
};
struct SrtpWaveAny {
    __device__ __forceinline__ bool operator()(bool b) const { return __builtin_amdgcn_ballot_w64(b) != 0u; }
};

// piece j of the frame's packets into the tile: item i = turn * 64 + lane is 16 bytes, quarter i & 3 of row i >> 2.  Bytes are read
// below s_lim[row] (<= stride) only, and a 16-byte load that would pass the slot's end goes dword by dword instead
template <bool NT>
__device__ __forceinline__ void srtp_load_tile(const uint8_t *base, uint32_t stride, uint32_t j, const uint32_t *s_lim, uint32_t *s_tile, uint32_t lane)
{
    uint4 v[4];
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
        const uint32_t i = u * 64u + lane, r = i >> 2, off = 64u * j + 16u * (i & 3u);
        v[u] = make_uint4(0u, 0u, 0u, 0u);
        if (off < s_lim[r]) {                                              // off + 4 <= stride: both multiples of 4
            const uint8_t *p = base + (uint64_t)r * stride + off;
            if (off + 16u <= stride) {
                if constexpr (NT) {
                    v[u] = ld16_dw(p);
                } else {
                    const u32x4_a4_t t = *reinterpret_cast<const u32x4_a4_t *>(p);
                    v[u] = make_uint4(t.x, t.y, t.z, t.w);
                }
            } else {
                const uint32_t *pd = reinterpret_cast<const uint32_t *>(p);
                v[u].x = pd[0];
                if (off + 8u <= stride) v[u].y = pd[1];
                if (off + 12u <= stride) v[u].z = pd[2];
            }
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
        const uint32_t i = u * 64u + lane;
        uint32_t *d = s_tile + (i >> 2) * kSrtpPitch + 4u * (i & 3u);       // < 64 * 17
        d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
    }
}

// piece j of the tile out: whole 16-byte items below s_full[row] wave-wide; the owner's odd tail (len & 15 bytes at len & ~15, when
// that lies in piece j) as dwords and bytes from its row.  Nothing at or behind len is written
__device__ __forceinline__ void srtp_store_tile(uint8_t *base, uint32_t ostride, uint32_t j, const uint32_t *s_full, const uint32_t *s_tile, uint32_t lane,
                                                uint32_t len)
{
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
        const uint32_t i = u * 64u + lane, r = i >> 2, off = 64u * j + 16u * (i & 3u);
        if (off + 16u <= s_full[r]) {                                      // <= the packet's length <= ostride
            const uint32_t *s = s_tile + r * kSrtpPitch + 4u * (i & 3u);
            u32x4_a4_t t; t.x = s[0]; t.y = s[1]; t.z = s[2]; t.w = s[3];
            *reinterpret_cast<u32x4_a4_t *>(base + (uint64_t)r * ostride + off) = t;
        }
    }
    const uint32_t t0 = len & ~15u, nt = len & 15u;
    if (nt != 0u && (t0 >> 6) == j) {
        const uint32_t *row = s_tile + lane * kSrtpPitch + ((t0 & 63u) >> 2);
        uint8_t *o = base + (uint64_t)lane * ostride + t0;
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k)
            if (4u * k + 4u <= nt) reinterpret_cast<uint32_t *>(o)[k] = row[k];
        const uint32_t last = row[nt >> 2], at = nt & ~3u;                 // (nt >> 2) <= 3: inside the row's 16 words
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k)
            if (k < (nt & 3u)) o[at + k] = (uint8_t)(last >> (8u * k));
    }
}

// One pass over the pieces 0 .. maxb - 1 (wave-uniform).  go: the lane works its packet, nb its number of pieces in this pass.
// GRAB: gather the received tag; CRYPT: XOR the keystream into the row; HASH: run the SHA-1 block; STORE: the tile goes out
template <bool NT, bool GRAB, bool CRYPT, bool HASH, bool STORE, class RK>
__device__ __forceinline__ void srtp_pass(const uint8_t *in_base, uint32_t stride, uint8_t *out_base, uint32_t ostride, uint32_t lane, bool go, uint32_t nb,
                                          uint32_t maxb, bool have0, uint32_t out_len, const SrtpPkt &p, uint32_t tag_len, const RK &rk,
                                          const uint32_t (&iv)[4], uint32_t (&hs)[5], uint32_t (&rt)[3], const uint32_t *s_te, uint32_t *s_tile,
                                          const uint32_t *s_lim, const uint32_t *s_full)
{
    uint32_t carry[4] = {0u, 0u, 0u, 0u};
    uint32_t *row = s_tile + lane * kSrtpPitch;
    for (uint32_t j = 0; j < maxb; ++j) {
        if (!(j == 0u && have0)) srtp_load_tile<NT>(in_base, stride, j, s_lim, s_tile, lane);
        wave_lds_fence();
        if (go && j < nb) {
            uint32_t pw[16];
            if constexpr (GRAB) srtp_grab_tag(reinterpret_cast<const uint8_t *>(row), j, p.end, tag_len, rt);
            if constexpr (CRYPT) {                                         // the keystream first: the row's words are not live through the AES rounds
                uint32_t x[16];
                srtp_ks_piece(rk, SrtpLdsTe{s_te}, SrtpWaveAny{}, iv, p.h, p.end, j, carry, x);
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
            if constexpr (HASH) srtp_hash_piece(hs, pw, j, p.end, p.v);
        }
        wave_lds_fence();
        if constexpr (STORE) {
            srtp_store_tile(out_base, ostride, j, s_full, s_tile, lane, out_len);
            wave_lds_fence();                                              // the next piece overwrites the tile
        }
    }
}

}  // namespace igdsp
