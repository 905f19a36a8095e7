// igdsp_spec.h — the spectrum stage's rule (include/igdsp.h, "Spectrum"; independent restatement: tests/spec_model.py) in plain C++17,
// so that the host entry igdsp_spec_frame (spec_frame_run below), the kernel k_spec and tests/route/spec_route_driver.cpp run the same
// code.  The arithmetic (the radix-8 butterfly, the twiddle products, the split pass, the dB value, the average) is written once, for
// the host and the device; so is the index arithmetic of the transform's data flow: which point a lane holds in which register in each
// pass, where it stores it in the exchange tile and where it loads the next pass's points from.  The host transform spec_transform walks
// the kernel's 64 lanes in a loop with the tile as an array, so a CPU test of igdsp_spec_frame is a test of the kernel's indexing too.
//
// The transform.  The 1 024 windowed samples y are packed as 512 complex points z[m] = y[2m] + i y[2m+1]; Z = DFT512(z) by
// m = 64 a + 8 b + c, k = k0 + 8 k1 + 64 k2 (w = e^(-2 pi i / 512)):
//   pass 1, lane 8 b + c, registers a:        A[k0] = sum_a w8^(a k0) z[64 a + 8 b + c];              A[k0] *= w^(8 b k0)
//   pass 2, lane 8 k0 + c, registers b:       B[k1] = sum_b w8^(b k1) A[k0; b, c];                    B[k1] *= w^(c (k0 + 8 k1))
//   pass 3, lane k0 + 8 k1, registers c:      Z[k0 + 8 k1 + 64 k2] = sum_c w8^(c k2) B[k0, k1; c]
// and the split pass X[k] = E[k] + e^(-2 pi i k / 1024) O[k], E = (Z[k] + conj Z[512 - k]) / 2, O = (Z[k] - conj Z[512 - k]) / 2i, with
// Z[512 - k] in lane (64 - lane) % 64, register 7 - k2 (lane 0: register (8 - k2) % 8).  The split's factor 1/2 is folded into the
// power's scale (2^-48 on |2 X|^2 is 2^-46 on |X|^2: powers of two, the same bits).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "igdsp.h"
#include "igdsp_route.h"
#include "igdsp_spec_tab.h"

#if defined(__HIPCC__)
#define IGDSP_SPEC_HD __host__ __device__ __forceinline__
#else
#define IGDSP_SPEC_HD inline
#endif

namespace igdsp {

static_assert(sizeof(igdsp_spec_state) == 4112 && alignof(igdsp_spec_state) == 4, "igdsp_spec_state layout (capi.SPEC_STATE mirrors it)");
static_assert(offsetof(igdsp_spec_state, avg) == 2048 && offsetof(igdsp_spec_state, since) == 4096, "the history and the averaged array are dword arrays");
static_assert(sizeof(igdsp_spec_rec) == 8 && sizeof(igdsp_spec_cfg) == 8, "capi.SPEC_REC, capi.SpecCfg");
static_assert(IGDSP_SPEC_N == 1024 && IGDSP_SPEC_BINS == 512 && IGDSP_MAX_PAYLOAD <= 256, "8 x 8 x 8 complex points; a row is at most 4 samples per lane");

constexpr uint32_t kSpecN = IGDSP_SPEC_N, kSpecBins = IGDSP_SPEC_BINS;
constexpr float kSpecPowScale = 0x1p-48f;                 // on |2 X|^2
constexpr float kSpecPowFloor = 1e-20f;

// the tables on the host (the device's copies: igdsp_k_spec.hip)
inline constexpr float kSpecWin[kSpecN] = {IGDSP_SPEC_WIN_VALUES};
inline constexpr float kSpecTw[2 * kSpecN] = {IGDSP_SPEC_TW_VALUES};

// ---- the configuration and the state's read rule
constexpr bool spec_cfg_ok(const igdsp_spec_cfg &c) { return c.hop_frames >= 1u && c.alpha > 0.0f && c.alpha <= 1.0f; }   // (a NaN fails both)
constexpr igdsp_spec_cfg spec_cfg_or_default(const igdsp_spec_cfg *c) { return c ? *c : igdsp_spec_cfg{1u, 0.25f}; }
constexpr bool spec_n_ok(uint32_t n) { return n != 0 && n <= IGDSP_MAX_PAYLOAD; }
constexpr uint32_t spec_since_read(uint32_t since, uint32_t hop) { return since < hop ? since : hop - 1u; }
// the first frame of a launch of F frames that hops, from the since read at its start (>= F: none), and the last one
constexpr uint64_t spec_first_hop(uint32_t since, uint32_t hop) { return (uint64_t)hop - 1u - since; }
constexpr uint64_t spec_last_hop(uint32_t since, uint32_t hop, uint32_t F)
{
    const uint64_t f0 = spec_first_hop(since, hop);
    return f0 >= F ? (uint64_t)F : f0 + (F - 1u - f0) / hop * hop;
}

// ---- the data flow: lanes, registers, tile slots, table indices (t[k] = e^(-2 pi i k / 1024): w^p = t[2 p], w64^p = t[16 p])
constexpr uint32_t spec_in_point(uint32_t lane, uint32_t a) { return 64u * a + lane; }                         // pass 1's z index
constexpr uint32_t spec_tw1(uint32_t lane, uint32_t k0) { return 16u * (lane >> 3) * k0; }                     // <= 784
constexpr uint32_t spec_x1_store(uint32_t lane, uint32_t k0) { return k0 * kSpecTileRow + lane; }
constexpr uint32_t spec_x1_load(uint32_t lane, uint32_t b) { return (lane >> 3) * kSpecTileRow + 8u * b + (lane & 7u); }
constexpr uint32_t spec_tw2(uint32_t lane, uint32_t k1) { return 2u * (lane & 7u) * ((lane >> 3) + 8u * k1); }  // <= 882
constexpr uint32_t spec_x2_store(uint32_t lane, uint32_t k1) { return k1 * kSpecTileRow + 9u * (lane & 7u) + (lane >> 3); }
constexpr uint32_t spec_x2_load(uint32_t lane, uint32_t c) { return (lane >> 3) * kSpecTileRow + 9u * c + (lane & 7u); }
constexpr uint32_t spec_bin(uint32_t lane, uint32_t k2) { return lane + 64u * k2; }                            // pass 3's Z index, the bin
constexpr uint32_t spec_mirror_lane(uint32_t lane) { return (64u - lane) & 63u; }
constexpr uint32_t spec_mirror_reg(uint32_t lane, uint32_t k2) { return lane ? 7u - k2 : (8u - k2) & 7u; }
static_assert(spec_tw1(63, 7) < kSpecN && spec_tw2(63, 7) < kSpecN && spec_x2_store(63, 7) < kSpecTile && spec_x1_load(63, 7) < kSpecTile);

// ---- the arithmetic
struct SpecC { float re, im; };
IGDSP_SPEC_HD SpecC spec_mul(const SpecC a, const SpecC t) { return SpecC{a.re * t.re - a.im * t.im, a.re * t.im + a.im * t.re}; }
IGDSP_SPEC_HD SpecC spec_add(const SpecC a, const SpecC b) { return SpecC{a.re + b.re, a.im + b.im}; }
IGDSP_SPEC_HD SpecC spec_sub(const SpecC a, const SpecC b) { return SpecC{a.re - b.re, a.im - b.im}; }
IGDSP_SPEC_HD SpecC spec_mul_mi(const SpecC a) { return SpecC{a.im, -a.re}; }                                   // a * -i

// 4-point DFT of c0 .. c3 into o0 .. o3
IGDSP_SPEC_HD void spec_r4(const SpecC c0, const SpecC c1, const SpecC c2, const SpecC c3, SpecC &o0, SpecC &o1, SpecC &o2, SpecC &o3)
{
    const SpecC s0 = spec_add(c0, c2), s1 = spec_sub(c0, c2), s2 = spec_add(c1, c3), s3 = spec_mul_mi(spec_sub(c1, c3));
    o0 = spec_add(s0, s2); o2 = spec_sub(s0, s2); o1 = spec_add(s1, s3); o3 = spec_sub(s1, s3);
}
// 8-point DFT in place, natural order in and out: v[k] = sum_j v[j] e^(-2 pi i j k / 8)
IGDSP_SPEC_HD void spec_r8(SpecC (&v)[8])
{
    constexpr float h = 0x1.6a09e6p-1f;                    // sqrt(1/2), rounded once
    const SpecC a0 = spec_add(v[0], v[4]), a1 = spec_add(v[1], v[5]), a2 = spec_add(v[2], v[6]), a3 = spec_add(v[3], v[7]);
    const SpecC b0 = spec_sub(v[0], v[4]), d1 = spec_sub(v[1], v[5]), d2 = spec_sub(v[2], v[6]), d3 = spec_sub(v[3], v[7]);
    const SpecC b1 = SpecC{(d1.re + d1.im) * h, (d1.im - d1.re) * h};       // d1 * (1 - i) / sqrt 2
    const SpecC b2 = spec_mul_mi(d2);
    const SpecC b3 = SpecC{(d3.im - d3.re) * h, -(d3.re + d3.im) * h};      // d3 * (-1 - i) / sqrt 2
    spec_r4(a0, a1, a2, a3, v[0], v[2], v[4], v[6]);
    spec_r4(b0, b1, b2, b3, v[1], v[3], v[5], v[7]);
}
// the split pass: 2 X[k] from Z[k], Z[512 - k] and t[k]
IGDSP_SPEC_HD SpecC spec_split2(const SpecC z, const SpecC zp, const SpecC t)
{
    const float sr = z.re + zp.re, dr = z.re - zp.re, si = z.im + zp.im, di = z.im - zp.im;
    return SpecC{sr + (t.re * si + t.im * dr), di + (t.im * si - t.re * dr)};
}
IGDSP_SPEC_HD float spec_db(const SpecC x2) { return 10.0f * ::log10f((x2.re * x2.re + x2.im * x2.im) * kSpecPowScale + kSpecPowFloor); }
IGDSP_SPEC_HD float spec_average(float avg, float raw, float alpha) { return avg + alpha * (raw - avg); }
// a float's bits as an unsigned key of the same order (no NaN comes out of spec_db), and back
IGDSP_SPEC_HD uint32_t spec_key(float v)
{
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
IGDSP_SPEC_HD float spec_unkey(uint32_t k)
{
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float v;
    __builtin_memcpy(&v, &u, 4);
    return v;
}

// ---- the host: the transform as the kernel's 64 lanes run it, and one frame of one channel
inline SpecC spec_tw_host(uint32_t k) { return SpecC{kSpecTw[2u * k], kSpecTw[2u * k + 1u]}; }
inline void spec_transform(const int16_t *x, float *raw)                        // x: 1 024 samples, oldest first; raw: 512
{
    SpecC v[64][8];
    SpecC tile[kSpecTile];
    for (uint32_t lane = 0; lane < 64u; ++lane) {
        for (uint32_t a = 0; a < 8u; ++a) {
            const uint32_t m = spec_in_point(lane, a);
            v[lane][a] = SpecC{(float)x[2u * m] * kSpecWin[2u * m], (float)x[2u * m + 1u] * kSpecWin[2u * m + 1u]};
        }
        spec_r8(v[lane]);
        for (uint32_t k0 = 1; k0 < 8u; ++k0) v[lane][k0] = spec_mul(v[lane][k0], spec_tw_host(spec_tw1(lane, k0)));
        for (uint32_t k0 = 0; k0 < 8u; ++k0) tile[spec_x1_store(lane, k0)] = v[lane][k0];
    }
    for (uint32_t lane = 0; lane < 64u; ++lane) {
        for (uint32_t b = 0; b < 8u; ++b) v[lane][b] = tile[spec_x1_load(lane, b)];
        spec_r8(v[lane]);
        for (uint32_t k1 = 0; k1 < 8u; ++k1) v[lane][k1] = spec_mul(v[lane][k1], spec_tw_host(spec_tw2(lane, k1)));
    }
    for (uint32_t lane = 0; lane < 64u; ++lane)
        for (uint32_t k1 = 0; k1 < 8u; ++k1) tile[spec_x2_store(lane, k1)] = v[lane][k1];
    for (uint32_t lane = 0; lane < 64u; ++lane) {
        for (uint32_t c = 0; c < 8u; ++c) v[lane][c] = tile[spec_x2_load(lane, c)];
        spec_r8(v[lane]);
    }
    for (uint32_t lane = 0; lane < 64u; ++lane)
        for (uint32_t k2 = 0; k2 < 8u; ++k2) {
            const uint32_t k = spec_bin(lane, k2);
            raw[k] = spec_db(spec_split2(v[lane][k2], v[spec_mirror_lane(lane)][spec_mirror_reg(lane, k2)], spec_tw_host(k)));
        }
}

// one frame of one channel: n and cfg checked by the caller.  rec and raw may be nullptr; raw is written on a hop only
inline void spec_frame_run(igdsp_spec_state &st, const int16_t *row, uint32_t n, const igdsp_spec_cfg &cfg, igdsp_spec_rec *rec, float *raw)
{
    std::memmove(st.hist, st.hist + n, (kSpecN - n) * sizeof(int16_t));
    std::memcpy(st.hist + (kSpecN - n), row, n * sizeof(int16_t));
    if (!(st.flags & IGDSP_SPEC_LIVE))
        for (uint32_t k = 0; k < kSpecBins; ++k) st.avg[k] = IGDSP_SPEC_FLOOR_DB;
    st.flags = IGDSP_SPEC_LIVE;
    uint32_t since = spec_since_read(st.since, cfg.hop_frames) + 1u;
    igdsp_spec_rec r{0, 0, 0.0f};
    if (since == cfg.hop_frames) {
        since = 0;
        float tmp[kSpecBins];
        float *out = raw ? raw : tmp;
        spec_transform(st.hist, out);
        uint32_t best = spec_key(out[0]), bin = 0;
        for (uint32_t k = 1; k < kSpecBins; ++k)
            if (spec_key(out[k]) > best) { best = spec_key(out[k]); bin = k; }          // the lowest bin wins a tie
        for (uint32_t k = 0; k < kSpecBins; ++k) st.avg[k] = spec_average(st.avg[k], out[k], cfg.alpha);
        st.hops += 1u;
        r = igdsp_spec_rec{(uint16_t)bin, (uint16_t)IGDSP_SPEC_HOP, spec_unkey(best)};
    }
    st.since = since;
    if (rec) *rec = r;
}

}  // namespace igdsp
