// igdsp_ns.h — the noise suppressor's rule (include/igdsp.h, "Noise suppression"; independent restatement: tests/ns_model.py) in plain
// C++17, so that the host entry igdsp_ns_frame and the kernel k_ns run the same code: how a state is read and written, one frame of one
// channel, hop by hop, with every rounding step of the transform.  What the two sides do differently is only who walks: a frame is
// worked by L lanes (the host: L = 1, lane 0; the kernel: L = kNsLanes = 16 lanes of a wave), each taking the items lane, lane + L, ...
// of a phase; between two phases stands sync() (the host: nothing; the kernel: a same-wave LDS fence).  Within a phase no item reads
// what another item of that phase writes, so the bits are the same for any L.  Every step is an exact integer operation and ">>" on a
// signed value an arithmetic shift on both sides.  The tables are passed in: the host reads kNsWin / kNsTw, the kernel its copies.
//
// THE TRANSFORM.  256 real points as 128 packed complex ones, z[k] = xw[2k] + i xw[2k+1], in place in NsWork::z (re, im interleaved).
// Forward: seven radix-2 passes, decimation in frequency (natural order in, bin k of the 128-point transform at position rev7(k)),
// then the split pass, pair (k, 128 - k) by pair, in place at rev7(k) and rev7(128 - k): the 256-point bins 0 .. 127 at rev7(k), bin
// 128 (real) in the imaginary half of bin 0 (real).  Inverse: the split pass backwards, then seven radix-2 passes, decimation in time
// (bit-reversed in, natural out): no pass permutes.  A product with a table entry is formed in 64 bits (int32 x Q30 int32), the two
// products of a complex product and the other addend are summed in 64 bits and rounded ONCE per component (ns_rnd): forward >> 30,
// the forward split >> 31 (its 1/2), the inverse split and every inverse pass >> 31 (1/2 each: the 1/256).
// The rule is the library's own, UNVERIFIED against speex, WebRTC and ITU-T G.160.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "igdsp.h"
#include "igdsp_ns_tab.h"

#if defined(__HIPCC__)
#define IGDSP_NS_HD __host__ __device__ inline __attribute__((always_inline))   // (no HIP header need come first)
#else
#define IGDSP_NS_HD inline
#endif

namespace igdsp {

static_assert(sizeof(igdsp_ns_cfg) == 16 && sizeof(igdsp_ns_state) == 1072 && sizeof(igdsp_ns_rec) == 16 && sizeof(igdsp_ns_state) % 16 == 0,
              "capi.NS_CFG, NS_STATE, NS_REC");
static_assert(offsetof(igdsp_ns_state, hops) == 4 && offsetof(igdsp_ns_state, flags) == 6 && offsetof(igdsp_ns_state, prev) == 16 &&
              offsetof(igdsp_ns_state, ola) == 176 && offsetof(igdsp_ns_state, S) == 496 && offsetof(igdsp_ns_state, N) == 752 &&
              offsetof(igdsp_ns_state, Gt) == 1008 && offsetof(igdsp_ns_rec, min_gain_q15) == 8 && offsetof(igdsp_ns_rec, noise_idx) == 12,
              "a state goes as 67 16-byte pieces, S and N 8-byte aligned in it, the record as one 16-byte store");

constexpr uint32_t kNsHop = IGDSP_NS_HOP, kNsWinLen = 2u * kNsHop, kNsPoints = 128, kNsBands = IGDSP_NS_BANDS, kNsMaxLanes = 16, kNsMaxFrame = 4u * kNsHop;
constexpr int32_t kNsUnity = IGDSP_NS_UNITY;
constexpr uint64_t kNsLevelMask = (1ull << 56) - 1u;     // S and N as read

inline constexpr int16_t kNsWin[kNsWinLen] = {IGDSP_NS_WIN_VALUES};
inline constexpr int32_t kNsTw[2 * kNsPoints] = {IGDSP_NS_TW_VALUES};

// ---- the widths.  xw: a sample times a window entry below 32768, >> 8
constexpr int64_t kNsXwMax = (32768ll * 32767ll + 128) >> 8;              // 4 194 176
// any value of the forward transform, pass by pass, is a partial transform of the packed points: its modulus is at most the sum of
// the moduli of the inputs, sum |z[k]| <= sum |xw[i]|, and a component no more; the split pass combines two such with |t| = 1:
// |X| <= sqrt(2) sum |xw|.  Rounding adds at most 1 per pass and doubles per pass: < 2^9
constexpr int64_t kNsSumXw = (int64_t)kNsWinLen * kNsXwMax;               // 671 068 160
constexpr int64_t kNsFwdMax = kNsSumXw * 14143 / 10000 + 512;             // >= sqrt(2) sum |xw| + rounding
// the inverse: |Y| <= |X| (a gain is at most 1), the inverse split gives |Z| <= (|Y[k]| + |Y[128-k]|) / 2 * 2 (even and odd part),
// a pass (a +- b t) / 2 does not grow the largest modulus; rounding adds at most 1 per pass
constexpr int64_t kNsInvMax = 2 * kNsFwdMax + 16;
constexpr int64_t kNsTwOne = 1ll << 30;
static_assert(kNsXwMax < (1ll << 22) && kNsFwdMax < (1ll << 30) && kNsInvMax < (1ll << 31), "every value of both transforms is an int32");
// the named 64-bit sums: forward pass a 2^30 + (d t): |d| <= 2 FwdMax per component, |d t| <= sqrt(2) 2 FwdMax 2^30;  the splits
// E 2^30 + O t with |E|, |O| <= 2 FwdMax per component (|O t| <= sqrt(2) |O|_inf 2^30);  inverse pass a 2^30 + b t;  all + 2^30
static_assert(2 * kNsFwdMax * kNsTwOne + 3 * kNsFwdMax * kNsTwOne + kNsTwOne < (1ull << 63) - 1 &&
              kNsInvMax * kNsTwOne + 2 * kNsInvMax * kNsTwOne + kNsTwOne < (1ull << 63) - 1, "the 64-bit sums of a butterfly");
// the band energy: four bins of modulus^2 <= 2 FwdMax^2 (both components at the component bound)
static_assert(4ull * 2ull * (uint64_t)kNsFwdMax * (uint64_t)kNsFwdMax < (1ull << 63) && ((4ull * 2ull * (uint64_t)kNsFwdMax * (uint64_t)kNsFwdMax) >> 14) < kNsLevelMask,
              "a band's energy in 64 bits; E, and so S and N, within the mask");
static_assert(64ull * kNsLevelMask < (1ull << 62), "over_q4 N and 4 N in 64 bits");

constexpr bool ns_n_ok(uint32_t n) { return n == kNsHop || n == 2u * kNsHop || n == 3u * kNsHop || n == 4u * kNsHop; }
constexpr uint32_t ns_ctl(uint32_t v) { return v <= 3u ? v : (uint32_t)IGDSP_NS_RUN; }
inline bool ns_cfg_ok(const igdsp_ns_cfg &c)
{
    return c.floor_q15 >= 1u && c.floor_q15 <= 32768u && c.over_q4 >= 16u && c.over_q4 <= 64u && c.init_hops >= 1u && c.init_hops <= 255u &&
           c.track_shift >= 1u && c.track_shift <= 8u && c.rise_shift >= 4u && c.rise_shift <= 12u;
}
inline void ns_cfg_default(igdsp_ns_cfg &c)
{
    std::memset(&c, 0, sizeof c);
    c.floor_q15 = 5827u; c.over_q4 = 24u; c.init_hops = 16u; c.track_shift = 4u; c.rise_shift = 9u;
}

// ---- the index arithmetic of the transform (tests/test_ns_route_cpu.py: every pass a permutation, the mirror pairing)
constexpr uint32_t ns_rev7(uint32_t k)
{
    return ((k & 1u) << 6) | ((k & 2u) << 4) | ((k & 4u) << 2) | (k & 8u) | ((k & 16u) >> 2) | ((k & 32u) >> 4) | ((k & 64u) >> 6);
}
// butterfly b (0 .. 63) of the pass with span 2 * half (half = 1 << sh): its two points and its twiddle's index in the table
struct NsFly { uint32_t i, j, t; };
constexpr NsFly ns_fly(uint32_t b, uint32_t sh)
{
    const uint32_t half = 1u << sh, pos = b & (half - 1u), i = ((b >> sh) << (sh + 1u)) + pos;
    return NsFly{i, i + half, pos << (7u - sh)};
}
// the band of bin k (1 .. 128); bin 0 takes band 0
constexpr uint32_t ns_band_of(uint32_t k) { return k == 0u ? 0u : (k - 1u) >> 2; }

IGDSP_NS_HD int32_t ns_rnd(int64_t acc, uint32_t shift) { return (int32_t)((acc + (1ll << (shift - 1u))) >> shift); }
IGDSP_NS_HD uint32_t ns_bitlen(uint64_t v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }

struct NsC { int32_t re, im; };
// a 2^30 + sg (d.re, d.im) (c, ts s) -> rounded at `shift`:  (d t).re = d.re c - ts d.im s, (d t).im = d.im c + ts d.re s;
// ts = -1 forward (t = c - i s), +1 inverse
IGDSP_NS_HD NsC ns_cmad(NsC a, NsC d, int32_t c, int32_t s, int32_t ts, int32_t sg, uint32_t shift)
{
    const int64_t pr = (int64_t)d.re * c - (int64_t)ts * ((int64_t)d.im * s), pi = (int64_t)d.im * c + (int64_t)ts * ((int64_t)d.re * s);
    return NsC{ns_rnd((int64_t)a.re * kNsTwOne + sg * pr, shift), ns_rnd((int64_t)a.im * kNsTwOne + sg * pi, shift)};   // (a product: a negative a is not shifted left)
}
// one output of a split pass from A = point k and Bc = conj(point 128 - k), (c, s) = table entry k:  E = A + Bc, O = A - Bc,
// forward (E + (-s - i c) O) / 2, inverse (E + (-s + i c) O) / 2
IGDSP_NS_HD NsC ns_split(NsC A, NsC Bc, int32_t c, int32_t s, bool inverse)
{
    const int64_t er = (int64_t)A.re + Bc.re, ei = (int64_t)A.im + Bc.im, orr = (int64_t)A.re - Bc.re, oi = (int64_t)A.im - Bc.im;
    const int64_t cc = inverse ? -(int64_t)c : (int64_t)c;
    return NsC{ns_rnd(er * kNsTwOne - (int64_t)s * orr + cc * oi, 31u), ns_rnd(ei * kNsTwOne - (int64_t)s * oi - cc * orr, 31u)};
}

// per channel: the transform's points, the band gains with the edge bands repeated, the lanes' partial sums
struct NsAcc {
    uint64_t in_sq, out_sq;
    uint32_t clipped, min_gain, learning, peak;
};
struct NsWork {
    int32_t z[2 * kNsPoints];
    uint32_t g[kNsBands + 2u], pad[2];
    NsAcc red[kNsMaxLanes];
};
static_assert(sizeof(NsAcc) == 32 && sizeof(NsWork) == 1024 + 144 + 512 && sizeof(NsWork) % 16 == 0 && offsetof(NsWork, red) % 8 == 0, "ns_lds_bytes");
struct NsHost { void operator()() const {} };

// a state as it is READ: another tag (or RESET) is fresh; under the tag S and N are masked and Gt clamped, everything else stands
IGDSP_NS_HD bool ns_fresh(uint32_t tag, bool reset) { return reset || tag != (uint32_t)IGDSP_NS_TAG; }
template <class Sync>
IGDSP_NS_HD void ns_open_state(igdsp_ns_state &st, bool fresh, uint32_t lane, uint32_t L, Sync sync)
{
    for (uint32_t i = lane; i < kNsHop; i += L) {
        if (fresh) { st.prev[i] = 0; st.ola[i] = 0; }
    }
    for (uint32_t b = lane; b < kNsBands; b += L) {
        st.S[b] = fresh ? 0u : st.S[b] & kNsLevelMask;
        st.N[b] = fresh ? 0u : st.N[b] & kNsLevelMask;
        st.Gt[b] = fresh ? (uint16_t)kNsUnity : (st.Gt[b] < kNsUnity ? st.Gt[b] : (uint16_t)kNsUnity);
    }
    if (lane == 0u && fresh) st.hops = 0u;
    sync();
}
// and as it is WRITTEN (one lane)
IGDSP_NS_HD void ns_close_state(igdsp_ns_state &st, uint32_t flags)
{
    st.tag = (uint32_t)IGDSP_NS_TAG; st.flags = (uint16_t)(flags & 0xFFu); st.reserved[0] = 0u; st.reserved[1] = 0u;
}

// ---- one hop of a channel that is not bypassed: row[0 .. 79] is the hop's input on entry and its output on return
template <class Sync>
IGDSP_NS_HD void ns_hop(const igdsp_ns_cfg &cfg, igdsp_ns_state &st, NsWork &ws, const int16_t *win, const int32_t *tw, int16_t *row, uint32_t hops,
                        bool frozen, uint32_t lane, uint32_t L, Sync sync, NsAcc &acc)
{
    int32_t *z = ws.z;
    // 1. the window, packed: point k = samples 2k, 2k + 1 of prev | row; points 80 .. 127 are the padding
    for (uint32_t k = lane; k < kNsPoints; k += L) {
        int32_t v[2] = {0, 0};
        if (k < kNsHop) {
            for (uint32_t h = 0; h < 2u; ++h) {
                const uint32_t i = 2u * k + h;
                const int32_t x = i < kNsHop ? (int32_t)st.prev[i] : (int32_t)row[i - kNsHop];
                v[h] = (x * (int32_t)win[i] + 128) >> 8;
            }
        }
        z[2u * k] = v[0]; z[2u * k + 1u] = v[1];
    }
    sync();
    for (uint32_t i = lane; i < kNsHop; i += L) st.prev[i] = row[i];
    // 2. forward, decimation in frequency: a' = a + b, b' = (a - b) t
    for (uint32_t sh = 7u; sh-- > 0u;) {
        for (uint32_t b = lane; b < kNsPoints / 2u; b += L) {
            const NsFly f = ns_fly(b, sh);
            const NsC p = {z[2u * f.i], z[2u * f.i + 1u]}, q = {z[2u * f.j], z[2u * f.j + 1u]};
            const NsC zero = {0, 0}, d = {p.re - q.re, p.im - q.im};
            const NsC r = ns_cmad(zero, d, tw[2u * f.t], tw[2u * f.t + 1u], -1, 1, 30u);
            z[2u * f.i] = p.re + q.re; z[2u * f.i + 1u] = p.im + q.im;
            z[2u * f.j] = r.re; z[2u * f.j + 1u] = r.im;
        }
        sync();
    }
    //    the split pass: pairs (k, 128 - k), k = 0 .. 64
    for (uint32_t k = lane; k <= kNsPoints / 2u; k += L) {
        if (k == 0u) {
            const int32_t zr = z[0], zi = z[1];
            z[0] = zr + zi; z[1] = zr - zi;                                // bins 0 and 128, both real
        } else {
            const uint32_t pa = 2u * ns_rev7(k), pb = 2u * ns_rev7(kNsPoints - k);
            const NsC A = {z[pa], z[pa + 1u]}, B = {z[pb], z[pb + 1u]}, Ac = {A.re, -A.im}, Bc = {B.re, -B.im};
            const NsC X = ns_split(A, Bc, tw[2u * k], tw[2u * k + 1u], false);
            const NsC Xm = ns_split(B, Ac, tw[2u * (kNsPoints - k)], tw[2u * (kNsPoints - k) + 1u], false);
            z[pb] = Xm.re; z[pb + 1u] = Xm.im;
            z[pa] = X.re; z[pa + 1u] = X.im;                               // (k == 64: the same point, the same value)
        }
    }
    sync();
    // 3 - 6. the bands: energy, smoothed energy, noise estimate, gain
    for (uint32_t b = lane; b < kNsBands; b += L) {
        uint64_t e = 0u;
        for (uint32_t q = 1u; q <= 4u; ++q) {
            const uint32_t k = 4u * b + q, p = 2u * ns_rev7(k & (kNsPoints - 1u));
            const int64_t re = k == kNsPoints ? (int64_t)z[1] : (int64_t)z[p], im = k == kNsPoints ? 0 : (int64_t)z[p + 1u];
            e += (uint64_t)(re * re) + (uint64_t)(im * im);
        }
        const int64_t E = (int64_t)(e >> 14), S0 = (int64_t)st.S[b];
        const int64_t S = hops == 0u ? E : S0 + ((E - S0) >> 2);
        int64_t N = (int64_t)st.N[b];
        if (!frozen) {
            if (hops < cfg.init_hops) N += (S - N) >> 2;
            else if (S < 4 * N) N += (S - N) >> cfg.track_shift;
            else N += (N >> cfg.rise_shift) + 1;
            st.S[b] = (uint64_t)S; st.N[b] = (uint64_t)N;
        }
        const int64_t d = S - (((int64_t)cfg.over_q4 * N) >> 4);
        uint32_t G = 0u;
        if (d > 0 && S != 0) {
            const uint32_t bl = ns_bitlen((uint64_t)S), t = bl > 16u ? bl - 16u : 0u;
            const uint32_t num = (uint32_t)(d >> t) << 15, den = (uint32_t)(S >> t);
            G = num / (den ? den : 1u);
            G = G < (uint32_t)kNsUnity ? G : (uint32_t)kNsUnity;
        }
        G = G > cfg.floor_q15 ? G : cfg.floor_q15;
        ws.g[b + 1u] = G;
        if (b == 0u) ws.g[0] = G;
        if (b == kNsBands - 1u) ws.g[kNsBands + 1u] = G;
    }
    if (!frozen && hops < cfg.init_hops) acc.learning = 1u;
    sync();
    // 7, 8. smoothing over bands and over time
    for (uint32_t b = lane; b < kNsBands; b += L) {
        const int32_t gs = (int32_t)((ws.g[b] + 2u * ws.g[b + 1u] + ws.g[b + 2u] + 2u) >> 2), g0 = (int32_t)st.Gt[b];
        const int32_t gt = gs >= g0 ? gs : g0 + ((gs - g0) >> 1);
        st.Gt[b] = (uint16_t)gt;
        acc.min_gain = (uint32_t)gt < acc.min_gain ? (uint32_t)gt : acc.min_gain;
    }
    sync();
    // 9, 10. the gains, the split pass backwards
    for (uint32_t k = lane; k <= kNsPoints / 2u; k += L) {
        if (k == 0u) {
            const int64_t r0 = ((int64_t)z[0] * st.Gt[0] + 16384) >> 15, r128 = ((int64_t)z[1] * st.Gt[kNsBands - 1u] + 16384) >> 15;
            z[0] = (int32_t)((r0 + r128 + 1) >> 1); z[1] = (int32_t)((r0 - r128 + 1) >> 1);
        } else {
            const uint32_t pa = 2u * ns_rev7(k), pb = 2u * ns_rev7(kNsPoints - k);
            const int64_t ga = st.Gt[ns_band_of(k)], gb = st.Gt[ns_band_of(kNsPoints - k)];
            const NsC A = {(int32_t)(((int64_t)z[pa] * ga + 16384) >> 15), (int32_t)(((int64_t)z[pa + 1u] * ga + 16384) >> 15)};
            const NsC B = {(int32_t)(((int64_t)z[pb] * gb + 16384) >> 15), (int32_t)(((int64_t)z[pb + 1u] * gb + 16384) >> 15)};
            const NsC Ac = {A.re, -A.im}, Bc = {B.re, -B.im};
            const NsC Z = ns_split(A, Bc, tw[2u * k], tw[2u * k + 1u], true);
            const NsC Zm = ns_split(B, Ac, tw[2u * (kNsPoints - k)], tw[2u * (kNsPoints - k) + 1u], true);
            z[pb] = Zm.re; z[pb + 1u] = Zm.im;
            z[pa] = Z.re; z[pa + 1u] = Z.im;
        }
    }
    sync();
    //     inverse, decimation in time, each pass halving: a' = (a + b t) / 2, b' = (a - b t) / 2
    for (uint32_t sh = 0u; sh < 7u; ++sh) {
        for (uint32_t b = lane; b < kNsPoints / 2u; b += L) {
            const NsFly f = ns_fly(b, sh);
            const NsC p = {z[2u * f.i], z[2u * f.i + 1u]}, q = {z[2u * f.j], z[2u * f.j + 1u]};
            const NsC u = ns_cmad(p, q, tw[2u * f.t], tw[2u * f.t + 1u], 1, 1, 31u), v = ns_cmad(p, q, tw[2u * f.t], tw[2u * f.t + 1u], 1, -1, 31u);
            z[2u * f.i] = u.re; z[2u * f.i + 1u] = u.im;
            z[2u * f.j] = v.re; z[2u * f.j + 1u] = v.im;
        }
        sync();
    }
    //     synthesis window, overlap and add: y[i] = z[i] (the packed points are the samples in order)
    for (uint32_t i = lane; i < kNsHop; i += L) {
        const int64_t lo = ((int64_t)z[i] * win[i] + 16384) >> 15, hi = ((int64_t)z[i + kNsHop] * win[i + kNsHop] + 16384) >> 15;
        const int64_t o = ((int64_t)st.ola[i] + lo + 64) >> 7;
        const int64_t oc = o < -32768 ? -32768 : (o > 32767 ? 32767 : o);
        acc.clipped += oc != o ? 1u : 0u;
        row[i] = (int16_t)oc;
        st.ola[i] = (int32_t)hi;
    }
    sync();
}

// one hop of a bypassed channel: the input through the same delay; ola holds what unity gains would leave.  Item i touches index i only
IGDSP_NS_HD void ns_hop_bypass(igdsp_ns_state &st, const int16_t *win, int16_t *row, uint32_t lane, uint32_t L)
{
    for (uint32_t i = lane; i < kNsHop; i += L) {
        const int32_t x = row[i], xw = (x * (int32_t)win[i + kNsHop] + 128) >> 8;
        row[i] = st.prev[i];
        st.prev[i] = (int16_t)x;
        st.ola[i] = (int32_t)(((int64_t)xw * win[i + kNsHop] + 16384) >> 15);
    }
}

// ---- one frame of one channel.  The state is open (ns_open_state); row[0 .. n-1] is the frame's input on entry and its output on
// return.  flags0: IGDSP_NS_WAS_RESET or 0.  Every lane returns the whole frame's record in w
template <class Sync>
IGDSP_NS_HD void ns_frame_core(const igdsp_ns_cfg &cfg, igdsp_ns_state &st, NsWork &ws, const int16_t *win, const int32_t *tw, int16_t *row, uint32_t n,
                               uint32_t ctl, uint32_t flags0, uint32_t lane, uint32_t L, Sync sync, uint32_t (&w)[4], uint64_t &out_sq, uint32_t &out_peak)
{
    const bool bypass = ctl == (uint32_t)IGDSP_NS_BYPASS, frozen = ctl == (uint32_t)IGDSP_NS_FREEZE;
    NsAcc acc = {0u, 0u, 0u, (uint32_t)kNsUnity, 0u, 0u};
    for (uint32_t i = lane; i < n; i += L) { const int64_t x = row[i]; acc.in_sq += (uint64_t)(x * x); }
    uint32_t hops = st.hops;
    sync();
    for (uint32_t h = 0; h < n; h += kNsHop) {
        if (bypass) {
            ns_hop_bypass(st, win, row + h, lane, L);
        } else {
            ns_hop(cfg, st, ws, win, tw, row + h, hops, frozen, lane, L, sync, acc);
            if (!frozen) hops = hops < 65535u ? hops + 1u : 65535u;
        }
    }
    sync();
    for (uint32_t i = lane; i < n; i += L) {
        const int32_t x = row[i];
        const uint32_t a = (uint32_t)(x < 0 ? -x : x);
        acc.out_sq += (uint64_t)a * a;
        acc.peak = a > acc.peak ? a : acc.peak;
    }
    ws.red[lane] = acc;
    if (lane == 0u) st.hops = (uint16_t)hops;
    sync();
    NsAcc t = {0u, 0u, 0u, (uint32_t)kNsUnity, 0u, 0u};
    for (uint32_t l = 0; l < L; ++l) {
        const NsAcc &r = ws.red[l];
        t.in_sq += r.in_sq; t.out_sq += r.out_sq; t.clipped += r.clipped; t.learning |= r.learning;
        t.min_gain = r.min_gain < t.min_gain ? r.min_gain : t.min_gain;
        t.peak = r.peak > t.peak ? r.peak : t.peak;
    }
    uint64_t nsum = 0u;
    for (uint32_t b = 0; b < kNsBands; ++b) nsum += st.N[b];
    uint32_t flags = bypass ? (uint32_t)IGDSP_NS_BYPASSED : flags0;
    if (!bypass) {
        flags |= (t.learning ? (uint32_t)IGDSP_NS_LEARNING : 0u) | (t.min_gain < (uint32_t)kNsUnity ? (uint32_t)IGDSP_NS_SUPPRESSING : 0u) |
                 (t.clipped ? (uint32_t)IGDSP_NS_CLIPPED : 0u) | (frozen ? (uint32_t)IGDSP_NS_FROZEN : 0u);
    }
    w[0] = (uint32_t)(t.in_sq >> 8); w[1] = (uint32_t)(t.out_sq >> 8);
    w[2] = t.min_gain | (t.clipped < 65535u ? t.clipped : 65535u) << 16;
    w[3] = ns_bitlen(nsum) | flags << 8;
    out_sq = t.out_sq; out_peak = t.peak;
    sync();                                                                // red is free for the next frame
}

// ---- the host: one frame of one channel.  n and cfg checked by the caller; out and rec may be nullptr
inline void ns_frame_run(const igdsp_ns_cfg &cfg, igdsp_ns_state &st, const int16_t *pcm, uint32_t n, uint32_t ctl_in, int16_t *out, igdsp_ns_rec *rec)
{
    const uint32_t ctl = ns_ctl(ctl_in);
    const bool fresh = ns_fresh(st.tag, ctl == (uint32_t)IGDSP_NS_RESET);
    NsWork ws;
    int16_t row[kNsMaxFrame];
    uint32_t w[4], peak = 0u;
    uint64_t sq = 0u;
    std::memset(&ws, 0, sizeof ws);
    std::memcpy(row, pcm, n * sizeof(int16_t));
    ns_open_state(st, fresh, 0u, 1u, NsHost{});
    ns_frame_core(cfg, st, ws, kNsWin, kNsTw, row, n, ctl, fresh ? (uint32_t)IGDSP_NS_WAS_RESET : 0u, 0u, 1u, NsHost{}, w, sq, peak);
    ns_close_state(st, w[3] >> 8);
    if (out) std::memcpy(out, row, n * sizeof(int16_t));
    if (rec) std::memcpy(rec, w, 16);
}

}  // namespace igdsp
