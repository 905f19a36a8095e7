// igdsp_k_rs.hip — the bridge's rate converter (igdsp_resample): the resampling pjmedia's conference bridge does on every call port
// when media_cfg.clock_rate is not the streams' 8 kHz (roip_ed137.cpp:3031-3032), batched over channels and frames, with the records.
// Semantics: include/igdsp.h, section "Rate converter"; the rules themselves: the constexpr functions of igdsp_route.h (rs_up_raw,
// rs_down_raw, rs_pair, rs_frame_run), which igdsp_rs_frame runs on the host; independent restatement: tests/rs_model.py.
//
// Shape (rs_route, igdsp_route.h).  A wave owns CH consecutive channels (UP 16, DOWN 4) for the frames of one chunk and keeps, per
// channel, the input row behind its HIST = 24 (UP) / 24 R (DOWN) predecessors in a tile of LDS, int16, the row's first sample on a
// 16-byte boundary.  Per frame:
//   1. the predecessors: in a chunk's first frame sample by sample from the state (g < 0) or the earlier rows (short rows: several of
//      them); in every later frame the tile's own last HIST samples, moved to its front through registers;
//   2. the row: 16-byte loads (8-byte for G.711, expanded through a 1 KiB signed table in LDS built from the segment formulas), zeros
//      past d_len; the general form loads a sample at a time;
//   3. a lane takes units of 8 narrow samples.  UP: the 32 tile samples that end with the unit's 8 inputs, as 16 dwords E (four
//      ds_read_b128) and the 15 dwords O between them (v_alignbit): output g R + p is 12 v_dot2c_i32_i16 of E (g odd) or O (g even) with
//      the phase's taps, which are constants of the instantiation (rs_pair: literals / SGPRs, no table in memory); R 16-byte stores.
//      DOWN: the 32 R tile samples that end with the unit's 8 R inputs; output g is 12 R dot products starting at dword (g + 1) R / 2
//      (O where (g + 1) R is odd: R = 3 only); one 16-byte store;
//   4. the records: per output piece four packed dot products and min / max of the eight values BEFORE the clamp (max |y| is
//      |clamp| of one of the two, and the clamp fired iff one of them left int16), three LDS atomics into the output row's slot; after
//      the frame a lane per slot writes the record.
// The accumulator starts at 8192 (the rounding term), so a sample is 12 (or 12 R) dot products, a shift and a v_med3.
// The state is written by k_rs_state behind the kernel on the stream: a block per channel at a time, a thread per history sample.
// COPY (the compute-free yardstick, tools/rs_bench.py): steps 1 - 3 with the same loads, LDS traffic and stores, an xor instead of the
// dot products, zero records, no state (the samples ahead of a launch's first frame are zeros; in the general form so are the tile
// samples between a row's end and its last unit's end).
#include "igdsp_device.h"
#include "igdsp_pcmrec.h"

namespace igdsp {

struct RsArgs {
    const uint8_t *g711, *codec;
    const int16_t *pcm;
    const uint16_t *len;
    igdsp_rs_state *state;
    int16_t *out;
    igdsp_frame_stats *stats;
    uint32_t C, F;
    uint32_t SI, LI, rows_in;          // the input side: sub-frames per frame, samples per row, rows per (sub-)frame
    uint32_t SO, LO, rows_out;         // the output side
    uint32_t pieces, groups, chunk_frames, chunks;
};

struct RsSlot { unsigned long long sq; int32_t mx, mn; };           // 16 bytes per output row of the frame
static_assert(sizeof(RsSlot) == 16, "rs_lds_bytes counts 16 bytes per slot");

template <int... I, class Fn> __device__ __forceinline__ void rs_for_impl(std::integer_sequence<int, I...>, Fn &&fn) { (fn(std::integral_constant<int, I>{}), ...); }
template <int N, class Fn> __device__ __forceinline__ void rs_for(Fn &&fn) { rs_for_impl(std::make_integer_sequence<int, N>{}, fn); }
template <uint32_t DIR, uint32_t R, uint32_t P, uint32_t T0> struct RsPair { static constexpr uint32_t v = rs_pair(DIR, R, P, T0); };

// signed expansion table: dec[alaw << 8 | code]
__device__ __forceinline__ void rs_fill_dec(int16_t *dec)
{
    for (uint32_t i = threadIdx.x; i < 512u; i += blockDim.x) {
        const int32_t m = (int32_t)((i & 256u) ? alaw_abs(i & 255u) : ulaw_abs(i & 255u));
        dec[i] = (int16_t)((i & 0x80u) ? m : -m);
    }
}

// where sample s of (f, c)'s input is: the row (also d_len's index), the sample's place in it, the element offset
__device__ __forceinline__ uint64_t rs_in_off(const RsArgs &a, uint64_t f, uint32_t c, uint32_t s, uint32_t &idx, uint64_t &row)
{
    const uint32_t sub = a.SI == 1u ? 0u : s / a.LI;
    idx = s - sub * a.LI;
    row = (f * a.SI + sub) * a.rows_in + c;
    return row * a.LI + idx;
}
// (g711: a.g711, or nullptr where the caller knows there is none: DOWN takes PCM only)
__device__ __forceinline__ int16_t rs_x(const RsArgs &a, const uint8_t *g711, const int16_t *dec, uint64_t f, uint32_t c, uint32_t s)
{
    uint32_t idx;
    uint64_t row;
    const uint64_t o = rs_in_off(a, f, c, s, idx, row);
    if (a.len && idx >= a.len[row]) return 0;
    if (g711) return dec[(a.codec[c] == IGDSP_PT_PCMA ? 256u : 0u) | g711[o]];
    return a.pcm[o];
}

__device__ __forceinline__ int32_t rs_dot(uint32_t x, uint32_t taps, int32_t acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2i16, x), __builtin_bit_cast(v2i16, taps), acc, false);
}
__device__ __forceinline__ uint32_t rs_pack(int32_t lo, int32_t hi) { return ((uint32_t)rs_clamp16(lo) & 0xFFFFu) | ((uint32_t)rs_clamp16(hi) << 16); }

// eight consecutive output samples q0 .. q0 + 7 of a channel's frame, before the clamp: the stores and the records' sums.  obase: the
// element offset of the frame's first output row of the channel; a further sub-frame is sstride elements on
template <bool VEC>
__device__ __forceinline__ void rs_emit(const RsArgs &a, RsSlot *slots, uint64_t obase, uint64_t sstride, uint32_t q0, const int32_t (&raw)[8])
{
    if constexpr (VEC) {                                                       // n % 8 == 0: the piece lies in one row
        const uint32_t sub = a.SO == 1u ? 0u : q0 / a.LO, idx = q0 - sub * a.LO;
        const uint4 v = make_uint4(rs_pack(raw[0], raw[1]), rs_pack(raw[2], raw[3]), rs_pack(raw[4], raw[5]), rs_pack(raw[6], raw[7]));
        if (a.out) *reinterpret_cast<uint4 *>(a.out + obase + (a.SO == 1u ? 0ull : sub * sstride) + idx) = v;
        if (a.stats) {
            // a dot product of two squares is at most 2^31 (two samples of -32768): an unsigned 32-bit value; the four are added in 64 bits
            const unsigned long long sq = (unsigned long long)(uint32_t)rs_dot(v.x, v.x, 0) + (uint32_t)rs_dot(v.y, v.y, 0) +
                                          (unsigned long long)(uint32_t)rs_dot(v.z, v.z, 0) + (uint32_t)rs_dot(v.w, v.w, 0);
            int32_t mx = raw[0], mn = raw[0];
#pragma unroll
            for (int i = 1; i < 8; ++i) { mx = max(mx, raw[i]); mn = min(mn, raw[i]); }
            lds_add(&slots[sub].sq, sq);
            __hip_atomic_fetch_max(&slots[sub].mx, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_min(&slots[sub].mn, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    } else {
        const uint32_t n_out = a.SO * a.LO;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t q = q0 + (uint32_t)i;
            if (q >= n_out) continue;
            const uint32_t sub = a.SO == 1u ? 0u : q / a.LO, idx = q - sub * a.LO;
            const int32_t y = rs_clamp16(raw[i]);
            if (a.out) a.out[obase + sub * sstride + idx] = (int16_t)y;
            if (a.stats) {
                lds_add(&slots[sub].sq, (unsigned long long)(uint32_t)(y * y));
                __hip_atomic_fetch_max(&slots[sub].mx, raw[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_min(&slots[sub].mn, raw[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
}

// (the second launch bound: waves per SIMD = resident blocks, the registers the route's residency allows)
template <int DIR, int R, bool COPY, bool VEC>
__global__ __launch_bounds__(kRsWaves * 64, rs_resident(DIR, R)) void k_rs(const RsArgs a)
{
    constexpr uint32_t CH = rs_ch(DIR), LANES = rs_lanes(DIR), HIST = rs_hist(DIR, R), TILE = rs_tile(DIR, R);
    constexpr bool UP = DIR == (int)IGDSP_RS_UP;
    constexpr uint32_t NE = UP ? 16u : 16u * R;                                // dwords a unit reads
    static_assert((TILE * 2u) % 16u == 0u && (HIST * 2u) % 16u == 0u && HIST <= kRsHist, "tile rows and their input rows start on 16 bytes");
    static_assert(((uint32_t)IGDSP_MAX_PAYLOAD / 8u - 1u) * (UP ? 8u : 8u * R) + 2u * NE <= TILE, "the last unit's reads end inside the tile");
    __shared__ __attribute__((aligned(16))) int16_t tiles[kRsWaves][CH][TILE];
    __shared__ __attribute__((aligned(16))) RsSlot slot_mem[kRsWaves][CH][R];
    __shared__ int16_t dec[UP ? 512 : 2];
    if constexpr (UP) {
        rs_fill_dec(dec);
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, k = lane / LANES, j = lane % LANES;
    int16_t (*tile)[TILE] = tiles[w];
    RsSlot (*slots)[R] = slot_mem[w];
    const uint32_t n_in = a.SI * a.LI;
    const uint8_t *const g711 = UP ? a.g711 : nullptr;
    const uint64_t sstride = (uint64_t)a.rows_out * a.LO;
    // (groups * chunks fits 32 bits: frames are cut only while the groups are fewer than the waves wanted, rs_route)
    const uint32_t n_items = a.groups * a.chunks, stride = gridDim.x * kRsWaves;
    for (uint32_t item = blockIdx.x * kRsWaves + w; item < n_items; item += stride) {
        const uint32_t ck = item / a.groups, g = item - ck * a.groups;            // neighbouring waves: neighbouring channels
        const uint32_t c0 = g * CH, f0 = ck * a.chunk_frames, f1 = min(a.F, f0 + a.chunk_frames);
        const uint32_t c = c0 + k;
        for (uint32_t f = f0; f < f1; ++f) {
            // 1. the predecessors
            if (f == f0) {
                for (uint32_t u = lane; u < CH * HIST; u += 64u) {
                    const uint32_t kk = u / HIST, h = u % HIST, cc = c0 + kk;
                    int16_t v = 0;
                    if (cc < a.C) {
                        const int64_t pos = (int64_t)((uint64_t)f * n_in) - (int64_t)HIST + (int64_t)h;
                        if (pos >= 0) v = rs_x(a, g711, dec, (uint64_t)pos / n_in, cc, (uint32_t)((uint64_t)pos % n_in));
                        else if (!COPY) v = a.state[cc].hist[(int64_t)kRsHist + pos];             // pos >= -HIST >= -144
                    }
                    tile[kk][h] = v;
                }
            } else {
                constexpr uint32_t NSH = (CH * HIST + 63u) / 64u;
                int16_t keep[NSH];
#pragma unroll
                for (uint32_t i = 0; i < NSH; ++i) {
                    const uint32_t u = lane + 64u * i;
                    keep[i] = u < CH * HIST ? tile[u / HIST][n_in + u % HIST] : (int16_t)0;
                }
                wave_lds_fence();
#pragma unroll
                for (uint32_t i = 0; i < NSH; ++i) {
                    const uint32_t u = lane + 64u * i;
                    if (u < CH * HIST) tile[u / HIST][u % HIST] = keep[i];
                }
            }
            // 2. the row
            if constexpr (VEC) {
                const uint32_t ppr = n_in >> 3;
                for (uint32_t u = lane; u < CH * ppr; u += 64u) {
                    const uint32_t kk = u / ppr, s0 = (u - kk * ppr) * 8u, cc = c0 + kk;
                    if (cc >= a.C) continue;
                    uint32_t idx;
                    uint64_t row;
                    const uint64_t o = rs_in_off(a, f, cc, s0, idx, row);
                    uint4 v;
                    if (g711) {
                        const uint2 cw = *reinterpret_cast<const uint2 *>(g711 + o);
                        if constexpr (COPY) {
                            v = make_uint4(cw.x, cw.y, cw.x, cw.y);
                        } else {
                            const uint32_t law = a.codec[cc] == IGDSP_PT_PCMA ? 256u : 0u;
                            auto two = [&](uint32_t wd, uint32_t sh) {
                                return (uint32_t)(uint16_t)dec[law | ((wd >> sh) & 255u)] | ((uint32_t)(uint16_t)dec[law | ((wd >> (sh + 8u)) & 255u)] << 16);
                            };
                            v = make_uint4(two(cw.x, 0u), two(cw.x, 16u), two(cw.y, 0u), two(cw.y, 16u));
                        }
                    } else {
                        v = ld_stream(reinterpret_cast<const uint4 *>(a.pcm + o));
                    }
                    if (a.len) {
                        const uint32_t l = a.len[row], valid = l > idx ? l - idx : 0u;
                        auto keep = [&](uint32_t first) { return valid > first + 1u ? 0xFFFFFFFFu : (valid > first ? 0xFFFFu : 0u); };
                        v.x &= keep(0u); v.y &= keep(2u); v.z &= keep(4u); v.w &= keep(6u);
                    }
                    *reinterpret_cast<uint4 *>(&tile[kk][HIST + s0]) = v;
                }
            } else {
                // (the yardstick folds whole units: it takes the samples between the row's end and its last unit's end as zeros, not as
                // what the LDS held; the filter's windows end at a valid sample and never read them)
                const uint32_t n_row = COPY ? a.pieces * (UP ? 8u : 8u * R) : n_in;
                for (uint32_t u = lane; u < CH * n_row; u += 64u) {
                    const uint32_t kk = u / n_row, s = u - kk * n_row, cc = c0 + kk;
                    if (cc < a.C) tile[kk][HIST + s] = (!COPY || s < n_in) ? rs_x(a, g711, dec, f, cc, s) : (int16_t)0;
                }
            }
            if (a.stats)
                for (uint32_t u = lane; u < CH * (uint32_t)R; u += 64u) slots[u / R][u % R] = RsSlot{0ull, INT32_MIN, INT32_MAX};
            wave_lds_fence();
            // 3. the units
            if (c < a.C) {
                const uint64_t obase = ((uint64_t)f * a.SO * a.rows_out + c) * a.LO;
                for (uint32_t pc = j; pc < a.pieces; pc += LANES) {
                    uint32_t E[NE];
                    const uint4 *src = reinterpret_cast<const uint4 *>(&tile[k][pc * (UP ? 8u : 8u * R)]);
#pragma unroll
                    for (uint32_t i = 0; i < NE / 4u; ++i) {
                        const uint4 t = src[i];
                        E[4 * i] = t.x; E[4 * i + 1] = t.y; E[4 * i + 2] = t.z; E[4 * i + 3] = t.w;
                    }
                    auto O = [&](uint32_t d) { return __builtin_amdgcn_alignbit(E[d + 1u], E[d], 16u); };   // samples 2 d + 1, 2 d + 2
                    constexpr int NOUT = UP ? R : 1;                           // 16-byte pieces a unit writes
                    int32_t raw[NOUT][8];
                    if constexpr (COPY) {
                        uint32_t x[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                        for (uint32_t d = 0; d < NE; ++d) x[d & 3u] ^= E[d];
#pragma unroll
                        for (int m = 0; m < NOUT; ++m)
#pragma unroll
                            for (int i = 0; i < 8; ++i) raw[m][i] = (int32_t)(int16_t)(x[i >> 1] >> (16 * (i & 1)));
                    } else if constexpr (UP) {
                        rs_for<8>([&](auto jc) {                               // narrow sample jc of the unit: window start jc + 1
                            rs_for<R>([&](auto pcn) {
                                constexpr int jn = decltype(jc)::value, p = decltype(pcn)::value, wst = jn + 1, li = jn * R + p;
                                int32_t acc = 8192;
                                rs_for<12>([&](auto mc) {
                                    constexpr int t0 = 2 * decltype(mc)::value;
                                    constexpr uint32_t taps = RsPair<IGDSP_RS_UP, R, p, t0>::v;
                                    if constexpr (wst % 2 == 0) acc = rs_dot(E[(wst + t0) / 2], taps, acc);
                                    else acc = rs_dot(O((wst + t0 - 1) / 2), taps, acc);
                                });
                                raw[li / 8][li % 8] = acc >> 14;
                            });
                        });
                    } else {
                        rs_for<8>([&](auto jc) {                               // narrow output jc of the unit: window start (jc + 1) R
                            constexpr int jn = decltype(jc)::value, wst = (jn + 1) * R;
                            int32_t acc = 8192;
                            rs_for<12 * R>([&](auto mc) {
                                constexpr int t0 = 2 * decltype(mc)::value;
                                constexpr uint32_t taps = RsPair<IGDSP_RS_DOWN, R, 0, t0>::v;
                                if constexpr (wst % 2 == 0) acc = rs_dot(E[(wst + t0) / 2], taps, acc);
                                else acc = rs_dot(O((wst + t0 - 1) / 2), taps, acc);
                            });
                            raw[0][jn] = acc >> 14;
                        });
                    }
#pragma unroll
                    for (int m = 0; m < NOUT; ++m) rs_emit<VEC>(a, slots[k], obase, sstride, pc * 8u * NOUT + 8u * m, raw[m]);
                }
            }
            // 4. the records
            if (a.stats) {
                wave_lds_fence();
                for (uint32_t u = lane; u < CH * a.SO; u += 64u) {
                    const uint32_t kk = u / a.SO, sub = u - kk * a.SO, cc = c0 + kk;
                    if (cc >= a.C) continue;
                    const RsSlot sl = slots[kk][sub];
                    uint4 rec = make_uint4(0u, 0u, 0u, 0u);                    // COPY: a zero record, flags 0
                    if (!COPY) {
                        const int32_t hi = rs_clamp16(sl.mx), lo = rs_clamp16(sl.mn);
                        const uint32_t peak = (uint32_t)max(hi < 0 ? -hi : hi, lo < 0 ? -lo : lo);
                        rec = pcm_record(sl.sq, peak, a.LO, sl.mx > 32767 || sl.mn < -32768 ? (uint32_t)IGDSP_FLAG_SATURATED : 0u);
                    }
                    a.stats[((uint64_t)f * a.SO + sub) * a.C + cc] = as_stats(rec);
                }
            }
            wave_lds_fence();                                                  // the tile and the slots are rewritten next
        }
    }
}

// the state behind k_rs: hist = the last 144 of (old hist, the launch's input), frames += F.  A block takes a channel at a time; every
// thread has read its sample before any writes
__global__ __launch_bounds__(kRsStateThreads) void k_rs_state(const RsArgs a)
{
    __shared__ int16_t dec[512];
    if (a.g711) {                                                            // (the same for every thread)
        rs_fill_dec(dec);
        __syncthreads();
    }
    const uint32_t i = threadIdx.x, n_in = a.SI * a.LI;
    const uint64_t total = (uint64_t)a.F * n_in;
    for (uint32_t c = blockIdx.x; c < a.C; c += gridDim.x) {                 // the same trips for every thread of a block
        int16_t v = 0;
        if (i < kRsHist) {
            if (total + i >= kRsHist) {
                const uint64_t pos = total + i - kRsHist;
                v = rs_x(a, a.g711, dec, pos / n_in, c, (uint32_t)(pos % n_in));
            } else {
                v = a.state[c].hist[total + i];
            }
        }
        __syncthreads();
        if (i < kRsHist) a.state[c].hist[i] = v;
        else if (i == kRsHist) a.state[c].frames += a.F;
    }
}

hipError_t launch_rs(const LaunchCfg &cfg, uint32_t dir, uint32_t R, uint32_t layout, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm,
                     const uint16_t *len, igdsp_rs_state *state, uint32_t C, uint32_t F, uint32_t n, uint32_t rows_narrow, uint32_t rows_wide,
                     int16_t *out, igdsp_frame_stats *stats, bool yardstick, hipStream_t s)
{
    const RsRoute r = rs_route(dir, R, C, F, n, g711 != nullptr, yardstick, reinterpret_cast<uintptr_t>(g711 ? (const void *)g711 : (const void *)pcm),
                               reinterpret_cast<uintptr_t>(out), (uint32_t)cfg.compute_units, rs_blocks_from_env());
    if (r.grid == 0) return hipSuccess;
    const bool up = dir == IGDSP_RS_UP, sub = layout == IGDSP_RS_SUBFRAMES;
    const uint32_t rn = rows_narrow ? rows_narrow : C, rw = rows_wide ? rows_wide : C, ws = sub ? R : 1u, wl = sub ? n : n * R;
    const RsArgs a{g711, codec, pcm, len, state, out, stats, C, F,
                   up ? 1u : ws, up ? n : wl, up ? rn : rw,
                   up ? ws : 1u, up ? wl : n, up ? rw : rn,
                   r.pieces, r.groups, r.chunk_frames, r.chunks};
    with_bool(yardstick, [&](auto Y) { with_bool(r.vec != 0u, [&](auto V) { with_key(Keys<2, 3, 4, 6>{}, (int)R, [&](auto RR) {
        if (up) hipLaunchKernelGGL((k_rs<(int)IGDSP_RS_UP, RR, Y, V>), dim3(r.grid), dim3(r.threads), 0, s, a);
        else hipLaunchKernelGGL((k_rs<(int)IGDSP_RS_DOWN, RR, Y, V>), dim3(r.grid), dim3(r.threads), 0, s, a); }); }); });
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (r.state_grid) hipLaunchKernelGGL(k_rs_state, dim3(r.state_grid), dim3(kRsStateThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace igdsp
