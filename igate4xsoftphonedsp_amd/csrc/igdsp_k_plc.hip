// igdsp_k_plc.hip — packet loss concealment (igdsp_plc_conceal): the jitter buffer's playout ticks to continuous PCM, LOST ticks filled
// in by repeating the last pitch period with G.711 Appendix I's envelope.  Semantics: include/igdsp.h, section "Packet loss
// concealment"; independent restatement: tests/plc_model.py.
//
// Shape (route: plc_route).  A wave owns kPlcCh consecutive channels for the ticks of one part (<= kPlcPart), in four phases:
//   A. kinds: the part's tick flags and lengths go into LDS; lane ch < kPlcCh walks its channel's ticks (flags only, no samples) and
//      marks each one PLAIN (good, no run to end), IDLE, START (a run starts), CONT (a run goes on) or RECOVER (the first good tick
//      after a run).  Whether a tick is plain depends on the flags alone, so this walk is all the serial work a lossless channel does.
//   B. bulk: the PLAIN and IDLE rows, tick-major (the rows of one tick are one contiguous run of memory), kPlcPiece samples per lane
//      and piece, kPlcU pieces of a lane in flight, in batches of whole rows; per-piece sums of squares and peaks go to LDS and one
//      lane per row reduces them into the row's record.
//   C. loss: the wave takes each channel with a START, CONT or RECOVER tick in turn and walks its ticks in order.  The channel's
//      history ring lives in LDS: synthetic and faded rows are written there as they are made.  A run start gathers the last 280
//      output samples from three places: the ring (the rows this walk made, and the state's ring for samples older than the
//      launch), the input (PLAIN rows: read-only, decoded again) and zeros (IDLE rows).  Nothing this launch wrote to global memory
//      is read back.  The pitch search (pitch_search_wave, igdsp_device.h) runs one lag per lane on biased samples with v_sad_u16, the
//      key (D << 7) | p is min-reduced over the wave; the delay buffer (k_dbuf) runs the same search.  At the end of its walk the
//      channel's final ring and state go out.
//   D. the final ring of every channel without loss (positions the part overwrote: decoded input or zeros) and every channel's
//      scalar state.  Each channel's ring is written once per part; the state's ring is read only for a run that starts before the
//      part has refilled it.
// COPY (the compute-free yardstick, tools/plc_bench.py): phases A, B and D with every tick taken as PLAIN and no decode, stats or
// ring arithmetic: the input bits are widened to the output, the records carry only the length.
#include "igdsp_lanes.h"

namespace igdsp {

static_assert(sizeof(igdsp_plc_state) == 832 && alignof(igdsp_plc_state) == 4, "igdsp_plc_state layout (capi.PLC_STATE mirrors it)");
static_assert(IGDSP_MAX_PAYLOAD < IGDSP_PLC_HIST, "a tick never overlaps itself");   // (the window and the key: igdsp_pitch.h)

constexpr uint32_t kPlcH = IGDSP_PLC_HIST;
enum : uint32_t { kPkPlain = 0, kPkIdle = 1, kPkStart = 2, kPkCont = 3, kPkRecover = 4 };
enum : uint32_t { kPcGood = 0, kPcIdle = 1, kPcLost = 2 };   // phase A's flag classes

struct PlcArgs {
    const uint8_t *flags;
    const uint8_t *g711;
    const uint8_t *codec;
    const int16_t *pcm;
    const uint16_t *len;
    uint32_t C, n, pieces, batch_rows, vec;
    uint32_t t0, pt;                       // this part: ticks t0 .. t0 + pt - 1
    igdsp_plc_state *state;
    int16_t *out;
    uint16_t *len_out;
    igdsp_frame_stats *stats;
};

// one wave's LDS
struct PlcLds {
    uint16_t rec[kPlcPart][kPlcCh];                        // kind | len << 4 (len = min(len, n))
    unsigned long long psq[64 * kPlcU];                    // phase B: per-piece sums of squares
    uint32_t ppk[64 * kPlcU];                              //          and peaks
    __attribute__((aligned(16))) int16_t ring[kPlcH];      // phase C: the channel's history ring
    __attribute__((aligned(16))) uint16_t yb[kPlcH];       //          y[k] ^ 0x8000, oldest first
    __attribute__((aligned(16))) uint16_t ys[kPlcH];       //          ys[k] = yb[k + 1]: odd lags read dword pairs from here
    __attribute__((aligned(16))) int16_t cyc[IGDSP_PLC_PMAX];
    uint32_t head[kPlcCh], pitch[kPlcCh], pos[kPlcCh], missing[kPlcCh], runs[kPlcCh], conc[kPlcCh];
    uint32_t first[kPlcCh];                                // first START tick of the part, or kPlcPart; 0xFFFF: no loss work at all
};

__device__ __forceinline__ bool plc_alaw(const PlcArgs &a, uint32_t c) { return a.g711 && a.codec[c] == IGDSP_PT_PCMA; }
// x[i] of tick t (in the part) of channel c: the decoded sample, 0 at or past l
__device__ __forceinline__ int32_t plc_x(const PlcArgs &a, uint32_t t, uint32_t c, uint32_t i, uint32_t l)
{
    if (i >= l) return 0;
    const uint64_t o = ((uint64_t)(a.t0 + t) * a.C + c) * a.n + i;
    return a.g711 ? g711_s16(a.g711[o], plc_alaw(a, c)) : (int32_t)a.pcm[o];
}
__device__ __forceinline__ int32_t plc_gain(uint32_t m)
{
    const int32_t d = m > (uint32_t)IGDSP_PLC_FLAT ? (int32_t)min(m - (uint32_t)IGDSP_PLC_FLAT, 1024u) * IGDSP_PLC_STEP : 0;
    return max(0, 32768 - d);
}

__device__ __forceinline__ void plc_record(const PlcArgs &a, uint64_t o, uint64_t sumsq, uint32_t peak, uint32_t flags, bool idle)
{
    if (a.len_out) a.len_out[o] = idle ? 0u : (uint16_t)a.n;
    if (!a.stats) return;
    a.stats[o] = as_stats(idle ? pcm_record_empty() : pcm_record(sumsq, peak, a.n, flags));
}

// the output sample j of the part (j = t * n + i; j < 0: before the part) of a channel whose loss rows are in L.ring
// (ring_lds) or which has none (its older samples are in the state's ring)
__device__ __forceinline__ int32_t plc_hist(const PlcArgs &a, const PlcLds &L, uint32_t ch, uint32_t c, int32_t j, uint32_t head0, bool ring_lds)
{
    const uint32_t r = (uint32_t)((int32_t)head0 + j + (int32_t)kPlcH) % kPlcH;
    if (j < 0) return ring_lds ? L.ring[r] : a.state[c].hist[r];
    const uint32_t t = (uint32_t)j / a.n, i = (uint32_t)j - t * a.n, rc = L.rec[t][ch], kind = rc & 7u;
    if (kind == kPkIdle) return 0;
    if (kind == kPkPlain) return plc_x(a, t, c, i, rc >> 4);
    return L.ring[r];
}

template <bool COPY>
__device__ __forceinline__ void plc_bulk(const PlcArgs &a, PlcLds &L, uint32_t c0, uint32_t nch, uint32_t lane)
{
    const uint32_t P = a.pieces, n = a.n, rows = a.pt * nch;
    for (uint32_t rb = 0; rb < rows; rb += a.batch_rows) {
        const uint32_t br = min(a.batch_rows, rows - rb), items = br * P;
        uint4 v[kPlcU];
        uint32_t info[kPlcU];                      // kind | len << 4 | piece << 16; ~0u: nothing
        uint64_t off[kPlcU];
#pragma unroll
        for (uint32_t u = 0; u < kPlcU; ++u) {
            const uint32_t j = u * 64u + lane;
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            info[u] = ~0u;
            off[u] = 0;
            if (j >= items) continue;
            const uint32_t row = rb + j / P, q = j - (j / P) * P, t = row / nch, ch = row - t * nch, c = c0 + ch;
            const uint32_t rc = COPY ? ((uint32_t)n << 4) : L.rec[t][ch];
            if ((rc & 7u) > kPkIdle) continue;     // a loss row: phase C
            info[u] = (rc & 0xFFFFu) | q << 16;
            off[u] = ((uint64_t)(a.t0 + t) * a.C + c) * n + (uint64_t)q * kPlcPiece;
            if ((rc & 7u) == kPkIdle) continue;
            if (a.vec) {
                if (a.g711) { const uint2 w = *reinterpret_cast<const uint2 *>(a.g711 + off[u]); v[u] = make_uint4(w.x, w.y, 0u, 0u); }
                else        v[u] = *reinterpret_cast<const uint4 *>(a.pcm + off[u]);
            } else {
                uint32_t x[4] = {0u, 0u, 0u, 0u};
                for (uint32_t k = 0; k < kPlcPiece && q * kPlcPiece + k < n; ++k) {
                    if (a.g711) x[k >> 2] |= (uint32_t)a.g711[off[u] + k] << (8u * (k & 3u));
                    else        x[k >> 1] |= (uint32_t)(uint16_t)a.pcm[off[u] + k] << (16u * (k & 1u));
                }
                v[u] = make_uint4(x[0], x[1], x[2], x[3]);
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kPlcU; ++u) {
            const uint32_t j = u * 64u + lane;
            unsigned long long sq = 0;
            uint32_t pk = 0;
            if (info[u] != ~0u) {
                const uint32_t kind = info[u] & 7u, l = (info[u] >> 4) & 0x1FFu, q = info[u] >> 16;
                const uint32_t row = rb + j / P, t = row / nch, c = c0 + (row - t * nch);
                const bool alaw = plc_alaw(a, c);
                const uint32_t in[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (uint32_t k = 0; k < kPlcPiece; ++k) {
                    const uint32_t s = q * kPlcPiece + k;
                    int32_t x;
                    if (COPY) x = a.g711 ? (int32_t)((in[k >> 2] >> (8u * (k & 3u))) & 0xFFu) : (int32_t)(int16_t)(in[k >> 1] >> (16u * (k & 1u)));
                    else if (kind == kPkIdle || s >= l) x = 0;
                    else if (a.g711) x = g711_s16((in[k >> 2] >> (8u * (k & 3u))) & 0xFFu, alaw);
                    else x = (int32_t)(int16_t)(in[k >> 1] >> (16u * (k & 1u)));
                    o[k >> 1] |= ((uint32_t)x & 0xFFFFu) << (16u * (k & 1u));
                    if (!COPY) {
                        const uint32_t ax = (uint32_t)(x < 0 ? -x : x);
                        sq += (unsigned long long)(ax * ax);
                        pk = max(pk, ax);
                    }
                }
                int16_t *dst = a.out + off[u];
                if (a.vec) *reinterpret_cast<uint4 *>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
                else
                    for (uint32_t k = 0; k < kPlcPiece && q * kPlcPiece + k < n; ++k) dst[k] = (int16_t)(o[k >> 1] >> (16u * (k & 1u)));
            }
            L.psq[j] = sq;
            L.ppk[j] = pk;
        }
        wave_lds_fence();
        for (uint32_t rl = lane; rl < br; rl += 64u) {                    // (short rows: a batch holds up to 4 x 64 of them)
            const uint32_t row = rb + rl, t = row / nch, ch = row - t * nch, c = c0 + ch;
            const uint32_t kind = COPY ? kPkPlain : (L.rec[t][ch] & 7u);
            if (kind <= kPkIdle) {
                unsigned long long sq = 0;
                uint32_t pk = 0;
                if (!COPY)
                    for (uint32_t q = 0; q < P; ++q) { sq += L.psq[rl * P + q]; pk = max(pk, L.ppk[rl * P + q]); }
                plc_record(a, (uint64_t)(a.t0 + t) * a.C + c, sq, pk, 0u, kind == kPkIdle);
            }
        }
        wave_lds_fence();
    }
}

// phase C: channel ch's loss rows, tick by tick; then its final ring, cycle and state (L.* scalars)
__device__ __forceinline__ void plc_walk(const PlcArgs &a, PlcLds &L, uint32_t ch, uint32_t c, uint32_t lane)
{
    const uint32_t n = a.n, head0 = L.head[ch];
    uint32_t pitch = L.pitch[ch], pos = L.pos[ch], missing = L.missing[ch], runs = L.runs[ch], conc = L.conc[ch];
    igdsp_plc_state *st = a.state + c;
    // the cycle of a run that goes on from the last launch (entries >= a new pitch stay as they are)
    for (uint32_t i = lane; i < IGDSP_PLC_PMAX / 2u; i += 64u)
        reinterpret_cast<uint32_t *>(L.cyc)[i] = reinterpret_cast<const uint32_t *>(st->cycle)[i];
    // the state's ring, only if a run starts before this part has written 280 samples
    if (L.first[ch] * n < kPlcH)
        for (uint32_t i = lane; i < kPlcH / 2u; i += 64u) reinterpret_cast<uint32_t *>(L.ring)[i] = reinterpret_cast<const uint32_t *>(st->hist)[i];
    wave_lds_fence();
    for (uint32_t t = 0; t < a.pt; ++t) {
        const uint32_t rc = L.rec[t][ch], kind = rc & 7u, l = rc >> 4;
        if (kind <= kPkIdle) { missing = 0; continue; }
        const uint64_t o = (uint64_t)(a.t0 + t) * a.C + c;
        uint32_t q = 0;
        if (kind == kPkStart) {
            // the last 280 output samples, biased for the unsigned SAD
            for (uint32_t k = lane; k < kPlcH; k += 64u) {
                const uint32_t y = (uint32_t)plc_hist(a, L, ch, c, (int32_t)(t * n) - (int32_t)kPlcH + (int32_t)k, head0, true) & 0xFFFFu;
                L.yb[k] = (uint16_t)(y ^ 0x8000u);
                if (k > 0u) L.ys[k - 1u] = (uint16_t)(y ^ 0x8000u);
            }
            wave_lds_fence();
            const uint32_t p = pitch_search_wave(L.yb, L.ys, lane);
            q = p >> 2;
            for (uint32_t i = lane; i < p; i += 64u) {
                const int32_t y0 = (int16_t)(L.yb[kPlcH - p + i] ^ 0x8000u);
                int32_t v = y0;
                if (i >= p - q) {
                    const int32_t w = pitch_w(i - (p - q), q), y1 = (int16_t)(L.yb[kPlcH - 2u * p + i] ^ 0x8000u);
                    v = pitch_q15(y0 * (32768 - w) + y1 * w);
                }
                L.cyc[i] = (int16_t)v;
            }
            wave_lds_fence();
            pitch = p; pos = 0; runs += 1u; missing = 0;
        } else if (kind == kPkRecover) {
            q = pitch >> 2;
        }
        // the row: lane takes samples i = lane + 64 u
        unsigned long long sq = 0;
        uint32_t pk = 0;
        for (uint32_t i = lane; i < n; i += 64u) {
            int32_t v;
            if (kind == kPkRecover && i >= q) {
                v = plc_x(a, t, c, i, l);
            } else {
                const int32_t s = pitch_q15((int32_t)L.cyc[(pos + i) % pitch] * plc_gain(missing + i));
                if (kind == kPkStart && i < q) {
                    const int32_t w = pitch_w(i, q), y = (int16_t)(L.yb[kPlcH - 1u - i] ^ 0x8000u);
                    v = pitch_q15(y * (32768 - w) + s * w);
                } else if (kind == kPkRecover) {
                    const int32_t w = pitch_w(i, q);
                    v = pitch_q15(s * (32768 - w) + plc_x(a, t, c, i, l) * w);
                } else {
                    v = s;
                }
            }
            a.out[o * n + i] = (int16_t)v;
            L.ring[(head0 + t * n + i) % kPlcH] = (int16_t)v;
            const uint32_t ax = (uint32_t)(v < 0 ? -v : v);
            sq += (unsigned long long)(ax * ax);
            pk = max(pk, ax);
        }
        if (kind == kPkRecover) {
            pos = (pos + min(q, n)) % pitch;
            missing = 0;
        } else {
            pos = (pos + n) % pitch;
            missing = min(missing + n, 65535u);
            conc += 1u;
        }
        const uint64_t sumsq = wave_sum_u64(sq);
        pk = wave_reduce_dpp(pk, OpMax{});
        if (lane == 0u) plc_record(a, o, sumsq, pk, kind == kPkRecover ? 0u : IGDSP_FLAG_CONCEALED, false);
        wave_lds_fence();
    }
    // the final ring: position r holds output sample j of the part (j < 0: untouched)
    const int32_t N = (int32_t)(a.pt * n);
    for (uint32_t r = lane; r < kPlcH; r += 64u) {
        const int32_t j = N - 1 - (int32_t)((uint32_t)(N - 1 + (int32_t)head0 + (int32_t)kPlcH - (int32_t)r) % kPlcH);
        if (j >= 0) st->hist[r] = (int16_t)plc_hist(a, L, ch, c, j, head0, true);
    }
    for (uint32_t i = lane; i < IGDSP_PLC_PMAX / 2u; i += 64u)
        reinterpret_cast<uint32_t *>(st->cycle)[i] = reinterpret_cast<const uint32_t *>(L.cyc)[i];
    if (lane == 0u) { L.pitch[ch] = pitch; L.pos[ch] = pos; L.missing[ch] = missing; L.runs[ch] = runs; L.conc[ch] = conc; }
    wave_lds_fence();
}

template <bool COPY>
__global__ __launch_bounds__(kPlcWaves * 64) void k_plc(const PlcArgs a)
{
    __shared__ PlcLds lds[kPlcWaves];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t c0l = ((uint64_t)blockIdx.x * kPlcWaves + w) * kPlcCh;
    if (c0l >= a.C) return;                                                // waves are independent: no block barrier below
    PlcLds &L = lds[w];
    const uint32_t c0 = (uint32_t)c0l, nch = min(kPlcCh, a.C - c0), pt = a.pt, n = a.n;

    // A. kinds: flag classes and lengths of the part into LDS, then one lane per channel walks them
    for (uint32_t j = lane; j < pt * nch; j += 64u) {
        const uint32_t t = j / nch, ch = j - t * nch;
        const uint64_t o = (uint64_t)(a.t0 + t) * a.C + c0 + ch;
        const uint32_t f = a.flags[o], l = a.len ? min((uint32_t)a.len[o], n) : n;
        const uint32_t cls = (f == IGDSP_JB_PLAYED && l > 0u) ? kPcGood : ((f == IGDSP_JB_LOST || f == IGDSP_JB_PLAYED) ? kPcLost : kPcIdle);
        L.rec[t][ch] = (uint16_t)(cls | l << 4);
    }
    if (lane < nch) {
        const igdsp_plc_state *st = a.state + c0 + lane;
        const uint32_t hp = *reinterpret_cast<const uint32_t *>(&st->head), pm = *reinterpret_cast<const uint32_t *>(&st->pos);
        const uint32_t pitch = min(max(hp >> 16, (uint32_t)IGDSP_PLC_PMIN), (uint32_t)IGDSP_PLC_PMAX);
        L.head[lane] = (hp & 0xFFFFu) % kPlcH;
        L.pitch[lane] = pitch;
        L.pos[lane] = (pm & 0xFFFFu) % pitch;
        L.missing[lane] = pm >> 16;
        L.runs[lane] = st->runs;
        L.conc[lane] = st->concealed;
    }
    wave_lds_fence();
    if (lane < nch) {
        bool run = L.missing[lane] != 0u, loss = false;
        uint32_t first = kPlcPart;
        for (uint32_t t = 0; t < pt; ++t) {
            const uint32_t rc = L.rec[t][lane], cls = rc & 7u;
            uint32_t kind;
            if (COPY)                { kind = kPkPlain; }
            else if (cls == kPcGood)      { kind = run ? kPkRecover : kPkPlain; run = false; }
            else if (cls == kPcIdle) { kind = kPkIdle; run = false; }
            else                     { kind = run ? kPkCont : kPkStart; run = true; if (kind == kPkStart) first = min(first, t); }
            loss |= kind > kPkIdle;
            L.rec[t][lane] = (uint16_t)((rc & ~7u) | kind);
        }
        L.first[lane] = loss ? first : 0xFFFFu;
        if (!loss) L.missing[lane] = 0u;                                   // a part without loss rows ends outside a run
    }
    wave_lds_fence();

    // B. the plain and IDLE rows
    plc_bulk<COPY>(a, L, c0, nch, lane);

    // C. the channels with loss, one at a time
    if (!COPY)
        for (uint32_t ch = 0; ch < nch; ++ch)
            if (L.first[ch] != 0xFFFFu) plc_walk(a, L, ch, c0 + ch, lane);

    // D. the final ring of the channels without loss, and every channel's scalars
    const int32_t N = (int32_t)(pt * n);
    for (uint32_t j0 = lane; j0 < nch * kPlcH; j0 += 64u) {
        const uint32_t ch = j0 / kPlcH, r = j0 - ch * kPlcH, c = c0 + ch;
        if (L.first[ch] != 0xFFFFu) continue;
        const uint32_t head0 = L.head[ch];
        const int32_t j = N - 1 - (int32_t)((uint32_t)(N - 1 + (int32_t)head0 + (int32_t)kPlcH - (int32_t)r) % kPlcH);
        if (j < 0) continue;
        int32_t v;
        if (COPY) {
            const uint32_t t = (uint32_t)j / n, i = (uint32_t)j - t * n;
            const uint64_t o = ((uint64_t)(a.t0 + t) * a.C + c) * n + i;
            v = a.g711 ? (int32_t)a.g711[o] : (int32_t)a.pcm[o];
        } else {
            v = plc_hist(a, L, ch, c, j, head0, false);
        }
        a.state[c].hist[r] = (int16_t)v;
    }
    if (lane < nch) {
        igdsp_plc_state *st = a.state + c0 + lane;
        *reinterpret_cast<uint32_t *>(&st->head) = ((L.head[lane] + pt * n) % kPlcH) | L.pitch[lane] << 16;
        *reinterpret_cast<uint32_t *>(&st->pos) = L.pos[lane] | L.missing[lane] << 16;
        st->runs = L.runs[lane];
        st->concealed = L.conc[lane];
    }
}

hipError_t launch_plc_conceal(const LaunchCfg &, const uint8_t *flags, const uint8_t *g711, const uint8_t *codec, const int16_t *pcm,
                              const uint16_t *len, uint32_t C, uint32_t T, uint32_t n, igdsp_plc_state *state, int16_t *out, uint16_t *len_out,
                              igdsp_frame_stats *stats, bool yardstick, hipStream_t s)
{
    const PlcRoute r = plc_route(C, T, n, pcm != nullptr, reinterpret_cast<uintptr_t>(pcm ? (const void *)pcm : (const void *)g711),
                                 reinterpret_cast<uintptr_t>(out));
    if (r.grid == 0) return hipSuccess;
    PlcArgs a{flags, g711, codec, pcm, len, C, n, r.pieces, r.batch_rows, r.vec, 0u, 0u, state, out, len_out, stats};
    const auto kernel = yardstick ? k_plc<true> : k_plc<false>;
    for (uint32_t p = 0; p < r.parts; ++p) {
        a.t0 = p * kPlcPart;
        a.pt = std::min(kPlcPart, T - a.t0);
        hipLaunchKernelGGL(kernel, dim3(r.grid), dim3(r.threads), 0, s, a);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace igdsp
