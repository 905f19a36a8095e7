// igdsp_k_tx.hip — the ED-137 TX packetizer (igdsp_tx_packetize): transport_send_rtp (TransportAdapter.cpp:635-874) batched over
// channels and frames.  Semantics: include/igdsp.h, section "ED-137 TX packetizer"; independent restatement: tests/tx_model.py.
//
// Shape.  A wavefront owns kTxCh consecutive channels for the whole launch (their state is a serial scan over the frames) and
// walks the frames in chunks of kTxFc:
//   decision  lanes 0 .. kTxCh-1, one per channel, state in registers: gate, keep-alive clock, debounce, ED-137 word, size / PT
//             ladder, counters.  One 16-byte record per (frame, channel) goes to the wave's LDS slice.
//   bulk      all 64 lanes walk the chunk's packets dword by dword (packet p = frame-major, kTxCh channels of a frame are
//             neighbours in memory): header dwords from the record, payload dwords re-encoded from the frame the record names
//             (this frame, an earlier gated frame of the launch, or the send buffer), plus this frame's own bytes where the
//             audioLevel sum (LDS add) and the silence probe (bytes 40 / 50 / 60) need them.  Dword stores only up to size.
//   close     lanes 0 .. kTxCh-1 again: sizes / info, the silence run and the last level, frame order.
// A wave touches only its own channels' state, send buffers and LDS slice, so no barrier is needed after the table load.
// PCM input of large launches reads the compressor from the context's 128 KiB table copied into LDS (k_encode_lut16's scheme);
// small launches evaluate enc_uni per sample instead of paying the copy per block.
#include "igdsp_device.h"

#include <atomic>

namespace igdsp {

static_assert(sizeof(igdsp_tx_chan) == 64 && alignof(igdsp_tx_chan) == 8, "igdsp_tx_chan is 64 bytes (capi.TX_CHAN)");
static_assert(sizeof(igdsp_tx_info) == 8, "igdsp_tx_info is 8 bytes (capi.TX_INFO)");

constexpr int kTxFc = 8;                        // frames per chunk
constexpr int kTxPk = kTxCh * kTxFc;            // packets per chunk (128)
#ifndef IGDSP_TX_UNROLL
#define IGDSP_TX_UNROLL 4
#endif
constexpr int kTxU = IGDSP_TX_UNROLL;           // bulk iterations whose loads are issued together

// record meta word
constexpr uint32_t kMSize20 = 1u, kMSizeFull = 2u;            // bits 0-1: size class
constexpr uint32_t kMValid = 1u << 25, kMProbeFail = 1u << 26;  // frame exists; a probe byte was not 0xD5

struct TxArgs {
    const int16_t *pcm;
    const uint8_t *g711;
    const uint8_t *ctl;
    uint32_t C, F, n;
    uint64_t t0;
    uint32_t frame_ms;
    igdsp_tx_chan *state;
    uint8_t *last;
    uint8_t *packets;
    uint32_t stride;
    uint16_t *sizes;
    igdsp_tx_info *info;
    const uint8_t *tab_g;
    uint32_t n_groups;
    uint32_t vec;      // n % 4 == 0 and every payload row dword (g711) / 8-byte (pcm) aligned
};

template <int FORM, int VARIANT>
__device__ __forceinline__ uint32_t enc_sample(int v, uint32_t law, const uint8_t *tab)
{
    if (FORM == kTxPcmTab) return tab[(law << 16) | ((uint32_t)v & 0xFFFFu)];
    return enc_uni<VARIANT>(v, enc_consts<VARIANT>(law != 0u));
}

// Encoded bytes 4q .. 4q+3 of frame row `row` (= f * C + c) as a little-endian dword; bytes at or past n read as 0.
template <int FORM, int VARIANT>
__device__ __forceinline__ uint32_t frame_dword(const TxArgs &a, uint64_t row, uint32_t q, uint32_t law, const uint8_t *tab)
{
    const uint64_t e = row * a.n + 4u * q;
    const uint32_t k = min(a.n - 4u * q, 4u);
    uint32_t d = 0;
    if (FORM == kTxG711) {
        if (a.vec) return *reinterpret_cast<const uint32_t *>(a.g711 + e);
        for (uint32_t i = 0; i < k; ++i) d |= (uint32_t)a.g711[e + i] << (8u * i);
    } else {
        if (a.vec) {
            const uint2 w = *reinterpret_cast<const uint2 *>(a.pcm + e);
            return enc_sample<FORM, VARIANT>((int)(int16_t)(w.x & 0xFFFFu), law, tab) | enc_sample<FORM, VARIANT>((int)(int16_t)(w.x >> 16), law, tab) << 8 |
                   enc_sample<FORM, VARIANT>((int)(int16_t)(w.y & 0xFFFFu), law, tab) << 16 | enc_sample<FORM, VARIANT>((int)(int16_t)(w.y >> 16), law, tab) << 24;
        }
        for (uint32_t i = 0; i < k; ++i) d |= enc_sample<FORM, VARIANT>((int)a.pcm[e + i], law, tab) << (8u * i);
    }
    return d;
}

// The vector form of frame_dword in two halves: the load, and the encode once the load is back.
template <int FORM>
__device__ __forceinline__ uint2 raw_load(const TxArgs &a, uint64_t row, uint32_t q)
{
    const uint64_t e = row * a.n + 4u * q;
    if (FORM == kTxG711) return make_uint2(*reinterpret_cast<const uint32_t *>(a.g711 + e), 0u);
    return *reinterpret_cast<const uint2 *>(a.pcm + e);
}

template <int FORM, int VARIANT>
__device__ __forceinline__ uint32_t encode_raw(uint2 w, uint32_t law, const uint8_t *tab)
{
    if (FORM == kTxG711) return w.x;
    return enc_sample<FORM, VARIANT>((int)(int16_t)(w.x & 0xFFFFu), law, tab) | enc_sample<FORM, VARIANT>((int)(int16_t)(w.x >> 16), law, tab) << 8 |
           enc_sample<FORM, VARIANT>((int)(int16_t)(w.y & 0xFFFFu), law, tab) << 16 | enc_sample<FORM, VARIANT>((int)(int16_t)(w.y >> 16), law, tab) << 24;
}

__device__ __forceinline__ uint32_t last_dword(const TxArgs &a, uint32_t c, uint32_t q)
{
    const uint64_t e = (uint64_t)c * a.n + 4u * q;
    if (a.vec) return *reinterpret_cast<const uint32_t *>(a.last + e);
    uint32_t d = 0;
    for (uint32_t i = 0, k = min(a.n - 4u * q, 4u); i < k; ++i) d |= (uint32_t)a.last[e + i] << (8u * i);
    return d;
}

// store bytes [0, k) of dword d at p (k == 4: one dword store; p is dword aligned)
__device__ __forceinline__ void put_dword(uint8_t *p, uint32_t d, uint32_t k)
{
    if (k >= 4u) { *reinterpret_cast<uint32_t *>(p) = d; return; }
    for (uint32_t i = 0; i < k; ++i) p[i] = (uint8_t)(d >> (8u * i));
}

template <int FORM, int VARIANT>
__global__ __launch_bounds__(kTxWaves * 64) void k_tx_packetize(const TxArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t tab[];          // kTxPcmTab: 2 x 65 536 compressor codes
    __shared__ uint32_t r_word[kTxWaves][kTxPk], r_meta[kTxWaves][kTxPk];
    __shared__ int32_t r_src[kTxWaves][kTxPk], r_sum[kTxWaves][kTxPk];
    __shared__ uint32_t c_seq[kTxWaves][kTxCh], c_ts[kTxWaves][kTxCh], c_ssrc[kTxWaves][kTxCh], c_law[kTxWaves][kTxCh];
    if (FORM == kTxPcmTab) {
        if (a.tab_g != nullptr) {
            for (uint32_t i = threadIdx.x * 16u; i < 2u * 65536u; i += blockDim.x * 16u)
                *reinterpret_cast<uint4 *>(tab + i) = *reinterpret_cast<const uint4 *>(a.tab_g + i);
        } else {
            const EncK ku = enc_consts<VARIANT>(false), ka = enc_consts<VARIANT>(true);
            for (uint32_t i = threadIdx.x; i < 2u * 65536u; i += blockDim.x)
                tab[i] = (uint8_t)enc_uni<VARIANT>((int)(int16_t)(i & 0xFFFFu), (i >> 16) ? ka : ku);
        }
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t n = a.n, C = a.C, F = a.F;
    const uint32_t D = 5u + (n + 3u) / 4u;                                  // dwords of a full packet's footprint
    const uint32_t q64 = 64u / D, r64 = 64u % D;
    uint32_t *rw = r_word[w], *rm = r_meta[w];
    int32_t *rs = r_src[w], *rl = r_sum[w];

    for (uint32_t g = blockIdx.x * kTxWaves + w; g < a.n_groups; g += gridDim.x * kTxWaves) {
        const uint32_t c0 = g * kTxCh;
        // ---- per-channel state (decision lanes) ----
        const uint32_t c = c0 + lane;
        const bool dl = lane < (uint32_t)kTxCh && c < C;
        TxState s;
        if (dl) {
            s.load(a.state + c);
            c_seq[w][lane] = s.seq; c_ts[w][lane] = s.ts; c_ssrc[w][lane] = s.ssrc; c_law[w][lane] = s.pt == IGDSP_PT_PCMA ? 1u : 0u;
        }
        int32_t glast = -1;                                                  // last frame the gate copied in this launch
        const uint32_t pt7 = s.pt & 0x7Fu;
        wave_sync();
        for (uint32_t f0 = 0; f0 < F; f0 += kTxFc) {
            // ---- decision: one lane per channel, frames in order ----
            if (lane < (uint32_t)kTxCh) {
                // the chunk's control bytes in one go (clamped addresses, no branches: eight loads in flight, not one per frame)
                uint32_t ctlv[kTxFc];
                const uint32_t cl = min(c, C - 1u);
#pragma unroll
                for (int fl = 0; fl < kTxFc; ++fl) ctlv[fl] = a.ctl ? a.ctl[(uint64_t)min(f0 + fl, F - 1u) * C + cl] : 0u;
#pragma unroll
                for (int fl = 0; fl < kTxFc; ++fl) {
                    const uint32_t f = f0 + fl, p = fl * kTxCh + lane;
                    if (!dl || f >= F) { rm[p] = 0u; continue; }
                    const uint32_t ctl = ctlv[fl];
                    if (ctl & IGDSP_TX_CTL_SET) { s.ptt = ctl & 1u; s.sql = (ctl >> 1) & 1u; }
                    const uint32_t mk = (ctl >> 2) & 1u;
                    const uint64_t now = a.t0 + (uint64_t)f * a.frame_ms;
                    // stream header bytes (level sum over the first min(n, 12))
                    const uint32_t seqf = (uint32_t)(uint16_t)(s.seq + f), tsf = s.ts + f * n;
                    const uint32_t h0 = 0x80u | (mk << 15 | pt7 << 8) | (seqf >> 8) << 16 | (seqf & 0xFFu) << 24;
                    const uint32_t h1 = bswap32(tsf), h2 = bswap32(s.ssrc);
                    const int hsum = sbyte_sum(h0, min(n, 4u)) + sbyte_sum(h1, n > 4u ? min(n - 4u, 4u) : 0u) + sbyte_sum(h2, n > 8u ? min(n - 8u, 4u) : 0u);
                    // :675-679 Idle-in zeroing
                    if ((s.calltype & IGDSP_TX_CT_IDLE) && s.call_in) { s.sql = 0; s.ptt = 0; }
                    // :680-706 gate / keep-alive clock
                    const bool gate = (s.ptt && !s.call_in) || (s.sql && s.call_in);
                    bool sent = true;
                    if (gate) glast = (int32_t)f;
                    else {
                        const uint64_t diff = now - s.r2s_send_ms, per = (uint64_t)(int64_t)s.keepalive_ms;
                        if (diff < per && !s.first_r2s) sent = false;
                        else if (diff >= per) s.r2s_send_ms = now;
                    }
                    uint32_t meta = kMValid, word = 0;
                    if (sent) {
                        // :712-796 header
                        const uint32_t m = (s.first_r2s && s.packet_cnt == 0) ? 1u : 0u;
                        const bool steady = s.tx_slave == s.tx_slave_changed && s.rx_slave == s.rx_slave_changed && s.slave_count >= 5;
                        if (!steady) {
                            s.tx_slave = s.tx_slave_changed; s.rx_slave = s.rx_slave_changed;
                            s.slave_count = min(s.slave_count + 1, 5);
                        }
                        const uint32_t rx = s.rx_slave, tx = s.tx_slave;
                        word = (rx == 0 && tx == 0) ? (steady ? 0u : 0x13100u) : (rx == 1 && tx == 1) ? 0x131c0u
                             : (rx == 1 && tx == 0) ? 0x13140u : (rx == 0 && tx == 1) ? 0x13180u : 0u;
                        if (s.sql) word |= 0x10000000u | (((uint32_t)s.bssi << 3) & 0xf8u);   // sqlpriority = 0 -> 0 at bit 22
                        else if (!s.ptt) word |= 1u << 22;
                        if (s.ptt) word |= (((uint32_t)s.pttid << 22) & 0x0fc00000u) | (((uint32_t)s.pttpriority << 29) & 0xe0000000u);
                        uint32_t opt = pt7;
                        const bool ct_rx = s.calltype & IGDSP_TX_CT_RX, ct_tx = s.calltype & IGDSP_TX_CT_TX;
                        if (ct_rx && !s.call_in) opt = IGDSP_PT_R2S;
                        // :804-839 size / PT ladder
                        bool full;
                        if (!s.ptt && !s.sql) full = false;
                        else if (ct_rx && !s.sql) full = false;
                        else if (ct_tx && s.ptt && s.call_in) full = s.call_recorder || s.sql;
                        else full = true;
                        if (!full) opt = IGDSP_PT_R2S;
                        // :849-856 counters
                        if (s.first_r2s && s.packet_cnt < 30) s.packet_cnt += 1;
                        else if (s.packet_cnt >= 30) s.first_r2s = 0;
                        uint32_t fl8 = IGDSP_TX_SENT | (m ? IGDSP_TX_MARKER : 0u) | (opt == IGDSP_PT_R2S ? IGDSP_TX_KEEPALIVE_PT : 0u);
                        if (full && !gate) fl8 |= IGDSP_TX_STALE_PAYLOAD;
                        if (opt != IGDSP_PT_R2S) fl8 |= IGDSP_TX_LEVEL_VALID;
                        meta |= (full ? kMSizeFull : kMSize20) | (m << 15 | opt << 8) | fl8 << 16;
                        rs[p] = full && !gate ? glast : (int32_t)f;
                    }
                    rw[p] = word;
                    rm[p] = meta;
                    rl[p] = hsum;
                }
            }
            wave_sync();
            // ---- bulk: every lane, packet dwords, kTxU iterations per step.  The loads of a step do not sit behind branches: every
            // iteration loads its frame's dword, its payload source's dword and its send-buffer dword from addresses that are always
            // valid (a header dword or an unneeded source reads a neighbour of the frame's own bytes), so the kTxU x 3 loads of a step
            // are in flight together; what is done with them is decided afterwards.
            {
                const uint32_t total = (uint32_t)kTxPk * D;
                uint32_t p = lane / D, o = lane % D;
                for (uint32_t i0 = lane; i0 < total; i0 += 64u * kTxU) {
                    uint32_t pu[kTxU], ou[kTxU], mu[kTxU];
                    uint2 vc[kTxU], vs[kTxU];
                    uint32_t vl[kTxU];
#pragma unroll
                    for (int u = 0; u < kTxU; ++u) {
                        const bool in = i0 + 64u * u < total;
                        const uint32_t pc = in ? p : 0u;
                        const uint32_t meta = rm[pc];
                        pu[u] = pc; ou[u] = o; mu[u] = in ? meta : 0u;
                        const uint32_t ch = pc % kTxCh, f = min(f0 + pc / kTxCh, F - 1u), cc = min(c0 + ch, C - 1u);
                        const uint32_t q = o >= 5u ? o - 5u : 0u;
                        const int32_t src = rs[pc];
                        const uint32_t sf = ((meta & 3u) == kMSizeFull && src >= 0 && (uint32_t)src < F) ? (uint32_t)src : f;
                        if (a.vec) {
                            vc[u] = raw_load<FORM>(a, (uint64_t)f * C + cc, q);
                            vs[u] = raw_load<FORM>(a, (uint64_t)sf * C + cc, q);
                            vl[u] = *reinterpret_cast<const uint32_t *>(a.last + (uint64_t)cc * n + 4u * q);
                        }
                        p += q64; o += r64;
                        if (o >= D) { o -= D; p += 1u; }
                    }
#pragma unroll
                    for (int u = 0; u < kTxU; ++u) {
                        const uint32_t meta = mu[u];
                        if (!(meta & kMValid)) continue;
                        const uint32_t pp = pu[u], oo = ou[u], ch = pp % kTxCh, f = f0 + pp / kTxCh, cc = c0 + ch;
                        const uint32_t szc = meta & 3u, fl8 = (meta >> 16) & 0xFFu;
                        const uint64_t row = (uint64_t)f * C + cc;
                        uint8_t *dst = a.packets + row * a.stride + 4u * oo;
                        if (oo < 5u) {
                            if (szc) {
                                uint32_t d;
                                if (oo == 0u) { const uint32_t sq = (uint16_t)(c_seq[w][ch] + f); d = 0x90u | (meta & 0xFF00u) | (sq >> 8) << 16 | (sq & 0xFFu) << 24; }
                                else if (oo == 1u) d = bswap32(c_ts[w][ch] + f * n);
                                else if (oo == 2u) d = bswap32(c_ssrc[w][ch]);
                                else if (oo == 3u) d = 0x01006701u;
                                else d = bswap32(rw[pp]);
                                *reinterpret_cast<uint32_t *>(dst) = d;
                            }
                            continue;
                        }
                        const uint32_t q = oo - 5u, law = c_law[w][ch], k = min(n - 4u * q, 4u);
                        const bool lvl = (fl8 & IGDSP_TX_LEVEL_VALID) && n > 12u && 4u * q < n - 12u;
                        const bool prb = n > 48u && (q == 7u || q == 9u || q == 12u);
                        const bool full = szc == kMSizeFull;
                        const int32_t src = full ? rs[pp] : (int32_t)f;
                        const bool own = full && src == (int32_t)f;
                        if (lvl || prb || own) {
                            const uint32_t d = a.vec ? encode_raw<FORM, VARIANT>(vc[u], law, tab) : frame_dword<FORM, VARIANT>(a, row, q, law, tab);
                            if (own) put_dword(dst, d, k);
                            if (lvl) atomicAdd(&rl[pp], sbyte_sum(d, min(n - 12u - 4u * q, 4u)));
                            if (prb) {
                                const uint32_t bt = (d >> (q == 9u ? 16u : 0u)) & 0xFFu;
                                if (bt != 0xD5u) atomicOr(&rm[pp], kMProbeFail);
                            }
                        }
                        if (full && !own) {
                            uint32_t d;
                            if (src >= 0) d = a.vec ? encode_raw<FORM, VARIANT>(vs[u], law, tab) : frame_dword<FORM, VARIANT>(a, (uint64_t)src * C + cc, q, law, tab);
                            else d = a.vec ? vl[u] : last_dword(a, cc, q);
                            put_dword(dst, d, k);
                        }
                    }
                }
            }
            wave_sync();
            // ---- close: records out, silence run, level ----
            if (dl) {
                for (uint32_t fl = 0; fl < (uint32_t)kTxFc; ++fl) {
                    const uint32_t f = f0 + fl, p = fl * kTxCh + lane;
                    if (f >= F) break;
                    const uint32_t meta = rm[p], szc = meta & 3u, fl8 = (meta >> 16) & 0xFFu;
                    if (n > 48u) s.tx_run = (meta & kMProbeFail) ? 0 : (int32_t)(int16_t)(s.tx_run + 1);
                    uint32_t lv = 0;
                    if (fl8 & IGDSP_TX_LEVEL_VALID) { lv = (uint32_t)(uint8_t)(rl[p] / (int)n); s.level = lv; }
                    const uint16_t size = (uint16_t)(szc == kMSizeFull ? 20u + n : szc == kMSize20 ? 20u : 0u);
                    const uint64_t row = (uint64_t)f * C + c;
                    a.sizes[row] = size;
                    igdsp_tx_info inf;
                    inf.ed137 = rw[p]; inf.size = size; inf.flags = (uint8_t)fl8; inf.level = (uint8_t)lv;
                    a.info[row] = inf;
                }
            }
            wave_sync();
        }
        // ---- end of launch: state and the send buffer ----
        if (dl) {
            s.seq = (uint16_t)(s.seq + F);
            s.ts += F * n;
            s.store(a.state + c);
            r_src[w][lane] = glast;                                  // (records are dead here) the frame each send buffer takes
        }
        wave_sync();
        const uint32_t nq = (n + 3u) / 4u;
        for (uint32_t i = lane; i < (uint32_t)kTxCh * nq; i += 64u) {
            const uint32_t ch = i / nq, q = i % nq, cc = c0 + ch;
            const int32_t src = r_src[w][ch];
            if (cc >= C || src < 0) continue;
            const uint32_t d = frame_dword<FORM, VARIANT>(a, (uint64_t)src * C + cc, q, c_law[w][ch], tab);
            put_dword(a.last + (uint64_t)cc * n + 4u * q, d, min(n - 4u * q, 4u));
        }
        wave_sync();
    }
}

// A/B yardstick (igdsp_internal_tx_copy, tools/tx_bench.py --ab): the same wave / channel-group / frame-chunk traversal and the same
// bytes moved as an all-audio k_tx_packetize launch — every packet 20 + n bytes, its payload read from the frame's input — with no
// decision pass, no LDS, no encoder (PCM: the low byte of each sample is stored) and no records.  Needs n % 4 == 0.
template <int FORM>
__global__ __launch_bounds__(kTxWaves * 64) void k_tx_copy_ab(const TxArgs a)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t n = a.n, C = a.C, F = a.F;
    const uint32_t D = 5u + n / 4u, q64 = 64u / D, r64 = 64u % D, total = (uint32_t)kTxPk * D;
    for (uint32_t g = blockIdx.x * kTxWaves + w; g < a.n_groups; g += gridDim.x * kTxWaves) {
        const uint32_t c0 = g * kTxCh;
        for (uint32_t f0 = 0; f0 < F; f0 += kTxFc) {
            uint32_t p = lane / D, o = lane % D;
            for (uint32_t i0 = lane; i0 < total; i0 += 64u * kTxU) {
                uint32_t pu[kTxU], ou[kTxU];
                uint2 v[kTxU];
#pragma unroll
                for (int u = 0; u < kTxU; ++u) {
                    pu[u] = i0 + 64u * u < total ? p : ~0u; ou[u] = o;
                    const uint32_t pc = pu[u] == ~0u ? 0u : p;
                    const uint32_t f = min(f0 + pc / kTxCh, F - 1u), cc = min(c0 + pc % kTxCh, C - 1u);
                    v[u] = raw_load<FORM>(a, (uint64_t)f * C + cc, o >= 5u ? o - 5u : 0u);
                    p += q64; o += r64;
                    if (o >= D) { o -= D; p += 1u; }
                }
#pragma unroll
                for (int u = 0; u < kTxU; ++u) {
                    const uint32_t pp = pu[u];
                    if (pp == ~0u) continue;
                    const uint32_t f = f0 + pp / kTxCh, cc = c0 + pp % kTxCh;
                    if (f >= F || cc >= C) continue;
                    const uint64_t row = (uint64_t)f * C + cc;
                    uint32_t d = FORM == kTxG711 ? v[u].x
                                                 : (v[u].x & 0xFFu) | ((v[u].x >> 16) & 0xFFu) << 8 | (v[u].y & 0xFFu) << 16 | (v[u].y >> 16) << 24;
                    if (ou[u] < 5u) d = (uint32_t)row * 0x9E3779B9u + ou[u];
                    *reinterpret_cast<uint32_t *>(a.packets + row * a.stride + 4u * ou[u]) = d;
                }
            }
        }
    }
}

// The 128 KiB of dynamic LDS the table form asks for exceeds the default limit.  Raised on the first large PCM launch on each device
// (igdsp_create does not depend on it); if that fails the launch takes the enc_uni form instead — same bytes, slower.
static bool tab_lds_ready()
{
    static std::atomic<int> state[64];                   // per device: 0 unknown, 1 raised, 2 refused
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    int st = state[dev].load(std::memory_order_acquire);
    if (st == 0) {
        bool ok = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_tx_packetize<kTxPcmTab, IGDSP_ENC_G191>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 65536) == hipSuccess &&
                  hipFuncSetAttribute(reinterpret_cast<const void *>(&k_tx_packetize<kTxPcmTab, IGDSP_ENC_SUN16>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 65536) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        st = ok ? 1 : 2;
        state[dev].store(st, std::memory_order_release);
    }
    return st == 1;
}

// The grid is tx_route's for the same arguments (the table form included), so the yardstick runs the blocks of the launch it is compared with
hipError_t launch_tx_copy_ab(const LaunchCfg &cfg, const int16_t *pcm, const uint8_t *g711, uint32_t C, uint32_t F, uint32_t n,
                             uint8_t *packets, uint32_t stride, hipStream_t s)
{
    const bool tab_lds = tx_wants_table(pcm != nullptr, C, F, n) && tab_lds_ready();
    const TxRoute r = tx_copy_route(C, F, n, reinterpret_cast<uintptr_t>(pcm), reinterpret_cast<uintptr_t>(g711), (uint32_t)cfg.compute_units, tab_lds);
    TxArgs a{pcm, g711, nullptr, C, F, n, 0, 0, nullptr, nullptr, packets, stride, nullptr, nullptr, nullptr, r.n_groups, 1u};
    if (pcm) hipLaunchKernelGGL((k_tx_copy_ab<kTxPcmTab>), dim3(r.grid), dim3(r.threads), 0, s, a);
    else     hipLaunchKernelGGL((k_tx_copy_ab<kTxG711>), dim3(r.grid), dim3(r.threads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tx_packetize(const LaunchCfg &cfg, const int16_t *pcm, const uint8_t *g711, const uint8_t *ctl, uint32_t C, uint32_t F,
                               uint32_t n, uint64_t t0, uint32_t frame_ms, igdsp_tx_chan *state, uint8_t *last, uint8_t *packets,
                               uint32_t stride, uint16_t *sizes, igdsp_tx_info *info, int variant, hipStream_t s)
{
    const bool tab_lds = tx_wants_table(pcm != nullptr, C, F, n) && tab_lds_ready();
    const TxRoute r = tx_route(C, F, n, reinterpret_cast<uintptr_t>(pcm), reinterpret_cast<uintptr_t>(g711), reinterpret_cast<uintptr_t>(last),
                               (uint32_t)cfg.compute_units, tab_lds);
    const TxArgs a{pcm, g711, ctl, C, F, n, t0, frame_ms, state, last, packets, stride, sizes, info, cfg.enc_tab, r.n_groups, r.vec};
    const dim3 g(r.grid), b(r.threads);
    switch (r.form) {
    case kTxG711: hipLaunchKernelGGL((k_tx_packetize<kTxG711, IGDSP_ENC_G191>), g, b, r.lds, s, a); break;   // (no encoder: one lineage)
    case kTxPcm: with_enc(variant, [&](auto V) { hipLaunchKernelGGL((k_tx_packetize<kTxPcm, V>), g, b, r.lds, s, a); }); break;
    case kTxPcmTab: with_enc(variant, [&](auto V) { hipLaunchKernelGGL((k_tx_packetize<kTxPcmTab, V>), g, b, r.lds, s, a); }); break;
    }
    return hipGetLastError();
}

}  // namespace igdsp
