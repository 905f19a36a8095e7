// igdsp_k_txstage.hip — k_tx_staged: the device step of igdsp_tx_flush, the staged form of transport_send_rtp
// (TransportAdapter.cpp:635-874).  Semantics: include/igdsp.h, section "Staged ED-137 send path"; independent restatement:
// tests/tx_stage_model.py.
//
// Input is one compacted upload block (csrc/igdsp_txstage.h): runs of 1 .. IGDSP_STAGE_DEPTH frames per leg, each frame with its
// own now_ms, n, setter word and the 12 + n bytes of pjmedia's stream packet.  Shape:
//   decision  lanes 0 .. kTsLegs-1, one per run, state in registers, frames in staging order: setters, the stream header, Idle-in
//             zeroing, gate / keep-alive clock, ED-137 word with debounce, size / PT ladder, counters.  One record per frame in the
//             wave's LDS slice (slot = leg lane x depth + frame), plus the chain of the leg's gated frames.
//   bulk      the whole wave per frame: lane i reads stream dword i (header dwords 1, 2 go out as they are; the audioLevel sum and
//             the silence probe read the same registers), lane 5 + q writes payload dword q of the packet from the send buffer
//             as the gated frames of this flush have left it.  Dword stores up to size, bytes past size in the last dword are 0.
//   close     decision lanes: silence run, level, igdsp_tx_info, the leg state (in place and the run's copy for the host).
//   buffer    the whole wave per leg with a gated frame: the send buffer after the leg's last gated frame.
// A wave touches only its own legs' state, send buffers and LDS slice: no block barrier.
#include "igdsp_device.h"
#include "igdsp_txstage.h"

namespace igdsp {

using igdsp_tx::TxRec;
using igdsp_tx::TxRun;
constexpr uint32_t kTsDepth = igdsp_tx::kTxDepth;
constexpr uint32_t kTsRec = kTsLegs * kTsDepth;            // record slots per wave (128)
constexpr uint32_t kTsMaxN = igdsp_tx::kTxMaxN;
constexpr uint32_t kTsNone = 0xFFu;                         // no gated frame (slot index)
static_assert(igdsp_tx::kTxSlot == 64u * 4u, "one output slot = one dword per lane");

// record meta word: bits 0-1 size class, 8-15 byte 1 of the packet (m << 7 | pt), 16-23 IGDSP_TX_* flags
constexpr uint32_t kSmSize20 = 1u, kSmSizeFull = 2u, kSmProbeFail = 1u << 26;
// record aux word: n | src << 8 | prev << 16 — src: the newest gated slot at or before this frame (the send buffer's last writer),
// prev (gated frames only): the gated slot before this one

struct TxStagedArgs {
    const TxRun *runs;
    const TxRec *recs;
    const uint32_t *stream;
    uint32_t n_runs, n_groups;
    igdsp_tx_chan *state;
    uint8_t *buf;
    igdsp_tx_info *info;
    igdsp_tx_chan *chan_out;
    uint32_t *packets;
};

// Dword q of leg `leg`'s send buffer as left by gated slot g (kTsNone: as the flush found it): byte b comes from the newest gated
// frame at or before g whose n covers it (memcpy(send_pkt_buff + 20, payload, payloadlen), :683), else from the stored buffer.
__device__ __forceinline__ uint32_t send_dword(const TxStagedArgs &a, const uint32_t *aux, const uint32_t *sdw, uint32_t g, uint32_t leg, uint32_t q)
{
    if (g != kTsNone && (aux[g] & 0xFFu) >= 4u * q + 4u) return a.stream[sdw[g] + 3u + q];
    const uint8_t *old = a.buf + (size_t)leg * kTsMaxN;
    if (g == kTsNone) return *reinterpret_cast<const uint32_t *>(old + 4u * q);
    uint32_t d = 0;
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint32_t b = 4u * q + i;
        uint32_t x = old[b];
        for (uint32_t h = g; h != kTsNone; h = (aux[h] >> 16) & 0xFFu)
            if ((aux[h] & 0xFFu) > b) { x = (a.stream[sdw[h] + 3u + q] >> (8u * i)) & 0xFFu; break; }
        d |= x << (8u * i);
    }
    return d;
}

__global__ __launch_bounds__(kTsWaves * 64) void k_tx_staged(const TxStagedArgs a)
{
    __shared__ uint32_t r_meta[kTsWaves][kTsRec], r_word[kTsWaves][kTsRec], r_sdw[kTsWaves][kTsRec], r_aux[kTsWaves][kTsRec];
    __shared__ int32_t r_sum[kTsWaves][kTsRec];
    __shared__ uint32_t l_cnt[kTsWaves][kTsLegs], l_leg[kTsWaves][kTsLegs], l_first[kTsWaves][kTsLegs], l_gl[kTsWaves][kTsLegs], l_maxn[kTsWaves][kTsLegs];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t *rm = r_meta[w], *rw = r_word[w], *rs = r_sdw[w], *rx = r_aux[w];
    int32_t *rl = r_sum[w];

    for (uint32_t g = blockIdx.x * kTsWaves + w; g < a.n_groups; g += gridDim.x * kTsWaves) {
        // ---- decision: one lane per run ----
        const uint32_t ri = g * kTsLegs + lane;
        const bool dl = lane < (uint32_t)kTsLegs && ri < a.n_runs;
        TxRun run{0u, 0u, 0u, 0u};
        TxState s;
        uint32_t glast = kTsNone, maxn = 0;
        if (dl) {
            run = a.runs[ri];
            s.load(a.state + run.leg);
            uint32_t off = run.off_dw;
            for (uint32_t k = 0; k < run.count; ++k) {
                const uint32_t p = lane * kTsDepth + k;
                const TxRec rc = a.recs[run.first + k];
                const uint64_t wd = rc.word;
                const uint32_t n = (uint32_t)(wd >> igdsp_tx::kRecNShift) & 0xFFu;
                const uint32_t h0 = a.stream[off], h1 = a.stream[off + 1u], h2 = a.stream[off + 2u];
                // the setters that returned before this frame was staged (TransportAdapter.cpp:135-223)
                if (wd & igdsp_tx::kSdPtt) { s.ptt = (uint32_t)wd & 1u; s.pttpriority = (uint32_t)(wd >> igdsp_tx::kSwPrioShift) & 0xFFu; }
                if (wd & igdsp_tx::kSdRec) s.call_recorder = ((uint32_t)wd >> 2) & 1u;
                if (wd & igdsp_tx::kSdSql) s.sql = ((uint32_t)wd >> 1) & 1u;
                if (wd & igdsp_tx::kSdBssi) s.bssi = (uint32_t)(wd >> igdsp_tx::kSwBssiShift) & 0xFFu;
                if (wd & igdsp_tx::kSdPttId) s.pttid = (uint32_t)(wd >> igdsp_tx::kSwPttIdShift) & 0xFFu;
                if (wd & igdsp_tx::kSdSlave) { s.rx_slave_changed = ((uint32_t)wd >> 3) & 1u; s.tx_slave_changed = ((uint32_t)wd >> 4) & 1u; s.slave_count = 0; }
                if (wd & igdsp_tx::kSdCt) s.calltype = ((uint32_t)wd >> igdsp_tx::kSwCtShift) & 7u;
                // the stream packet's header: pt, seq, ts, ssrc as pjmedia wrote them
                const uint32_t pt7 = (h0 >> 8) & 0x7Fu;
                s.seq = ((((h0 >> 16) & 0xFFu) << 8 | h0 >> 24) + 1u) & 0xFFFFu;
                s.ts = bswap32(h1) + n;
                s.ssrc = bswap32(h2);
                s.pt = pt7;
                const uint64_t now = rc.now_ms;
                // :675-679 Idle-in zeroing
                if ((s.calltype & IGDSP_TX_CT_IDLE) && s.call_in) { s.sql = 0; s.ptt = 0; }
                // :680-706 gate / keep-alive clock
                const bool gate = (s.ptt && !s.call_in) || (s.sql && s.call_in);
                bool sent = true;
                uint32_t src = glast, prev = kTsNone;
                if (gate) { prev = glast; glast = src = p; maxn = max(maxn, n); }
                else {
                    const uint64_t diff = now - s.r2s_send_ms, per = (uint64_t)(int64_t)s.keepalive_ms;
                    if (diff < per && !s.first_r2s) sent = false;
                    else if (diff >= per) s.r2s_send_ms = now;
                }
                uint32_t meta = 0, word = 0;
                if (sent) {
                    // :712-796 header
                    const uint32_t m = (s.first_r2s && s.packet_cnt == 0) ? 1u : 0u;
                    const bool steady = s.tx_slave == s.tx_slave_changed && s.rx_slave == s.rx_slave_changed && s.slave_count >= 5;
                    if (!steady) {
                        s.tx_slave = s.tx_slave_changed; s.rx_slave = s.rx_slave_changed;
                        s.slave_count = min(s.slave_count + 1, 5);
                    }
                    const uint32_t rxe = s.rx_slave, txe = s.tx_slave;
                    word = (rxe == 0 && txe == 0) ? (steady ? 0u : 0x13100u) : (rxe == 1 && txe == 1) ? 0x131c0u
                         : (rxe == 1 && txe == 0) ? 0x13140u : (rxe == 0 && txe == 1) ? 0x13180u : 0u;
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
                    meta = (full ? kSmSizeFull : kSmSize20) | (m << 15 | opt << 8) | fl8 << 16;
                }
                rm[p] = meta;
                rw[p] = word;
                rs[p] = off;
                rx[p] = n | src << 8 | prev << 16;
                rl[p] = 0;
                off += igdsp_tx::stream_dwords(n);
            }
        }
        if (lane < (uint32_t)kTsLegs) {
            l_cnt[w][lane] = run.count; l_leg[w][lane] = run.leg; l_first[w][lane] = run.first;
            l_gl[w][lane] = glast; l_maxn[w][lane] = maxn;
        }
        wave_sync();
        // ---- bulk: the whole wave per frame ----
        for (uint32_t j = 0; j < (uint32_t)kTsLegs; ++j) {
            const uint32_t cnt = l_cnt[w][j], leg = l_leg[w][j], first = l_first[w][j];
            for (uint32_t k = 0; k < cnt; ++k) {
                const uint32_t p = j * kTsDepth + k, meta = rm[p], aux = rx[p], n = aux & 0xFFu, off = rs[p];
                const uint32_t d = lane < igdsp_tx::stream_dwords(n) ? a.stream[off + lane] : 0u;     // stream dword `lane`
                const uint32_t d2 = __shfl(d, (int)((lane + 62u) & 63u));                            // stream dword lane - 2
                // :657-673 silence probe on stream bytes 40, 50, 60
                if (12u + n > 60u) {
                    const bool bad = (lane == 10u && (d & 0xFFu) != 0xD5u) || (lane == 12u && ((d >> 16) & 0xFFu) != 0xD5u) ||
                                     (lane == 15u && (d & 0xFFu) != 0xD5u);
                    if (__ballot(bad) != 0u && lane == 0u) rm[p] = meta | kSmProbeFail;
                }
                const uint32_t fl8 = (meta >> 16) & 0xFFu, szc = meta & 3u;
                // roip_ed137.cpp:6510-6517 audioLevel: the first n stream bytes as signed char
                if (fl8 & IGDSP_TX_LEVEL_VALID) {
                    int v = 4u * lane < n ? sbyte_sum(d, min(n - 4u * lane, 4u)) : 0;
                    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
                    if (lane == 0u) rl[p] = v;
                }
                if (szc == 0u) continue;
                const uint32_t size = szc == kSmSizeFull ? 20u + n : 20u;
                if (lane >= (size + 3u) / 4u) continue;
                uint32_t v;
                if (lane == 0u) v = 0x90u | (meta & 0xFF00u) | (d & 0xFFFF0000u);                   // x = 1, m, pt; the stream's seq
                else if (lane < 3u) v = d;                                                          // ts, ssrc
                else if (lane == 3u) v = 0x01006701u;                                               // profile 0x0167, length 1
                else if (lane == 4u) v = bswap32(rw[p]);
                else {
                    const uint32_t q = lane - 5u, src = (aux >> 8) & 0xFFu;
                    v = src == p ? d2 : send_dword(a, rx, rs, src, leg, q);
                    if (4u * q + 4u > n) v &= 0xFFFFFFFFu >> (8u * (4u * q + 4u - n));
                }
                a.packets[(size_t)(first + k) * 64u + lane] = v;
            }
        }
        wave_sync();
        // ---- close: silence run, level, info, state ----
        if (dl) {
            for (uint32_t k = 0; k < run.count; ++k) {
                const uint32_t p = lane * kTsDepth + k, meta = rm[p], n = rx[p] & 0xFFu, szc = meta & 3u, fl8 = (meta >> 16) & 0xFFu;
                if (12u + n > 60u) s.tx_run = (meta & kSmProbeFail) ? 0 : (int32_t)(int16_t)(s.tx_run + 1);
                uint32_t lv = 0;
                if (fl8 & IGDSP_TX_LEVEL_VALID) { lv = (uint32_t)(uint8_t)(rl[p] / (int)n); s.level = lv; }
                igdsp_tx_info inf;
                inf.ed137 = rw[p];
                inf.size = (uint16_t)(szc == kSmSizeFull ? 20u + n : szc == kSmSize20 ? 20u : 0u);
                inf.flags = (uint8_t)fl8;
                inf.level = (uint8_t)lv;
                a.info[run.first + k] = inf;
            }
            s.store(a.state + run.leg);
            igdsp_tx_chan *o = a.chan_out + ri;
            s.store(o);
            *reinterpret_cast<uint4 *>(reinterpret_cast<uint8_t *>(o) + 48) = make_uint4(0u, 0u, 0u, 0u);
        }
        // ---- send buffers: as the leg's last gated frame leaves them (the bulk pass has read the old bytes) ----
        for (uint32_t j = 0; j < (uint32_t)kTsLegs; ++j) {
            const uint32_t gl = l_gl[w][j], leg = l_leg[w][j];
            if (gl == kTsNone) continue;
            const uint32_t nq = (l_maxn[w][j] + 3u) / 4u;
            const uint32_t v = lane < nq ? send_dword(a, rx, rs, gl, leg, lane) : 0u;
            if (lane < nq) *reinterpret_cast<uint32_t *>(a.buf + (size_t)leg * kTsMaxN + 4u * lane) = v;
        }
        wave_sync();
    }
}

hipError_t launch_tx_staged(const LaunchCfg &cfg, const void *runs, const void *recs, const uint32_t *stream, uint32_t n_runs,
                            igdsp_tx_chan *state, uint8_t *send_buf, igdsp_tx_info *info, igdsp_tx_chan *chan_out, uint32_t *packets,
                            hipStream_t s)
{
    if (n_runs == 0) return hipSuccess;
    const TxStagedRoute r = tx_staged_route(n_runs, (uint32_t)cfg.compute_units);
    const TxStagedArgs a{static_cast<const TxRun *>(runs), static_cast<const TxRec *>(recs), stream, n_runs, r.n_groups, state, send_buf, info,
                         chan_out, packets};
    hipLaunchKernelGGL(k_tx_staged, dim3(r.grid), dim3(r.threads), r.lds, s, a);
    return hipGetLastError();
}

}  // namespace igdsp
