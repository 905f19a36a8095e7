// igdsp_capi_tx.hip — the staged ED-137 send path of include/igdsp.h (transport_send_rtp as pjmedia calls it,
// TransportAdapter.cpp:635-874): everything igdsp_tx_open creates on first use, the igdsp_tx_* entries over it and the two
// measurement helpers that need its insides.  The staging itself is host-only code in igdsp_txstage.h.
#include "igdsp_ctx.h"
#include "igdsp_txstage.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

using namespace igdsp;

// ---- the staged ED-137 send path: everything igdsp_tx_open creates on first use ----
struct igdsp_ctx::TxSide {
    igdsp_tx::Stager st;                                // per-leg rings + setter words (csrc/igdsp_txstage.h)
    hipStream_t stream = nullptr;                       // its own stream: a TX flush never waits behind an RX flush, nor the reverse
    hipEvent_t ev[4] = {};                              // igdsp_internal_tx_timing: around the upload, the kernel and the download
    igdsp_tx_chan *d_state = nullptr;                   // [legs]
    uint8_t *d_buf = nullptr;                           // [legs][236]: send_pkt_buff + 20
    uint8_t *h_up = nullptr, *d_up = nullptr, *h_out = nullptr, *d_out = nullptr;   // grown on demand, never shared with RX
    size_t up_cap = 0, out_cap = 0;
    std::vector<igdsp_tx_chan> chan;                    // per leg, as of the last finished flush
    std::vector<int32_t> call_of;                       // per leg: the call that opened it
    std::vector<igdsp_tx_packet> results;               // the last flush's packets
    std::unique_ptr<SnapshotPool> pool;                 // the snapshot's helpers, sized as the RX flush's (igdsp_snappool.h)
    bool timing = false;
    float t_ms[5] = {};                                 // last flush: snapshot, upload, kernel, download, whole call
    std::mutex mu;                                      // owner entries: open / close / flush / results / get_chan

    ~TxSide()
    {
        pool.reset();
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        for (void *p : {(void *)h_up, (void *)h_out}) if (p) (void)hipHostFree(p);
        for (void *p : {(void *)d_state, (void *)d_buf, (void *)d_up, (void *)d_out}) if (p) (void)hipFree(p);
    }
};

namespace {
// A pinned block and its device mirror of at least `need` bytes (grown by doubling; the contents are not kept).
hipError_t tx_reserve(igdsp_ctx::TxSide *tx, uint8_t **h, uint8_t **d, size_t *cap, size_t need)
{
    if (need <= *cap) return hipSuccess;
    const size_t want = std::max(need, 2 * *cap);
    hipError_t e = hipStreamSynchronize(tx->stream);
    if (*h) { (void)hipHostFree(*h); *h = nullptr; }
    if (*d) { (void)hipFree(*d); *d = nullptr; }
    *cap = 0;
    if (e == hipSuccess) e = hipHostMalloc((void **)h, want, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void **)d, want);
    if (e == hipSuccess) *cap = want;
    return e;
}

igdsp_ctx::TxSide *tx_side(igdsp_ctx *ctx, int *rc)
{
    if (igdsp_ctx::TxSide *tx = ctx->tx.load(std::memory_order_acquire)) return tx;
    std::lock_guard<std::mutex> g(ctx->tx_init_mu);
    if (igdsp_ctx::TxSide *tx = ctx->tx.load(std::memory_order_acquire)) return tx;
    auto *tx = new (std::nothrow) igdsp_ctx::TxSide();
    const uint32_t legs = ctx->max_channels;
    bool ok = tx && tx->st.init(legs);
    if (ok) {
        tx->chan.assign(legs, igdsp_tx_chan{});
        tx->call_of.assign(legs, -1);
    }
    ok = ok && hipSetDevice(ctx->device) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&tx->stream, hipStreamNonBlocking) == hipSuccess;
    if (ok) for (hipEvent_t &e : tx->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    ok = ok && hipMalloc((void **)&tx->d_state, (size_t)legs * sizeof(igdsp_tx_chan)) == hipSuccess;
    ok = ok && hipMalloc((void **)&tx->d_buf, (size_t)legs * igdsp_tx::kTxMaxN) == hipSuccess;
    ok = ok && hipMemset(tx->d_buf, 0, (size_t)legs * igdsp_tx::kTxMaxN) == hipSuccess;
    if (!ok) {
        delete tx;
        *rc = IGDSP_ENOMEM;
        return nullptr;
    }
    tx->pool = make_pool(legs);
    ctx->tx.store(tx, std::memory_order_release);
    return tx;
}
}  // namespace

void igdsp_tx_drop(igdsp_ctx *ctx) { delete ctx->tx.exchange(nullptr); }

extern "C" {

// ---- staged ED-137 send path (transport_send_rtp as pjmedia calls it, TransportAdapter.cpp:635-874) ----
// the TX side and channel of call_id (whether or not a leg is open there), or nullptr with *rc set
static igdsp_ctx::TxSide *tx_chan_of(igdsp_ctx *ctx, int32_t call_id, uint32_t *leg, int *rc)
{
    *rc = IGDSP_ENOENT;
    const uint32_t ch = lookup(ctx, call_id);
    if (ch == kNoChan) return nullptr;
    igdsp_ctx::TxSide *tx = ctx->tx.load(std::memory_order_acquire);
    if (!tx) return nullptr;
    *leg = ch;
    *rc = IGDSP_OK;
    return tx;
}

static int tx_set(igdsp_ctx *ctx, int32_t call_id, uint64_t dirty, uint64_t values)
{
    if (!ctx) return IGDSP_EINVAL;
    uint32_t leg = 0;
    int rc;
    igdsp_ctx::TxSide *tx = tx_chan_of(ctx, call_id, &leg, &rc);
    return tx ? tx->st.set(leg, dirty, values) : rc;
}

int igdsp_tx_open(igdsp_ctx *ctx, int32_t call_id, const char *calltype, int call_in, int32_t keepalive_ms, uint64_t now_ms)
{
    if (!ctx || !calltype) return IGDSP_EINVAL;
    const uint32_t leg = lookup(ctx, call_id);
    if (leg == kNoChan) return IGDSP_ENOENT;
    int rc = IGDSP_OK;
    igdsp_ctx::TxSide *tx = tx_side(ctx, &rc);
    if (!tx) return fail(ctx, rc, "igdsp_tx_open: TX staging / device state");
    std::lock_guard<std::mutex> g(tx->mu);
    igdsp_tx_chan h;
    (void)igdsp_tx_chan_init(&h, calltype, call_in, 0, 0, 0, 0, keepalive_ms, now_ms);   // the stream's fields come with each packet
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(tx->d_state + leg, &h, sizeof h, hipMemcpyHostToDevice, tx->stream));
    HIP_TRY(ctx, hipMemsetAsync(tx->d_buf + (size_t)leg * igdsp_tx::kTxMaxN, 0, igdsp_tx::kTxMaxN, tx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(tx->stream));
    tx->chan[leg] = h;
    tx->call_of[leg] = call_id;
    tx->st.open(leg);
    return IGDSP_OK;
}

int igdsp_tx_close(igdsp_ctx *ctx, int32_t call_id)
{
    if (!ctx) return IGDSP_EINVAL;
    uint32_t leg = 0;
    int rc;
    igdsp_ctx::TxSide *tx = tx_chan_of(ctx, call_id, &leg, &rc);
    if (!tx) return rc;
    std::lock_guard<std::mutex> g(tx->mu);
    if (!tx->st.is_open(leg)) return IGDSP_ENOENT;
    tx->st.close(leg);
    return IGDSP_OK;
}

int igdsp_tx_set_ptt(igdsp_ctx *ctx, int32_t call_id, int ptt, int priority, int user_rec)
{
    using namespace igdsp_tx;
    return tx_set(ctx, call_id, kSdPtt | kSdRec,
                  (ptt ? kSwPtt : 0u) | (uint64_t)(priority & 0xFF) << kSwPrioShift | (user_rec ? kSwRec : 0u));
}

int igdsp_tx_set_sql(igdsp_ctx *ctx, int32_t call_id, int sql, int priority, int32_t bssi)
{
    using namespace igdsp_tx;
    (void)priority;                                      // sqlpriority is zeroed before every use (:739)
    return tx_set(ctx, call_id, kSdSql | (bssi >= 0 ? kSdBssi : 0u), (sql ? kSwSql : 0u) | (uint64_t)(bssi & 0xFF) << kSwBssiShift);
}

int igdsp_tx_set_ptt_id(igdsp_ctx *ctx, int32_t call_id, int pttid)
{
    return tx_set(ctx, call_id, igdsp_tx::kSdPttId, (uint64_t)(pttid & 0xFF) << igdsp_tx::kSwPttIdShift);
}

int igdsp_tx_set_slave(igdsp_ctx *ctx, int32_t call_id, int rx, int tx)
{
    using namespace igdsp_tx;
    return tx_set(ctx, call_id, kSdSlave, (rx ? kSwSlaveRx : 0u) | (tx ? kSwSlaveTx : 0u));
}

int igdsp_tx_set_recorder(igdsp_ctx *ctx, int32_t call_id, int on)
{
    return tx_set(ctx, call_id, igdsp_tx::kSdRec, on ? igdsp_tx::kSwRec : 0u);
}

int igdsp_tx_set_calltype(igdsp_ctx *ctx, int32_t call_id, const char *calltype)
{
    if (!calltype) return IGDSP_EINVAL;
    return tx_set(ctx, call_id, igdsp_tx::kSdCt, (uint64_t)igdsp_tx_calltype_bits(calltype) << igdsp_tx::kSwCtShift);
}

int igdsp_on_tx_frame(igdsp_ctx *ctx, int32_t call_id, const void *pkt, uint32_t size, uint64_t now_ms)
{
    if (!ctx) return IGDSP_EINVAL;
    if (!igdsp_tx::stream_packet_ok(static_cast<const uint8_t *>(pkt), size)) return IGDSP_EINVAL;
    uint32_t leg = 0;
    int rc;
    igdsp_ctx::TxSide *tx = tx_chan_of(ctx, call_id, &leg, &rc);
    return tx ? tx->st.stage(leg, static_cast<const uint8_t *>(pkt), size, now_ms) : rc;
}

int igdsp_tx_flush(igdsp_ctx *ctx, uint32_t *n_frames_out)
{
    if (!ctx) return IGDSP_EINVAL;
    if (n_frames_out) *n_frames_out = 0;
    igdsp_ctx::TxSide *tx = ctx->tx.load(std::memory_order_acquire);
    if (!tx) return IGDSP_OK;                            // no leg was ever opened
    std::lock_guard<std::mutex> g(tx->mu);
    const auto t0 = std::chrono::steady_clock::now();
    tx->results.clear();
    // 1. snapshot: count, then emit each part's legs at its offsets (a pool of helpers at many legs, as the RX flush)
    using igdsp_tx::Stager;
    const uint32_t legs = tx->st.legs();
    Stager::Counts cnt[kMaxParts], base[kMaxParts];
    const uint32_t n_parts = for_each_part(tx->pool.get(), legs, [&](uint32_t i, uint32_t l0, uint32_t l1) { cnt[i] = tx->st.count(l0, l1); });
    Stager::Counts tot;
    for (uint32_t i = 0; i < n_parts; ++i) {
        base[i] = tot;
        tot.runs += cnt[i].runs; tot.frames += cnt[i].frames; tot.dwords += cnt[i].dwords;
    }
    if (tot.frames == 0) return IGDSP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const igdsp_tx::TxUploadLayout L = igdsp_tx::upload_layout(tot.runs, tot.frames, tot.dwords);
    const igdsp_tx::TxOutLayout O = igdsp_tx::out_layout(tot.runs, tot.frames);
    if (hipError_t e = tx_reserve(tx, &tx->h_up, &tx->d_up, &tx->up_cap, L.total)) {   // before emit: a failure leaves the frames staged
        return fail(ctx, e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation ? IGDSP_ENOMEM : IGDSP_EDEVICE, "igdsp_tx_flush: upload block", e);
    }
    if (hipError_t e = tx_reserve(tx, &tx->h_out, &tx->d_out, &tx->out_cap, O.total))
        return fail(ctx, e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation ? IGDSP_ENOMEM : IGDSP_EDEVICE, "igdsp_tx_flush: result block", e);
    for_each_part(tx->pool.get(), legs, [&](uint32_t i, uint32_t l0, uint32_t l1) { tx->st.emit(l0, l1, tx->h_up, L, base[i]); });
    const auto t1 = std::chrono::steady_clock::now();
    // 2. upload, packetise, download, on the TX stream
    hipStream_t s = tx->stream;
    uint8_t *d = tx->d_up, *o = tx->d_out;
    if (tx->timing) HIP_TRY(ctx, hipEventRecord(tx->ev[0], s));
    HIP_TRY(ctx, hipMemcpyAsync(d, tx->h_up, L.total, hipMemcpyHostToDevice, s));
    if (tx->timing) HIP_TRY(ctx, hipEventRecord(tx->ev[1], s));
    HIP_TRY(ctx, launch_tx_staged(igdsp::LaunchCfg{ctx->cus, nullptr}, d + L.runs, d + L.recs, reinterpret_cast<const uint32_t *>(d + L.bytes), tot.runs,
                                  tx->d_state, tx->d_buf, reinterpret_cast<igdsp_tx_info *>(o + O.info), reinterpret_cast<igdsp_tx_chan *>(o + O.chan),
                                  reinterpret_cast<uint32_t *>(o + O.pkts), s));
    if (tx->timing) HIP_TRY(ctx, hipEventRecord(tx->ev[2], s));
    HIP_TRY(ctx, hipMemcpyAsync(tx->h_out, o, O.total, hipMemcpyDeviceToHost, s));
    if (tx->timing) HIP_TRY(ctx, hipEventRecord(tx->ev[3], s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    // 3. publish: one entry per frame, legs in channel order, frames in staging order
    const auto *runs = reinterpret_cast<const igdsp_tx::TxRun *>(tx->h_up + L.runs);
    const auto *info = reinterpret_cast<const igdsp_tx_info *>(tx->h_out + O.info);
    const auto *chan = reinterpret_cast<const igdsp_tx_chan *>(tx->h_out + O.chan);
    tx->results.resize(tot.frames);
    for (uint32_t r = 0; r < tot.runs; ++r) {
        const igdsp_tx::TxRun &run = runs[r];
        tx->chan[run.leg] = chan[r];
        for (uint32_t k = 0; k < run.count; ++k) {
            const uint32_t f = run.first + k;
            const igdsp_tx_info &in = info[f];
            tx->results[f] = igdsp_tx_packet{tx->h_out + O.pkts + (size_t)f * igdsp_tx::kTxSlot, tx->call_of[run.leg], in.ed137, in.size, in.flags, in.level};
        }
    }
    if (tx->timing) {
        const auto t2 = std::chrono::steady_clock::now();
        tx->t_ms[0] = std::chrono::duration<float, std::milli>(t1 - t0).count();
        for (int i = 0; i < 3; ++i) HIP_TRY(ctx, hipEventElapsedTime(&tx->t_ms[1 + i], tx->ev[i], tx->ev[i + 1]));
        tx->t_ms[4] = std::chrono::duration<float, std::milli>(t2 - t0).count();
    }
    if (n_frames_out) *n_frames_out = tot.frames;
    return IGDSP_OK;
}

int igdsp_tx_results(igdsp_ctx *ctx, const igdsp_tx_packet **out, uint32_t *n_out)
{
    if (!ctx || !out || !n_out) return IGDSP_EINVAL;
    *out = nullptr;
    *n_out = 0;
    igdsp_ctx::TxSide *tx = ctx->tx.load(std::memory_order_acquire);
    if (!tx) return IGDSP_OK;
    std::lock_guard<std::mutex> g(tx->mu);
    *out = tx->results.data();
    *n_out = (uint32_t)tx->results.size();
    return IGDSP_OK;
}

int igdsp_tx_get_chan(igdsp_ctx *ctx, int32_t call_id, igdsp_tx_chan *out)
{
    if (!ctx || !out) return IGDSP_EINVAL;
    uint32_t leg = 0;
    int rc;
    igdsp_ctx::TxSide *tx = tx_chan_of(ctx, call_id, &leg, &rc);
    if (!tx) return rc;
    std::lock_guard<std::mutex> g(tx->mu);
    if (!tx->st.is_open(leg)) return IGDSP_ENOENT;
    *out = tx->chan[leg];
    return IGDSP_OK;
}

int igdsp_tx_counts(igdsp_ctx *ctx, int32_t call_id, uint32_t *refused, uint32_t *dropped)
{
    if (!ctx) return IGDSP_EINVAL;
    uint32_t leg = 0;
    int rc;
    igdsp_ctx::TxSide *tx = tx_chan_of(ctx, call_id, &leg, &rc);
    if (!tx) return rc;
    if (refused) *refused = tx->st.refused(leg);
    if (dropped) *dropped = tx->st.dropped(leg);
    return IGDSP_OK;
}

// Measurement helper (not in include/igdsp.h, tools/tx_stage_bench.py): what the media threads do in one bridge tick, in one native
// loop — `frames_per_call` igdsp_on_tx_frame calls for each of the calls first_call .. first_call + n_calls - 1, frame f of call k
// taken from pkts[(f * n_calls + k) % n_pkts][size] at now_ms + f * frame_ms.  Returns the number of calls that did not return IGDSP_OK.
int igdsp_internal_tx_stage_many(igdsp_ctx *ctx, int32_t first_call, uint32_t n_calls, uint32_t frames_per_call, const uint8_t *pkts,
                                 uint32_t n_pkts, uint32_t size, uint64_t now_ms, uint32_t frame_ms)
{
    if (!ctx || !pkts || n_pkts == 0) return IGDSP_EINVAL;
    int bad = 0;
    for (uint32_t f = 0; f < frames_per_call; ++f)
        for (uint32_t k = 0; k < n_calls; ++k)
            if (igdsp_on_tx_frame(ctx, first_call + (int32_t)k, pkts + (size_t)((f * n_calls + k) % n_pkts) * size, size, now_ms + (uint64_t)f * frame_ms) != IGDSP_OK)
                ++bad;
    return bad;
}

// Measurement-only (not in include/igdsp.h, tools/tx_stage_bench.py): enable != 0 makes every igdsp_tx_flush time its phases; out[5]
// (optional) receives the last flush's snapshot (host clock), upload, kernel, download (HIP events) and whole-call times in ms.
int igdsp_internal_tx_timing(igdsp_ctx *ctx, int enable, float *out)
{
    if (!ctx) return IGDSP_EINVAL;
    igdsp_ctx::TxSide *tx = ctx->tx.load(std::memory_order_acquire);
    if (!tx) return IGDSP_ENOENT;
    std::lock_guard<std::mutex> g(tx->mu);
    tx->timing = enable != 0;
    if (out) std::memcpy(out, tx->t_ms, sizeof tx->t_ms);
    return IGDSP_OK;
}

}  // extern "C"
