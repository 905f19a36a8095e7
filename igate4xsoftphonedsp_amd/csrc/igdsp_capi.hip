// igdsp_capi.hip — the extern "C" boundary of include/igdsp.h over the gfx950
// kernels.  Host-side responsibilities only: context / stream / buffers, the
// single-frame staging slab behind setIncomingRTP/setOutgoingRTP
// (roip_ed137.cpp:6500-6587), call-id routing (roip_ed137.cpp:6519-6534) and
// argument validation.  There is NO CPU compute path here: when the HIP runtime
// or a gfx950 device is missing every entry fails with IGDSP_ENODEV.
#include "igdsp_ctx.h"
#include "igdsp_txstage.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

using namespace igdsp;
using igdsp_rx::kSlot;
using igdsp_rx::kStageDepth;

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

extern "C" {

int igdsp_abi_version(void) { return IGDSP_ABI_VERSION; }

int igdsp_create(igdsp_ctx **out, int device, uint32_t max_channels)
{
    if (!out || max_channels == 0 || max_channels > (1u << 24)) return IGDSP_EINVAL;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return IGDSP_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return IGDSP_ENODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return IGDSP_ENODEV;   // code objects are gfx950-only
    if (hipSetDevice(device) != hipSuccess) return IGDSP_ENODEV;

    igdsp_ctx *ctx = new (std::nothrow) igdsp_ctx();
    if (!ctx) return IGDSP_ENOMEM;
    ctx->device = device;
    ctx->cus = prop.multiProcessorCount;
    ctx->name = prop.name;
    ctx->max_channels = max_channels;
    ctx->direct = std::vector<std::atomic<uint32_t>>(kDirectCalls);
    for (auto &d : ctx->direct) d.store(kNoChan, std::memory_order_relaxed);
    const size_t max_frames = (size_t)max_channels * kStageDepth;       // most frames one flush can take
    ctx->up_bytes = igdsp_rx::upload_layout(max_frames, max_channels).total;
    bool ok = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&ctx->flush_done, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < igdsp_rx::RingMem::kArrays; ++i)
        ok = ok && hipHostMalloc(ctx->ring.array(i), igdsp_rx::RingMem::bytes(max_channels, i), hipHostMallocDefault) == hipSuccess;
    if (ok) ctx->rx.init(max_channels, ctx->ring);
    ok = ok && hipHostMalloc((void **)&ctx->h_up, ctx->up_bytes, hipHostMallocDefault) == hipSuccess;
    for (uint32_t i = 0; i < 2; ++i) {
        igdsp_rx::Published &pb = ctx->pub.set(i);
        ok = ok && hipHostMalloc((void **)&pb.last, max_channels * sizeof(igdsp_frame_stats), hipHostMallocDefault) == hipSuccess;
        ok = ok && hipHostMalloc((void **)&pb.hold, max_channels * sizeof(igdsp_chan_hold), hipHostMallocDefault) == hipSuccess;
        ok = ok && hipHostMalloc((void **)&pb.probe, max_channels * sizeof(igdsp_chan_probe), hipHostMallocDefault) == hipSuccess;
    }
    ok = ok && hipMalloc((void **)&ctx->d_up, ctx->up_bytes) == hipSuccess;
    ok = ok && hipMalloc((void **)&ctx->d_stats, 2 * max_frames * sizeof(igdsp_frame_stats)) == hipSuccess;   // group A | group B
    ok = ok && hipMalloc((void **)&ctx->d_last, max_channels * sizeof(igdsp_frame_stats)) == hipSuccess;
    ok = ok && hipMalloc((void **)&ctx->d_hold, max_channels * sizeof(igdsp_chan_hold)) == hipSuccess;
    ok = ok && hipMalloc((void **)&ctx->d_probe, max_channels * sizeof(igdsp_chan_probe)) == hipSuccess;
    ok = ok && hipMalloc((void **)&ctx->d_queues, kQueueRing * 32u * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipMemset(ctx->d_queues, 0, kQueueRing * 32u * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipMemset(ctx->d_last, 0, max_channels * sizeof(igdsp_frame_stats)) == hipSuccess;
    ok = ok && hipMemset(ctx->d_probe, 0, max_channels * sizeof(igdsp_chan_probe)) == hipSuccess;
    if (const char *e = std::getenv("IGDSP_GLOBAL_QUEUE")) ctx->global_queue = std::atoi(e) != 0;
    if (const char *e = std::getenv("IGDSP_IO_SPARE_CHUNKS")) ctx->io_spare_cap = (size_t)std::max(0, std::atoi(e));
    if (!ok) {
        igdsp_destroy(ctx);
        return IGDSP_ENOMEM;
    }
    if (init_device_attributes() != hipSuccess) {      // this device's kernel attributes (hipSetDevice above)
        igdsp_destroy(ctx);
        return IGDSP_EDEVICE;
    }
    bool up = launch_hold_reset(ctx->d_hold, max_channels, nullptr, ctx->stream) == hipSuccess;
    for (uint32_t i = 0; i < 2; ++i) {
        igdsp_rx::Published &pb = ctx->pub.set(i);
        std::memset(pb.last, 0, max_channels * sizeof(igdsp_frame_stats));
        std::memset(pb.probe, 0, max_channels * sizeof(igdsp_chan_probe));
        up = up && hipMemcpyAsync(pb.hold, ctx->d_hold, max_channels * sizeof(igdsp_chan_hold), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
    }
    if (!up || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        igdsp_destroy(ctx);
        return IGDSP_EDEVICE;
    }
    ctx->pool = make_pool(max_channels);
    *out = ctx;
    return IGDSP_OK;
}

int igdsp_destroy(igdsp_ctx *ctx)
{
    if (!ctx) return IGDSP_OK;                       // tolerate NULL like the reference's setters (TransportAdapter.cpp:135-223)
    ctx->pool.reset();
    if (ctx->device >= 0) (void)hipSetDevice(ctx->device);
    delete ctx->tx.load();
    igdsp_io_drop_spares(ctx);
    if (ctx->stream) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamDestroy(ctx->stream); }
    if (ctx->flush_done) (void)hipEventDestroy(ctx->flush_done);
    for (int i = 0; i < igdsp_rx::RingMem::kArrays; ++i) if (*ctx->ring.array(i)) (void)hipHostFree(*ctx->ring.array(i));
    const igdsp_rx::Published &p0 = ctx->pub.set(0), &p1 = ctx->pub.set(1);
    void *hosts[] = {ctx->h_up, p0.last, p0.hold, p0.probe, p1.last, p1.hold, p1.probe};
    for (void *p : hosts) if (p) (void)hipHostFree(p);
    void *devs[] = {ctx->d_up, ctx->d_stats, ctx->d_last, ctx->d_hold, ctx->d_probe, ctx->d_queues, ctx->d_enc_tab[0], ctx->d_enc_tab[1]};
    for (void *p : devs) if (p) (void)hipFree(p);
    delete ctx;
    return IGDSP_OK;
}

const char *igdsp_last_error(const igdsp_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }

int igdsp_device_info(const igdsp_ctx *ctx, int *device, int *compute_units, char *name, size_t name_len)
{
    if (!ctx) return IGDSP_EINVAL;
    if (device) *device = ctx->device;
    if (compute_units) *compute_units = ctx->cus;
    if (name && name_len) { std::strncpy(name, ctx->name.c_str(), name_len - 1); name[name_len - 1] = 0; }
    return IGDSP_OK;
}

int igdsp_set_variant(igdsp_ctx *ctx, int variant)
{
    if (!ctx || variant < 0 || variant > 4) return IGDSP_EINVAL;
    ctx->variant = variant;
    return IGDSP_OK;
}

// ---------------------------------------------------------------- routing (a4)
static uint32_t lookup(igdsp_ctx *ctx, int32_t call_id)
{
    if (call_id >= 0 && call_id < kDirectCalls) return ctx->direct[(size_t)call_id].load(std::memory_order_acquire);
    std::lock_guard<std::mutex> g(ctx->far_mu);
    auto it = ctx->far.find(call_id);
    return it == ctx->far.end() ? kNoChan : it->second;
}

int igdsp_map_call(igdsp_ctx *ctx, int32_t call_id, uint32_t channel)
{
    if (!ctx) return IGDSP_EINVAL;
    if (channel >= ctx->max_channels) return IGDSP_ERANGE;
    if (call_id >= 0 && call_id < kDirectCalls) ctx->direct[(size_t)call_id].store(channel, std::memory_order_release);
    else { std::lock_guard<std::mutex> g(ctx->far_mu); ctx->far[call_id] = channel; }
    return IGDSP_OK;
}

int igdsp_unmap_call(igdsp_ctx *ctx, int32_t call_id)
{
    if (!ctx) return IGDSP_EINVAL;
    if (call_id >= 0 && call_id < kDirectCalls) ctx->direct[(size_t)call_id].store(kNoChan, std::memory_order_release);
    else { std::lock_guard<std::mutex> g(ctx->far_mu); ctx->far.erase(call_id); }
    return IGDSP_OK;
}

// ---------------------------------------------------------------- single-frame entry
int igdsp_on_rtp_frame(igdsp_ctx *ctx, int32_t call_id, uint8_t pt, const uint8_t *payload, uint32_t payloadlen)
{
    if (!ctx) return IGDSP_EINVAL;
    if (pt != IGDSP_PT_PCMU && pt != IGDSP_PT_PCMA) return IGDSP_OK;   // keep-alive (123) / other codecs: not metered
    if (payloadlen > kSlot || (payloadlen && !payload)) return IGDSP_EINVAL;
    const uint32_t ch = lookup(ctx, call_id);
    if (ch == kNoChan) return IGDSP_ENOENT;          // the reference's if-chain falls through silently; we report it
    return ctx->rx.stage(ch, pt, payload, payloadlen);
}

// setIncomingED137Value (roip_ed137.h:273): the word the call's frames carry from now on
int igdsp_set_ed137(igdsp_ctx *ctx, int32_t call_id, uint32_t ed137_value)
{
    if (!ctx) return IGDSP_EINVAL;
    const uint32_t ch = lookup(ctx, call_id);
    if (ch == kNoChan) return IGDSP_ENOENT;
    ctx->rx.set_word(ch, ed137_value);
    return IGDSP_OK;
}

int igdsp_set_gate_mode(igdsp_ctx *ctx, uint32_t gate_mode)
{
    if (!ctx || gate_mode > IGDSP_GATE_SQU_OR_PTT) return IGDSP_EINVAL;
    ctx->gate_mode.store(gate_mode, std::memory_order_relaxed);
    return IGDSP_OK;
}

static int flush_end_locked(igdsp_ctx *ctx, int wait)
{
    if (!ctx->flush_open) return IGDSP_OK;
    if (!wait) {
        const hipError_t q = hipEventQuery(ctx->flush_done);
        if (q == hipErrorNotReady) return IGDSP_EBUSY;
        if (q != hipSuccess) return fail(ctx, IGDSP_EDEVICE, "hipEventQuery(flush_done)", q);
    } else {
        HIP_TRY(ctx, hipEventSynchronize(ctx->flush_done));
    }
    ctx->pub.flip();                                                    // the back set is complete: make it the front set
    ctx->flush_open = false;
    return IGDSP_OK;
}

static int flush_begin_locked(igdsp_ctx *ctx, uint32_t *n_frames_out)
{
    if (int rc = flush_end_locked(ctx, 1)) return rc;               // one flush at a time: the upload block is single
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t nch = ctx->rx.channels_seen();
    if (n_frames_out) *n_frames_out = 0;
    if (nch == 0) return IGDSP_OK;
    const size_t max_frames = (size_t)ctx->max_channels * kStageDepth;
    const igdsp_rx::UploadLayout L = igdsp_rx::upload_layout(max_frames, ctx->max_channels);
    // 1. snapshot every channel's staged frames (oldest first) into the upload block, compacted per worker region
    igdsp_rx::SnapPart parts[kMaxParts];
    const uint32_t n_parts = for_each_part(nch >= kPoolMinChannels ? ctx->pool.get() : nullptr, nch, [&](uint32_t i, uint32_t c0, uint32_t c1) {
        parts[i].c0 = c0;
        parts[i].c1 = c1;
        ctx->rx.snapshot(parts[i], ctx->h_up, L);
    });
    uint32_t staged = 0, endA = 0, endB = 0, endS = 0;
    for (uint32_t i = 0; i < n_parts; ++i) {
        staged += parts[i].nSeq;
        if (parts[i].nA) endA = parts[i].c0 * kStageDepth + parts[i].nA;
        if (parts[i].nB) endB = parts[i].c0 * kStageDepth + parts[i].nB;
        if (parts[i].nSeq) endS = parts[i].c0 * kStageDepth + parts[i].nSeq;
    }
    if (n_frames_out) *n_frames_out = staged;
    if (staged == 0) return IGDSP_OK;
    // 2. upload what is used: the payload regions per worker (the big ones), the small sections as one span each; meter group A
    //    and group B over their spans (frames between two workers' regions are stale bytes: their records are never looked at),
    //    fold every channel's frames in arrival order, download the per-channel state into the back set
    hipStream_t s = ctx->stream;
    uint8_t *up = ctx->h_up, *d = ctx->d_up;
    auto copy = [&](size_t off, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(d + off, up + off, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    for (uint32_t i = 0; i < n_parts; ++i) {
        const size_t base = (size_t)parts[i].c0 * kStageDepth;
        HIP_TRY(ctx, copy(L.payA + base * IGDSP_SAMPLES_PER_FRAME, (size_t)parts[i].nA * IGDSP_SAMPLES_PER_FRAME));
        HIP_TRY(ctx, copy(L.payB + base * kSlot, (size_t)parts[i].nB * kSlot));
    }
    HIP_TRY(ctx, copy(L.ptA, endA));
    HIP_TRY(ctx, copy(L.ptB, endB));
    HIP_TRY(ctx, copy(L.lenB, (size_t)endB * sizeof(uint16_t)));
    HIP_TRY(ctx, copy(L.seq, (size_t)endS * 2 * sizeof(uint32_t)));
    HIP_TRY(ctx, copy(L.runs, (size_t)nch * 2 * sizeof(uint32_t)));
    // records: group A's at d_stats[id], group B's at d_stats[max_frames + id] (ids are region-based, so each group may reach max_frames)
    igdsp_frame_stats *stA = ctx->d_stats, *stB = ctx->d_stats + max_frames;
    if (endA)   // whole 160-byte frames, dense: the chunk kernel takes every 64, the general kernel the < 64 left over
        HIP_TRY(ctx, launch_decode_meter(cfg_of(ctx, s), 0, d + L.payA, d + L.ptA, nullptr, endA, 1, IGDSP_SAMPLES_PER_FRAME, stA, nullptr, nullptr, 0, s));
    for (uint32_t i = 0; i < n_parts; ++i)   // every other length (rare): 256-byte slots with a length per frame, one launch per region that has any
        if (parts[i].nB) {
            const size_t base = (size_t)parts[i].c0 * kStageDepth;
            HIP_TRY(ctx, launch_decode_meter(cfg_of(ctx, s), 1, d + L.payB + base * kSlot, d + L.ptB + base, reinterpret_cast<const uint16_t *>(d + L.lenB) + base,
                                             parts[i].nB, 1, kSlot, stB + base, nullptr, nullptr, 0, s));
        }
    HIP_TRY(ctx, launch_flush_fold(stA, stB, reinterpret_cast<const uint16_t *>(d + L.lenB), reinterpret_cast<const uint2 *>(d + L.seq),
                                   reinterpret_cast<const uint2 *>(d + L.runs), nch, ctx->gate_mode.load(std::memory_order_relaxed), IGDSP_PROBE_ALARM,
                                   ctx->d_hold, ctx->d_probe, ctx->d_last, s));
    const igdsp_rx::Published &back = ctx->pub.back();
    HIP_TRY(ctx, hipMemcpyAsync(back.last, ctx->d_last, (size_t)nch * sizeof(igdsp_frame_stats), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(back.hold, ctx->d_hold, (size_t)nch * sizeof(igdsp_chan_hold), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(back.probe, ctx->d_probe, (size_t)nch * sizeof(igdsp_chan_probe), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipEventRecord(ctx->flush_done, s));
    ctx->flush_open = true;
    ctx->flush_nch = nch;
    return IGDSP_OK;
}

int igdsp_flush_begin(igdsp_ctx *ctx, uint32_t *n_frames_out)
{
    if (!ctx) return IGDSP_EINVAL;
    std::lock_guard<std::mutex> g(ctx->flush_mu);
    return flush_begin_locked(ctx, n_frames_out);
}

int igdsp_flush_end(igdsp_ctx *ctx, int wait)
{
    if (!ctx) return IGDSP_EINVAL;
    std::lock_guard<std::mutex> g(ctx->flush_mu);
    return flush_end_locked(ctx, wait);
}

int igdsp_flush(igdsp_ctx *ctx, uint32_t *n_frames_out)
{
    if (!ctx) return IGDSP_EINVAL;
    std::lock_guard<std::mutex> g(ctx->flush_mu);
    if (int rc = flush_begin_locked(ctx, n_frames_out)) return rc;
    return flush_end_locked(ctx, 1);
}

int igdsp_poll(igdsp_ctx *ctx, uint32_t channel, igdsp_level *out)
{
    if (!ctx || !out) return IGDSP_EINVAL;
    if (channel >= ctx->max_channels) return IGDSP_ERANGE;
    igdsp_frame_stats s;
    uint16_t peak_hold = 0;
    ctx->pub.read([&](const igdsp_rx::Published &p) { s = p.last[channel]; peak_hold = p.hold[channel].peak_hold; });
    out->byte_mean = s.byte_mean;
    out->flags = s.flags;
    out->peak = s.peak;
    out->rms = s.rms;
    out->percent = (int32_t)(float)(((double)s.rms * 100.0) / (double)IGDSP_METER_FULL_SCALE);   // audiometer.cpp:30-31
    out->peak_hold = peak_hold;
    out->dropped = (uint16_t)std::min<uint32_t>(ctx->rx.frames_dropped(channel), 65535u);
    out->frames = ctx->rx.frames_seen(channel);
    return IGDSP_OK;
}

int igdsp_poll_call(igdsp_ctx *ctx, int32_t call_id, igdsp_level *out)
{
    if (!ctx || !out) return IGDSP_EINVAL;
    const uint32_t ch = lookup(ctx, call_id);
    if (ch == kNoChan) return IGDSP_ENOENT;
    return igdsp_poll(ctx, ch, out);
}

int igdsp_reset_hold(igdsp_ctx *ctx, uint32_t channel)
{
    if (!ctx) return IGDSP_EINVAL;
    if (channel != 0xFFFFFFFFu && channel >= ctx->max_channels) return IGDSP_ERANGE;
    std::lock_guard<std::mutex> g(ctx->flush_mu);
    if (int rc = flush_end_locked(ctx, 1)) return rc;                  // a flush under way folds into the window being reset: finish it first
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t c0 = (channel == 0xFFFFFFFFu) ? 0 : channel;
    const uint32_t cn = (channel == 0xFFFFFFFFu) ? ctx->max_channels : 1;
    HIP_TRY(ctx, launch_hold_reset(ctx->d_hold + c0, cn, nullptr, ctx->stream));
    // both published sets show the reset window at once (no flush is open, so nothing else writes them)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->pub.back().hold + c0, ctx->d_hold + c0, cn * sizeof(igdsp_chan_hold), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->pub.rewrite_front([&](igdsp_rx::Published &front, const igdsp_rx::Published &back) {
        std::memcpy(front.hold + c0, back.hold + c0, cn * sizeof(igdsp_chan_hold));
    });
    return IGDSP_OK;
}

int igdsp_get_hold(igdsp_ctx *ctx, uint32_t channel, igdsp_chan_hold *out)
{
    if (!ctx || !out) return IGDSP_EINVAL;
    if (channel >= ctx->max_channels) return IGDSP_ERANGE;
    ctx->pub.read([&](const igdsp_rx::Published &p) { *out = p.hold[channel]; });
    return IGDSP_OK;
}

int igdsp_get_probe(igdsp_ctx *ctx, uint32_t channel, igdsp_chan_probe *out)
{
    if (!ctx || !out) return IGDSP_EINVAL;
    if (channel >= ctx->max_channels) return IGDSP_ERANGE;
    ctx->pub.read([&](const igdsp_rx::Published &p) { *out = p.probe[channel]; });
    return IGDSP_OK;
}

// ---------------------------------------------------------------- batched device entries
static int check_shape(uint32_t C, uint32_t F, uint32_t n)
{
    if (n == 0 || n > IGDSP_MAX_PAYLOAD) return IGDSP_EINVAL;
    if ((uint64_t)C * F >= 0xFFFFFFE0ull) return IGDSP_ERANGE;     // frame indices are 32-bit on the device
    return IGDSP_OK;
}

int igdsp_decode_meter(igdsp_ctx *ctx, const uint8_t *d_payload, const uint8_t *d_codec, const uint16_t *d_len,
                       uint32_t C, uint32_t F, uint32_t n, igdsp_frame_stats *d_stats, int16_t *d_pcm,
                       igdsp_aggregate *d_agg, uint32_t rank, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)C * F == 0) return IGDSP_OK;                      // empty batch: nothing to do
    if (!d_payload || !d_codec || !d_stats) return IGDSP_EINVAL;
    if (int rc = check_shape(C, F, n)) return rc;
    if (rank >= IGDSP_AGG_MAX_RANKS) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_decode_meter(cfg_of(ctx, pick(ctx, stream)), ctx->variant, d_payload, d_codec, d_len, C, F, n, d_stats, d_pcm, d_agg, rank, pick(ctx, stream)));
    return IGDSP_OK;
}

// The context's 16-bit compressor table of one lineage (tab[law << 16 | uint16(v)]), built on the device the first time a large
// batch asks for it; nullptr if that failed (the kernels then evaluate the table themselves).
static const uint8_t *enc_table(igdsp_ctx *ctx, int variant)
{
    const int v = variant == IGDSP_ENC_G191 ? 1 : 0;
    std::call_once(ctx->enc_once[v], [&]() {
        uint8_t *t = nullptr;
        hipStream_t bs = nullptr;
        bool ok = hipMalloc((void **)&t, 2u * 65536u) == hipSuccess && hipStreamCreateWithFlags(&bs, hipStreamNonBlocking) == hipSuccess;
        ok = ok && igdsp::launch_build_enc_table(variant, t, bs) == hipSuccess && hipStreamSynchronize(bs) == hipSuccess;
        if (bs) (void)hipStreamDestroy(bs);
        if (ok) ctx->d_enc_tab[v] = t;                          // complete before any launch that reads it is enqueued
        else { if (t) (void)hipFree(t); (void)hipGetLastError(); }   // the kernel evaluates the table itself, as before
    });
    return ctx->d_enc_tab[v];
}

int igdsp_encode(igdsp_ctx *ctx, const int16_t *d_pcm, const uint8_t *d_codec, uint32_t C, uint32_t F, uint32_t n,
                 uint8_t *d_out, int variant, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)C * F == 0) return IGDSP_OK;
    if (!d_pcm || !d_codec || !d_out) return IGDSP_EINVAL;
    if (variant != IGDSP_ENC_SUN16 && variant != IGDSP_ENC_G191) return IGDSP_EINVAL;
    if (int rc = check_shape(C, F, n)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    igdsp::LaunchCfg cfg = cfg_of(ctx, pick(ctx, stream));
    if (encode_wants_table(encode_route(C, F, n, reinterpret_cast<uintptr_t>(d_pcm), reinterpret_cast<uintptr_t>(d_out), (uint32_t)cfg.compute_units)))
        cfg.enc_tab = enc_table(ctx, variant);
    HIP_TRY(ctx, launch_encode(cfg, d_pcm, d_codec, C, F, n, d_out, variant, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_roundtrip_peakhold(igdsp_ctx *ctx, const uint8_t *d_payload, const uint8_t *d_codec, uint32_t C, uint32_t F,
                             uint32_t n, uint8_t *d_out, igdsp_frame_stats *d_stats, igdsp_chan_hold *d_hold,
                             const uint8_t *d_gate, int variant, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)C * F == 0) return IGDSP_OK;
    if (!d_payload || !d_codec || !d_out || !d_stats || !d_hold) return IGDSP_EINVAL;
    if (variant != IGDSP_ENC_SUN16 && variant != IGDSP_ENC_G191) return IGDSP_EINVAL;
    if (int rc = check_shape(C, F, n)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_stats) & 7u) || (reinterpret_cast<uintptr_t>(d_hold) & 7u)) return IGDSP_EINVAL;   // natural struct alignment
    // every shape is served: whole groups of 64 channels of 160-byte frames by the fused channel-group-major kernel,
    // the remaining channels and every other geometry by the general wave-per-channel kernel (launch_roundtrip)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    igdsp::LaunchCfg cfg = cfg_of(ctx, pick(ctx, stream));
    cfg.out_spread = ctx->is_spread(d_out);
    HIP_TRY(ctx, launch_roundtrip(cfg, ctx->variant, d_payload, d_codec, C, F, n, d_out, d_stats, d_hold, d_gate, variant, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_hold_update(igdsp_ctx *ctx, const igdsp_frame_stats *d_stats, uint32_t C, uint32_t F, uint32_t n,
                      igdsp_chan_hold *d_hold, const uint8_t *d_gate, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)C * F == 0) return IGDSP_OK;
    if (!d_stats || !d_hold) return IGDSP_EINVAL;
    if (int rc = check_shape(C, F, n)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_hold_update(d_stats, nullptr, C, F, n, d_hold, d_gate, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_hold_reset(igdsp_ctx *ctx, igdsp_chan_hold *d_hold, uint32_t C, const uint8_t *d_mask, void *stream)
{
    if (!ctx || (!d_hold && C)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_hold_reset(d_hold, C, d_mask, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_agg_reset(igdsp_ctx *ctx, igdsp_aggregate *d_agg, void *stream)
{
    if (!ctx || !d_agg) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(d_agg, 0, sizeof(igdsp_aggregate), pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_depayload(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_radio, uint32_t C,
                    uint32_t F, uint32_t pkt_stride, uint32_t n, uint8_t *d_payload_out, uint16_t *d_len_out,
                    igdsp_rtp_info *d_info_out, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)C * F == 0) return IGDSP_OK;
    if (!d_packets || !d_radio || !d_payload_out || !d_len_out || !d_info_out) return IGDSP_EINVAL;
    if (int rc = check_shape(C, F, n)) return rc;
    // slots hold at least a 20-byte header, are dword-granular (so header words and payload dwords are aligned)
    if (pkt_stride < 20u || (pkt_stride & 3u) || pkt_stride > 2048u || (reinterpret_cast<uintptr_t>(d_packets) & 3u)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_depayload(cfg_of(ctx, pick(ctx, stream)), d_packets, d_sizes, d_radio, C, F, pkt_stride, n, d_payload_out, d_len_out, d_info_out, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_decode_meter_rtp(igdsp_ctx *ctx, const uint8_t *d_slots, const uint8_t *d_codec, uint32_t C, uint32_t F,
                           igdsp_frame_stats *d_stats, igdsp_rtp_info *d_info, igdsp_aggregate *d_agg, uint32_t rank, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)C * F == 0) return IGDSP_OK;
    if (!d_slots || !d_codec || !d_stats || rank >= IGDSP_AGG_MAX_RANKS) return IGDSP_EINVAL;
    if (int rc = check_shape(C, F, IGDSP_SAMPLES_PER_FRAME)) return rc;
    // the fused kernel consumes whole 64-slot super-chunks of 16-byte aligned slots; other shapes take the
    // two-step route (igdsp_depayload + igdsp_decode_meter) — rejected here rather than silently re-routed
    if (((uint64_t)C * F) % 64u || (reinterpret_cast<uintptr_t>(d_slots) & 15u) || (reinterpret_cast<uintptr_t>(d_stats) & 15u) ||
        (reinterpret_cast<uintptr_t>(d_info) & 7u))
        return fail(ctx, IGDSP_EINVAL, "decode_meter_rtp needs C*F % 64 == 0 and 16-byte aligned slots / stats");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_decode_meter_rtp(cfg_of(ctx, pick(ctx, stream)), d_slots, nullptr, d_codec, C, F, 0, 20, d_stats, d_info, d_agg, rank, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_decode_meter_packets(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_codec, uint32_t C,
                               uint32_t F, uint32_t pkt_stride, uint32_t hdr_bytes, igdsp_frame_stats *d_stats,
                               igdsp_rtp_info *d_info, igdsp_aggregate *d_agg, uint32_t rank, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)C * F == 0) return IGDSP_OK;
    if (!d_packets || !d_codec || !d_stats || rank >= IGDSP_AGG_MAX_RANKS) return IGDSP_EINVAL;
    if (hdr_bytes != 12u && hdr_bytes != 20u) return IGDSP_EINVAL;
    if (int rc = check_shape(C, F, IGDSP_SAMPLES_PER_FRAME)) return rc;
    if (pkt_stride < hdr_bytes + IGDSP_SAMPLES_PER_FRAME || pkt_stride < 20u || (pkt_stride & 3u) || pkt_stride > 2048u ||
        (uint64_t)C * F * pkt_stride > 0xFFFFFFFFull * 4ull)
        return IGDSP_EINVAL;
    if (((uint64_t)C * F) % 64u || (reinterpret_cast<uintptr_t>(d_packets) & 3u) || (reinterpret_cast<uintptr_t>(d_stats) & 15u) ||
        (reinterpret_cast<uintptr_t>(d_info) & 7u) || (reinterpret_cast<uintptr_t>(d_sizes) & 1u))
        return fail(ctx, IGDSP_EINVAL, "decode_meter_packets needs C*F % 64 == 0, dword-aligned packets, 16-byte aligned stats");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_decode_meter_rtp(cfg_of(ctx, pick(ctx, stream)), d_packets, d_sizes, d_codec, C, F, pkt_stride, hdr_bytes, d_stats, d_info, d_agg, rank, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_decode_meter_packets_mixed(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_codec,
                                     const uint8_t *d_radio, uint32_t C, uint32_t F, uint32_t pkt_stride, igdsp_frame_stats *d_stats,
                                     igdsp_rtp_info *d_info, igdsp_aggregate *d_agg, uint32_t rank, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)C * F == 0) return IGDSP_OK;
    if (!d_packets || !d_codec || !d_radio || !d_stats || rank >= IGDSP_AGG_MAX_RANKS) return IGDSP_EINVAL;
    if (int rc = check_shape(C, F, IGDSP_SAMPLES_PER_FRAME)) return rc;
    if (pkt_stride < 180u || (pkt_stride & 3u) || pkt_stride > 2048u || (uint64_t)C * F * pkt_stride > 0xFFFFFFFFull * 4ull)
        return IGDSP_EINVAL;
    if (((uint64_t)C * F) % 64u || (reinterpret_cast<uintptr_t>(d_packets) & 3u) || (reinterpret_cast<uintptr_t>(d_stats) & 15u) ||
        (reinterpret_cast<uintptr_t>(d_info) & 7u) || (reinterpret_cast<uintptr_t>(d_sizes) & 1u))
        return fail(ctx, IGDSP_EINVAL, "decode_meter_packets_mixed needs C*F % 64 == 0, dword-aligned packets, 16-byte aligned stats");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_decode_meter_rtp(cfg_of(ctx, pick(ctx, stream)), d_packets, d_sizes, d_codec, C, F, pkt_stride, 12, d_stats, d_info, d_agg, rank, pick(ctx, stream), d_radio));
    return IGDSP_OK;
}

// ---------------------------------------------------------------- ED-137 gated window (last clause)
size_t igdsp_window_work_bytes(uint32_t n_channels) { return (size_t)kWinMaxSeg * 3u * n_channels * sizeof(uint4); }

static int check_window(igdsp_ctx *ctx, const igdsp_window *win)
{
    if (!win || !win->d_hold || win->gate_mode > IGDSP_GATE_SQU_OR_PTT) return IGDSP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(win->d_hold) & 7u) || (reinterpret_cast<uintptr_t>(win->d_probe) & 3u) || (reinterpret_cast<uintptr_t>(win->d_work) & 15u))
        return fail(ctx, IGDSP_EINVAL, "igdsp_window: d_hold 8-byte, d_probe 4-byte, d_work 16-byte aligned");
    return IGDSP_OK;
}

int igdsp_window_update(igdsp_ctx *ctx, const igdsp_frame_stats *d_stats, const igdsp_rtp_info *d_info, const uint16_t *d_len,
                        uint32_t C, uint32_t F, uint32_t n, const igdsp_window *win, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    if (int rc = check_window(ctx, win)) return rc;
    if ((uint64_t)C * F == 0) return IGDSP_OK;
    if (!d_stats) return IGDSP_EINVAL;
    if (int rc = check_shape(C, F, n)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_window_update(d_stats, d_info, d_len, C, F, n, win->gate_mode, win->probe_alarm ? win->probe_alarm : IGDSP_PROBE_ALARM,
                                      win->d_hold, win->d_gate, win->d_probe, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_decode_meter_window(igdsp_ctx *ctx, uint32_t layout, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_codec,
                              const uint8_t *d_radio, uint32_t C, uint32_t F, uint32_t pkt_stride, uint32_t hdr_bytes,
                              igdsp_frame_stats *d_stats, igdsp_rtp_info *d_info, igdsp_aggregate *d_agg, uint32_t rank,
                              const igdsp_window *win, void *stream)
{
    if (!ctx || layout > IGDSP_PKT_MIXED) return IGDSP_EINVAL;
    if (int rc = check_window(ctx, win)) return rc;
    if ((uint64_t)C * F == 0) return IGDSP_OK;
    if (!d_packets || !d_codec || rank >= IGDSP_AGG_MAX_RANKS) return IGDSP_EINVAL;
    if (layout == IGDSP_PKT_MIXED && !d_radio) return IGDSP_EINVAL;
    const bool fused = C % 64u == 0u && win->d_work != nullptr;
    if (!d_stats && !fused) return fail(ctx, IGDSP_EINVAL, "decode_meter_window: d_stats may only be NULL on the fused path (n_channels % 64 == 0, d_work given)");
    if (int rc = check_shape(C, F, IGDSP_SAMPLES_PER_FRAME)) return rc;
    // the argument rules of the three fused entries
    uint32_t stride = 0, hdr = 20;
    const uint8_t *radio = nullptr;
    const uint16_t *sizes = nullptr;
    if (layout == IGDSP_PKT_SLOTS) {
        if (reinterpret_cast<uintptr_t>(d_packets) & 15u) return fail(ctx, IGDSP_EINVAL, "decode_meter_window: slots need 16-byte alignment");
    } else {
        stride = pkt_stride; sizes = d_sizes;
        if (layout == IGDSP_PKT_PACKED) {
            if (hdr_bytes != 12u && hdr_bytes != 20u) return IGDSP_EINVAL;
            hdr = hdr_bytes;
        } else { hdr = 12; radio = d_radio; }
        const uint32_t need = (layout == IGDSP_PKT_MIXED ? 20u : hdr) + IGDSP_SAMPLES_PER_FRAME;
        if (pkt_stride < need || pkt_stride < 20u || (pkt_stride & 3u) || pkt_stride > 2048u || (uint64_t)C * F * pkt_stride > 0xFFFFFFFFull * 4ull ||
            (reinterpret_cast<uintptr_t>(d_packets) & 3u) || (reinterpret_cast<uintptr_t>(d_sizes) & 1u))
            return IGDSP_EINVAL;
    }
    if (((uint64_t)C * F) % 64u || (reinterpret_cast<uintptr_t>(d_stats) & 15u) || (reinterpret_cast<uintptr_t>(d_info) & 7u))
        return fail(ctx, IGDSP_EINVAL, "decode_meter_window needs C*F % 64 == 0, 16-byte aligned stats, 8-byte aligned info");
    const uint32_t alarm = win->probe_alarm ? win->probe_alarm : IGDSP_PROBE_ALARM;
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (fused) {   // channel-group-major fused kernel with the window folded in (launch_decode_meter_window)
        bool too_long = false;
        HIP_TRY(ctx, launch_decode_meter_window(cfg_of(ctx, s), d_packets, sizes, d_codec, C, F, stride, hdr, radio, d_stats, d_info, d_agg, rank, *win,
                                                &too_long, s));
        if (too_long) return fail(ctx, IGDSP_ERANGE, "decode_meter_window: more than 8 x 65535 frames per launch");
        return IGDSP_OK;
    }
    // other channel counts: the plain fused kernel, then the record-wise window fold on the same stream
    if (!d_info) return fail(ctx, IGDSP_EINVAL, "decode_meter_window: channel counts that are not multiples of 64 (or a window without d_work) need d_info");
    HIP_TRY(ctx, launch_decode_meter_rtp(cfg_of(ctx, s), d_packets, sizes, d_codec, C, F, stride, hdr, d_stats, d_info, d_agg, rank, s, radio));
    HIP_TRY(ctx, launch_window_update(d_stats, d_info, nullptr, C, F, IGDSP_SAMPLES_PER_FRAME, win->gate_mode, alarm, win->d_hold, win->d_gate, win->d_probe, s));
    return IGDSP_OK;
}

int igdsp_wav_expand(igdsp_ctx *ctx, const uint8_t *d_payload, uint32_t C, uint32_t F, uint32_t n, uint32_t rate,
                     uint8_t *d_files, uint64_t file_stride, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)C * F == 0) return IGDSP_OK;
    if (!d_payload || !d_files) return IGDSP_EINVAL;
    if (int rc = check_shape(C, F, n)) return rc;
    const uint64_t file_bytes = 44ull + 2ull * F * n;
    if (file_stride < file_bytes || 2ull * F * n > 0xFFFFFFFFull - 36ull) return IGDSP_EINVAL;   // the header's sizes are 32-bit
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_wav_expand(cfg_of(ctx, pick(ctx, stream)), d_payload, C, F, n, rate, d_files, file_stride, pick(ctx, stream)));
    return IGDSP_OK;
}

// ---- ED-137 TX packetizer (transport_send_rtp, TransportAdapter.cpp:635-874) ----
int igdsp_tx_calltype_bits(const char *ct)
{
    if (!ct) return 0;
    int b = 0;
    if (std::strstr(ct, "Idle")) b |= IGDSP_TX_CT_IDLE;                                   // :675
    if (std::strstr(ct, "Rxonly") || std::strcmp(ct, "Rx") == 0) b |= IGDSP_TX_CT_RX;     // :795, :811
    if (std::strstr(ct, "Tx") || std::strstr(ct, "TRx")) b |= IGDSP_TX_CT_TX;             // :816, :821
    return b;
}

int igdsp_tx_chan_init(igdsp_tx_chan *h, const char *calltype, int call_in, uint8_t pt, uint32_t ssrc, uint16_t seq0, uint32_t ts0,
                       int32_t keepalive_ms, uint64_t now_ms)
{
    if (!h || pt > 127u) return IGDSP_EINVAL;
    std::memset(h, 0, sizeof *h);                          // PJ_POOL_ZALLOC_T (TransportAdapter.cpp:97)
    h->seq = seq0;
    h->ts = ts0;
    h->ssrc = ssrc;
    h->pt = pt;
    h->call_in = call_in ? 1 : 0;                          // :111
    h->keepalive_ms = keepalive_ms;                        // :115
    h->calltype = (uint8_t)igdsp_tx_calltype_bits(calltype);   // :118
    h->r2s_send_ms = now_ms;                               // :123
    h->first_r2s = 1;                                      // :124 (packetCnt 0, callRecorder / slave enables false: :125-128)
    return IGDSP_OK;
}

int igdsp_tx_packetize(igdsp_ctx *ctx, const int16_t *d_pcm, const uint8_t *d_g711, const uint8_t *d_ctl, uint32_t C, uint32_t F,
                       uint32_t n, uint64_t t0_ms, uint32_t frame_ms, igdsp_tx_chan *d_state, uint8_t *d_last_payload, uint8_t *d_packets,
                       uint32_t pkt_stride, uint16_t *d_sizes, igdsp_tx_info *d_info, int variant, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)C * F == 0) return IGDSP_OK;
    if ((d_pcm == nullptr) == (d_g711 == nullptr)) return IGDSP_EINVAL;                   // exactly one input form
    if (!d_state || !d_last_payload || !d_packets || !d_sizes || !d_info) return IGDSP_EINVAL;
    if (d_pcm && variant != IGDSP_ENC_SUN16 && variant != IGDSP_ENC_G191) return IGDSP_EINVAL;
    if (int rc = check_shape(C, F, n)) return rc;
    if (pkt_stride < 20u + n || (pkt_stride & 3u) || pkt_stride > 2048u || (reinterpret_cast<uintptr_t>(d_packets) & 3u)) return IGDSP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_state) & 7u) || (reinterpret_cast<uintptr_t>(d_info) & 3u) || (reinterpret_cast<uintptr_t>(d_sizes) & 1u) ||
        (reinterpret_cast<uintptr_t>(d_pcm) & 1u))
        return IGDSP_EINVAL;
    if ((uint64_t)F * n >= 0x80000000ull) return IGDSP_ERANGE;                              // ts + f * n and frame indices stay 32-bit
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    igdsp::LaunchCfg cfg = cfg_of(ctx, pick(ctx, stream));
    if (tx_wants_table(d_pcm != nullptr, C, F, n)) cfg.enc_tab = enc_table(ctx, variant);
    HIP_TRY(ctx, launch_tx_packetize(cfg, d_pcm, d_g711, d_ctl, C, F, n, t0_ms, frame_ms, d_state, d_last_payload, d_packets, pkt_stride,
                                     d_sizes, d_info, variant, pick(ctx, stream)));
    return IGDSP_OK;
}

// ---- conference mix: pjmedia's bridge step as the reference drives it (pjsua_conf_connect roip_ed137.cpp:4907-4917, Functions.cpp:718-740;
// pjsua_conf_adjust_rx_level in setSlotVolume roip_ed137.cpp:5190-5233, setvolumeSiteTone roip_ed137.cpp:6869-6878) ----
int igdsp_conf_level_q7(float level)
{
    if (!(level == level)) return IGDSP_EINVAL;                                               // NaN
    const float adj = (level - 1.0f) * 128.0f;                                                // float, as pjsua does it
    if (!(adj > -1.0e6f && adj < 1.0e6f)) return IGDSP_EINVAL;                                // (int) of it must be defined
    const int q = 128 + (int)adj;                                                             // (int): toward zero
    return (q < 0 || q > 65535) ? IGDSP_EINVAL : q;
}

int igdsp_conf_build(const uint32_t *channel, const uint32_t *port, uint32_t n_conn, uint32_t n_channels, uint32_t n_ports,
                     uint32_t *port_ptr, uint32_t *members, uint32_t *n_members)
{
    if (!port_ptr || !n_members || (n_conn && (!channel || !port || !members))) return IGDSP_EINVAL;
    std::vector<uint64_t> key;
    try { key.resize(n_conn); } catch (...) { return IGDSP_ENOMEM; }
    for (uint32_t i = 0; i < n_conn; ++i) {
        if (channel[i] >= n_channels || port[i] >= n_ports) return IGDSP_EINVAL;
        key[i] = (uint64_t)port[i] << 32 | channel[i];
    }
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    uint32_t j = 0;
    for (uint32_t p = 0; p <= n_ports; ++p) {
        while (j < key.size() && (key[j] >> 32) < p) ++j;
        port_ptr[p] = j;
    }
    for (size_t i = 0; i < key.size(); ++i) members[i] = (uint32_t)key[i];
    *n_members = (uint32_t)key.size();
    return IGDSP_OK;
}

// igdsp_conf_mix, or with yardstick its compute-free twin igdsp_internal_conf_copy
static int conf_mix(igdsp_ctx *ctx, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm, const uint16_t *d_len,
                    const uint16_t *d_gain, const uint32_t *d_port_ptr, const uint32_t *d_members, uint32_t n_members, uint32_t C, uint32_t P,
                    uint32_t F, uint32_t n, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)P * F == 0) return IGDSP_OK;                                               // nothing to write
    if ((d_payload == nullptr) == (d_pcm == nullptr) || (d_payload && !d_codec)) return IGDSP_EINVAL;   // exactly one input form
    if (!d_out && !d_stats) return IGDSP_EINVAL;
    if (!d_gain || !d_port_ptr || (n_members && !d_members)) return IGDSP_EINVAL;
    if (int rc = check_shape(C, F, n)) return rc;
    if (int rc = check_shape(P, F, n)) return rc;
    const uintptr_t a2 = reinterpret_cast<uintptr_t>(d_pcm) | reinterpret_cast<uintptr_t>(d_len) | reinterpret_cast<uintptr_t>(d_gain) |
                         reinterpret_cast<uintptr_t>(d_out);
    const uintptr_t a4 = reinterpret_cast<uintptr_t>(d_port_ptr) | reinterpret_cast<uintptr_t>(d_members);
    if ((a2 & 1u) || (a4 & 3u) || (reinterpret_cast<uintptr_t>(d_stats) & 7u)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_conf_mix(cfg_of(ctx, pick(ctx, stream)), d_payload, d_codec, d_pcm, d_len, d_gain, d_port_ptr, d_members, n_members, C, P,
                                 F, n, d_out, d_stats, yardstick, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_conf_mix(igdsp_ctx *ctx, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm, const uint16_t *d_len,
                   const uint16_t *d_gain, const uint32_t *d_port_ptr, const uint32_t *d_members, uint32_t n_members, uint32_t C, uint32_t P,
                   uint32_t F, uint32_t n, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return conf_mix(ctx, d_payload, d_codec, d_pcm, d_len, d_gain, d_port_ptr, d_members, n_members, C, P, F, n, d_out, d_stats, stream, false);
}

// ---- best signal selection: the receiver vote of checkEvents (roip_ed137.cpp:5985-6119; get_IPRadioSquelch / get_IPRadioBss,
// Functions.cpp:1001-1022; setvolume, Functions.cpp:1664-1705) ----
// igdsp_bss_select, or with yardstick its compute-free twin igdsp_internal_bss_copy
static int bss_select(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                      const uint16_t *d_len, const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members, uint32_t n_members,
                      const uint8_t *d_mute, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t vote_frames, igdsp_bss_state *d_state,
                      uint32_t *d_words, int32_t *d_sel, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)G * F == 0) return IGDSP_OK;                                               // nothing to do
    if (!d_info || !d_group_ptr || !d_state) return IGDSP_EINVAL;
    if (n_members && (!d_members || !d_words)) return IGDSP_EINVAL;
    if (n_members > (1u << 24)) return IGDSP_EINVAL;                                          // positions are 24-bit in the vote key
    if (d_payload && d_pcm) return IGDSP_EINVAL;                                              // at most one input form
    if (d_payload && !d_codec) return IGDSP_EINVAL;
    if ((d_out || d_stats) && !d_payload && !d_pcm) return IGDSP_EINVAL;                      // audio outputs need audio
    if (int rc = check_shape(C, F, n)) return rc;
    if (int rc = check_shape(G, F, n)) return rc;
    const uintptr_t a2 = reinterpret_cast<uintptr_t>(d_pcm) | reinterpret_cast<uintptr_t>(d_len) | reinterpret_cast<uintptr_t>(d_gain) |
                         reinterpret_cast<uintptr_t>(d_out);
    const uintptr_t a4 = reinterpret_cast<uintptr_t>(d_info) | reinterpret_cast<uintptr_t>(d_group_ptr) | reinterpret_cast<uintptr_t>(d_members) |
                         reinterpret_cast<uintptr_t>(d_state) | reinterpret_cast<uintptr_t>(d_words) | reinterpret_cast<uintptr_t>(d_sel);
    if ((a2 & 1u) || (a4 & 3u) || (reinterpret_cast<uintptr_t>(d_stats) & 7u)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_bss_select(cfg_of(ctx, pick(ctx, stream)), d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members,
                                   n_members, d_mute, C, G, F, n, vote_frames, d_state, d_words, d_sel, d_out, d_stats, yardstick,
                                   pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_bss_select(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                     const uint16_t *d_len, const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members, uint32_t n_members,
                     const uint8_t *d_mute, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t vote_frames, igdsp_bss_state *d_state,
                     uint32_t *d_words, int32_t *d_sel, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return bss_select(ctx, d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, d_mute, C, G, F, n, vote_frames,
                      d_state, d_words, d_sel, d_out, d_stats, stream, false);
}

// ---- PTT priority arbitration: the CLIENT-mode block of checkEvents (roip_ed137.cpp:6124-6231; get_IPRadioPttStatus,
// Functions.cpp:1045-1139; the PTT id, Functions.cpp:1141-1151) ----
// igdsp_ptt_arbitrate, or with yardstick its compute-free twin igdsp_internal_ptt_copy
static int ptt_arbitrate(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                         const uint16_t *d_len, const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members,
                         uint32_t n_members, const uint8_t *d_rxonly, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t release_frames,
                         igdsp_ptt_state *d_state, igdsp_ptt_slot *d_slots, int32_t *d_sel, igdsp_ptt_tick *d_tick, uint8_t *d_ctl_out,
                         int16_t *d_out, igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    if (n == 0 || n > IGDSP_MAX_PAYLOAD || n_members > (1u << 24) || release_frames > 255u) return IGDSP_EINVAL;   // always checked
    if ((uint64_t)G * F == 0) return IGDSP_OK;                                               // nothing to do
    if (!d_info || !d_group_ptr || !d_state) return IGDSP_EINVAL;
    if (n_members && (!d_members || !d_slots)) return IGDSP_EINVAL;
    if (d_payload && d_pcm) return IGDSP_EINVAL;                                              // at most one input form
    if (d_payload && !d_codec) return IGDSP_EINVAL;
    if ((d_out || d_stats) && !d_payload && !d_pcm) return IGDSP_EINVAL;                      // audio outputs need audio
    if (int rc = check_shape(C, F, n)) return rc;
    if (int rc = check_shape(G, F, n)) return rc;
    const uintptr_t a2 = reinterpret_cast<uintptr_t>(d_pcm) | reinterpret_cast<uintptr_t>(d_len) | reinterpret_cast<uintptr_t>(d_gain) |
                         reinterpret_cast<uintptr_t>(d_out);
    const uintptr_t a4 = reinterpret_cast<uintptr_t>(d_info) | reinterpret_cast<uintptr_t>(d_group_ptr) | reinterpret_cast<uintptr_t>(d_members) |
                         reinterpret_cast<uintptr_t>(d_state) | reinterpret_cast<uintptr_t>(d_slots) | reinterpret_cast<uintptr_t>(d_sel) |
                         reinterpret_cast<uintptr_t>(d_tick);
    if ((a2 & 1u) || (a4 & 3u) || (reinterpret_cast<uintptr_t>(d_stats) & 7u)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_ptt_arbitrate(cfg_of(ctx, pick(ctx, stream)), d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members,
                                      n_members, d_rxonly, C, G, F, n, release_frames, d_state, d_slots, d_sel, d_tick, d_ctl_out, d_out,
                                      d_stats, yardstick, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_ptt_arbitrate(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                        const uint16_t *d_len, const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members,
                        uint32_t n_members, const uint8_t *d_rxonly, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t release_frames,
                        igdsp_ptt_state *d_state, igdsp_ptt_slot *d_slots, int32_t *d_sel, igdsp_ptt_tick *d_tick, uint8_t *d_ctl_out,
                        int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return ptt_arbitrate(ctx, d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, d_rxonly, C, G, F, n,
                         release_frames, d_state, d_slots, d_sel, d_tick, d_ctl_out, d_out, d_stats, stream, false);
}

// ---- R2S link supervision and the device event list: the body of detectR2SPacketAndReconn (roip_ed137.cpp:1764-1780, :2009-2040) and
// the rtpAudio edge of transport_rtp_cb (TransportAdapter.cpp:286-315) ----
size_t igdsp_link_work_bytes(uint32_t n_channels, uint32_t n_ticks) { return (size_t)link_work_bytes(n_channels, n_ticks); }

// igdsp_link_watch, or with yardstick its compute-free twin igdsp_internal_link_copy
static int link_watch(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint16_t *d_sizes, const uint8_t *d_up, const uint16_t *d_period_ms,
                      uint32_t C, uint32_t T, uint32_t S, uint64_t t0_ms, uint32_t tick_ms, uint32_t miss_ticks, uint32_t event_mask,
                      igdsp_link_state *d_state, uint8_t *d_kind, igdsp_link_event *d_events, uint32_t event_cap, uint32_t *d_event_count,
                      void *d_work, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    if (S == 0 || S > IGDSP_STAGE_DEPTH || tick_ms == 0 || miss_ticks > 65535u) return IGDSP_EINVAL;   // always checked
    if (!d_events && event_cap) return IGDSP_EINVAL;
    const bool list = d_event_count != nullptr;
    if (list && (!d_work || (reinterpret_cast<uintptr_t>(d_work) & 15u))) return IGDSP_EINVAL;
    const uintptr_t a2 = reinterpret_cast<uintptr_t>(d_sizes) | reinterpret_cast<uintptr_t>(d_period_ms);
    const uintptr_t a4 = reinterpret_cast<uintptr_t>(d_info) | reinterpret_cast<uintptr_t>(d_events) | reinterpret_cast<uintptr_t>(d_event_count);
    if ((a2 & 1u) || (a4 & 3u) || (reinterpret_cast<uintptr_t>(d_state) & 7u)) return IGDSP_EINVAL;
    const bool work = (uint64_t)C * T != 0;
    if (work && (!d_info || !d_state)) return IGDSP_EINVAL;
    if ((uint64_t)C * T * S >= 0xFFFFFFE0ull) return IGDSP_ERANGE;                             // list indices and counts are 32-bit
    if (!work && !list) return IGDSP_OK;                                                     // nothing to do, nothing to write
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_link_watch(cfg_of(ctx, pick(ctx, stream)), d_info, d_sizes, d_up, d_period_ms, C, T, S, t0_ms, tick_ms, miss_ticks, event_mask,
                                   d_state, d_kind, d_events, event_cap, d_event_count, d_work, yardstick, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_link_watch(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint16_t *d_sizes, const uint8_t *d_up, const uint16_t *d_period_ms,
                     uint32_t n_channels, uint32_t n_ticks, uint32_t slots_per_tick, uint64_t t0_ms, uint32_t tick_ms, uint32_t miss_ticks,
                     uint32_t event_mask, igdsp_link_state *d_state, uint8_t *d_kind, igdsp_link_event *d_events, uint32_t event_cap,
                     uint32_t *d_event_count, void *d_work, void *stream)
{
    return link_watch(ctx, d_info, d_sizes, d_up, d_period_ms, n_channels, n_ticks, slots_per_tick, t0_ms, tick_ms, miss_ticks, event_mask, d_state,
                      d_kind, d_events, event_cap, d_event_count, d_work, stream, false);
}

// ---- jitter buffer: the pjmedia stream behind adapter->stream_rtp_cb (TransportAdapter.cpp:301): RFC 3550 A.1 / A.3 / A.8 and playout ----
size_t igdsp_jb_ring_bytes(uint32_t n_channels, uint32_t samples_per_frame)
{
    if (samples_per_frame == 0 || samples_per_frame > IGDSP_MAX_PAYLOAD) return 0;
    return (size_t)jb_ring_bytes(n_channels, samples_per_frame);
}

int igdsp_jb_report(const igdsp_jb_state *s, igdsp_jb_prior *prior, igdsp_jb_rr *out)
{
    if (!s || !prior || !out) return IGDSP_EINVAL;
    *out = igdsp_jb_rr{};
    if (!(s->flags & IGDSP_JB_HEARD)) return IGDSP_OK;
    const uint32_t ext = s->cycles + s->max_seq;
    const uint32_t expected = ext - s->base_seq + 1u;
    const int64_t lost = (int64_t)expected - (int64_t)s->received;
    const bool same = prior->epoch == s->epoch;                                 // init_seq zeroes the priors
    const uint32_t exp_int = expected - (same ? prior->expected_prior : 0u), rec_int = s->received - (same ? prior->received_prior : 0u);
    const int64_t lost_int = (int64_t)exp_int - (int64_t)rec_int;
    out->ssrc = s->ssrc;
    out->ext_max_seq = ext;
    out->cum_lost = (int32_t)std::min<int64_t>(std::max<int64_t>(lost, -0x800000), 0x7FFFFF);
    out->jitter = s->jitter >> 4;
    out->fraction_lost = (exp_int == 0u || lost_int <= 0) ? 0u : (uint8_t)std::min<int64_t>((lost_int << 8) / exp_int, 255);
    out->valid = 1;
    prior->expected_prior = expected;
    prior->received_prior = s->received;
    prior->epoch = s->epoch;
    return IGDSP_OK;
}

void igdsp_jb_adapt_cfg_default(igdsp_jb_adapt_cfg *cfg)
{
    if (cfg) *cfg = igdsp_jb_adapt_cfg{IGDSP_JB_ADAPT_MIN, IGDSP_JB_ADAPT_MAX, IGDSP_JB_DELAY, IGDSP_JB_ADAPT_MULT, IGDSP_JB_ADAPT_LATE_RESTART, {0, 0, 0}};
}

int igdsp_jb_adapt_next(const igdsp_jb_adapt_cfg *cfg, uint32_t jitter_q4, uint32_t samples_per_frame, igdsp_jb_adapt *a)
{
    igdsp_jb_adapt_cfg c;
    igdsp_jb_adapt_cfg_default(&c);
    if (cfg) c = *cfg;
    if (!a || !jb_adapt_cfg_ok(c) || samples_per_frame == 0 || samples_per_frame > IGDSP_MAX_PAYLOAD) return IGDSP_EINVAL;
    return (int)jb_adapt_start(c, jitter_q4, samples_per_frame, *a);
}

// igdsp_jb_receive, or with yardstick its compute-free twin igdsp_internal_jb_copy (which leaves d_pkt_status alone)
static int jb_receive(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_radio, const uint32_t *d_arrival,
                      uint32_t C, uint32_t T, uint32_t S, uint32_t stride, uint32_t n, uint32_t delay, igdsp_jb_state *d_state, void *d_ring,
                      uint8_t *d_payload, uint16_t *d_len, igdsp_rtp_info *d_info, uint8_t *d_tick_flags, uint8_t *d_pkt_status, void *stream,
                      bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)C * T == 0) return IGDSP_OK;                                               // nothing to do
    if (!d_packets || !d_radio || !d_state || !d_ring || !d_payload || !d_len || !d_info) return IGDSP_EINVAL;
    if (S == 0 || S > IGDSP_STAGE_DEPTH || delay >= IGDSP_JB_DEPTH) return IGDSP_EINVAL;
    if (stride < 20u || (stride & 3u) || stride > 2048u) return IGDSP_EINVAL;
    if (int rc = check_shape(C, T, n)) return rc;
    if ((uint64_t)C * T * S >= 0xFFFFFFE0ull) return IGDSP_ERANGE;
    const uintptr_t a2 = reinterpret_cast<uintptr_t>(d_sizes) | reinterpret_cast<uintptr_t>(d_len);
    const uintptr_t a4 = reinterpret_cast<uintptr_t>(d_packets) | reinterpret_cast<uintptr_t>(d_arrival) | reinterpret_cast<uintptr_t>(d_state) |
                         reinterpret_cast<uintptr_t>(d_info);
    if ((a2 & 1u) || (a4 & 3u) || (reinterpret_cast<uintptr_t>(d_info) & 7u) || (reinterpret_cast<uintptr_t>(d_ring) & 15u)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_jb_receive(cfg_of(ctx, pick(ctx, stream)), d_packets, d_sizes, d_radio, d_arrival, C, T, S, stride, n, delay, d_state, d_ring,
                                   d_payload, d_len, d_info, d_tick_flags, yardstick ? nullptr : d_pkt_status, yardstick, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_jb_receive(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_radio, const uint32_t *d_arrival,
                     uint32_t C, uint32_t T, uint32_t S, uint32_t pkt_stride, uint32_t n, uint32_t delay_frames, igdsp_jb_state *d_state,
                     void *d_ring, uint8_t *d_payload_out, uint16_t *d_len_out, igdsp_rtp_info *d_info_out, uint8_t *d_tick_flags,
                     uint8_t *d_pkt_status, void *stream)
{
    return jb_receive(ctx, d_packets, d_sizes, d_radio, d_arrival, C, T, S, pkt_stride, n, delay_frames, d_state, d_ring, d_payload_out, d_len_out,
                      d_info_out, d_tick_flags, d_pkt_status, stream, false);
}

int igdsp_jb_receive_adaptive(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_radio, const uint32_t *d_arrival,
                              uint32_t C, uint32_t T, uint32_t S, uint32_t stride, uint32_t n, const igdsp_jb_adapt_cfg *cfg, igdsp_jb_state *d_state,
                              void *d_ring, igdsp_jb_adapt *d_adapt, uint8_t *d_payload, uint16_t *d_len, igdsp_rtp_info *d_info,
                              uint8_t *d_tick_flags, uint8_t *d_pkt_status, uint8_t *d_delay_out, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)C * T == 0) return IGDSP_OK;                                               // nothing to do
    if (!d_packets || !d_radio || !d_state || !d_ring || !d_adapt || !d_payload || !d_len || !d_info) return IGDSP_EINVAL;
    igdsp_jb_adapt_cfg c;
    igdsp_jb_adapt_cfg_default(&c);
    if (cfg) c = *cfg;
    if (S == 0 || S > IGDSP_STAGE_DEPTH || !jb_adapt_cfg_ok(c)) return IGDSP_EINVAL;
    if (stride < 20u || (stride & 3u) || stride > 2048u) return IGDSP_EINVAL;
    if (int rc = check_shape(C, T, n)) return rc;
    if ((uint64_t)C * T * S >= 0xFFFFFFE0ull) return IGDSP_ERANGE;
    const uintptr_t a2 = reinterpret_cast<uintptr_t>(d_sizes) | reinterpret_cast<uintptr_t>(d_len);
    const uintptr_t a4 = reinterpret_cast<uintptr_t>(d_packets) | reinterpret_cast<uintptr_t>(d_arrival) | reinterpret_cast<uintptr_t>(d_state) |
                         reinterpret_cast<uintptr_t>(d_info) | reinterpret_cast<uintptr_t>(d_adapt);
    if ((a2 & 1u) || (a4 & 3u) || (reinterpret_cast<uintptr_t>(d_info) & 7u) || (reinterpret_cast<uintptr_t>(d_ring) & 15u)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_jb_adaptive(cfg_of(ctx, pick(ctx, stream)), d_packets, d_sizes, d_radio, d_arrival, C, T, S, stride, n, c, d_state, d_ring, d_adapt,
                                    d_payload, d_len, d_info, d_tick_flags, d_pkt_status, d_delay_out, pick(ctx, stream)));
    return IGDSP_OK;
}

// ---- packet loss concealment between the jitter buffer and the bridge (the pjmedia stream's PLC; G.711 Appendix I's structure) ----
// igdsp_plc_conceal, or with yardstick its compute-free twin igdsp_internal_plc_copy
static int plc_conceal(igdsp_ctx *ctx, const uint8_t *d_tick_flags, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                       const uint16_t *d_len, uint32_t C, uint32_t T, uint32_t n, igdsp_plc_state *d_state, int16_t *d_out, uint16_t *d_len_out,
                       igdsp_frame_stats *d_stats, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    if ((uint64_t)C * T == 0) return IGDSP_OK;                                               // nothing to do
    if (!d_tick_flags || !d_state || !d_out) return IGDSP_EINVAL;
    if ((d_payload == nullptr) == (d_pcm == nullptr) || (d_payload && !d_codec)) return IGDSP_EINVAL;   // exactly one input form
    if (int rc = check_shape(C, T, n)) return rc;
    const uintptr_t a2 = reinterpret_cast<uintptr_t>(d_pcm) | reinterpret_cast<uintptr_t>(d_len) | reinterpret_cast<uintptr_t>(d_out) |
                         reinterpret_cast<uintptr_t>(d_len_out);
    if ((a2 & 1u) || (reinterpret_cast<uintptr_t>(d_state) & 3u) || (reinterpret_cast<uintptr_t>(d_stats) & 7u)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_plc_conceal(cfg_of(ctx, pick(ctx, stream)), d_tick_flags, d_payload, d_codec, d_pcm, d_len, C, T, n, d_state, d_out,
                                    d_len_out, d_stats, yardstick, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_plc_conceal(igdsp_ctx *ctx, const uint8_t *d_tick_flags, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                      const uint16_t *d_len, uint32_t C, uint32_t T, uint32_t n, igdsp_plc_state *d_state, int16_t *d_out, uint16_t *d_len_out,
                      igdsp_frame_stats *d_stats, void *stream)
{
    return plc_conceal(ctx, d_tick_flags, d_payload, d_codec, d_pcm, d_len, C, T, n, d_state, d_out, d_len_out, d_stats, stream, false);
}

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

int igdsp_g726_reorder(igdsp_ctx *ctx, const uint8_t *d_in, uint8_t *d_out, uint64_t n_bytes, int mode, void *stream)
{
    if (!ctx || mode < 1 || mode > 4) return IGDSP_EINVAL;
    if (n_bytes == 0) return IGDSP_OK;
    if (!d_in || !d_out) return IGDSP_EINVAL;
    const uint64_t group = (mode == 2) ? 3 : (mode == 4 ? 5 : 1);
    if (n_bytes % group) return IGDSP_EINVAL;               // the reference over-reads on partial groups
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_g726(cfg_of(ctx, pick(ctx, stream)), d_in, d_out, n_bytes, mode, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_gen_uniform(igdsp_ctx *ctx, uint8_t *d_out, uint64_t n_bytes, uint64_t seed, uint64_t first_byte, void *stream)
{
    if (!ctx || (!d_out && n_bytes)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_gen_uniform(d_out, n_bytes, seed, first_byte, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_stream_read(igdsp_ctx *ctx, const void *d_src, size_t bytes, uint64_t *d_sink, void *stream)
{
    if (!ctx || !d_src || !d_sink || (reinterpret_cast<uintptr_t>(d_src) & 15u)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_read(cfg_of(ctx, pick(ctx, stream)), d_src, bytes, d_sink, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_probe_placement(igdsp_ctx *ctx, const void *d_in, size_t bytes, void *d_out, uint32_t reps, float *ms_per_launch, void *stream)
{
    if (!ctx || !d_in || !ms_per_launch || reps == 0 || bytes < 10240u || (reinterpret_cast<uintptr_t>(d_in) & 15u) ||
        (reinterpret_cast<uintptr_t>(d_out) & 15u))
        return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    void *scratch = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    if (!d_out) {
        if (hipMalloc(&scratch, bytes / 10u + 4096u) != hipSuccess) return fail(ctx, IGDSP_ENOMEM, "probe scratch");
        d_out = scratch;
    }
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = launch_stream_rw(cfg_of(ctx, s), d_in, bytes, d_out, s);
    if (e == hipSuccess) e = hipEventRecord(a, s);
    for (uint32_t i = 0; i < reps && e == hipSuccess; ++i) e = launch_stream_rw(cfg_of(ctx, s), d_in, bytes, d_out, s);
    if (e == hipSuccess) e = hipEventRecord(b, s);
    if (e == hipSuccess) e = hipEventSynchronize(b);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    if (scratch) (void)hipFree(scratch);
    if (e != hipSuccess) return fail(ctx, IGDSP_EDEVICE, "igdsp_probe_placement", e);
    *ms_per_launch = ms / (float)reps;
    return IGDSP_OK;
}

// Measurement / test helper (not in include/igdsp.h): what `n_calls` media threads do between two ticks, in one native loop —
// `frames_per_call` calls of igdsp_on_rtp_frame for each of the calls first_call .. first_call + n_calls - 1, frame f of call k
// taken from payloads[(f * n_calls + k) % n_payloads][payloadlen].  Returns the number of calls that did not return IGDSP_OK.
int igdsp_internal_stage_many(igdsp_ctx *ctx, int32_t first_call, uint32_t n_calls, uint32_t frames_per_call, uint8_t pt,
                              const uint8_t *payloads, uint32_t n_payloads, uint32_t payloadlen)
{
    if (!ctx || !payloads || n_payloads == 0) return IGDSP_EINVAL;
    int bad = 0;
    for (uint32_t f = 0; f < frames_per_call; ++f)
        for (uint32_t k = 0; k < n_calls; ++k)
            if (igdsp_on_rtp_frame(ctx, first_call + (int32_t)k, pt, payloads + (size_t)((f * n_calls + k) % n_payloads) * payloadlen, payloadlen) != IGDSP_OK) ++bad;
    return bad;
}

// Test-only (not in include/igdsp.h): the table-driven compressor the fused round-trip kernel uses, on arbitrary PCM.
int igdsp_internal_encode_table(igdsp_ctx *ctx, const int16_t *d_pcm, const uint8_t *d_codec, uint32_t C, uint32_t F, uint32_t n,
                                uint8_t *d_out, int variant, void *stream)
{
    if (!ctx || !d_pcm || !d_codec || !d_out || (variant != IGDSP_ENC_SUN16 && variant != IGDSP_ENC_G191)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_encode_table(cfg_of(ctx, pick(ctx, stream)), d_pcm, d_codec, C, F, n, d_out, variant, pick(ctx, stream)));
    return IGDSP_OK;
}

// Calibration-only (not in include/igdsp.h): bare load/store kernel with the meter kernel's exact traffic
// (10 KiB read + 1 KiB record store per super-chunk); d_dst needs bytes / 10 bytes.
int igdsp_internal_stream_rw(igdsp_ctx *ctx, const void *d_src, size_t bytes, void *d_dst, void *stream)
{
    if (!ctx || !d_src || !d_dst || (reinterpret_cast<uintptr_t>(d_src) & 15u) || (reinterpret_cast<uintptr_t>(d_dst) & 15u)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_rw(cfg_of(ctx, pick(ctx, stream)), d_src, bytes, d_dst, pick(ctx, stream)));
    return IGDSP_OK;
}

// Calibration-only (not in include/igdsp.h): the meter's 10 : 1 traffic with the record stores of k consecutive super-chunks clustered
int igdsp_internal_stream_cluster(igdsp_ctx *ctx, const void *d_src, size_t bytes, void *d_dst, int k, void *stream)
{
    if (!ctx || !d_src || !d_dst || ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) & 15u)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_cluster(cfg_of(ctx, pick(ctx, stream)), d_src, bytes, d_dst, k, pick(ctx, stream)));
    return IGDSP_OK;
}

// Calibration-only (not in include/igdsp.h): the dword-aligned piece pattern of the packed packet / strided kernels, no per-sample work
// (launch_stream_pieces).  src needs n_items * 64 * stride + 16 bytes, dst n_items KiB, dst2 (optional) n_items * 512 bytes.
int igdsp_internal_stream_pieces(igdsp_ctx *ctx, const void *d_src, uint32_t n_items, uint32_t stride, uint32_t hdr, int mode, int rows, void *d_dst, void *d_dst2, void *stream)
{
    if (!ctx || !d_src || !d_dst || (stride & 3u) || stride < 16u * (uint32_t)(rows - (mode == 0 ? 2 : 1))) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_pieces(cfg_of(ctx, pick(ctx, stream)), d_src, n_items, stride, hdr, mode, rows, d_dst, d_dst2, pick(ctx, stream)));
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

// Calibration-only (not in include/igdsp.h): the compute-free packet writer that moves the bytes of an all-audio igdsp_tx_packetize launch
// in the same traversal (tools/tx_bench.py --ab).  Exactly one of d_pcm / d_g711; n % 4 == 0.
int igdsp_internal_tx_copy(igdsp_ctx *ctx, const int16_t *d_pcm, const uint8_t *d_g711, uint32_t C, uint32_t F, uint32_t n, uint8_t *d_packets,
                           uint32_t pkt_stride, void *stream)
{
    if (!ctx || (d_pcm == nullptr) == (d_g711 == nullptr) || !d_packets || (n & 3u) || n == 0 || n > IGDSP_MAX_PAYLOAD || pkt_stride < 20u + n ||
        (pkt_stride & 3u) || (reinterpret_cast<uintptr_t>(d_packets) & 3u) || (reinterpret_cast<uintptr_t>(d_pcm) & 7u) ||
        (reinterpret_cast<uintptr_t>(d_g711) & 3u))
        return IGDSP_EINVAL;
    if ((uint64_t)C * F == 0) return IGDSP_OK;
    if (int rc = check_shape(C, F, n)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_tx_copy_ab(cfg_of(ctx, pick(ctx, stream)), d_pcm, d_g711, C, F, n, d_packets, pkt_stride, pick(ctx, stream)));
    return IGDSP_OK;
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of igdsp_conf_mix (tools/conf_bench.py) — the same traversal,
// the same bytes read and written, no decode / scale / clamp / stats.  Arguments as igdsp_conf_mix.
int igdsp_internal_conf_copy(igdsp_ctx *ctx, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm, const uint16_t *d_len,
                             const uint16_t *d_gain, const uint32_t *d_port_ptr, const uint32_t *d_members, uint32_t n_members, uint32_t C,
                             uint32_t P, uint32_t F, uint32_t n, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return conf_mix(ctx, d_payload, d_codec, d_pcm, d_len, d_gain, d_port_ptr, d_members, n_members, C, P, F, n, d_out, d_stats, stream, true);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of igdsp_bss_select (tools/bss_bench.py) — the same traversal,
// the same bytes read and written, no decode / scale / clamp / stats / state machine (every non-empty group "selects" its first
// member).  Arguments as igdsp_bss_select; the state is not touched, and sel / out / stats hold raw bytes.
int igdsp_internal_bss_copy(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                            const uint16_t *d_len, const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members,
                            uint32_t n_members, const uint8_t *d_mute, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t vote_frames,
                            igdsp_bss_state *d_state, uint32_t *d_words, int32_t *d_sel, int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return bss_select(ctx, d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, d_mute, C, G, F, n, vote_frames,
                      d_state, d_words, d_sel, d_out, d_stats, stream, true);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of igdsp_jb_receive (tools/jb_bench.py) — the rows of an
// in-order lossless launch (arrival slot 0 of every tick copied as igdsp_depayload would), with no header walk, state machine or ring
// store.  Arguments as igdsp_jb_receive; the state, the ring and d_pkt_status are not touched.
int igdsp_internal_jb_copy(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint8_t *d_radio, const uint32_t *d_arrival,
                           uint32_t C, uint32_t T, uint32_t S, uint32_t pkt_stride, uint32_t n, uint32_t delay_frames, igdsp_jb_state *d_state,
                           void *d_ring, uint8_t *d_payload_out, uint16_t *d_len_out, igdsp_rtp_info *d_info_out, uint8_t *d_tick_flags,
                           uint8_t *d_pkt_status, void *stream)
{
    return jb_receive(ctx, d_packets, d_sizes, d_radio, d_arrival, C, T, S, pkt_stride, n, delay_frames, d_state, d_ring, d_payload_out, d_len_out,
                      d_info_out, d_tick_flags, d_pkt_status, stream, true);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of igdsp_ptt_arbitrate (tools/ptt_bench.py) — the same
// traversal (info records, ops passes, the first member of every group emitted undecoded), the same bytes in and out, no debounce,
// arbitration, decode or records.  Arguments as igdsp_ptt_arbitrate; the group state is not touched, the slots are stepped as by a
// launch, and sel / out / stats hold raw bytes (tick and ctl_out are not written).
int igdsp_internal_ptt_copy(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                            const uint16_t *d_len, const uint16_t *d_gain, const uint32_t *d_group_ptr, const uint32_t *d_members,
                            uint32_t n_members, const uint8_t *d_rxonly, uint32_t C, uint32_t G, uint32_t F, uint32_t n, uint32_t release_frames,
                            igdsp_ptt_state *d_state, igdsp_ptt_slot *d_slots, int32_t *d_sel, igdsp_ptt_tick *d_tick, uint8_t *d_ctl_out,
                            int16_t *d_out, igdsp_frame_stats *d_stats, void *stream)
{
    return ptt_arbitrate(ctx, d_info, d_payload, d_codec, d_pcm, d_len, d_gain, d_group_ptr, d_members, n_members, d_rxonly, C, G, F, n,
                         release_frames, d_state, d_slots, d_sel, d_tick, d_ctl_out, d_out, d_stats, stream, true);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of igdsp_link_watch (tools/link_bench.py) — the same passes
// (count, scan and write with a list, one pass without), the same records and sizes read, the state stored as it was read, kind bytes
// of 0 and an empty list; no state machine.  Arguments as igdsp_link_watch.
int igdsp_internal_link_copy(igdsp_ctx *ctx, const igdsp_rtp_info *d_info, const uint16_t *d_sizes, const uint8_t *d_up, const uint16_t *d_period_ms,
                             uint32_t n_channels, uint32_t n_ticks, uint32_t slots_per_tick, uint64_t t0_ms, uint32_t tick_ms, uint32_t miss_ticks,
                             uint32_t event_mask, igdsp_link_state *d_state, uint8_t *d_kind, igdsp_link_event *d_events, uint32_t event_cap,
                             uint32_t *d_event_count, void *d_work, void *stream)
{
    return link_watch(ctx, d_info, d_sizes, d_up, d_period_ms, n_channels, n_ticks, slots_per_tick, t0_ms, tick_ms, miss_ticks, event_mask, d_state,
                      d_kind, d_events, event_cap, d_event_count, d_work, stream, true);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of igdsp_plc_conceal (tools/plc_bench.py) — the same
// traversal with every tick taken as PLAIN: the input bits widened to the output, no decode, pitch search, synthesis or stats (the
// records carry only the length); the state's ring and scalars are written.  Arguments as igdsp_plc_conceal.
int igdsp_internal_plc_copy(igdsp_ctx *ctx, const uint8_t *d_tick_flags, const uint8_t *d_payload, const uint8_t *d_codec, const int16_t *d_pcm,
                            const uint16_t *d_len, uint32_t C, uint32_t T, uint32_t n, igdsp_plc_state *d_state, int16_t *d_out,
                            uint16_t *d_len_out, igdsp_frame_stats *d_stats, void *stream)
{
    return plc_conceal(ctx, d_tick_flags, d_payload, d_codec, d_pcm, d_len, C, T, n, d_state, d_out, d_len_out, d_stats, stream, true);
}

// Calibration-only (not in include/igdsp.h): the packed-packet piece stream in the channel-group-major order of the fused window kernel
int igdsp_internal_stream_walk(igdsp_ctx *ctx, const void *d_src, uint32_t n_items, uint32_t stride, uint32_t hdr, uint32_t groups, uint32_t n_seg,
                               uint32_t trickle, void *d_dst, void *d_dst2, void *stream)
{
    if (!ctx || !d_src || !d_dst || (stride & 3u) || n_seg == 0 || (groups && n_items % groups)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_walk(cfg_of(ctx, pick(ctx, stream)), d_src, n_items, stride, hdr, groups, n_seg, trickle, d_dst, d_dst2, pick(ctx, stream)));
    return IGDSP_OK;
}

// Calibration-only (not in include/igdsp.h): bare read : write mix, r and w 1 KiB pieces per wave item
// (pairs built: 0:8, 8:8, 8:4, 4:8, 10:1, 10:0, 8:1, 8:2, 20:2, 5:1; `waves` per block 1..16); src needs n_items * r KiB, dst n_items * w KiB.
int igdsp_internal_stream_mix(igdsp_ctx *ctx, const void *d_src, void *d_dst, uint32_t n_items, int r, int w, int waves, void *stream)
{
    // the source may be only dword aligned: that is what the calibration of misaligned 16-byte loads needs
    if (!ctx || !d_src || !d_dst || (reinterpret_cast<uintptr_t>(d_src) & 3u) || (reinterpret_cast<uintptr_t>(d_dst) & 15u)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_mix(cfg_of(ctx, pick(ctx, stream)), d_src, d_dst, n_items, r, w, waves, pick(ctx, stream)));
    return IGDSP_OK;
}

// same, odd items write into a second window (d_dst2 addressed like d_dst) and, if d_src2 is given, read from a second one
int igdsp_internal_stream_mix2(igdsp_ctx *ctx, const void *d_src, void *d_dst, void *d_dst2, uint32_t n_items, int r, int w, int waves, void *stream,
                               const void *d_src2)
{
    if (!ctx || !d_src || !d_dst || !d_dst2 || (reinterpret_cast<uintptr_t>(d_src2) & 15u) || ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst) | reinterpret_cast<uintptr_t>(d_dst2)) & 15u)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_mix(cfg_of(ctx, pick(ctx, stream)), d_src, d_dst, n_items, r, w, waves, pick(ctx, stream), d_dst2, d_src2));
    return IGDSP_OK;
}

// Diagnostic-only (not in include/igdsp.h): stamps of the headline kernel's DIAG instantiation, kDiagWords = 16 x u64 per wavefront
// (d_diag holds 16 x 8 bytes per wave of the grid): {t_begin, t_lut_ready, t_end, sum setup, sum half X, iterations, sum half Y, xcc id,
// realtime begin, realtime end, sum frame-reduce, wave, t_prologue_loads_issued, realtime of the last batch draw, realtime of the
// first draw past the end of the work, block}.
int igdsp_internal_diag_chunk32(igdsp_ctx *ctx, const uint8_t *d_payload, const uint8_t *d_codec, uint32_t C, uint32_t F,
                                igdsp_frame_stats *d_stats, uint64_t *d_diag, void *stream)
{
    if (!ctx || !d_payload || !d_codec || !d_stats || !d_diag || C < 32) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_diag_chunk32(cfg_of(ctx, pick(ctx, stream)), d_payload, d_codec, C, F, d_stats, d_diag, pick(ctx, stream)));
    return IGDSP_OK;
}

// ---------------------------------------------------------------- memory helpers
int igdsp_dev_alloc(igdsp_ctx *ctx, void **d_ptr, size_t bytes)
{
    if (!ctx || !d_ptr) return IGDSP_EINVAL;
    *d_ptr = nullptr;
    if (bytes == 0) return IGDSP_OK;
    if (hipSetDevice(ctx->device) != hipSuccess) return IGDSP_ENODEV;
    hipError_t e = hipMalloc(d_ptr, bytes);
    return e == hipSuccess ? IGDSP_OK : fail(ctx, IGDSP_ENOMEM, "hipMalloc", e);
}

int igdsp_dev_free(igdsp_ctx *ctx, void *d_ptr)
{
    if (!ctx) return IGDSP_EINVAL;
    if (!d_ptr) return IGDSP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipFree(d_ptr));
    return IGDSP_OK;
}

int igdsp_dev_alloc_far(igdsp_ctx *ctx, void **d_ptr, size_t bytes, const void *d_in, size_t in_bytes, uint32_t max_tries,
                        size_t spacer_bytes, float *ms_first, float *ms_kept)
{
    if (!ctx || !d_ptr || !d_in || bytes == 0 || in_bytes < 10240u || max_tries == 0) return IGDSP_EINVAL;
    *d_ptr = nullptr;
    if (hipSetDevice(ctx->device) != hipSuccess) return IGDSP_ENODEV;
    if (spacer_bytes == 0) spacer_bytes = (size_t)12 << 30;
    const size_t cand_bytes = std::max(bytes, in_bytes / 10u + 4096u);       // the probe writes in_bytes / 10
    std::vector<void *> spacers;
    void *best = nullptr;
    float t_best = 0.f, t_first = 0.f;
    int rc = IGDSP_OK;
    for (uint32_t k = 0; k < max_tries; ++k) {
        if (k > 0) {
            void *sp = nullptr;
            if (hipMalloc(&sp, spacer_bytes) != hipSuccess) { (void)hipGetLastError(); break; }   // out of memory: stop widening
            spacers.push_back(sp);
        }
        void *cand = nullptr;
        if (hipMalloc(&cand, cand_bytes) != hipSuccess) { (void)hipGetLastError(); break; }
        float ms = 0.f;
        rc = igdsp_probe_placement(ctx, d_in, in_bytes, cand, 6, &ms, nullptr);
        if (rc != IGDSP_OK) { (void)hipFree(cand); break; }
        if (k == 0) t_first = ms;
        if (best == nullptr || ms < t_best) {
            if (best) (void)hipFree(best);
            best = cand; t_best = ms;
        } else {
            (void)hipFree(cand);
        }
        if (t_best < 0.92f * t_first) break;                                 // another class found
    }
    for (void *sp : spacers) (void)hipFree(sp);
    if (rc != IGDSP_OK) { if (best) (void)hipFree(best); return rc; }
    if (!best) return fail(ctx, IGDSP_ENOMEM, "igdsp_dev_alloc_far");
    *d_ptr = best;
    if (ms_first) *ms_first = t_first;
    if (ms_kept) *ms_kept = t_best;
    return IGDSP_OK;
}

int igdsp_copy_h2d(igdsp_ctx *ctx, void *d_dst, const void *h_src, size_t bytes)
{
    if (!ctx || (bytes && (!d_dst || !h_src))) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return IGDSP_OK;
}

int igdsp_copy_d2h(igdsp_ctx *ctx, void *h_dst, const void *d_src, size_t bytes)
{
    if (!ctx || (bytes && (!h_dst || !d_src))) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return IGDSP_OK;
}

int igdsp_dev_memset(igdsp_ctx *ctx, void *d_ptr, int value, size_t bytes)
{
    if (!ctx || (bytes && !d_ptr)) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemset(d_ptr, value, bytes));
    return IGDSP_OK;
}

int igdsp_sync(igdsp_ctx *ctx, void *stream)
{
    if (!ctx) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t pos;
    const uint32_t launches = queue_mark(ctx, pick(ctx, stream), &pos);
    HIP_TRY(ctx, hipStreamSynchronize(pick(ctx, stream)));
    queue_release_if_idle(ctx, pick(ctx, stream), pos, launches);      // an idle stream gives its work-counter pair back
    return IGDSP_OK;
}

// ---------------------------------------------------------------- timers (HIP events on the launch stream)
struct igdsp_timer { hipEvent_t a, b; };

int igdsp_timer_create(igdsp_ctx *ctx, void **timer)
{
    if (!ctx || !timer) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    igdsp_timer *t = new (std::nothrow) igdsp_timer();
    if (!t) return IGDSP_ENOMEM;
    if (hipEventCreate(&t->a) != hipSuccess || hipEventCreate(&t->b) != hipSuccess) { delete t; return fail(ctx, IGDSP_EDEVICE, "hipEventCreate"); }
    *timer = t;
    return IGDSP_OK;
}

int igdsp_timer_destroy(igdsp_ctx *ctx, void *timer)
{
    if (!ctx || !timer) return IGDSP_EINVAL;
    igdsp_timer *t = (igdsp_timer *)timer;
    (void)hipEventDestroy(t->a); (void)hipEventDestroy(t->b);
    delete t;
    return IGDSP_OK;
}

int igdsp_timer_start(igdsp_ctx *ctx, void *timer, void *stream)
{
    if (!ctx || !timer) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipEventRecord(((igdsp_timer *)timer)->a, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_timer_stop(igdsp_ctx *ctx, void *timer, void *stream)
{
    if (!ctx || !timer) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipEventRecord(((igdsp_timer *)timer)->b, pick(ctx, stream)));
    return IGDSP_OK;
}

int igdsp_timer_elapsed_ms(igdsp_ctx *ctx, void *timer, float *ms)
{
    if (!ctx || !timer || !ms) return IGDSP_EINVAL;
    igdsp_timer *t = (igdsp_timer *)timer;
    HIP_TRY(ctx, hipEventSynchronize(t->b));
    HIP_TRY(ctx, hipEventElapsedTime(ms, t->a, t->b));
    return IGDSP_OK;
}

}  // extern "C"
