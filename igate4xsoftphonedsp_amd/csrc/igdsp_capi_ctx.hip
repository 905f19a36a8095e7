// igdsp_capi_ctx.hip — the context side of the extern "C" boundary of include/igdsp.h: create / destroy / info, call-id routing
// (roip_ed137.cpp:6519-6534), the single-frame staging entry behind setIncomingRTP/setOutgoingRTP (roip_ed137.cpp:6500-6587) with
// its flush and poll entries, the memory helpers, igdsp_sync and the timers.  Host-side responsibilities only; there is NO CPU compute
// path: when the HIP runtime or a gfx950 device is missing every entry fails with IGDSP_ENODEV.  The batched device entries are in
// igdsp_capi.hip, the staged send path in igdsp_capi_tx.hip, calibration and diagnostic entries in igdsp_capi_bench.hip.
#include "igdsp_ctx.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

using namespace igdsp;
using igdsp_rx::kSlot;
using igdsp_rx::kStageDepth;

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
    igdsp_tx_drop(ctx);
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

// ---------------------------------------------------------------- routing (a4): lookup is in igdsp_ctx.h
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
