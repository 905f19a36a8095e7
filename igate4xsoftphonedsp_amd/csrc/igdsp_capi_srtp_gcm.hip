// igdsp_capi_srtp_gcm.hip — the AES-GCM SRTP entries of include/igdsp.h: igdsp_srtp_gcm_protect / igdsp_srtp_gcm_unprotect and their
// compute-free yardstick igdsp_internal_srtp_gcm_move, and the host-only igdsp_srtp_gcm_derive / igdsp_srtp_gcm_protect_packet /
// igdsp_srtp_gcm_unprotect_packet, which run the rule of igdsp_srtp_gcm.h that k_srtp_gcm runs.  The batched entries read as every batched
// entry does (igdsp_capi.hip): null ctx, the argument rule of igdsp_args.h, hipSetDevice, the stream and its launch configuration, the
// launch.
#include "igdsp_args.h"
#include "igdsp_ctx.h"
#include "igdsp_srtp_gcm.h"

using namespace igdsp;

static int srtp_gcm_entry(igdsp_ctx *ctx, const char *name, int dir, const uint8_t *d_ctl, const uint8_t *d_packets, const uint16_t *d_sizes, uint32_t C, uint32_t F,
                          uint32_t pkt_stride, igdsp_srtp_gcm_state *d_state, uint8_t *d_out, uint32_t out_stride, uint16_t *d_sizes_out, igdsp_srtp_rec *d_rec,
                          void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, name, args::srtp_gcm_run(d_ctl, d_packets, d_sizes, C, F, pkt_stride, d_state, d_out, out_stride, d_sizes_out, d_rec));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_srtp_gcm(cfg_of(ctx, s), dir, d_ctl, d_packets, d_sizes, C, F, pkt_stride, d_state, d_out, out_stride, d_sizes_out, d_rec, yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- RFC 7714 on the packets of a batch ----
int igdsp_srtp_gcm_protect(igdsp_ctx *ctx, const uint8_t *d_ctl, const uint8_t *d_packets, const uint16_t *d_sizes, uint32_t n_channels, uint32_t n_frames,
                           uint32_t pkt_stride, igdsp_srtp_gcm_state *d_state, uint8_t *d_out, uint32_t out_stride, uint16_t *d_sizes_out, igdsp_srtp_rec *d_rec,
                           void *stream)
{
    return srtp_gcm_entry(ctx, "igdsp_srtp_gcm_protect", kSrtpDirProtect, d_ctl, d_packets, d_sizes, n_channels, n_frames, pkt_stride, d_state, d_out, out_stride,
                          d_sizes_out, d_rec, stream, false);
}

int igdsp_srtp_gcm_unprotect(igdsp_ctx *ctx, const uint8_t *d_ctl, const uint8_t *d_packets, const uint16_t *d_sizes, uint32_t n_channels, uint32_t n_frames,
                             uint32_t pkt_stride, igdsp_srtp_gcm_state *d_state, uint8_t *d_out, uint32_t out_stride, uint16_t *d_sizes_out, igdsp_srtp_rec *d_rec,
                             void *stream)
{
    return srtp_gcm_entry(ctx, "igdsp_srtp_gcm_unprotect", kSrtpDirUnprotect, d_ctl, d_packets, d_sizes, n_channels, n_frames, pkt_stride, d_state, d_out, out_stride,
                          d_sizes_out, d_rec, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick (tools/srtp_gcm_bench.py) — protect's piece loads, tile stores,
// row reads and writes, state load and store and output stores, the header parse and the size rules; no AES round, no multiply.
// Arguments as igdsp_srtp_gcm_protect; d_ctl is not read.  A packet protect would accept goes out unchanged with 16 zero bytes behind it
// and a BYPASSED record; the state's words are stored as read.
int igdsp_internal_srtp_gcm_move(igdsp_ctx *ctx, const uint8_t *d_ctl, const uint8_t *d_packets, const uint16_t *d_sizes, uint32_t n_channels, uint32_t n_frames,
                                 uint32_t pkt_stride, igdsp_srtp_gcm_state *d_state, uint8_t *d_out, uint32_t out_stride, uint16_t *d_sizes_out,
                                 igdsp_srtp_rec *d_rec, void *stream)
{
    return srtp_gcm_entry(ctx, "igdsp_srtp_gcm_protect", kSrtpDirProtect, d_ctl, d_packets, d_sizes, n_channels, n_frames, pkt_stride, d_state, d_out, out_stride,
                          d_sizes_out, d_rec, stream, true);
}

// ---- host only
int igdsp_srtp_gcm_derive(const uint8_t *key_salt, uint32_t key_bytes, uint32_t roc0, igdsp_srtp_gcm_state *out)
{
    if (!key_salt || !out) return IGDSP_EINVAL;
    return srtp_gcm_derive(key_salt, key_bytes, roc0, *out) ? IGDSP_OK : IGDSP_EINVAL;
}

int igdsp_srtp_gcm_protect_packet(igdsp_srtp_gcm_state *st, uint32_t ctl, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity, uint32_t *size_out,
                                  igdsp_srtp_rec *rec)
{
    if (!st || !out || !size_out || (!in && size)) return IGDSP_EINVAL;
    igdsp_srtp_rec r;
    srtp_gcm_packet_run<kSrtpProtect>(*st, ctl, in, size, kSrtpMaxPacket, out, out_capacity, *size_out, r);
    if (rec) *rec = r;
    return IGDSP_OK;
}

int igdsp_srtp_gcm_unprotect_packet(igdsp_srtp_gcm_state *st, uint32_t ctl, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity, uint32_t *size_out,
                                    igdsp_srtp_rec *rec)
{
    if (!st || !out || !size_out || (!in && size)) return IGDSP_EINVAL;
    igdsp_srtp_rec r;
    srtp_gcm_packet_run<kSrtpUnprotect>(*st, ctl, in, size, kSrtpMaxPacket, out, out_capacity, *size_out, r);
    if (rec) *rec = r;
    return IGDSP_OK;
}

}  // extern "C"
