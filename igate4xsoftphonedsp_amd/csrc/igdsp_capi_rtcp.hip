// igdsp_capi_rtcp.hip — the RTCP / SRTCP entries of include/igdsp.h: igdsp_rtcp_build, igdsp_rtcp_parse, igdsp_srtcp_protect /
// igdsp_srtcp_unprotect and the yardsticks igdsp_internal_rtcp_build_move, igdsp_internal_rtcp_parse_move and
// igdsp_internal_srtcp_move, and the host-only igdsp_srtcp_derive, igdsp_srtcp_*_packet, igdsp_rtcp_build_packet /
// igdsp_rtcp_parse_packet, which run the rules of igdsp_rtcp.h that the kernels run.  The batched entries read as every batched entry
// does (igdsp_capi.hip): null ctx, the argument rule of igdsp_args.h, hipSetDevice, the stream and its launch configuration, the launch.
#include "igdsp_args.h"
#include "igdsp_ctx.h"
#include "igdsp_rtcp.h"

using namespace igdsp;

static int srtcp_entry(igdsp_ctx *ctx, const char *name, int dir, const uint8_t *d_ctl, const uint8_t *d_packets, const uint16_t *d_sizes, uint32_t C, uint32_t F,
                       uint32_t pkt_stride, igdsp_srtp_state *d_state, uint8_t *d_out, uint32_t out_stride, uint16_t *d_sizes_out, igdsp_srtp_rec *d_rec,
                       void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, name, args::srtcp_run(d_ctl, d_packets, d_sizes, C, F, pkt_stride, d_state, d_out, out_stride, d_sizes_out, d_rec));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_srtcp(cfg_of(ctx, s), dir, d_ctl, d_packets, d_sizes, C, F, pkt_stride, d_state, d_out, out_stride, d_sizes_out, d_rec, yardstick, s));
    return IGDSP_OK;
}

static int build_entry(igdsp_ctx *ctx, const uint8_t *d_ctl, const igdsp_jb_state *d_jb, const igdsp_rtcp_src *d_src, const uint64_t *d_now, const uint8_t *d_cname,
                       const uint8_t *d_cname_len, uint32_t C, uint32_t F, igdsp_rtcp_state *d_state, uint8_t *d_packets, uint32_t pkt_stride, uint16_t *d_sizes,
                       igdsp_rtcp_built *d_rec, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_rtcp_build", args::rtcp_build(d_ctl, d_jb, d_src, d_now, d_cname, d_cname_len, C, F, d_state, d_packets, pkt_stride, d_sizes, d_rec));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_rtcp_build(cfg_of(ctx, s), d_ctl, d_jb, d_src, d_now, d_cname, d_cname_len, C, F, d_state, d_packets, pkt_stride, d_sizes, d_rec, yardstick, s));
    return IGDSP_OK;
}

static int parse_entry(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint32_t *d_arrival, const uint32_t *d_local_ssrc, uint32_t C, uint32_t F,
                       uint32_t pkt_stride, igdsp_rtcp_state *d_state, igdsp_rtcp_seen *d_rec, void *stream, bool yardstick)
{
    if (!ctx) return IGDSP_EINVAL;
    ARGS_TRY(ctx, "igdsp_rtcp_parse", args::rtcp_parse(d_packets, d_sizes, d_arrival, d_local_ssrc, C, F, pkt_stride, d_state, d_rec));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, launch_rtcp_parse(cfg_of(ctx, s), d_packets, d_sizes, d_arrival, d_local_ssrc, C, F, pkt_stride, d_state, d_rec, yardstick, s));
    return IGDSP_OK;
}

extern "C" {

// ---- RFC 3550 reports from the device's own statistics, and the peer's reports ----
int igdsp_rtcp_build(igdsp_ctx *ctx, const uint8_t *d_ctl, const igdsp_jb_state *d_jb, const igdsp_rtcp_src *d_src, const uint64_t *d_now, const uint8_t *d_cname,
                     const uint8_t *d_cname_len, uint32_t n_channels, uint32_t n_frames, igdsp_rtcp_state *d_state, uint8_t *d_packets, uint32_t pkt_stride,
                     uint16_t *d_sizes, igdsp_rtcp_built *d_rec, void *stream)
{
    return build_entry(ctx, d_ctl, d_jb, d_src, d_now, d_cname, d_cname_len, n_channels, n_frames, d_state, d_packets, pkt_stride, d_sizes, d_rec, stream, false);
}

int igdsp_rtcp_parse(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint32_t *d_arrival, const uint32_t *d_local_ssrc, uint32_t n_channels,
                     uint32_t n_frames, uint32_t pkt_stride, igdsp_rtcp_state *d_state, igdsp_rtcp_seen *d_rec, void *stream)
{
    return parse_entry(ctx, d_packets, d_sizes, d_arrival, d_local_ssrc, n_channels, n_frames, pkt_stride, d_state, d_rec, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardsticks of igdsp_rtcp_build and igdsp_rtcp_parse (tools/rtcp_bench.py),
// their arguments.  Build: the same loads, the size rule, a packet of that size filled with one loaded word, a record with the size and
// no flag; parse: the same loads, tile traffic and row reads, the record the size's verdict alone.  The state's words are stored as read.
int igdsp_internal_rtcp_build_move(igdsp_ctx *ctx, const uint8_t *d_ctl, const igdsp_jb_state *d_jb, const igdsp_rtcp_src *d_src, const uint64_t *d_now,
                                   const uint8_t *d_cname, const uint8_t *d_cname_len, uint32_t n_channels, uint32_t n_frames, igdsp_rtcp_state *d_state,
                                   uint8_t *d_packets, uint32_t pkt_stride, uint16_t *d_sizes, igdsp_rtcp_built *d_rec, void *stream)
{
    return build_entry(ctx, d_ctl, d_jb, d_src, d_now, d_cname, d_cname_len, n_channels, n_frames, d_state, d_packets, pkt_stride, d_sizes, d_rec, stream, true);
}

int igdsp_internal_rtcp_parse_move(igdsp_ctx *ctx, const uint8_t *d_packets, const uint16_t *d_sizes, const uint32_t *d_arrival, const uint32_t *d_local_ssrc,
                                   uint32_t n_channels, uint32_t n_frames, uint32_t pkt_stride, igdsp_rtcp_state *d_state, igdsp_rtcp_seen *d_rec, void *stream)
{
    return parse_entry(ctx, d_packets, d_sizes, d_arrival, d_local_ssrc, n_channels, n_frames, pkt_stride, d_state, d_rec, stream, true);
}

// ---- RFC 3711 3.4 on the packets of a batch ----
int igdsp_srtcp_protect(igdsp_ctx *ctx, const uint8_t *d_ctl, const uint8_t *d_packets, const uint16_t *d_sizes, uint32_t n_channels, uint32_t n_frames,
                        uint32_t pkt_stride, igdsp_srtp_state *d_state, uint8_t *d_out, uint32_t out_stride, uint16_t *d_sizes_out, igdsp_srtp_rec *d_rec,
                        void *stream)
{
    return srtcp_entry(ctx, "igdsp_srtcp_protect", kSrtpDirProtect, d_ctl, d_packets, d_sizes, n_channels, n_frames, pkt_stride, d_state, d_out, out_stride,
                       d_sizes_out, d_rec, stream, false);
}

int igdsp_srtcp_unprotect(igdsp_ctx *ctx, const uint8_t *d_ctl, const uint8_t *d_packets, const uint16_t *d_sizes, uint32_t n_channels, uint32_t n_frames,
                          uint32_t pkt_stride, igdsp_srtp_state *d_state, uint8_t *d_out, uint32_t out_stride, uint16_t *d_sizes_out, igdsp_srtp_rec *d_rec,
                          void *stream)
{
    return srtcp_entry(ctx, "igdsp_srtcp_unprotect", kSrtpDirUnprotect, d_ctl, d_packets, d_sizes, n_channels, n_frames, pkt_stride, d_state, d_out, out_stride,
                       d_sizes_out, d_rec, stream, false);
}

// Calibration-only (not in include/igdsp.h): the compute-free yardstick of igdsp_srtcp_protect — its piece loads, tile stores, row
// reads and writes, state load and store and output stores and the size rules; no AES round, no compression.  Arguments as
// igdsp_srtcp_protect; d_ctl is not read.  A packet protect would accept goes out unchanged with 14 zero bytes behind it and a BYPASSED
// record; the state's words are stored as read.
int igdsp_internal_srtcp_move(igdsp_ctx *ctx, const uint8_t *d_ctl, const uint8_t *d_packets, const uint16_t *d_sizes, uint32_t n_channels, uint32_t n_frames,
                              uint32_t pkt_stride, igdsp_srtp_state *d_state, uint8_t *d_out, uint32_t out_stride, uint16_t *d_sizes_out, igdsp_srtp_rec *d_rec,
                              void *stream)
{
    return srtcp_entry(ctx, "igdsp_srtcp_protect", kSrtpDirProtect, d_ctl, d_packets, d_sizes, n_channels, n_frames, pkt_stride, d_state, d_out, out_stride,
                       d_sizes_out, d_rec, stream, true);
}

// ---- host only
int igdsp_srtcp_derive(const uint8_t key_salt[30], uint32_t index0, igdsp_srtp_state *out)
{
    if (!key_salt || !out) return IGDSP_EINVAL;
    srtcp_derive(key_salt, index0, *out);
    return IGDSP_OK;
}

int igdsp_srtcp_protect_packet(igdsp_srtp_state *st, uint32_t ctl, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity, uint32_t *size_out,
                               igdsp_srtp_rec *rec)
{
    if (!st || !out || !size_out || (!in && size)) return IGDSP_EINVAL;
    igdsp_srtp_rec r;
    srtcp_packet_run<kSrtpProtect>(*st, ctl, in, size, kSrtpMaxPacket, out, out_capacity, *size_out, r);
    if (rec) *rec = r;
    return IGDSP_OK;
}

int igdsp_srtcp_unprotect_packet(igdsp_srtp_state *st, uint32_t ctl, const uint8_t *in, uint32_t size, uint8_t *out, uint32_t out_capacity, uint32_t *size_out,
                                 igdsp_srtp_rec *rec)
{
    if (!st || !out || !size_out || (!in && size)) return IGDSP_EINVAL;
    igdsp_srtp_rec r;
    srtcp_packet_run<kSrtpUnprotect>(*st, ctl, in, size, kSrtpMaxPacket, out, out_capacity, *size_out, r);
    if (rec) *rec = r;
    return IGDSP_OK;
}

int igdsp_rtcp_build_packet(igdsp_rtcp_state *st, uint32_t ctl, const igdsp_jb_state *jb, const igdsp_rtcp_src *src, uint64_t now, const uint8_t *cname,
                            uint32_t cname_len, uint8_t *out, uint32_t out_capacity, uint32_t *size_out, igdsp_rtcp_built *rec)
{
    if (!st || !src || !out || !size_out || out_capacity < (uint32_t)IGDSP_RTCP_MAX_BUILT) return IGDSP_EINVAL;
    igdsp_rtcp_built r;
    rtcp_build_run(*st, ctl, jb, *src, now, cname, cname_len, out, *size_out, r);
    if (rec) *rec = r;
    return IGDSP_OK;
}

int igdsp_rtcp_parse_packet(igdsp_rtcp_state *st, const uint8_t *in, uint32_t size, uint32_t arrival, uint32_t local_ssrc, igdsp_rtcp_seen *rec)
{
    if (!st || (!in && size)) return IGDSP_EINVAL;
    igdsp_rtcp_seen r;
    rtcp_parse_run(*st, in, size, kSrtpMaxPacket, arrival, local_ssrc, r);
    if (rec) *rec = r;
    return IGDSP_OK;
}

}  // extern "C"
