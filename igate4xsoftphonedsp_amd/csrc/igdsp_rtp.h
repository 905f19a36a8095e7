// igdsp_rtp.h — the RTP header parse of transport_rtp_cb (TransportAdapter.cpp:240-292; header layout ed137_rtp.h:22-48) as
// igdsp_depayload records it: the payload length it keeps and the igdsp_rtp_info of the packet.  Shared by the depayload kernels
// (igdsp_k_packets.hip) and the jitter buffer (igdsp_k_jb.hip), whose PLAYED frames must be bit-identical to igdsp_depayload's.
#pragma once
#include "igdsp_device.h"

namespace igdsp {

struct FrameHdr { uint32_t len; igdsp_rtp_info info; };

__device__ __forceinline__ FrameHdr parse_rtp_words(uint32_t w0, uint32_t w3, uint32_t w4, uint32_t size, uint32_t hdr, bool radio, uint32_t n)
{
    // w0 = packet bytes 0-3, w3 = bytes 12-15 (extension profile / length), w4 = bytes 16-19 (ED-137 word); w3 / w4 are
    // only looked at for radio packets of at least 20 bytes
    FrameHdr r;
    r.len = 0; r.info.ed137 = 0; r.info.payload_len = 0; r.info.pt = 0; r.info.flags = 0;
    if (size < hdr) {
        r.info.flags = IGDSP_RTP_RUNT;
        if (size >= 2u) r.info.pt = (uint8_t)((w0 >> 8) & 0x7Fu);
        return r;
    }
    const uint32_t pt = (w0 >> 8) & 0x7Fu;
    uint32_t fl = (((w0 >> 6) & 3u) == 2u ? IGDSP_RTP_V2 : 0u) | ((w0 & 0x10u) ? IGDSP_RTP_X : 0u) | ((w0 & 0x8000u) ? IGDSP_RTP_MARKER : 0u);
    if (radio) {
        if (pt == 8u || pt == 0u || pt == 18u || pt == 123u) r.info.ed137 = __builtin_bswap32(w4);   // ntohl
        if ((w0 & 0x10u) && w3 == 0x01006701u) fl |= IGDSP_RTP_ED137_OK;                               // bytes 01 67 00 01
    }
    if (pt == 123u) fl |= IGDSP_RTP_KEEPALIVE;
    const uint32_t pl = size - hdr;
    if (pl > n) fl |= IGDSP_RTP_OVERSIZE;
    else if ((pt == 0u || pt == 8u) && pl > 0u) { fl |= IGDSP_RTP_METERED; r.len = pl; }
    r.info.pt = (uint8_t)pt; r.info.payload_len = (uint16_t)pl; r.info.flags = (uint8_t)fl;
    return r;
}

__device__ __forceinline__ FrameHdr parse_rtp(const uint8_t *pkt, uint32_t size, uint32_t hdr, bool radio, uint32_t n)
{
    const uint32_t *w = reinterpret_cast<const uint32_t *>(pkt);
    const bool wide = radio && size >= hdr;
    return parse_rtp_words(w[0], wide ? w[3] : 0u, wide ? w[4] : 0u, size, hdr, radio, n);
}

}  // namespace igdsp
