// igdsp_pitch.h — the integer pitch rules two stages share (include/igdsp.h: "Packet loss concealment" step 1, "Delay buffer" shrink):
// the AMDF search key over a window of IGDSP_PLC_HIST samples, the Q15 cross-fade weight and the Q15 rounding.  Plain C++17, constexpr:
// the kernels (k_plc, k_dbuf), the host entry igdsp_dbuf_step and tests/route/dbuf_route_driver.cpp run the same functions.  The
// wave-wide form of the search (one lag per lane, v_sad_u16 on biased samples in LDS) is pitch_search_wave, igdsp_device.h.
#pragma once
#include <cstdint>

#include "igdsp.h"

namespace igdsp {

static_assert(IGDSP_PLC_HIST == IGDSP_PLC_SPAN + IGDSP_PLC_PMAX, "the window holds the span and the longest lag in front of it");
static_assert(IGDSP_PLC_PMAX - IGDSP_PLC_PMIN + 1 <= 128, "the pitch fits 7 bits of the search key");

// w(i) of a cross-fade over q samples: ((i + 1) << 15) / (q + 1), 0 < w < 32768
constexpr int32_t pitch_w(uint32_t i, uint32_t q) { return (int32_t)(((i + 1u) << 15) / (q + 1u)); }
// Q15 product or blend to a sample: round half up, >> arithmetic (a floor)
constexpr int32_t pitch_q15(int32_t acc) { return (acc + 16384) >> 15; }
// the search key: the smallest key is the smallest D, and the smallest p among equal D (D <= 160 * 65535 < 2^24)
constexpr uint32_t pitch_key(uint32_t d, uint32_t p) { return d << 7 | p; }

// D(p) = sum_{i < SPAN} |z[PMAX + i] - z[PMAX + i - p]| over a window z[0 .. HIST), oldest first
constexpr uint32_t pitch_amdf(const int16_t *z, uint32_t p)
{
    uint32_t d = 0;
    for (uint32_t i = 0; i < (uint32_t)IGDSP_PLC_SPAN; ++i) {
        const int32_t e = (int32_t)z[IGDSP_PLC_PMAX + i] - (int32_t)z[IGDSP_PLC_PMAX + i - p];
        d += (uint32_t)(e < 0 ? -e : e);
    }
    return d;
}
// the period of the window: the lag in PMIN .. PMAX of the smallest key
constexpr uint32_t pitch_search(const int16_t *z)
{
    uint32_t best = ~0u;
    for (uint32_t p = IGDSP_PLC_PMIN; p <= (uint32_t)IGDSP_PLC_PMAX; ++p) {
        const uint32_t key = pitch_key(pitch_amdf(z, p), p);
        best = key < best ? key : best;
    }
    return best & 127u;
}

}  // namespace igdsp
