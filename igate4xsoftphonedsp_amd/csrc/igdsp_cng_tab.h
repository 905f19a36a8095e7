// igdsp_cng_tab.h — the comfort-noise generator's gain table (include/igdsp.h, "Comfort noise"): G[d] = isqrt(T8[d]), d = 0 .. 127, the
// floor integer square root of the voice detector's level table (igdsp_vad_tab.h), as a list of constants: the rms of a -d dBov signal
// in Q2 (G[0] = 2^17), 0 from d = 106 on.  tests/test_cng_cpu.py recomputes the 128 values from T8 and pins their SHA-256 as
// little-endian uint32.  The list initialises kCngG (igdsp_cng.h, host) and the device copy in igdsp_k_cng.hip.
#pragma once
#define IGDSP_CNG_G_VALUES \
    131072u, 116818u, 104114u, 92791u, 82700u, 73707u, 65691u, 58547u, 52180u, 46506u, 41448u, 36941u, \
    32923u, 29343u, 26152u, 23308u, 20773u, 18514u, 16500u, 14706u, 13107u, 11681u, 10411u, 9279u, \
    8270u, 7370u, 6569u, 5854u, 5218u, 4650u, 4144u, 3694u, 3292u, 2934u, 2615u, 2330u, \
    2077u, 1851u, 1650u, 1470u, 1310u, 1168u, 1041u, 927u, 827u, 737u, 656u, 585u, \
    521u, 465u, 414u, 369u, 329u, 293u, 261u, 233u, 207u, 185u, 165u, 147u, \
    131u, 116u, 104u, 92u, 82u, 73u, 65u, 58u, 52u, 46u, 41u, 36u, \
    32u, 29u, 26u, 23u, 20u, 18u, 16u, 14u, 13u, 11u, 10u, 9u, \
    8u, 7u, 6u, 5u, 5u, 4u, 4u, 3u, 3u, 3u, 2u, 2u, \
    2u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 0u, 0u, \
    0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, \
    0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u
