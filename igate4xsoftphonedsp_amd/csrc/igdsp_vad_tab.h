// igdsp_vad_tab.h — the voice detector's level table (include/igdsp.h, "Voice activity"): T8[d] = floor(2^34 * 10^(-d / 10) + 1/2),
// d = 0 .. 127, as a list of constants: no libm call at run time, the same bits on the host and on the device.  2^34 is the largest
// energy per sample in the v domain times 2^8: level(e) compares (e << 8) with n * T8[d].  tests/test_vad_cpu.py recomputes the 128
// values with decimal arithmetic and pins their SHA-256 as little-endian uint64.  The list initialises kVadT8 (igdsp_vad.h, host) and
// the device copy in igdsp_k_vad.hip.
#pragma once
#define IGDSP_VAD_T8_VALUES \
    17179869184ull, 13646455162ull, 10839764639ull, 8610331110ull, 6839429111ull, 5432751653ull, 4315388030ull, 3427834556ull, \
    2722825772ull, 2162817389ull, 1717986918ull, 1364645516ull, 1083976464ull, 861033111ull, 683942911ull, 543275165ull, \
    431538803ull, 342783456ull, 272282577ull, 216281739ull, 171798692ull, 136464552ull, 108397646ull, 86103311ull, \
    68394291ull, 54327517ull, 43153880ull, 34278346ull, 27228258ull, 21628174ull, 17179869ull, 13646455ull, \
    10839765ull, 8610331ull, 6839429ull, 5432752ull, 4315388ull, 3427835ull, 2722826ull, 2162817ull, \
    1717987ull, 1364646ull, 1083976ull, 861033ull, 683943ull, 543275ull, 431539ull, 342783ull, \
    272283ull, 216282ull, 171799ull, 136465ull, 108398ull, 86103ull, 68394ull, 54328ull, \
    43154ull, 34278ull, 27228ull, 21628ull, 17180ull, 13646ull, 10840ull, 8610ull, \
    6839ull, 5433ull, 4315ull, 3428ull, 2723ull, 2163ull, 1718ull, 1365ull, \
    1084ull, 861ull, 684ull, 543ull, 432ull, 343ull, 272ull, 216ull, \
    172ull, 136ull, 108ull, 86ull, 68ull, 54ull, 43ull, 34ull, \
    27ull, 22ull, 17ull, 14ull, 11ull, 9ull, 7ull, 5ull, \
    4ull, 3ull, 3ull, 2ull, 2ull, 1ull, 1ull, 1ull, \
    1ull, 1ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, \
    0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, \
    0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull
