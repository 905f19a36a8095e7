// igdsp_k_snd.hip — the sound-card splitter / combiner (igdsp_snd_combine, igdsp_snd_split): pjmedia's splitcomb between the bridge's
// ports and the card (initSlaveSoundCard, roip_ed137.cpp:3314-3435), batched over frames and cards, with the per-channel VU records.
// Semantics: include/igdsp.h, section "Sound-card splitter / combiner"; independent restatement: tests/snd_model.py.
//
// Shape (snd_route, igdsp_route.h).  An item is one card-frame: K * n * 2 contiguous bytes at the same offset of both buffers.  A wave
// takes kSndU consecutive items: it issues the loads of all of them (kSndU x kSndLanePieces 16-byte pieces per lane in flight), then
// passes them one at a time through its 4 KiB LDS tile.  The tile always holds the item row-major ([k][s]):
//   combine: the pieces go into the tile as they were loaded (16-byte LDS stores); a lane builds each output piece from eight 2-byte
//            LDS reads and stores it.
//   split:   a lane scatters the eight samples of each loaded piece into the tile (2-byte LDS stores); the output pieces are 16-byte
//            LDS reads, stored as they are.
// Where the eight samples of a piece sit in the tile depends on the piece alone, not on the item: a lane works out the 32 slots of its
// four pieces once per launch (snd_slots: one snd_div per piece, then a (k, s) walk) and keeps them in registers, so the per-item
// work of a sample is one LDS access and half a pack.  No lane is masked in the LDS phases: samples past the item go to a dump slot
// behind its data, inside the wave's own tile.
// The records come from the tile: lane (k = lane >> 3, j = lane & 7) sums row k's 16-byte chunks j, j + 8, .. (n % 8 == 0, packed
// 16-bit math) or samples j, j + 8, .. (any n), three row_shr DPP steps fold the eight lanes of a row, and lane j == 7 stores row k's
// record: the K records of an item are one contiguous run.  Integer sums: any order gives the same bits.  Nothing is read back from
// memory.  The general form (K * n odd, or a buffer aligned to 2 only) fills and empties the same tile a sample at a time.
#include "igdsp_device.h"
#include "igdsp_pcmrec.h"

namespace igdsp {

static_assert(kSndTileBytes == 4096u && kSndLanePieces == 4u, "a lane holds an item in four 16-byte pieces");
static_assert(kSndWaves >= 1 && kSndWaves <= 16 && kSndU >= 1 && kSndU <= 8, "block size and register budget");

struct SndArgs {
    const int16_t *in;
    int16_t *out;
    igdsp_frame_stats *stats;
    uint32_t K, n, nk;                 // nk = n * K samples per item
    uint32_t items;                    // F * D
    uint32_t pieces, tail_dwords;      // vector form (SndRoute)
    uint32_t magic_k;                  // snd_div_magic(K)
};

// a piece of `dwords` (1 .. 4) dwords at dword alignment; the dwords past it read as 0
__device__ __forceinline__ uint4 snd_ld(const uint8_t *p, uint32_t dwords)
{
    if (dwords == 4u) return ld16_dw(p);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
    uint4 v = make_uint4(q[0], 0u, 0u, 0u);
    if (dwords > 1u) v.y = q[1];
    if (dwords > 2u) v.z = q[2];
    return v;
}
__device__ __forceinline__ void snd_st(uint8_t *p, uint32_t dwords, const uint4 v)
{
    if (dwords == 4u) {
        u32x4_a4_t t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
        *reinterpret_cast<u32x4_a4_t *>(p) = t;
        return;
    }
    uint32_t *q = reinterpret_cast<uint32_t *>(p);
    q[0] = v.x;
    if (dwords > 1u) q[1] = v.y;
    if (dwords > 2u) q[2] = v.z;
}

// The tile slots (byte offsets) of the eight interleaved samples r0 .. r0 + 7 of an item: r = s * K + k sits row-major at k * n + s.
// They depend on the piece alone, not on the item, so a lane works them out once per launch for each of its pieces.  Samples past
// the item (the rest of a last partial piece, and pieces past the item) get the `dump` slot behind the item's data: what is
// scattered there is never read, what is gathered from there is never stored.
__device__ __forceinline__ void snd_slots(const SndArgs &a, uint32_t r0, uint32_t dump, uint32_t (&slot)[8])
{
    uint32_t q = snd_div(min(r0, 4095u), a.magic_k), k = r0 - q * a.K, idx = k * a.n + q;
#pragma unroll
    for (uint32_t i = 0; i < 8u; ++i) {
        slot[i] = r0 + i < a.nk ? 2u * idx : dump;
        ++k; idx += a.n;
        if (k == a.K) { k = 0u; ++q; idx = q; }
    }
}
__device__ __forceinline__ uint4 snd_gather(const uint4 *tile, const uint32_t (&slot)[8])
{
    const uint8_t *t = reinterpret_cast<const uint8_t *>(tile);
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        o[i] = (uint32_t)*reinterpret_cast<const uint16_t *>(t + slot[2 * i]) | ((uint32_t)*reinterpret_cast<const uint16_t *>(t + slot[2 * i + 1]) << 16);
    return make_uint4(o[0], o[1], o[2], o[3]);
}
__device__ __forceinline__ void snd_scatter(uint4 *tile, const uint32_t (&slot)[8], const uint4 v)
{
    uint8_t *t = reinterpret_cast<uint8_t *>(tile);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<uint16_t *>(t + slot[2 * i]) = (uint16_t)w[i];
        *reinterpret_cast<uint16_t *>(t + slot[2 * i + 1]) = (uint16_t)(w[i] >> 16);
    }
}

// The K records of item `item` from its row-major tile (every lane of the wave active).
__device__ __forceinline__ void snd_records(const SndArgs &a, const uint4 *tile, uint64_t item, uint32_t lane)
{
    const uint16_t *tile16 = reinterpret_cast<const uint16_t *>(tile);
    const uint32_t k = lane >> 3, j = lane & 7u, n = a.n;
    uint64_t sq = 0;                                                               // <= 32 samples of a lane: < 2^35
    uint32_t pk = 0;
    if (k < a.K) {
        if ((n & 7u) == 0u) {                                                      // rows start on 16 bytes
            const uint4 *row = tile + ((k * n) >> 3);
            v2u16_t pk2 = (v2u16_t)(0);
            for (uint32_t c = j; c < (n >> 3); c += 8u) {
                const uint4 v = row[c];
                pcm_acc2(v.x, sq, pk2); pcm_acc2(v.y, sq, pk2); pcm_acc2(v.z, sq, pk2); pcm_acc2(v.w, sq, pk2);
            }
            pk = max((uint32_t)pk2.x, (uint32_t)pk2.y);
        } else {
            for (uint32_t s = j; s < n; s += 8u) pcm_acc(tile16[k * n + s], sq, pk);
        }
    }
    const uint2 limbs = group_limbs<8>(sq);                                        // lane 8 k + 7 gets row k's
    pk = group_fold<8>(pk, OpMax{});
    if (j == 7u && k < a.K) {
        // pcm_record's steps one by one, the sum joined in the storing lane: in this order k_snd compiles to the instructions it had;
        // as one pcm_record(group_sum_u64<8>(sq), ..) call the vector forms scheduled differently and S1 split measured 0.4 % slower
        // (profiles/pcm_record_isa.md)
        const uint64_t sumsq = limbs_u64(limbs);
        const float rms = pcm_rms(sumsq, n);
        const uint32_t flags = pcm_flags(pk, 0u);
        st_record_block(a.stats + item * a.K, k, pcm_pack(sumsq, rms, pk, flags));
    }
}

template <int DIR, int MODE, bool VEC>
__global__ __launch_bounds__(kSndWaves * 64) void k_snd(const SndArgs a)
{
    constexpr bool COPY = MODE == kSndCopy, BULK = MODE != kSndStats, STATS = MODE == kSndBoth || MODE == kSndStats;
    __shared__ __attribute__((aligned(16))) uint4 tiles[COPY ? 1 : kSndWaves][COPY ? 1 : kSndTileBytes / 16u];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint4 *tile = tiles[COPY ? 0 : w];
    uint16_t *tile16 = reinterpret_cast<uint16_t *>(tile);
    (void)tile16;
    const uint64_t item_bytes = 2ull * a.nk;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(a.in);
    uint8_t *out = reinterpret_cast<uint8_t *>(a.out);
    const uint64_t n_groups = ((uint64_t)a.items + kSndU - 1u) / kSndU, stride = (uint64_t)gridDim.x * kSndWaves;
    // vector form: the last piece of an item and its dwords; the tile slots of the lane's pieces
    const uint32_t last = a.pieces - 1u, last_dwords = a.tail_dwords ? a.tail_dwords : 4u;
    uint32_t slot[VEC && !COPY ? kSndLanePieces : 1][8];
    if constexpr (VEC && !COPY) {
        const uint32_t dump = min(2u * a.nk, kSndTileBytes - 2u);
#pragma unroll
        for (uint32_t jj = 0; jj < kSndLanePieces; ++jj) snd_slots(a, 8u * (lane + 64u * jj), dump, slot[jj]);
    }
    (void)last; (void)last_dwords; (void)slot;
    for (uint64_t g = (uint64_t)blockIdx.x * kSndWaves + w; g < n_groups; g += stride) {
        const uint64_t it0 = g * kSndU;
        const uint32_t cnt = (uint32_t)min((uint64_t)kSndU, a.items - it0);
        if constexpr (VEC) {
            uint4 v[kSndU][kSndLanePieces];
#pragma unroll
            for (int u = 0; u < kSndU; ++u) {
#pragma unroll
                for (uint32_t jj = 0; jj < kSndLanePieces; ++jj) {
                    const uint32_t p = lane + 64u * jj;
                    v[u][jj] = make_uint4(0u, 0u, 0u, 0u);
                    if ((uint32_t)u < cnt && p < a.pieces) v[u][jj] = snd_ld(in + (it0 + u) * item_bytes + 16u * p, p == last ? last_dwords : 4u);
                }
            }
#pragma unroll
            for (int u = 0; u < kSndU; ++u) {
                if ((uint32_t)u >= cnt) break;                                     // wave-uniform
                const uint64_t item = it0 + u;
                uint8_t *dst = out + item * item_bytes;
                if constexpr (COPY) {
#pragma unroll
                    for (uint32_t jj = 0; jj < kSndLanePieces; ++jj) {
                        const uint32_t p = lane + 64u * jj;
                        if (p < a.pieces) snd_st(dst + 16u * p, p == last ? last_dwords : 4u, v[u][jj]);
                    }
                } else {
                    // (a round of 64 pieces is skipped as a whole where the item has none of them; within a round every lane takes part:
                    // pieces past the item land behind its data, inside the wave's own tile)
#pragma unroll
                    for (uint32_t jj = 0; jj < kSndLanePieces; ++jj) {
                        if (64u * jj >= a.pieces) break;                           // wave-uniform
                        if (DIR == kSndCombine) tile[lane + 64u * jj] = v[u][jj];
                        else snd_scatter(tile, slot[jj], v[u][jj]);
                    }
                    wave_sync();
                    if constexpr (BULK) {
#pragma unroll
                        for (uint32_t jj = 0; jj < kSndLanePieces; ++jj) {
                            const uint32_t p = lane + 64u * jj;
                            if (64u * jj >= a.pieces) break;                       // wave-uniform
                            const uint4 o = DIR == kSndCombine ? snd_gather(tile, slot[jj]) : tile[p];
                            if (p < a.pieces) snd_st(dst + 16u * p, p == last ? last_dwords : 4u, o);
                        }
                    }
                    if constexpr (STATS) snd_records(a, tile, item, lane);
                    wave_sync();                                                   // the next item overwrites the tile
                }
            }
        } else {
            for (uint32_t u = 0; u < cnt; ++u) {
                const uint64_t item = it0 + u;
                const uint16_t *src16 = reinterpret_cast<const uint16_t *>(in + item * item_bytes);
                uint16_t *dst16 = reinterpret_cast<uint16_t *>(out + item * item_bytes);
                if constexpr (COPY) {
                    for (uint32_t e = lane; e < a.nk; e += 64u) dst16[e] = src16[e];
                } else {
                    for (uint32_t e = lane; e < a.nk; e += 64u) {
                        const uint32_t q = snd_div(e, a.magic_k);
                        tile16[DIR == kSndCombine ? e : (e - q * a.K) * a.n + q] = src16[e];
                    }
                    wave_sync();
                    if constexpr (BULK) {
                        for (uint32_t e = lane; e < a.nk; e += 64u) {
                            const uint32_t q = snd_div(e, a.magic_k);
                            dst16[e] = tile16[DIR == kSndCombine ? (e - q * a.K) * a.n + q : e];
                        }
                    }
                    if constexpr (STATS) snd_records(a, tile, item, lane);
                    wave_sync();
                }
            }
        }
    }
}

hipError_t launch_snd(const LaunchCfg &cfg, int dir, const int16_t *in, uint32_t D, uint32_t K, uint32_t F, uint32_t n, int16_t *out,
                      igdsp_frame_stats *stats, bool yardstick, hipStream_t s)
{
    const SndRoute r = snd_route(D, K, F, n, out != nullptr, stats != nullptr, yardstick, reinterpret_cast<uintptr_t>(in),
                                 reinterpret_cast<uintptr_t>(out), (uint32_t)cfg.compute_units);
    if (r.grid == 0) return hipSuccess;
    if (yardstick && out == nullptr) return hipErrorInvalidValue;                  // the yardstick moves bulk bytes only
    const SndArgs a{in, out, stats, K, n, n * K, r.items, r.pieces, r.tail_dwords, snd_div_magic(K)};
    with_bool(r.vec != 0u, [&](auto V) {
        if (r.mode == kSndCopy) {
            hipLaunchKernelGGL((k_snd<kSndCombine, kSndCopy, V>), dim3(r.grid), dim3(r.threads), 0, s, a);
            return;
        }
        with_key(Keys<kSndCombine, kSndSplit>{}, dir, [&](auto DIR) { with_key(Keys<kSndBoth, kSndBulk, kSndStats>{}, r.mode, [&](auto M) {
            hipLaunchKernelGGL((k_snd<DIR, M, V>), dim3(r.grid), dim3(r.threads), 0, s, a); }); });
    });
    return hipGetLastError();
}

}  // namespace igdsp
