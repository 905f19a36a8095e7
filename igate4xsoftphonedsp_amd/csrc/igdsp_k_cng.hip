// igdsp_k_cng.hip — comfort noise from RFC 3389 SIDs (igdsp_cng_run): per channel and frame either the leg's voice row passed through or a
// row of synthetic noise at the held payload's level and spectral shape.  Semantics: include/igdsp.h, section "Comfort noise"; the
// rule's arithmetic: igdsp_cng.h (igdsp_cng_frame runs the same functions on the host); independent restatement: tests/cng_model.py.
//
// Shape (route: cng_route).  The lattice is ten dependent stages per sample and serial in the sample, so the parallelism is across
// channels: a lane owns a channel for the launch's frames, with b[10], kq[10], the gain and the counters in registers (cng_sample's
// stage loop has constant bounds and unrolls: no register array is indexed at run time, no scratch).  A block is one wave.  Per frame:
//   - the lane reads its kind and payload length (the next frame's are in flight), classifies the frame and, behind a wave-uniform
//     ballot, takes a SID: the payload's 16-byte load, ten 64-bit products and an integer square root, rare;
//   - each lane says in LDS who fills its row: nobody (zeros), the wave (a voice row) or the lane (noise);
//   - the wave fills the voice rows of the tile: 16 bytes of PCM or 8 of codes per lane and turn, consecutive in memory, four
//     turns' loads in flight at once (skipped, wave-uniform, when no row is voice);
//   - the lanes that generate run the sample loop (skipped, wave-uniform, when none does) and store a sample pair per dword into their
//     row of the tile; the excitation of a sample depends on nothing but its index, so it issues ahead of the chain;
//   - the wave stores the tile as 16-byte pieces, consecutive in memory (a lane-per-channel store of the rows would be uncoalesced);
//   - with d_stats the lane folds its row from the tile (pcm_acc2, the PCM record of igdsp_pcmrec.h); record, length and stats are one
//     store per lane, consecutive across the wave.
// The state is 24 dwords per lane, loaded once and stored once.
// COPY (the compute-free yardstick, tools/cng_bench.py): every channel as under BYPASS, so the same kind, length, voice-row loads and
// decode, tile stores and reads, state load and store and output stores; a row that is not voice is written to the tile by its lane as
// zeros (the LDS traffic of a generated row); no excitation, lattice, gain step or SID step; d_ctl and the payloads are not read.
// The tile's addressing (tile_item, tile_piece) and the G.711 piece (g711_decode8) are igdsp_lanes.h's.
// Everything is written with vector stores in plain C++.
#include "igdsp_cng.h"
#include "igdsp_lanes.h"

namespace igdsp {

__device__ const uint32_t d_cng_g[128] = {IGDSP_CNG_G_VALUES};

struct CngArgs {
    const uint8_t *kind, *sid, *sid_len, *g711, *codec;
    const int16_t *pcm;
    const uint8_t *ctl;
    const uint32_t *seed;
    uint32_t C, F, n, passes, inv;
    igdsp_cng_state *state;
    int16_t *out;
    uint16_t *len_out;
    igdsp_cng_rec *rec;
    igdsp_frame_stats *stats;
};

constexpr uint32_t kCngRowZero = 0, kCngRowVoice = 1, kCngRowLane = 2;    // who fills a row of the tile (bits 0..1 of its byte)
constexpr uint32_t kCngRowAlaw = 4;                                       // and its law, for the wave that decodes it

template <int IN, bool COPY>
__global__ __launch_bounds__(64) void k_cng(const CngArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t cng_lds[];
    const uint32_t lane = threadIdx.x, n = a.n, P = n >> 3, stride = tile_row_dwords(n);
    uint32_t *tile = cng_lds;                                              // [kCngChans][stride]
    uint8_t *who = reinterpret_cast<uint8_t *>(cng_lds + kCngChans * stride);   // [kCngChans]
    const uint64_t c0 = (uint64_t)blockIdx.x * kCngChans;                  // < C: the grid
    const uint32_t rows = (uint32_t)((uint64_t)a.C - c0 < kCngChans ? (uint64_t)a.C - c0 : kCngChans), items = rows * P;
    const bool chan = lane < rows;
    const uint32_t c = chan ? (uint32_t)c0 + lane : a.C - 1u;              // lanes past the end load the last channel and store nothing
    const bool alaw = IN == kCngG711 && a.codec[c] == IGDSP_PT_PCMA;
    uint32_t ctl = COPY ? (uint32_t)IGDSP_CNG_BYPASS : (a.ctl ? cng_ctl(a.ctl[c]) : (uint32_t)IGDSP_CNG_RUN);

    // ---- the state: six 16-byte loads per lane (d_state 16-byte aligned: the argument rule)
    uint32_t sw[kCngStateWords];
    {
        const uint4 *sp = reinterpret_cast<const uint4 *>(a.state + c);
#pragma unroll
        for (uint32_t i = 0; i < 6u; ++i) {
            const uint4 v = sp[i];
            sw[4u * i] = v.x; sw[4u * i + 1u] = v.y; sw[4u * i + 2u] = v.z; sw[4u * i + 3u] = v.w;
        }
    }
    const bool reset = ctl == IGDSP_CNG_RESET, is_reset = cng_is_reset(sw[0], reset);
    CngRun r = cng_read(sw, reset, is_reset && a.seed ? a.seed[c] : 0u);
    uint32_t flags = is_reset ? 0u : (sw[21] >> 8) & 0xFFu;               // the yardstick writes them back as read
    if (reset) ctl = IGDSP_CNG_RUN;
    const bool bypass = ctl == IGDSP_CNG_BYPASS, frozen = ctl == IGDSP_CNG_FREEZE;
    const uint32_t hs = cng_mix(r.seed);
    uint32_t *row = tile + lane * stride;                                  // lane < kCngChans = 64: the block is one wave

    uint32_t kind_n = a.kind[c], slen_n = a.sid_len ? a.sid_len[c] : 11u;
    for (uint32_t f = 0; f < a.F; ++f) {
        const uint32_t o = f * a.C + c;                                    // < 2^32 - 32: the argument rule
        const uint64_t t0 = (uint64_t)f * a.C + c0;                        // the tile's first row
        const uint32_t kind = kind_n, len = cng_len(slen_n);
        if (f + 1u < a.F) { kind_n = a.kind[o + a.C]; slen_n = a.sid_len ? a.sid_len[o + a.C] : 11u; }   // in flight during the frame

        // ---- steps 1 and 2; the SID step behind a wave-uniform test
        bool take = false;
        const uint32_t cls = cng_classify(kind, frozen, len, take);
        const bool voice_row = IN != kCngNone && (cls & IGDSP_CNG_F_VOICE) != 0u;
        if constexpr (!COPY) {
            if (!bypass) {
                take = take && chan;
                if (__builtin_amdgcn_ballot_w64(take) != 0u) {
                    if (take) {
                        const uint4 pay = reinterpret_cast<const uint4 *>(a.sid)[o];
                        const uint32_t pw[3] = {pay.x, pay.y, pay.z}, level = pay.x & 0xFFu;
                        const uint32_t sp = cng_model(pw, len, r.kq);
                        cng_take(r, level, len, d_cng_g[level < 127u ? level : 127u], sp);
                    }
                }
                flags = cng_step(r, cls, take);
            } else {
                flags = (uint32_t)IGDSP_CNG_F_BYPASSED;
            }
        }
        const bool gen = !COPY && chan && !bypass && (flags & IGDSP_CNG_F_GENERATED) != 0u;
        const bool own = COPY ? chan && !voice_row : gen;                       // the lane writes its row itself
        who[lane] = (uint8_t)((voice_row ? kCngRowVoice : (own ? kCngRowLane : kCngRowZero)) | (alaw ? kCngRowAlaw : 0u));
        wave_lds_fence();

        // ---- the voice rows, wave-wide: item i is piece i % P of row i / P, 16 bytes of the tile's memory.  kCngBatch turns of loads are
        // issued before the first is used: with one wave per SIMD nothing else hides a load's latency
        if (IN != kCngNone && __builtin_amdgcn_ballot_w64(voice_row && chan) != 0u) {
            constexpr uint32_t kCngBatch = 4u;                             // (eight turns of codes took the G.711 form past 128 VGPRs)
            for (uint32_t it0 = 0; it0 < a.passes; it0 += kCngBatch) {
                uint4 v[kCngBatch];
                uint32_t wh[kCngBatch];
#pragma unroll
                for (uint32_t u = 0; u < kCngBatch; ++u) {
                    const uint32_t i = (it0 + u) * 64u + lane;
                    wh[u] = i < items ? who[tile_item(i, a.inv, P).row] : (uint32_t)kCngRowZero;   // items <= 64 passes: a turn past the last holds no item
                    v[u] = make_uint4(0u, 0u, 0u, 0u);
                    if ((wh[u] & 3u) == kCngRowVoice) {
                        if constexpr (IN == kCngG711) {
                            const uint2 q = reinterpret_cast<const uint2 *>(a.g711 + t0 * n)[i];
                            v[u].x = q.x; v[u].y = q.y;
                        } else {
                            v[u] = reinterpret_cast<const uint4 *>(a.pcm + t0 * n)[i];
                        }
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < kCngBatch; ++u) {
                    const uint32_t i = (it0 + u) * 64u + lane;
                    if ((wh[u] & 3u) == kCngRowVoice) {
                        const uint4 x = IN == kCngG711 ? g711_decode8(v[u].x, v[u].y, (wh[u] & kCngRowAlaw) != 0u) : v[u];
                        uint32_t *d = tile_piece(tile, stride, tile_item(i, a.inv, P));
                        d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
                    }
                }
            }
        }
        // ---- step 5's sample loop, lane per channel
        if constexpr (COPY) {
            if (own)
                for (uint32_t j = 0; j < n; j += 2u) row[j >> 1] = 0u;
        } else if (__builtin_amdgcn_ballot_w64(gen) != 0u) {
            if (gen) {
                uint32_t clip = 0u;
                for (uint32_t j = 0; j < n; j += 2u) {
                    const int32_t e0 = cng_exc(r.ctr + j, hs), e1 = cng_exc(r.ctr + j + 1u, hs);
                    const int32_t o0 = cng_out(cng_sample(e0, (int32_t)r.g, r.b, r.kq));
                    const int32_t o1 = cng_out(cng_sample(e1, (int32_t)r.g, r.b, r.kq));
                    clip |= (uint32_t)(cng_clips(o0) || cng_clips(o1));
                    row[j >> 1] = ((uint32_t)o0 & 0xFFFFu) | ((uint32_t)o1 << 16);
                }
                if (clip) flags |= (uint32_t)IGDSP_CNG_F_CLIPPED;
            }
        }
        if (!COPY && !bypass) r.ctr += n;
        wave_lds_fence();

        // ---- the tile goes out, wave-wide; a row nobody filled goes out as zeros
        {
            uint4 *dst = reinterpret_cast<uint4 *>(a.out + t0 * n);       // d_out 16-byte aligned, n a multiple of 8: the argument rule
            for (uint32_t it = 0; it < a.passes; ++it) {
                const uint32_t i = it * 64u + lane;
                const TileItem t = tile_item(i, a.inv, P);
                if (i < items) {
                    uint4 v = make_uint4(0u, 0u, 0u, 0u);
                    if ((who[t.row] & 3u) != kCngRowZero) {
                        const uint32_t *s = tile_piece(tile, stride, t);
                        v = make_uint4(s[0], s[1], s[2], s[3]);
                    }
                    dst[i] = v;
                }
            }
        }
        // ---- length, record, stats: one store per lane
        const bool live = voice_row || gen;
        if (chan) {
            if (a.len_out) a.len_out[o] = (uint16_t)(live ? n : 0u);
            if (a.rec) {
                uint32_t w[4];
                cng_pack_rec(r, COPY ? (uint32_t)IGDSP_CNG_F_BYPASSED : flags, w);
                *reinterpret_cast<uint4 *>(a.rec + o) = make_uint4(w[0], w[1], w[2], w[3]);
            }
            if (a.stats) {
                uint4 rec = pcm_record_empty();
                if (live) {
                    uint64_t sq = 0u;
                    v2u16_t pk2 = (v2u16_t)(0);
                    for (uint32_t j = 0; j < n / 2u; ++j) pcm_acc2(row[j], sq, pk2);
                    rec = pcm_record(sq, max((uint32_t)pk2.x, (uint32_t)pk2.y), n, 0u);
                }
                *reinterpret_cast<uint4 *>(a.stats + o) = rec;
            }
        }
        wave_lds_fence();                                                  // the next frame overwrites the tile
    }

    // ---- the state goes back once; a bypassed channel's bytes are not touched (the yardstick writes the state as it was read)
    if (chan && (COPY || !bypass)) {
        cng_write(r, flags, sw);
        uint4 *sp = reinterpret_cast<uint4 *>(a.state + c);
#pragma unroll
        for (uint32_t i = 0; i < 6u; ++i) sp[i] = make_uint4(sw[4u * i], sw[4u * i + 1u], sw[4u * i + 2u], sw[4u * i + 3u]);
    }
}

hipError_t launch_cng(const LaunchCfg &, const uint8_t *kind, const uint8_t *sid, const uint8_t *sid_len, const uint8_t *g711, const uint8_t *codec,
                      const int16_t *pcm, const uint8_t *ctl, const uint32_t *seed, uint32_t C, uint32_t F, uint32_t n, igdsp_cng_state *state,
                      int16_t *out, uint16_t *len_out, igdsp_cng_rec *rec, igdsp_frame_stats *stats, bool yardstick, hipStream_t s)
{
    const CngRoute r = cng_route(C, F, n, g711 != nullptr, pcm != nullptr, yardstick);
    if (r.grid == 0) return hipSuccess;
    const CngArgs a{kind, sid, sid_len, g711, codec, pcm, ctl, seed, C, F, n, r.passes, r.inv, state, out, len_out, rec, stats};
    with_key(Keys<kCngNone, kCngG711, kCngPcm>{}, r.in, [&](auto IN) {
        with_bool(r.copy, [&](auto Y) { hipLaunchKernelGGL((k_cng<IN, Y>), dim3(r.grid), dim3(r.threads), r.lds, s, a); });
    });
    return hipGetLastError();
}

}  // namespace igdsp
