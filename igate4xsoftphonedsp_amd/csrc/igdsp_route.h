// igdsp_route.h — which kernel serves a shape, and with what geometry.  Host-only, plain C++17 (no HIP): the launchers in
// igdsp_k_*.hip call these functions and only launch what they return; tests/route/route_driver.cpp compiles them with g++
// and tests/test_route_cpu.py pins the routes.  Every route function is pure: the shape, the buffers' addresses (alignment
// only), the CU count and the env knobs (Knobs, read once per launcher call by knobs_from_env) go in, a route comes out.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <optional>
#include <type_traits>
#include <utility>

#include "igdsp.h"
#include "igdsp_rs_tab.h"
#include "igdsp_tone_tab.h"

namespace igdsp {

// ---- Geometry shared by the kernels and their routes

// Geometry of the tuned n == 160 path: a wavefront owns a super-chunk of 64 consecutive channel-frames
// (10 240 contiguous bytes), processed as two halves of 32 frames = 5120 bytes = 5 wave-wide 16 B/lane loads each.
constexpr int kFrame = IGDSP_SAMPLES_PER_FRAME;        // 160 B
constexpr int kChunkFrames = 32;
constexpr int kChunkBytes = kChunkFrames * kFrame;     // 5120
constexpr int kPiecesPerFrame = kFrame / 16;           // 10 x 16 B
constexpr int kPiecesPerChunk = kChunkFrames * kPiecesPerFrame;  // 320
constexpr int kLoadsPerChunk = kPiecesPerChunk / 64;   // 5
constexpr int kWavesPerBlock = 16;                     // 1024 threads, one block per CU
constexpr int kBlockThreads = kWavesPerBlock * 64;
constexpr int kSuperFrames = 2 * kChunkFrames;         // 64
constexpr int kLutEntries = 256 * 32;                  // the 32-replica expansion LUT, uint2 each
constexpr uint32_t kWinMaxSeg = 8;                     // igdsp_window_work_bytes = kWinMaxSeg x C x 48

// k_meter_chunk64 waves per block: 16 (1024 threads, 128 VGPRs) for the meter-only kernel: a read-heavy kernel wants every wave it can
// get, each has one super-chunk of loads in flight.  The PCM-store variant writes two bytes for every byte it reads, and a 1 : 2 mix is
// fastest with FEW resident waves per CU — 12 / 10 / 8 / 6 / 5 / 4 / 3 / 2 waves: 0.6706 / 0.6680 / 0.6636 / 0.6573 / 0.6520 / 0.6388 / 0.6995 /
// 1.013 ms in same-box A/B builds (late round 3; 12 had been chosen for its registers) — every wave is one more front of 20 KiB
// write bursts, and four already keep enough loads in flight.
#ifndef IGDSP_STORE_WAVES
#define IGDSP_STORE_WAVES 4
#endif
template <bool STORE_PCM> struct ChunkGeom { static constexpr int kWaves = STORE_PCM ? IGDSP_STORE_WAVES : kWavesPerBlock; };
constexpr int kFatWaves = 8;
constexpr uint32_t kImgMaxWaves = 12;          // 768 threads: up to 170 VGPRs, room for the sixteen piece registers of the next item
// k_meter_strided<Q, TAIL, AGG, STORE>, QP = Q + TAIL pieces per frame.
#ifndef IGDSP_SSTORE_WAVES
#define IGDSP_SSTORE_WAVES 0
#endif
// (the PCM-store variant, a 1 : 2 read : write mix, is fastest with few waves, as k_meter_chunk64<STORE>: 164-byte frames 12 / 8 / 6 / 5 / 4
// waves 0.7264 / 0.7133 / 0.7036 / 0.741 / 0.861 ms; 240: 10 / 8 / 6 / 5 / 4 0.9926 / 0.9865 / 0.980 / 0.9766 / 0.9975; 80: 12 / 10 / 8 / 6 0.3472 / 0.3462 / 0.3424 / 0.3402)
constexpr int strided_meter_waves(int qp, bool store) { return store ? (IGDSP_SSTORE_WAVES ? IGDSP_SSTORE_WAVES : (qp <= 2 ? 16 : 6)) : (qp <= 11 ? 16 : 12); }
template <int QP, bool STORE = false> struct StridedGeom { static constexpr int kWaves = strided_meter_waves(QP, STORE); };
constexpr int kTinyWaves = 16, kTinyDepth = 4;           // k_meter_tiny
// items per queue slot (>= kTinyDepth: the prologue).  16 made a wave's share two slots, i.e. static in effect; 32 / 16 / 8 / 4 items: 0.0683 /
// 0.0693 / 0.0682 / 0.0676 ms at 24-byte frames, 65 536 x 128 (same-box A/B builds, late round 3)
#ifndef IGDSP_TINY_SLOT
#define IGDSP_TINY_SLOT 4
#endif
constexpr uint32_t kTinySlot = IGDSP_TINY_SLOT;

// Waves per block of k_encode_lut16 (late round 3, same-box A/B builds): 16 / 14 / 12 / 10 / 8 / 6 / 4 → 0.651–0.662 / 0.650–0.658 / 0.641–0.642 /
// 0.636–0.637 / 0.646–0.648 / 0.770 / 1.05 ms.  The 2 : 1 read : write mix sits between the read-heavy kernels (the more waves the better) and the
// store / round-trip kernels (4–6): ten waves of 8 KiB chunks keep enough loads in flight, more only add write fronts.
#ifndef IGDSP_ENC_WAVES
#define IGDSP_ENC_WAVES 10
#endif
constexpr int kEncWaves = IGDSP_ENC_WAVES;
#ifndef IGDSP_RT_WAVES
#define IGDSP_RT_WAVES 12
#endif
constexpr int kRtWaves = IGDSP_RT_WAVES;                  // k_roundtrip_chunk64
#ifndef IGDSP_RTL_WAVES
#define IGDSP_RTL_WAVES 12
#endif
constexpr int kRtlWaves = IGDSP_RTL_WAVES;                // k_roundtrip_lut64, k_roundtrip_strided
constexpr int kRtbWaves = 12;                             // strips for up to 12 waves; the launcher starts fewer (rtb_waves)
constexpr int kRtsbWaves = 10;                            // the same for k_roundtrip_strided<BLK> (its strips and rings are larger)
constexpr int kRtpWaves = 12;                             // k_meter_rtp64: 64 KiB LUT + 84 KiB strips
constexpr int kTxWaves = 8;
constexpr int kTxCh = 16;                                 // k_tx_packetize: channels per wave
enum : int { kTxG711 = 0, kTxPcm = 1, kTxPcmTab = 2 };    // k_tx_packetize<FORM>

static inline uint32_t blocks_for(uint64_t items, uint32_t per_block, uint32_t cap)
{
    const uint64_t b = std::max<uint64_t>(1u, (items + per_block - 1) / per_block);
    return (uint32_t)(b > cap ? cap : b);
}

// ---- Env knobs (experiments and tests).  Read on every launcher call: the GPU tests set them between calls on one context.
struct Knobs {
    bool no_tiny = false, no_strided = false;      // IGDSP_NO_TINY / IGDSP_NO_STRIDED: set at all
    std::optional<int> img_waves;                  // IGDSP_IMG_WAVES
    std::optional<int> rt_order, rt_mid, rt_nseg, rt_gpb, rt_blk, rtb_waves;   // IGDSP_RT_ORDER / _MID / _NSEG / _GPB / _BLK, IGDSP_RTB_WAVES
    std::optional<int> win_nseg, win_gpb, win_blk, win_waves;                  // IGDSP_WIN_NSEG / _GPB / _BLK / _WAVES
};

inline Knobs knobs_from_env()
{
    auto num = [](const char *name) -> std::optional<int> {
        if (const char *e = std::getenv(name)) return std::atoi(e);
        return std::nullopt;
    };
    Knobs k;
    k.no_tiny = std::getenv("IGDSP_NO_TINY") != nullptr;
    k.no_strided = std::getenv("IGDSP_NO_STRIDED") != nullptr;
    k.img_waves = num("IGDSP_IMG_WAVES");
    k.rt_order = num("IGDSP_RT_ORDER"); k.rt_mid = num("IGDSP_RT_MID"); k.rt_nseg = num("IGDSP_RT_NSEG");
    k.rt_gpb = num("IGDSP_RT_GPB"); k.rt_blk = num("IGDSP_RT_BLK"); k.rtb_waves = num("IGDSP_RTB_WAVES");
    k.win_nseg = num("IGDSP_WIN_NSEG"); k.win_gpb = num("IGDSP_WIN_GPB"); k.win_blk = num("IGDSP_WIN_BLK"); k.win_waves = num("IGDSP_WIN_WAVES");
    return k;
}

// ---- Compile-time dispatch: a runtime choice among a fixed set of template arguments.  Only the listed values are instantiated.
template <class Fn> void with_bool(bool b, Fn &&fn) { b ? fn(std::true_type{}) : fn(std::false_type{}); }
// the compressor lineage: IGDSP_ENC_G191, or (anything else) IGDSP_ENC_SUN16
template <class Fn> void with_enc(int variant, Fn &&fn)
{
    variant == IGDSP_ENC_G191 ? fn(std::integral_constant<int, IGDSP_ENC_G191>{}) : fn(std::integral_constant<int, IGDSP_ENC_SUN16>{});
}
template <int... Ks> using Keys = std::integer_sequence<int, Ks...>;
template <int... Ks> constexpr bool has_key(Keys<Ks...>, int k) { return ((k == Ks) || ...); }
template <int... Ks, class Fn> void with_key(Keys<Ks...>, int k, Fn &&fn) { ((k == Ks ? (fn(std::integral_constant<int, Ks>{}), 0) : 0), ...); }

// The strided kernels are instantiated per (Q, TAIL): frames of Q 16-byte pieces plus, with TAIL, 4 or 8 bytes more.
constexpr int qt_key(uint32_t q, bool tail) { return (int)q * 2 + (tail ? 1 : 0); }
constexpr int key_q(int key) { return key / 2; }
constexpr bool key_tail(int key) { return (key & 1) != 0; }
// (15, true) = 244 / 248 bytes: 16 pieces x 12 waves of strip do not fit
using MeterStridedKeys = Keys<qt_key(1, false), qt_key(1, true), qt_key(4, false), qt_key(4, true), qt_key(5, false), qt_key(5, true),
                              qt_key(6, false), qt_key(6, true), qt_key(8, false), qt_key(8, true), qt_key(10, false), qt_key(10, true),
                              qt_key(12, false), qt_key(12, true), qt_key(15, false)>;
// with PCM output, and the round trip: the reference's own sizes (24, 80, 164 / 168, 240)
using ReferenceSizeKeys = Keys<qt_key(1, true), qt_key(5, false), qt_key(10, true), qt_key(10, false), qt_key(15, false)>;
using RoundtripStridedKeys = Keys<qt_key(1, true), qt_key(5, false), qt_key(10, true), qt_key(15, false)>;

constexpr bool aligned(uintptr_t p, uintptr_t a) { return (p & (a - 1u)) == 0u; }

// ---- Block-owned form (round trip and fused window): a block owns gpb = 1 << gsh consecutive channel groups of 64 for the launch.
// gpb: as many groups per block (<= 4: the LDS) as still give every CU a block; `force` (IGDSP_RT_GPB / IGDSP_WIN_GPB, tests) picks
// 1, 2 or 4 where it divides n_groups.
constexpr int kBlkCh = 256;                               // channels a block can own (7 dwords of LDS each: BlkHoldWindow, igdsp_device.h)
inline uint32_t groups_per_block(uint32_t n_groups, uint32_t cus, std::optional<int> force)
{
    static_assert(4 * kSuperFrames <= kBlkCh, "the kernels' LDS windows hold the channels of the largest gpb");
    uint32_t gpb = 1u;
    for (uint32_t g = 4u; g > 1u; g >>= 1) if (n_groups % g == 0u && n_groups / g >= cus) { gpb = g; break; }
    if (force) { const uint32_t g = (uint32_t)*force; if ((g == 1u || g == 2u || g == 4u) && n_groups % g == 0u) gpb = g; }
    return gpb;
}
inline uint32_t gpb_shift(uint32_t gpb) { return gpb == 4u ? 2u : (gpb == 2u ? 1u : 0u); }
inline uint32_t rounds_of(uint32_t blocks, uint32_t cus) { return (blocks + cus - 1u) / cus; }

// Where the block-owned round trip pays (65 536 channels = 256 blocks of four groups is the tuned case; measured around it, 128 frames,
// placed buffers, static / block-owned ms): 0.6 to 1 round of blocks — 10 240 ch 0.0863 / 0.0841, 12 288 ch 0.1108 / 0.0856.  Below 0.6 of a
// round the static form spreads its units over more CUs (8 192 ch 0.0754 / 0.0804, 4 096 ch 0.0649 / 0.0769); 1.5 rounds idle half the chip
// in the second (24 576 ch 0.2003 / 0.2099, 49 152 ch 0.3572 / 0.3769), and even two whole rounds lose to the static form, whose blocks
// stay (131 072 ch 0.9216 / 0.9311).
inline bool roundtrip_block_fills(uint32_t blocks, uint32_t cus) { return rounds_of(blocks, cus) == 1u && blocks * 10u >= cus * 6u; }

// Where the block-owned window pays: up to one round of blocks, and where the blocks fill whole rounds of the CUs to 85 % (a launch
// of 1.25 rounds would idle 3/8 of the chip in its second round: the register form has no such steps).  (Measured around the tuned
// 65 536 channels, register form / block form ms: 2 048 ch 0.0992 / 0.0658, 8 192 ch 0.1014 / 0.0685, 12 288 ch 0.1021 / 0.0705 — up
// to one round of blocks the block form always wins, the register form walks its segments serially — 24 576 ch 0.1218 / 0.1397,
// 49 152 ch 0.2332 / 0.2559: 1.5 rounds idle half the chip in the second.)
inline bool window_block_fills(uint32_t blocks, uint32_t cus)
{
    const uint32_t rounds = rounds_of(blocks, cus);
    return rounds == 1u || (uint64_t)blocks * 100u >= (uint64_t)rounds * cus * 85u;
}

// ---- igdsp_decode_meter (launch_decode_meter)
enum class MeterFast { none, fat, chunk, tiny, strided };
enum class MeterRest { none, image, wave_per_frame };
struct MeterRoute {
    MeterFast fast = MeterFast::none;
    bool store = false;              // chunk / strided: the PCM-storing instantiation
    int key = 0;                     // tiny: n / 4; strided: qt_key(Q, TAIL)
    uint32_t grid = 0, threads = 0;
    uint32_t done = 0;               // frames [0, done) go to the fast kernel, [done, C * F) to the rest kernel
    MeterRest rest = MeterRest::none;
    uint32_t rest_grid = 0, rest_threads = 0, rest_lds = 0;
};

// variant: the context's experiment variant (igdsp_set_variant: 1 = the general kernels only, 3 = k_meter_fat).
inline MeterRoute decode_meter_route(uint32_t C, uint32_t F, uint32_t n, int variant, bool has_len, uintptr_t payload, uintptr_t pcm,
                                     uintptr_t stats, uint32_t cus, const Knobs &k)
{
    MeterRoute r;
    if ((uint64_t)C * F == 0) return r;
    const uint32_t n_frames = C * F;
    const bool chunk_ok = n == (uint32_t)kFrame && !has_len && aligned(payload, 16) && aligned(pcm, 16) && aligned(stats, 16);
    // tuned path takes the whole super-chunks (64 frames); the < 64 remaining frames, and every shape it
    // does not cover, go through the rest kernel on the same stream.
    const uint32_t n_super = n_frames / kSuperFrames, whole = n_super * kSuperFrames;
    if (variant == 3 && chunk_ok && pcm == 0 && n_frames >= (uint32_t)kSuperFrames) {
        r.fast = MeterFast::fat;
        r.grid = blocks_for(n_super, kFatWaves, cus); r.threads = kFatWaves * 64; r.done = whole;
    } else if (variant != 1 && chunk_ok && n_frames >= (uint32_t)kSuperFrames) {
        const int w = pcm ? ChunkGeom<true>::kWaves : ChunkGeom<false>::kWaves;
        r.fast = MeterFast::chunk; r.store = pcm != 0;
        r.grid = blocks_for(n_super, w, cus); r.threads = w * 64; r.done = whole;
    }
    // 16 .. 32-byte frames, records only: a lane per frame (k_meter_tiny)
    if (r.done == 0 && variant != 1 && !has_len && pcm == 0 && (n & 3u) == 0u && n >= 16u && n <= 32u && n_frames >= (uint32_t)kSuperFrames &&
        aligned(payload, 4) && aligned(stats, 16) && !k.no_tiny) {
        r.fast = MeterFast::tiny; r.key = (int)(n >> 2);
        r.grid = blocks_for((n_super + kTinySlot - 1u) / kTinySlot, kTinyWaves, cus); r.threads = kTinyWaves * 64; r.done = whole;
    }
    // dense frames of 16 Q + 4 T bytes, Q in {1, 4, 5, 6, 8, 10, 12, 15}, T <= 2 (the reference's 164 / 24 and the 5 ms multiples
    // up to 240) keep the chunk pipeline: k_meter_strided.  With PCM output: the reference's own sizes (24, 80, 164 / 168, 240).
    // (160-byte frames land here only when their buffer is not 16-byte aligned.)
    if (r.done == 0 && variant != 1 && !has_len && (n & 3u) == 0u && n_frames >= (uint32_t)kSuperFrames && ((n >> 2) & 3u) != 3u && n >= 16u &&
        aligned(pcm, 4) && aligned(payload, 4) && aligned(stats, 16) && !k.no_strided) {
        const int key = qt_key(n >> 4, (n & 15u) != 0u);
        if (pcm ? has_key(ReferenceSizeKeys{}, key) : has_key(MeterStridedKeys{}, key)) {
            const int w = strided_meter_waves(key_q(key) + (key_tail(key) ? 1 : 0), pcm != 0);
            r.fast = MeterFast::strided; r.store = pcm != 0; r.key = key;
            r.grid = blocks_for(n_super, w, cus); r.threads = w * 64; r.done = whole;
        }
    }
    if (r.done < n_frames) {
        // what the fast kernels do not take: other frame sizes, ragged lengths, the < 64-frame tail.  Meter-only work with
        // n % 4 == 0 goes through the LDS-image kernel (every lane meters one frame); PCM output, n % 4 != 0 and unaligned
        // buffers through the literal wave-per-frame kernel.
        const bool image_ok = variant != 1 && pcm == 0 && (n & 3u) == 0u && aligned(stats, 16) && aligned(payload, 4) && n_frames - r.done >= 16u;
        if (image_ok) {
            const uint32_t img = (uint32_t)kSuperFrames * n;
            const uint32_t lut_bytes = (uint32_t)kLutEntries * 8u;
            uint32_t waves = std::max(1u, std::min(kImgMaxWaves, (160u * 1024u - lut_bytes - 2048u) / img));
            if (k.img_waves) waves = std::max(1u, std::min(waves, (uint32_t)*k.img_waves));   // experiments
            const uint32_t items = (n_frames - r.done + (uint32_t)kSuperFrames - 1u) / (uint32_t)kSuperFrames;
            r.rest = MeterRest::image;
            r.rest_grid = blocks_for(items, waves, cus); r.rest_threads = waves * 64u;
            r.rest_lds = waves * img;              // dynamic part: the images (the LUT is static)
        } else {
            r.rest = MeterRest::wave_per_frame;
            r.rest_grid = blocks_for((n_frames - r.done + 7) / 8, 4, cus * 8u); r.rest_threads = 256;
        }
    }
    return r;
}

// ---- igdsp_roundtrip_peakhold (launch_roundtrip)
enum class RtForm { none, lut64, chunk64, blk64, strided, strided_blk };
struct RtRoute {
    RtForm form = RtForm::none;
    int key = 0;                           // strided forms: qt_key(Q, TAIL)
    uint32_t grid = 0, threads = 0;
    uint32_t n_groups = 0;                 // whole groups of 64 channels the fused form takes
    uint32_t n_seg = 0, order = 0;         // register forms
    uint32_t gpb = 0, gsh = 0, mid_start = 0;      // block-owned forms
    uint32_t c_first = 0, gen_grid = 0;    // channels [c_first, C) go to k_roundtrip_general (256 threads), if any
};

// Waves per block of the block-owned round-trip kernels.  Unlike the read-heavy kernels (the more waves the better: each has one
// item of loads in flight) the 1 : 1 read / write mix is fastest with FEW resident waves per CU: at 160-byte frames 16 / 14 / 12 / 10
// / 8 / 6 / 4 / 3 waves ran 0.4613 / 0.4607 / 0.4580 / 0.4552 / 0.4522 / 0.4498 / 0.4519 / 0.4785 ms in same-box A/B builds.
inline uint32_t rtb_waves(uint32_t n, int max_waves, uint32_t gpb, const Knobs &k)
{
    // about 60 KB of loads in flight per CU: 6 waves at 160 bytes per frame, 4 at 240, 10 (the strips' limit) at 80 and below; the tailed
    // sizes want two more (164 bytes: 4 / 6 / 8 / 10 waves 0.6413 / 0.5146 / 0.4854 / 0.4915 ms; 240: 0.6636 / 0.6740 / 0.6746 / 0.6804)
    uint32_t w = n >= 200u ? 4u : (n > 160u ? 8u : (n >= 120u ? 6u : (n >= 48u ? 10u : 16u)));
    if (k.rtb_waves) w = (uint32_t)std::max(1, *k.rtb_waves);   // experiments
    return std::max(std::max(gpb, 1u), std::min(w, (uint32_t)max_waves));   // (a wave per owned group folds it at the block's end)
}

// Segments of the register forms: at least one work item per resident wave; a segment is never shorter than 8 frames, and
// the fused kernels count silent / clipped frames of a segment in 16 bits.
inline uint32_t roundtrip_segments(uint32_t n_groups, uint32_t F, uint32_t cus, int waves, std::optional<int> force)
{
    const uint32_t want = cus * (uint32_t)waves;
    uint32_t n_seg = n_groups >= want ? 1u : (want + n_groups - 1u) / n_groups;
    if (force) n_seg = (uint32_t)std::max(1, *force);   // experiments
    n_seg = std::max(1u, std::min(n_seg, std::max(1u, F / 8u)));
    return std::max(n_seg, F / 65535u + 1u);
}

// kernel_variant: the context's experiment variant (1 = the general kernel only, 4 = k_roundtrip_chunk64, kept for A/B runs).
inline RtRoute roundtrip_route(uint32_t C, uint32_t F, uint32_t n, int kernel_variant, uintptr_t payload, uintptr_t out, uintptr_t stats,
                               bool out_spread, uint32_t cus, const Knobs &k)
{
    RtRoute r;
    if ((uint64_t)C * F == 0) return r;
    // Item order of the register forms.  Consecutive groups per block pay when the output's halves lie in two memory classes
    // (0.4695 vs 0.4756 ms); with the whole output in one class it is the other way round (0.5116 vs 0.4920 ms): tools/rt_knobs.py,
    // alternating in one process.  IGDSP_RT_ORDER overrides (experiments, and the test of the order the placement would pick).
    const uint32_t order = k.rt_order ? (uint32_t)*k.rt_order : (out_spread ? 1u : 0u);
    // block-owned forms: odd blocks walk the frames from the middle (both halves of a spread output written at any moment)
    const uint32_t mid_start = k.rt_mid ? (*k.rt_mid != 0 ? 1u : 0u) : (out_spread ? 1u : 0u);   // (IGDSP_RT_MID: experiments)
    const uint32_t cus1 = std::max(1u, cus);
    // The fused channel-group-major kernels take whole groups of 64 channels of 160-byte frames in 16-byte aligned buffers
    // (k_roundtrip_lut64; kernel_variant 4: the compressor-cell-table form k_roundtrip_chunk64), and of the reference's other
    // frame sizes (24, 80, 164 / 168, 240) in dword-aligned buffers (k_roundtrip_strided).  The C % 64 channels left over, and
    // every other shape, go through k_roundtrip_general on the same stream.
    const uint32_t Tn = (n >> 2) & 3u;
    const int key = qt_key(n >> 4, Tn != 0u);
    const bool strided = kernel_variant != 1 && n != (uint32_t)kFrame && (n & 3u) == 0u && Tn != 3u && n >= 16u && aligned(payload | out, 4) &&
                         aligned(stats, 16) && has_key(RoundtripStridedKeys{}, key) && C >= (uint32_t)kSuperFrames;
    const bool fused160 = n == (uint32_t)kFrame && aligned(payload | out | stats, 16) && kernel_variant != 1 && C >= (uint32_t)kSuperFrames;
    if (strided || fused160) {
        const uint32_t n_groups = C / kSuperFrames;
        const int waves = kernel_variant == 4 && !strided ? kRtWaves : kRtlWaves;
        const uint32_t n_seg = roundtrip_segments(n_groups, F, cus, waves, strided ? std::nullopt : k.rt_nseg);
        // block-owned form: taken where roundtrip_block_fills says it pays and F fits the 16-bit silent / clipped counts
        const uint32_t gpb = groups_per_block(n_groups, cus1, k.rt_gpb);
        const uint32_t blocks = n_groups / gpb;
        const bool blk_ok = F <= 65535u && (strided || kernel_variant != 4);
        const bool blk = blk_ok && (k.rt_blk ? *k.rt_blk != 0 : roundtrip_block_fills(blocks, cus1));   // (IGDSP_RT_BLK: experiments and tests)
        r.n_groups = n_groups; r.c_first = n_groups * (uint32_t)kSuperFrames;
        if (strided) r.key = key;
        if (blk) {
            r.form = strided ? RtForm::strided_blk : RtForm::blk64;
            r.grid = blocks; r.gpb = gpb; r.gsh = gpb_shift(gpb); r.mid_start = mid_start;
            r.threads = rtb_waves(n, strided ? (key_q(key) <= 1 ? 16 : kRtsbWaves) : kRtbWaves, gpb, k) * 64u;
        } else {
            r.form = strided ? RtForm::strided : (kernel_variant == 4 ? RtForm::chunk64 : RtForm::lut64);
            r.grid = blocks_for((uint64_t)n_groups * n_seg, waves, cus); r.threads = waves * 64;
            r.n_seg = n_seg; r.order = order;
        }
    }
    if (C > r.c_first) r.gen_grid = blocks_for(C - r.c_first, 4, cus * 8u);
    return r;
}

// ---- igdsp_encode (launch_encode)
enum class EncForm { none, lut16, v8_table, v8, scalar };
struct EncRoute {
    EncForm form = EncForm::none;
    uint32_t grid = 0, threads = 0;
    uint64_t groups = 0;                   // 8-sample groups (v8 forms) or samples (scalar)
};

inline EncRoute encode_route(uint32_t C, uint32_t F, uint32_t n, uintptr_t pcm, uintptr_t out, uint32_t cus)
{
    EncRoute r;
    const uint64_t n_samples = (uint64_t)C * F * n;
    if (n_samples == 0) return r;
    const bool v8 = (n & 7u) == 0u && aligned(pcm, 16) && aligned(out, 8);
    if (v8 && n_samples >= (1u << 25) && (n_samples >> 3) < 0xFFFF0000ull) {   // large batches: full 16-bit table, one block per CU (32-bit group ids)
        r = {EncForm::lut16, blocks_for(n_samples >> 3, 1024, cus), (uint32_t)kEncWaves * 64u, n_samples >> 3};
    } else if (v8 && n_samples >= (1u << 22)) {                                 // big batches: table-driven compressor, persistent blocks
        r = {EncForm::v8_table, blocks_for(n_samples >> 3, 1024, cus * 2u), 1024u, n_samples >> 3};
    } else if (v8) {
        r = {EncForm::v8, blocks_for(n_samples >> 3, 256, cus * 8u), 256u, n_samples >> 3};
    } else {
        r = {EncForm::scalar, blocks_for(n_samples, 256, cus * 8u), 256u, n_samples};
    }
    return r;
}
// k_encode_lut16 reads the context's ready-made 16-bit compressor table (igdsp_encode builds it only for these launches)
inline bool encode_wants_table(const EncRoute &r) { return r.form == EncForm::lut16; }

// ---- igdsp_decode_meter_window, fused path: C % 64 == 0 and a work buffer (launch_decode_meter_window)
struct WinRoute {
    bool fits = false;                     // F / n_seg <= 65 535: silent / clipped counts of a unit are 16 bits (else IGDSP_ERANGE)
    bool blk = false;                      // block-owned form (no summaries, no finish kernel) or register form + k_window_finish
    uint32_t n_groups = 0, n_seg = 0;
    uint32_t gpb = 0, gsh = 0, parts = 1;  // block-owned form: launched as `parts` equal launches of <= 255 frames
    uint32_t grid = 0, threads = 0;
};

inline WinRoute window_route(uint32_t C, uint32_t F, uint32_t cus, const Knobs &k)
{
    WinRoute r;
    r.n_groups = C / 64u;
    // Register form: the windows live in registers; at least one unit per resident wave, a segment is never shorter than 8 frames
    // nor longer than 65 535.  (16 units per CU for its 12 waves: at 65 536 channels 4 segments — a third of the waves take a second
    // unit — measured 0.2873-0.2929 ms against 0.2973-0.3023 with 3 segments = one unit per wave, 0.2906-0.2954 with 5, 0.2903-0.2957 with 8)
    const uint32_t want = cus * 16u;
    uint32_t n_seg = r.n_groups >= want ? 1u : (want + r.n_groups - 1u) / r.n_groups;
    if (k.win_nseg) n_seg = (uint32_t)std::max(1, *k.win_nseg);   // experiments
    r.n_seg = std::max(1u, std::min(std::min(n_seg, kWinMaxSeg), std::max(1u, F / 8u)));
    r.fits = F / r.n_seg <= 65535u;
    // Block-owned form (the default where it fits): a block owns gpb = 4, 2 or 1 consecutive channel groups for the launch,
    // hands their items to its waves in (frame, group) order and keeps their windows and runs in its LDS — the item-level
    // balance of the time-major kernels inside a block, no summaries, no finish kernel.  The packed LDS counters hold 255
    // frames: longer launches go out as equal parts on the stream (hold / probe / the aggregate carry across them).
    const uint32_t cus1 = std::max(1u, cus);
    const uint32_t gpb = groups_per_block(r.n_groups, cus1, k.win_gpb);
    r.blk = k.win_blk ? *k.win_blk != 0 : window_block_fills(r.n_groups / gpb, cus1);   // (IGDSP_WIN_BLK: 0 = never, 1 = always)
    uint32_t waves = kRtpWaves;
    if (k.win_waves) waves = (uint32_t)std::max(1, std::min((int)kRtpWaves, *k.win_waves));   // experiments
    r.threads = waves * 64u;
    if (r.blk) {
        r.gpb = gpb; r.gsh = gpb_shift(gpb); r.parts = (F + 254u) / 255u;
        r.grid = r.n_groups / gpb;
        if (waves < gpb) r.threads = gpb * 64u;   // (a wave per group folds it at the block's end)
    } else {
        r.grid = blocks_for((uint64_t)r.n_groups * r.n_seg, waves, cus);
    }
    return r;
}

// ---- igdsp_tx_packetize (launch_tx_packetize)
struct TxRoute {
    int form = kTxG711;
    uint32_t vec = 0;                      // dword / 8-byte aligned inputs: vector loads
    uint32_t n_groups = 0, grid = 0, threads = 0, lds = 0;
};

// Large PCM launches encode through the context's LDS table (kTxPcmTab), as k_encode_lut16 does
inline bool tx_wants_table(bool pcm, uint32_t C, uint32_t F, uint32_t n) { return pcm && (uint64_t)C * F * n >= (1ull << 22); }

// tab_lds: the table form's 128 KiB LDS limit is raised on this device (checked only where tx_wants_table)
inline TxRoute tx_route(uint32_t C, uint32_t F, uint32_t n, uintptr_t pcm, uintptr_t g711, uintptr_t last, uint32_t cus, bool tab_lds)
{
    TxRoute r;
    r.n_groups = (C + kTxCh - 1) / kTxCh;
    r.vec = ((n & 3u) == 0u && aligned(pcm ? pcm : g711, pcm ? 8 : 4) && aligned(last, 4)) ? 1u : 0u;
    const bool tab = tx_wants_table(pcm != 0, C, F, n) && tab_lds;
    r.form = pcm == 0 ? kTxG711 : (tab ? kTxPcmTab : kTxPcm);
    r.grid = blocks_for(r.n_groups, kTxWaves, cus * (tab ? 1u : 2u));
    r.threads = kTxWaves * 64;
    r.lds = tab ? 2u * 65536u : 0u;
    return r;
}

// igdsp_internal_tx_copy (launch_tx_copy_ab): the groups, grid and block of the igdsp_tx_packetize launch of the same arguments; the
// yardstick has no send buffer, no LDS table of its own and always the vector loads (args::tx_copy asks for n % 4 == 0)
inline TxRoute tx_copy_route(uint32_t C, uint32_t F, uint32_t n, uintptr_t pcm, uintptr_t g711, uint32_t cus, bool tab_lds)
{
    TxRoute r = tx_route(C, F, n, pcm, g711, 0, cus, tab_lds);
    r.vec = 1u;
    r.lds = 0u;
    return r;
}

// ---- igdsp_conf_mix (launch_conf_mix): k_conf_mix<IN, COPY>.  An item is one (frame, port); a block of kConfWaves
// waves takes groups of kConfWaves consecutive items.  Which ports are narrow (a wave mixes the port-frame alone) and which are wide
// (the block splits the member list among its waves) is decided per item on the device from the CSR, so a launch with a skewed
// table needs no copy of it to the host; the route only picks the input form, the vector paths and the grid.
constexpr int kConfWaves = 16;                            // 1024 threads, one block per CU (64 KiB LUT + 32 KiB wide-form partials)
constexpr int kConfU = 8;                                 // frame loads of a wave in flight together (divides 64)
constexpr uint32_t kConfWideMin = 128;                    // members above which a port is mixed by the whole block
enum : int { kConfG711 = 0, kConfPcm = 1 };               // k_conf_mix<IN>
struct ConfRoute {
    int form = kConfG711;
    uint32_t vec_in = 0, vec_out = 0;      // n % 4 == 0 and rows aligned: dword (G.711) / 8-byte (PCM) loads, 8-byte stores
    uint32_t grid = 0, threads = 0;
};
inline ConfRoute conf_route(uint32_t P, uint32_t F, uint32_t n, bool pcm, uintptr_t in, uintptr_t out, uint32_t cus)
{
    ConfRoute r;
    const uint64_t items = (uint64_t)P * F;
    if (items == 0) return r;
    r.form = pcm ? kConfPcm : kConfG711;
    r.vec_in = ((n & 3u) == 0u && aligned(in, pcm ? 8 : 4)) ? 1u : 0u;
    r.vec_out = ((n & 3u) == 0u && aligned(out, 8)) ? 1u : 0u;
    r.grid = blocks_for((items + kConfWaves - 1) / kConfWaves, 1, std::max(1u, cus));
    r.threads = kConfWaves * 64;
    return r;
}

// ---- igdsp_bss_select (launch_bss_select): k_bss_select<IN, COPY> + k_bss_words.  A wave owns gpw consecutive
// groups for the frames of a part: its lanes gather the members' info records (one member slot per lane, a 64-slot chunk at a time)
// and fold each frame's open members into a vote key per group in LDS; lanes 0 .. gpw-1 then step the groups' state machines over
// the part's frames, and the whole wave emits the voted frames.  gpw is chosen so that a wave's groups fill about one chunk of 64
// member slots.  The vote keys of a part live in LDS ([kBssPart][kBssGroups] per wave), so a launch of more frames goes out in
// parts of kBssPart frames; after each part k_bss_words (a thread per member slot) stores the slots' last words, which the next
// part reads.  The state is carried through d_state, as between launches.
constexpr int kBssWaves = 4;                              // waves per block: they share the 64 KiB LUT (+ 32 KiB of vote keys)
constexpr uint32_t kBssGroups = 16;                       // groups per wave at most (decision lanes)
constexpr uint32_t kBssPart = 128;                        // frames per part
constexpr uint32_t kBssU = 8;                             // loads of a lane in flight together
constexpr uint32_t kBssWordsThreads = 256;                // k_bss_words
enum : int { kBssNone = 2 };                              // k_bss_select<IN>: kConfG711, kConfPcm, or no audio
struct BssRoute {
    int form = kBssNone;
    uint32_t gpw = 0;                      // groups per wave
    uint32_t vec_in = 0, vec_out = 0;      // as ConfRoute
    uint32_t grid = 0, threads = 0;        // k_bss_select, every part
    uint32_t part_frames = 0, parts = 0;   // the last part takes the rest
    uint32_t words_grid = 0;               // k_bss_words, every part (0: no member slots)
};
inline BssRoute bss_route(uint32_t G, uint32_t F, uint32_t n, uint32_t n_members, int form, uintptr_t in, uintptr_t out)
{
    BssRoute r;
    if ((uint64_t)G * F == 0) return r;
    r.form = form;
    const uint64_t avg = std::max<uint64_t>(1u, ((uint64_t)n_members + G - 1) / G);
    r.gpw = kBssGroups;
    while (r.gpw > 1u && r.gpw * avg > 64u) r.gpw >>= 1;
    r.vec_in = form != kBssNone && (n & 3u) == 0u && aligned(in, form == kConfPcm ? 8 : 4) ? 1u : 0u;
    r.vec_out = form != kBssNone && (n & 3u) == 0u && aligned(out, 8) ? 1u : 0u;
    const uint64_t waves = ((uint64_t)G + r.gpw - 1) / r.gpw;
    r.grid = (uint32_t)((waves + kBssWaves - 1) / kBssWaves);
    r.threads = kBssWaves * 64;
    r.part_frames = std::min(F, kBssPart);
    r.parts = (F + kBssPart - 1) / kBssPart;
    r.words_grid = (uint32_t)(((uint64_t)n_members + kBssWordsThreads - 1) / kBssWordsThreads);
    return r;
}

// ---- igdsp_ptt_arbitrate (launch_ptt_arbitrate): k_ptt_arbitrate<IN, COPY> + k_ptt_slots.  The wave geometry of bss_route:
// a wave owns gpw consecutive groups for the frames of a part, about one chunk of 64 member slots.  Its lanes step the member slots
// (one slot per lane: word, debounce, effective PTT type) through the part's frames and leave an op per (frame, slot) in LDS; lanes
// 0 .. gpw-1 then walk their group's members in order, frame by frame, and the whole wave emits the holders' frames.  The ops of a
// wave are kPttOps 16-bit entries: a window of W = min(its slots rounded up to 64, kPttOps) slots times kPttOps / W frames.  A wave
// with more frames or slots than that takes the part in several passes (64 slots: 2 passes of 64 frames; more than kPttOps slots: a
// frame at a time, window by window), every pass stepping its slots again from the part's first frame.  Nothing is read back within a
// launch: the group state is read and written by its own lane, and the slots are only read; after each part k_ptt_slots (a thread
// per member slot) steps every slot through the part and stores it, which the next part reads.
constexpr int kPttWaves = 4;                              // waves per block: they share the 64 KiB LUT (+ 32 KiB selections, 32 KiB ops)
constexpr uint32_t kPttGroups = 16;                       // groups per wave at most (decision lanes)
constexpr uint32_t kPttPart = 128;                        // frames per part
constexpr uint32_t kPttU = 8;                             // loads of a lane in flight together
constexpr uint32_t kPttOps = 4096;                        // (frame, slot) ops of a wave in LDS
constexpr uint32_t kPttSlotsThreads = 256;                // k_ptt_slots
struct PttRoute {
    int form = kBssNone;                   // kConfG711, kConfPcm, or no audio
    uint32_t gpw = 0;                      // groups per wave
    uint32_t vec_in = 0, vec_out = 0;      // as ConfRoute
    uint32_t grid = 0, threads = 0;        // k_ptt_arbitrate, every part
    uint32_t part_frames = 0, parts = 0;   // the last part takes the rest
    uint32_t pass_frames = 0;              // frames per pass of a wave with the average slot count (a wider wave takes fewer)
    uint32_t slots_grid = 0;               // k_ptt_slots, every part (0: no member slots)
};
inline PttRoute ptt_route(uint32_t G, uint32_t F, uint32_t n, uint32_t n_members, int form, uintptr_t in, uintptr_t out)
{
    PttRoute r;
    if ((uint64_t)G * F == 0) return r;
    r.form = form;
    const uint64_t avg = std::max<uint64_t>(1u, ((uint64_t)n_members + G - 1) / G);
    r.gpw = kPttGroups;
    while (r.gpw > 1u && r.gpw * avg > 64u) r.gpw >>= 1;
    r.vec_in = form != kBssNone && (n & 3u) == 0u && aligned(in, form == kConfPcm ? 8 : 4) ? 1u : 0u;
    r.vec_out = form != kBssNone && (n & 3u) == 0u && aligned(out, 8) ? 1u : 0u;
    const uint64_t waves = ((uint64_t)G + r.gpw - 1) / r.gpw;
    r.grid = (uint32_t)((waves + kPttWaves - 1) / kPttWaves);
    r.threads = kPttWaves * 64;
    r.part_frames = std::min(F, kPttPart);
    r.parts = (F + kPttPart - 1) / kPttPart;
    const uint64_t window = std::min<uint64_t>(kPttOps, (r.gpw * avg + 63u) / 64u * 64u);
    r.pass_frames = std::min(r.part_frames, (uint32_t)(kPttOps / window));
    r.slots_grid = (uint32_t)(((uint64_t)n_members + kPttSlotsThreads - 1) / kPttSlotsThreads);
    return r;
}

// ---- igdsp_link_watch (launch_link_watch): k_link_watch<COPY, PASS, SIZES> + k_link_scan.  A lane owns a channel for the ticks of one part
// (<= kLinkPart ticks) and walks the part's arrival slots in order, kLinkU record loads in flight; a wave is 64 consecutive channels.
// Without an event list one pass (kLinkSingle) walks and stores the state and the kind bytes.  With a list a part takes three
// launches: the count pass (kLinkCount) walks and leaves the number of event lanes per (tick, wave) in d_work, tick-major; k_link_scan
// (one block) turns the counts into exclusive offsets in place, starting at the offset the launch's earlier parts reached (d_work's
// header carries it) and writes the two totals after the last part; the write pass (kLinkWrite) replays the walk from the same state
// and stores the state, the kind bytes and each event at its wave's offset plus the lane's rank among the wave's event lanes.
// Nothing is read back within a kernel: the hand-offs are kernel boundaries on the stream.
constexpr int kLinkWaves = 4;                             // waves per block, independent of each other
constexpr uint32_t kLinkPart = 128;                       // ticks per part
constexpr uint32_t kLinkU = 16;                           // record loads of a lane in flight together
constexpr uint32_t kLinkScanThreads = 1024;               // k_link_scan: one block
constexpr uint32_t kLinkWorkHead = 16;                    // d_work: {offset reached, 0, 0, 0}, then the counts / offsets [part ticks][waves]
enum : int { kLinkSingle = 0, kLinkCount = 1, kLinkWrite = 2 };   // k_link_watch<COPY, PASS, SIZES>
struct LinkRoute {
    uint32_t waves = 0;                    // waves of 64 channels: the row of the counts
    uint32_t grid = 0, threads = 0;        // k_link_watch, every pass of every part
    uint32_t part_ticks = 0, parts = 0;    // the last part takes the rest
    uint32_t passes = 0;                   // walks per part: 1, or 2 with a list
    uint32_t scan_threads = 0;             // k_link_scan, every part (0: no list)
    uint64_t work_bytes = 0;               // what the launch uses of d_work (0: no list)
};
inline uint32_t link_waves(uint32_t C) { return C / 64u + (C % 64u != 0u ? 1u : 0u); }
inline uint64_t link_work_bytes(uint32_t C, uint32_t T)
{
    return kLinkWorkHead + (((uint64_t)std::min(T, kLinkPart) * link_waves(C) * 4u + 15u) & ~15ull);
}
inline LinkRoute link_route(uint32_t C, uint32_t T, bool list)
{
    LinkRoute r;
    if ((uint64_t)C * T == 0) return r;
    r.waves = link_waves(C);
    r.grid = (r.waves + kLinkWaves - 1) / kLinkWaves;
    r.threads = kLinkWaves * 64;
    r.part_ticks = std::min(T, kLinkPart);
    r.parts = (T + kLinkPart - 1) / kLinkPart;
    r.passes = list ? 2u : 1u;
    r.scan_threads = list ? kLinkScanThreads : 0u;
    r.work_bytes = list ? link_work_bytes(C, T) : 0u;
    return r;
}

// ---- the event list behind a stage's dense records [F][C] (igdsp_tone_detect, igdsp_vad_run; launch_event_list): the records lie in
// d_rec, or in d_work behind the counts when there is none; the stage's list kernel counts the event lanes per (frame, wave of 64
// channels), k_link_scan turns the counts into offsets and writes the two totals, the list kernel's second pass stores the events.
constexpr int kListWaves = 4;                             // waves per block of a list kernel, independent of each other
struct ListRoute {
    uint32_t waves = 0;                    // waves of 64 channels: the counts' row
    uint32_t list_grid = 0;                // the list kernel, both passes (0: no list)
    uint64_t counts_bytes = 0;             // d_work: head + counts, rounded to 16
    uint64_t work_bytes = 0;               // d_work in all: + the records when d_rec is NULL
};
inline uint64_t list_counts_bytes(uint32_t C, uint32_t F) { return kLinkWorkHead + (((uint64_t)F * link_waves(C) * 4u + 15u) & ~15ull); }
inline uint64_t list_work_bytes(uint32_t C, uint32_t F, bool with_rec, uint32_t rec_bytes) { return list_counts_bytes(C, F) + (with_rec ? 0u : (uint64_t)C * F * rec_bytes); }
inline ListRoute list_route(uint32_t C, uint32_t F, bool list, bool with_rec, uint32_t rec_bytes)
{
    ListRoute r;
    r.waves = link_waves(C);
    if (list) {
        r.list_grid = (uint32_t)(((uint64_t)F * r.waves + kListWaves - 1u) / kListWaves);
        r.counts_bytes = list_counts_bytes(C, F);
        r.work_bytes = list_work_bytes(C, F, with_rec, rec_bytes);
    }
    return r;
}

// ---- igdsp_jb_receive (launch_jb_receive): k_jb_receive<COPY>.  A wave owns kJbCh consecutive channels for the ticks
// of one part (<= kJbPart ticks).  Lanes 0 .. kJbCh - 1 step their channel's state machine over the part's arrivals with the ring tags in
// LDS and leave a source descriptor per (tick, channel) there: an arrival of the part, a ring slot, or none; then the whole wave writes
// the records and copies the payload rows in 16-byte pieces, and stores the packets still unplayed at the part's end into the ring.  A
// launch of more ticks goes out in parts; the state and the ring carry between them as between launches.
constexpr int kJbWaves = 4;                               // waves per block, independent of each other
constexpr uint32_t kJbCh = 16;                            // channels per wave (decision lanes)
constexpr uint32_t kJbPart = 128;                         // ticks per part
constexpr uint32_t kJbU = 4;                              // loads of a lane in flight together
constexpr uint32_t kJbSlotHead = 16;                      // ring slot: {ed137, payload_len | pt << 16 | flags << 24, len, 0}, then payload
inline uint64_t jb_slot_bytes(uint32_t n) { return kJbSlotHead + (((uint64_t)n + 15u) & ~15ull); }
inline uint64_t jb_ring_bytes(uint32_t C, uint32_t n)         // tags [C][IGDSP_JB_DEPTH] u32, then slots [C][IGDSP_JB_DEPTH]
{
    return (uint64_t)C * IGDSP_JB_DEPTH * (4u + jb_slot_bytes(n));
}
struct JbRoute {
    uint32_t vec = 0;                      // n % 16 == 0 and a 16-byte aligned payload output: 16-byte stores
    uint32_t pieces = 0;                   // 16-byte pieces per frame
    uint32_t grid = 0, threads = 0;        // every part
    uint32_t part_ticks = 0, parts = 0;    // the last part takes the rest
};
inline JbRoute jb_route(uint32_t C, uint32_t T, uint32_t n, uintptr_t payload_out)
{
    JbRoute r;
    if ((uint64_t)C * T == 0) return r;
    r.vec = (n & 15u) == 0u && aligned(payload_out, 16) ? 1u : 0u;
    r.pieces = (n + 15u) / 16u;
    const uint64_t waves = ((uint64_t)C + kJbCh - 1) / kJbCh;
    r.grid = (uint32_t)((waves + kJbWaves - 1) / kJbWaves);
    r.threads = kJbWaves * 64;
    r.part_ticks = std::min(T, kJbPart);
    r.parts = (T + kJbPart - 1) / kJbPart;
    return r;
}

// igdsp_jb_receive_adaptive's Start rule (include/igdsp.h, "Jitter buffer, adaptive"): the new delay from the cfg, the A.8 jitter J
// (scaled by 16) and n samples per frame; updates a.  constexpr, so k_jb_adaptive and igdsp_jb_adapt_next run the same function.
constexpr bool jb_adapt_cfg_ok(const igdsp_jb_adapt_cfg &c)
{
    return c.min_frames <= c.init_frames && c.init_frames <= c.max_frames && c.max_frames <= IGDSP_JB_DEPTH - 1 && c.jitter_mult <= 16;
}
constexpr uint32_t jb_adapt_start(const igdsp_jb_adapt_cfg &cfg, uint32_t J, uint32_t n, igdsp_jb_adapt &a)
{
    const bool set = (a.flags & IGDSP_JB_ADAPT_SET) != 0;
    const uint32_t cur = set ? a.delay : cfg.init_frames, lo = cfg.min_frames, hi = cfg.max_frames;
    const uint64_t q = ((uint64_t)cfg.jitter_mult * J + 16u * n - 1u) / (16u * n);
    const uint32_t tj = q < hi ? (uint32_t)q : hi;
    const uint32_t want = tj > a.need ? tj : a.need;
    uint32_t nw = want >= cur ? want : cur - 1u;
    nw = nw < lo ? lo : (nw > hi ? hi : nw);
    if (set && nw > a.delay && a.grows != 0xFFFFu) ++a.grows;
    if (set && nw < a.delay && a.shrinks != 0xFFFFu) ++a.shrinks;
    a.delay = (uint8_t)nw;
    a.flags |= IGDSP_JB_ADAPT_SET;
    a.need = 0;
    a.late_run = 0;
    return nw;
}

// ---- igdsp_plc_conceal (launch_plc_conceal): k_plc<COPY>.  A wave owns kPlcCh consecutive channels for the ticks of
// one part (<= kPlcPart ticks).  Lanes 0 .. kPlcCh - 1 walk their channel's tick flags (no samples: which ticks are plain, which start
// or continue a run, which recover) and leave a kind and a length per (tick, channel) in LDS; the whole wave then decodes and stores
// the plain and IDLE rows, kPlcPiece samples per lane and piece, kPlcU pieces of a lane in flight, in batches of whole rows (the
// records are reduced from per-piece partials in LDS); then it walks the channels with loss one at a time, tick by tick, for the
// synthetic rows; last it writes every channel's final history ring.  A launch of more ticks goes out in parts; the state carries
// between them as between launches.
constexpr int kPlcWaves = 4;                              // waves per block, independent of each other
constexpr uint32_t kPlcCh = 16;                           // channels per wave
constexpr uint32_t kPlcPart = 128;                        // ticks per part
constexpr uint32_t kPlcU = 4;                             // pieces of a lane in flight together
constexpr uint32_t kPlcPiece = 8;                         // samples per piece: 16 bytes out
struct PlcRoute {
    uint32_t vec = 0;                      // n % 8 == 0, the output 16-byte and the input 8-byte (G.711) / 16-byte (PCM) aligned
    uint32_t pieces = 0;                   // pieces per row
    uint32_t batch_rows = 0;               // rows per batch: kPlcU * 64 / pieces
    uint32_t grid = 0, threads = 0;        // every part
    uint32_t part_ticks = 0, parts = 0;    // the last part takes the rest
};
inline PlcRoute plc_route(uint32_t C, uint32_t T, uint32_t n, bool pcm, uintptr_t in, uintptr_t out)
{
    PlcRoute r;
    if ((uint64_t)C * T == 0 || n == 0) return r;
    r.vec = (n % kPlcPiece) == 0u && aligned(out, 16) && aligned(in, pcm ? 16 : 8) ? 1u : 0u;
    r.pieces = (n + kPlcPiece - 1) / kPlcPiece;
    r.batch_rows = kPlcU * 64u / r.pieces;
    const uint64_t waves = ((uint64_t)C + kPlcCh - 1) / kPlcCh;
    r.grid = (uint32_t)((waves + kPlcWaves - 1) / kPlcWaves);
    r.threads = kPlcWaves * 64;
    r.part_ticks = std::min(T, kPlcPart);
    r.parts = (T + kPlcPart - 1) / kPlcPart;
    return r;
}

// ---- igdsp_snd_combine / igdsp_snd_split (launch_snd): k_snd<DIR, MODE, VEC>.  An item is one card-frame (frame f, card d): K rows
// of n samples on the mono side, n samples of K channels on the card side, the same K * n * 2 bytes at the same offset of both buffers.
// A wave takes kSndU consecutive items at a time (static, grid-stride): it issues the loads of all of them, then passes them one after
// the other through its LDS tile, which always holds the item row-major ([k][s]); the records are read from the tile.
//   vector form: K * n even and both buffers dword aligned.  16-byte pieces in memory order on both sides (16-byte aligned where the
//             base and K * n * 2 are, dword aligned otherwise) and a last piece of 1 .. 3 dwords where K * n * 2 is no multiple of 16.
//   general form: everything else (K * n odd, a buffer aligned to 2 only): the same tile, filled and emptied a sample at a time.
// Interleaved index r = s * K + k of an item <-> row-major index k * n + s: s = r / K by snd_div, exact on the device's range.
#ifndef IGDSP_SND_WAVES
#define IGDSP_SND_WAVES 8
#endif
#ifndef IGDSP_SND_U
#define IGDSP_SND_U 4
#endif
constexpr int kSndWaves = IGDSP_SND_WAVES;                // waves per block, independent of each other (a 4 KiB tile each)
constexpr int kSndU = IGDSP_SND_U;                        // items of a wave in flight together
constexpr uint32_t kSndTileBytes = IGDSP_SND_MAX_CHANNELS * IGDSP_MAX_PAYLOAD * 2u;   // the largest item: 4 KiB
constexpr uint32_t kSndLanePieces = kSndTileBytes / 16u / 64u;                        // 16-byte pieces of a lane per item: 4
enum : int { kSndCombine = 0, kSndSplit = 1 };            // k_snd<DIR>
enum : int { kSndBoth = 0, kSndBulk = 1, kSndStats = 2, kSndCopy = 3 };   // k_snd<, MODE>: what is written; kSndCopy: the yardstick
// r / d as (r * magic) >> 20 with magic = ceil(2^20 / d): exact for r < 4096 and d <= 256 (the error term r * (d * magic - 2^20) stays
// below 2^20, and r * magic below 2^32).  constexpr: the kernel and tests/route/snd_route_driver.cpp run the same function.
constexpr uint32_t snd_div_magic(uint32_t d) { return ((1u << 20) + d - 1u) / d; }
constexpr uint32_t snd_div(uint32_t r, uint32_t magic) { return (r * magic) >> 20; }
struct SndRoute {
    int mode = kSndBoth;
    uint32_t vec = 0;                      // the vector form
    uint32_t pieces = 0, tail_dwords = 0;  // vector form: pieces per item (the last of tail_dwords dwords if that is not 0)
    uint32_t items = 0, grid = 0, threads = 0;
};
inline SndRoute snd_route(uint32_t D, uint32_t K, uint32_t F, uint32_t n, bool bulk, bool stats, bool yardstick, uintptr_t in, uintptr_t out,
                          uint32_t cus)
{
    SndRoute r;
    const uint64_t items = (uint64_t)D * F;
    if (items == 0 || K == 0 || K > IGDSP_SND_MAX_CHANNELS || n == 0 || n > IGDSP_MAX_PAYLOAD || items * K >= 0xFFFFFFE0ull) return r;
    if (!bulk && !stats) return r;
    r.mode = yardstick ? kSndCopy : (bulk && stats ? kSndBoth : (bulk ? kSndBulk : kSndStats));
    const uint32_t bytes = K * n * 2u;
    r.vec = (bytes & 3u) == 0u && aligned(in | out, 4) ? 1u : 0u;
    if (r.vec) { r.tail_dwords = (bytes & 15u) >> 2; r.pieces = (bytes + 15u) >> 4; }
    r.items = (uint32_t)items;
    r.grid = blocks_for((items + kSndU - 1u) / kSndU, kSndWaves, std::max(1u, cus));
    r.threads = kSndWaves * 64;
    return r;
}

// ---- igdsp_tone_generate (launch_tone): the rules of include/igdsp.h, "Tone generator", as constexpr functions, so that the host
// entries (igdsp_tone_plan_build, igdsp_tone_frame), k_tone and tests/route/tone_route_driver.cpp run the same code; then tone_route.
// The oscillator reads the table as (value, delta) pairs: T[i] in the low half, T[i + 1] - T[i] (|delta| <= 202) in the high half, one
// 4-byte lookup per oscillator sample.  kTonePairs is the host's copy; k_tone builds the same pairs in LDS from its own copy of the list.
inline constexpr int16_t kToneSin[1024] = {IGDSP_TONE_SIN_VALUES};
constexpr uint32_t tone_pair(int32_t v, int32_t next) { return (uint32_t)(uint16_t)v | ((uint32_t)(next - v) << 16); }
struct TonePairs { uint32_t w[1024]; };
constexpr TonePairs tone_make_pairs()
{
    TonePairs p{};
    for (uint32_t i = 0; i < 1024u; ++i) p.w[i] = tone_pair(kToneSin[i], kToneSin[(i + 1u) & 1023u]);
    return p;
}
inline constexpr TonePairs kTonePairs = tone_make_pairs();

// T[i] + (((T[i + 1] - T[i]) * fr) >> 16) at phase ph: i = ph >> 22, fr = (ph >> 6) & 0xFFFF (>> of a negative value: arithmetic = floor).
// tone_interp takes the pair already fetched: k_tone's whole-piece path issues the lookups of a piece together, then interpolates.
constexpr int32_t tone_interp(uint32_t w, uint32_t ph)
{
    const int32_t v = (int16_t)(uint16_t)w, d = (int32_t)w >> 16, fr = (int32_t)((ph >> 6) & 0xFFFFu);
    return v + ((d * fr) >> 16);
}
constexpr int32_t tone_osc(const uint32_t *pairs, uint32_t ph) { return tone_interp(pairs[ph >> 22], ph); }
// the sample before the fades from the oscillators' values (the product in unsigned: a volume above 32767, which only a plan that
// igdsp_tone_plan_build did not make can carry, wraps instead of overflowing)
constexpr int32_t tone_scale1(const igdsp_tone_seg &sg, int32_t o1) { return (int32_t)((uint32_t)o1 * sg.vol) >> 15; }
constexpr int32_t tone_scale2(const igdsp_tone_seg &sg, int32_t o1, int32_t o2) { return (int32_t)((uint32_t)(o1 + o2) * sg.vol) >> 16; }
constexpr int32_t tone_amp(const uint32_t *pairs, const igdsp_tone_seg &sg, uint32_t ph1, uint32_t ph2)
{
    const int32_t o1 = tone_osc(pairs, ph1);
    return sg.step2 == 0u ? tone_scale1(sg, o1) : tone_scale2(sg, o1, tone_osc(pairs, ph2));
}
constexpr int32_t tone_fade(const igdsp_tone_seg &sg, uint32_t k, int32_t a)
{
    if (k < sg.fade_in) a = a * (int32_t)k / (int32_t)sg.fade_in;
    if (sg.fade_out != 0u && (uint64_t)k + sg.fade_out >= sg.on) a = a * (int32_t)(sg.on - 1u - k) / (int32_t)sg.fade_out;
    return a;
}
// THE sample rule: offset k < sg.on inside a tone's ON period.  k_tone's whole-piece path runs the same tone_interp / tone_scale steps
// with the phases advanced by addition ((k + 1) * step == k * step + step in 32 bits) and skips tone_fade where no sample of the piece
// fades.
constexpr int32_t tone_sample(const uint32_t *pairs, const igdsp_tone_seg &sg, uint32_t k)
{
    return tone_fade(sg, k, tone_amp(pairs, sg, k * sg.step1, k * sg.step2));
}
// A plan is read as it is (the device cannot reject one): more than IGDSP_TONE_MAX tones count as IGDSP_TONE_MAX, a cycle of 0 plays
// nothing, a position no segment holds is silence.
constexpr uint32_t tone_count(const igdsp_tone_plan &p) { return p.n_tones < IGDSP_TONE_MAX ? p.n_tones : (uint32_t)IGDSP_TONE_MAX; }
constexpr uint32_t tone_seg_end(const igdsp_tone_plan &p, uint32_t i) { return i + 1u < tone_count(p) ? p.seg[i + 1u].start : p.cycle; }
constexpr int32_t tone_seg_of(const igdsp_tone_plan &p, uint32_t q)          // the segment that holds cycle position q, or -1
{
    for (uint32_t i = 0; i < tone_count(p); ++i)
        if (q >= p.seg[i].start && q < tone_seg_end(p, i)) return (int32_t)i;
    return -1;
}
constexpr int32_t tone_at(const uint32_t *pairs, const igdsp_tone_plan &p, uint32_t q)   // the sample at cycle position q < p.cycle
{
    const int32_t i = tone_seg_of(p, q);
    if (i < 0) return 0;
    const uint32_t k = q - p.seg[i].start;
    return k < p.seg[i].on ? tone_sample(pairs, p.seg[i], k) : 0;
}
// sample s of a live frame whose sample 0 is at q0 (pos + f * n; looping: any value, not looping: q0 < cycle)
constexpr int32_t tone_frame_sample(const uint32_t *pairs, const igdsp_tone_plan &p, uint64_t q0, uint32_t s)
{
    uint64_t q = q0 + s;
    if ((p.options & IGDSP_TONE_LOOP) != 0u && q >= p.cycle) { q -= p.cycle; if (q >= p.cycle) q %= p.cycle; }   // (mostly one subtraction)
    return q < p.cycle ? tone_at(pairs, p, (uint32_t)q) : 0;
}
constexpr igdsp_tone_state tone_cmd(igdsp_tone_state st, uint32_t cmd)
{
    if ((cmd & IGDSP_TONE_CMD_STOP) != 0u) st.flags &= ~IGDSP_TONE_PLAYING;
    else if ((cmd & IGDSP_TONE_CMD_REWIND) != 0u) { st.pos = 0u; st.flags |= IGDSP_TONE_PLAYING; }
    return st;
}
// st: after tone_cmd.  A port that plays (not held, a plan, PLAYING) produces the frame at q0 = pos + f * n when this holds
constexpr bool tone_plays(const igdsp_tone_plan &p, const igdsp_tone_state &st) { return (st.flags & IGDSP_TONE_PLAYING) != 0u && p.cycle != 0u; }
constexpr bool tone_live(const igdsp_tone_plan &p, uint64_t q0) { return (p.options & IGDSP_TONE_LOOP) != 0u || q0 < p.cycle; }
// the state after `samples` samples of a port that was not held (st: after tone_cmd)
constexpr igdsp_tone_state tone_advance(const igdsp_tone_plan &p, igdsp_tone_state st, uint64_t samples)
{
    if (!tone_plays(p, st)) return st;
    const uint64_t q = (uint64_t)st.pos + samples;
    if ((p.options & IGDSP_TONE_LOOP) != 0u) { st.pos = (uint32_t)(q % p.cycle); return st; }
    st.pos = q < p.cycle ? (uint32_t)q : p.cycle;
    if (st.pos >= p.cycle) st.flags &= ~IGDSP_TONE_PLAYING;
    return st;
}
// igdsp_tone_plan_build's rule; false: nothing written
constexpr bool tone_plan_make(const igdsp_tone_desc *tones, uint32_t count, uint32_t clock_rate, uint32_t options, igdsp_tone_plan &out)
{
    if (!tones || count == 0u || count > IGDSP_TONE_MAX || clock_rate < 8000u || clock_rate > 48000u || clock_rate % 1000u != 0u) return false;
    if ((options & ~(IGDSP_TONE_LOOP | IGDSP_TONE_NO_FADE)) != 0u) return false;
    igdsp_tone_plan p{};
    const uint32_t top = clock_rate / 2u - 1u;
    uint32_t at = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const igdsp_tone_desc &t = tones[i];
        if (t.freq1 == 0u || t.freq1 > top || t.freq2 > top || t.volume > 32767u || t.reserved != 0u) return false;
        igdsp_tone_seg &sg = p.seg[i];
        const uint32_t on = t.on_msec * clock_rate / 1000u, off = t.off_msec * clock_rate / 1000u;
        sg.start = at; sg.on = on;
        sg.step1 = (uint32_t)((((uint64_t)t.freq1 << 32) + clock_rate / 2u) / clock_rate);
        sg.step2 = t.freq2 ? (uint32_t)((((uint64_t)t.freq2 << 32) + clock_rate / 2u) / clock_rate) : 0u;
        sg.vol = t.volume ? t.volume : (uint16_t)IGDSP_TONE_VOLUME;
        const uint32_t fi = clock_rate / 1000u, fo = clock_rate / 500u;
        const bool fade = (options & IGDSP_TONE_NO_FADE) == 0u && on >= fi + fo;
        sg.fade_in = (uint16_t)(fade ? fi : 0u); sg.fade_out = (uint16_t)(fade ? fo : 0u);
        at += on + off;
    }
    if (at == 0u) return false;
    p.n_tones = count; p.options = options; p.cycle = at; p.clock_rate = clock_rate;
    out = p;
    return true;
}

// k_tone<VEC, MODE>.  A wave owns kTonePorts consecutive ports for the frames of one chunk: kToneLanes lanes per port.  The lanes of a
// port read its plan index, cmd and state once per item, step the cycle position by n per frame and keep the segment that holds it in
// registers; each takes the 8-sample pieces j, j + kToneLanes, .. of the row.  A piece that lies wholly in the un-faded part of an ON
// period advances two phases by addition; one wholly in an OFF period or in an EMPTY row is zeros; the rest (a segment edge, a fade,
// the wrap, the end of a plan that does not loop) goes sample by sample through tone_frame_sample.  Consecutive rows of a frame are
// consecutive in memory, so a wave's stores of one frame cover one run of kTonePorts rows.  The lanes of a row fold their sums by DPP.
//   vector form: n % 8 == 0 and d_pcm 16-byte aligned: one 16-byte store per piece.
//   general form: everything else: the same pieces, the last one partial, stored a sample at a time.
// Frames are cut into chunks only where the port groups alone would leave waves idle (few ports, many frames); a launch of one chunk
// writes the state itself, otherwise k_tone_state (a thread per port) does, behind the kernel on the stream.
constexpr int kToneWaves = 16;                            // waves per block: they share the 4 KiB pair table
constexpr uint32_t kToneLanes = 4;                        // lanes per port
constexpr uint32_t kTonePorts = 64u / kToneLanes;         // ports per wave: 16
constexpr uint32_t kToneStateThreads = 256;               // k_tone_state
enum : int { kToneBoth = 0, kTonePcm = 1, kToneStats = 2, kToneFill = 3 };   // k_tone<, MODE>: what is written; kToneFill: the yardstick
struct ToneRoute {
    int mode = kToneBoth;
    uint32_t vec = 0;                      // the vector form
    uint32_t pieces = 0;                   // 8-sample pieces per row
    uint32_t groups = 0;                   // port groups of kTonePorts
    uint32_t chunk_frames = 0, chunks = 0; // frames per chunk (the last takes the rest); items = groups * chunks
    uint32_t grid = 0, threads = 0;
    uint32_t state_grid = 0;               // k_tone_state behind the kernel (0: the kernel writes the state, or the yardstick: nobody does)
};
inline ToneRoute tone_route(uint32_t P, uint32_t F, uint32_t n, bool pcm, bool stats, bool yardstick, uintptr_t out, uint32_t cus)
{
    ToneRoute r;
    if ((uint64_t)P * F == 0 || n == 0 || n > IGDSP_MAX_PAYLOAD || (uint64_t)P * F >= 0xFFFFFFE0ull) return r;
    if (!pcm && !stats) return r;
    r.mode = yardstick ? kToneFill : (pcm && stats ? kToneBoth : (pcm ? kTonePcm : kToneStats));
    r.vec = (n & 7u) == 0u && aligned(out, 16) ? 1u : 0u;
    r.pieces = (n + 7u) / 8u;
    r.groups = (uint32_t)(((uint64_t)P + kTonePorts - 1u) / kTonePorts);
    const uint32_t want = std::max(1u, cus) * (uint32_t)kToneWaves;
    const uint32_t cuts = r.groups >= want ? 1u : std::min(F, (want + r.groups - 1u) / r.groups);
    r.chunk_frames = (F + cuts - 1u) / cuts;
    r.chunks = (F + r.chunk_frames - 1u) / r.chunk_frames;
    r.grid = blocks_for((uint64_t)r.groups * r.chunks, kToneWaves, std::max(1u, cus));
    r.threads = kToneWaves * 64;
    r.state_grid = !yardstick && r.chunks > 1u ? (P + kToneStateThreads - 1u) / kToneStateThreads : 0u;
    return r;
}

// ---- igdsp_resample (launch_rs): the rules of include/igdsp.h, "Rate converter", as constexpr functions, so that the host entries
// (igdsp_rs_frame, igdsp_rs_taps), k_rs and tests/route/rs_route_driver.cpp run the same code; then rs_route.
inline constexpr int16_t kRsUp2[2 * IGDSP_RS_TAPS] = {IGDSP_RS_UP2_VALUES}, kRsDown2[2 * IGDSP_RS_TAPS] = {IGDSP_RS_DOWN2_VALUES};
inline constexpr int16_t kRsUp3[3 * IGDSP_RS_TAPS] = {IGDSP_RS_UP3_VALUES}, kRsDown3[3 * IGDSP_RS_TAPS] = {IGDSP_RS_DOWN3_VALUES};
inline constexpr int16_t kRsUp4[4 * IGDSP_RS_TAPS] = {IGDSP_RS_UP4_VALUES}, kRsDown4[4 * IGDSP_RS_TAPS] = {IGDSP_RS_DOWN4_VALUES};
inline constexpr int16_t kRsUp6[6 * IGDSP_RS_TAPS] = {IGDSP_RS_UP6_VALUES}, kRsDown6[6 * IGDSP_RS_TAPS] = {IGDSP_RS_DOWN6_VALUES};
constexpr uint32_t kRsTaps = IGDSP_RS_TAPS, kRsHist = IGDSP_RS_HIST;
constexpr bool rs_factor_ok(uint32_t R) { return R == 2u || R == 3u || R == 4u || R == 6u; }
constexpr bool rs_dir_ok(uint32_t dir) { return dir == IGDSP_RS_UP || dir == IGDSP_RS_DOWN; }
// U_R in [p][k] order or D_R, 24 R values each; nullptr for a direction or factor that does not exist
constexpr const int16_t *rs_table(uint32_t dir, uint32_t R)
{
    if (!rs_dir_ok(dir)) return nullptr;
    const bool up = dir == IGDSP_RS_UP;
    return R == 2u ? (up ? kRsUp2 : kRsDown2) : R == 3u ? (up ? kRsUp3 : kRsDown3) : R == 4u ? (up ? kRsUp4 : kRsDown4)
         : R == 6u ? (up ? kRsUp6 : kRsDown6) : nullptr;
}
constexpr int32_t rs_clamp16(int32_t v) { return v > 32767 ? 32767 : (v < -32768 ? -32768 : v); }
constexpr int32_t rs_round(int32_t acc) { return (acc + 8192) >> 14; }     // arithmetic shift: a floor
// THE sample rules, before the clamp.  xg points at x[g] (UP) / x[g R + R - 1] (DOWN) of a stream with its predecessors in front of it
constexpr int32_t rs_up_raw(const int16_t *tab, uint32_t p, const int16_t *xg)
{
    int32_t acc = 0;
    for (uint32_t k = 0; k < kRsTaps; ++k) acc += (int32_t)tab[p * kRsTaps + k] * xg[-(int32_t)k];
    return rs_round(acc);
}
constexpr int32_t rs_down_raw(const int16_t *tab, uint32_t R, const int16_t *xe)
{
    int32_t acc = 0;
    for (uint32_t j = 0; j < kRsTaps * R; ++j) acc += (int32_t)tab[j] * xe[-(int32_t)j];
    return rs_round(acc);
}
// k_rs reads a window oldest sample first, two samples per dword: the taps of window samples t0 (low half) and t0 + 1 (high half) of
// the 24 (UP, phase p) / 24 R (DOWN) samples that end at x[g] / x[g R + R - 1]
constexpr uint32_t rs_pair(uint32_t dir, uint32_t R, uint32_t p, uint32_t t0)
{
    const int16_t *tab = rs_table(dir, R);
    const uint32_t last = dir == IGDSP_RS_UP ? p * kRsTaps + kRsTaps - 1u : kRsTaps * R - 1u;
    return (uint32_t)(uint16_t)tab[last - t0] | ((uint32_t)(uint16_t)tab[last - t0 - 1u] << 16);
}
// igdsp_rs_frame's rule: one frame of one channel, n_in input samples (checked by the caller), the state advanced; *sat (optional):
// the clamp fired
inline void rs_frame_run(igdsp_rs_state &st, uint32_t dir, uint32_t R, const int16_t *in, uint32_t n_in, int16_t *out, bool *sat = nullptr)
{
    int16_t x[kRsHist + IGDSP_MAX_PAYLOAD * 6u];
    for (uint32_t i = 0; i < kRsHist; ++i) x[i] = st.hist[i];
    for (uint32_t i = 0; i < n_in; ++i) x[kRsHist + i] = in[i];
    const int16_t *tab = rs_table(dir, R);
    bool clamped = false;
    const uint32_t n_out = dir == IGDSP_RS_UP ? n_in * R : n_in / R;
    for (uint32_t q = 0; q < n_out; ++q) {
        const int32_t v = dir == IGDSP_RS_UP ? rs_up_raw(tab, q % R, x + kRsHist + q / R) : rs_down_raw(tab, R, x + kRsHist + q * R + R - 1u);
        clamped |= v != rs_clamp16(v);
        out[q] = (int16_t)rs_clamp16(v);
    }
    for (uint32_t i = 0; i < kRsHist; ++i) st.hist[i] = x[n_in + i];
    st.frames += 1u;
    if (sat) *sat = clamped;
}

// k_rs<DIR, R, COPY, VEC>.  A wave owns ch consecutive channels for the frames of one chunk, lanes lanes per channel, and keeps each
// channel's input row with its hist = 24 (UP) / 24 R (DOWN) predecessors in a tile of LDS: the predecessors of a chunk's first frame
// come sample by sample from the state or the earlier rows, those of every later frame are the tile's own tail moved to its front.  A
// lane takes units of 8 narrow samples: UP it reads the 32 tile samples that end with its 8 inputs and writes R 16-byte pieces, DOWN
// it reads the 32 R tile samples that end with its 8 R inputs and writes one.  The taps are compile-time constants of the
// instantiation (rs_pair), the samples come as dwords in both packings (the odd one by a funnel shift of two neighbours).
//   vector form: n % 8 == 0, the input base 16-byte (G.711: 8-byte) and d_out 16-byte aligned: 16-byte loads and stores;
//   general form: everything else: the same units, loaded and stored a sample at a time.
// Records: per output piece packed dot products and min / max of the values before the clamp, folded per output row in LDS.
// The grid is sized for the blocks a CU holds (rs_resident); frames are cut into chunks until a wave has about kRsItemsPerWave items.
// The state is written by k_rs_state behind the kernel on the stream (the chunks of a channel all read it).
constexpr int kRsWaves = 4;                               // waves per block, one per SIMD, independent of each other: the largest tiles (DOWN by 6) stay below 64 KiB
constexpr uint32_t kRsMaxResident = 3;                    // blocks per CU the grid is sized for where the LDS admits them: 12 waves per CU (the sweep: DESIGN 3.18)
constexpr uint32_t kRsItemsPerWave = 4;                   // frames are cut until a wave has about this many items: the grid-stride tail is a quarter at most
constexpr uint32_t kRsStateThreads = 192;                 // k_rs_state: a block takes a channel at a time, a thread per history sample
constexpr uint32_t rs_ch(uint32_t dir) { return dir == IGDSP_RS_UP ? 16u : 4u; }          // channels of a wave
constexpr uint32_t rs_lanes(uint32_t dir) { return 64u / rs_ch(dir); }                     // lanes per channel
constexpr uint32_t rs_hist(uint32_t dir, uint32_t R) { return dir == IGDSP_RS_UP ? kRsTaps : kRsTaps * R; }   // predecessors kept in the tile
constexpr uint32_t rs_tile(uint32_t dir, uint32_t R) { return rs_hist(dir, R) + (dir == IGDSP_RS_UP ? IGDSP_MAX_PAYLOAD : IGDSP_MAX_PAYLOAD * R); }          // samples per channel
// LDS of a block: the tiles, a 16-byte slot per channel and output sub-frame for the records, the 1 KiB G.711 table (UP)
constexpr uint32_t rs_lds_bytes(uint32_t dir, uint32_t R)
{
    return (uint32_t)kRsWaves * rs_ch(dir) * (rs_tile(dir, R) * 2u + R * 16u) + (dir == IGDSP_RS_UP ? 1024u : 0u);
}
// blocks of k_rs a CU holds: what 160 KiB of LDS admit, kRsMaxResident at most; k_rs's launch bound gives each wave 512 / this many VGPRs
constexpr uint32_t rs_resident(uint32_t dir, uint32_t R) { return std::min(kRsMaxResident, 163840u / (rs_lds_bytes(dir, R) + 16u)); }
// IGDSP_RS_BLOCKS: blocks per CU of k_rs's grid, for tools/rs_bench.py's sweep, which changes it between launches of one process: the one
// variable is looked up per launch, nothing else is parsed
inline std::optional<int> rs_blocks_from_env()
{
    if (const char *e = std::getenv("IGDSP_RS_BLOCKS")) return std::atoi(e);
    return std::nullopt;
}
struct RsRoute {
    uint32_t vec = 0;                      // the vector form
    uint32_t pieces = 0;                   // units of 8 narrow samples per row
    uint32_t ch = 0, groups = 0;           // channels per wave; channel groups
    uint32_t chunk_frames = 0, chunks = 0; // frames per chunk (the last takes the rest); items = groups * chunks
    uint32_t grid = 0, threads = 0, lds = 0;
    uint32_t state_grid = 0;               // k_rs_state behind the kernel (0: the yardstick: nobody writes the state)
};
inline RsRoute rs_route(uint32_t dir, uint32_t R, uint32_t C, uint32_t F, uint32_t n, bool g711, bool yardstick, uintptr_t in, uintptr_t out,
                        uint32_t cus, std::optional<int> blocks = std::nullopt)
{
    RsRoute r;
    if (!rs_dir_ok(dir) || !rs_factor_ok(R) || (uint64_t)C * F == 0 || n == 0 || n > IGDSP_MAX_PAYLOAD || (uint64_t)C * F >= 0xFFFFFFE0ull) return r;
    if (g711 && dir != IGDSP_RS_UP) return r;
    r.vec = (n & 7u) == 0u && aligned(in, g711 ? 8 : 16) && aligned(out, 16) ? 1u : 0u;
    r.pieces = (n + 7u) / 8u;
    r.ch = rs_ch(dir);
    r.groups = (uint32_t)(((uint64_t)C + r.ch - 1u) / r.ch);
    const uint32_t per_cu = blocks && *blocks >= 1 && *blocks <= 8 ? (uint32_t)*blocks : rs_resident(dir, R);
    const uint32_t want = std::max(1u, cus) * per_cu * (uint32_t)kRsWaves * kRsItemsPerWave;
    const uint32_t cuts = r.groups >= want ? 1u : std::min(F, (want + r.groups - 1u) / r.groups);
    r.chunk_frames = (F + cuts - 1u) / cuts;
    r.chunks = (F + r.chunk_frames - 1u) / r.chunk_frames;
    r.grid = blocks_for((uint64_t)r.groups * r.chunks, kRsWaves, std::max(1u, cus) * per_cu);
    r.threads = kRsWaves * 64;
    r.lds = rs_lds_bytes(dir, R);
    r.state_grid = yardstick ? 0u : std::min(C, std::max(1u, cus) * 8u);
    return r;
}

// ---- igdsp_dbuf_run (launch_dbuf_run): k_dbuf<COPY>.  A wave owns one channel for the steps of one part (<= kDbufPart steps) and walks
// them in order: the scalars in registers, the samples in the channel's ring in global memory (a step touches the row it appends, the
// row it takes and the 280 samples of a shrink), the shrink's window in the wave's LDS.  A launch of more steps goes out in parts; the
// state carries between them as between launches.  The grid is one wave per channel, and the kernel is kept small enough for
// kDbufResident blocks on a CU (8 waves per SIMD: at most 64 VGPRs each, tests/test_dbuf_resources_cpu.py): the walk is a chain of
// dependent memory round trips, and only other waves hide them.
//   vector form: n even, d_in and d_out dword aligned: a row moves as dwords while the channel's ring position is even;
//   general form: everything else, and a channel of the vector form while its ring position is odd: a sample at a time.
constexpr int kDbufWaves = 4;                             // waves per block, a channel each, independent of each other
constexpr uint32_t kDbufPart = 128;                       // steps per part
constexpr uint32_t kDbufResident = 8;                     // blocks per CU k_dbuf's registers and LDS admit
constexpr uint32_t kDbufLdsBytes = kDbufWaves * 2u * IGDSP_DBUF_WIN * 2u;   // a block's LDS: per wave the window and its shifted copy
struct DbufRoute {
    uint32_t vec = 0;                      // the vector form
    uint32_t grid = 0, threads = 0, lds = 0;
    uint32_t part_steps = 0, parts = 0;    // the last part takes the rest
};
inline DbufRoute dbuf_route(uint32_t C, uint32_t T, uint32_t n, uint32_t M, uintptr_t in, uintptr_t out)
{
    DbufRoute r;
    if ((uint64_t)C * T == 0 || (uint64_t)C * T >= 0xFFFFFFE0ull || n == 0 || n > IGDSP_MAX_PAYLOAD || M < 2u * n || M > IGDSP_DBUF_CAP) return r;
    r.vec = (n & 1u) == 0u && aligned(in | out, 4) ? 1u : 0u;
    r.grid = (uint32_t)(((uint64_t)C + kDbufWaves - 1) / kDbufWaves);
    r.threads = kDbufWaves * 64;
    r.lds = kDbufLdsBytes;
    r.part_steps = std::min(T, kDbufPart);
    r.parts = (T + kDbufPart - 1) / kDbufPart;
    return r;
}

// ---- igdsp_spectrum (launch_spectrum): k_spec<COPY>.  A wave owns one channel for all the launch's frames, because the averaged array
// is sequential in time: the 1 024 samples of history as a ring in the wave's LDS, the averaged array in registers (8 bins per lane),
// the next frame's row load in flight during the transform.  A hop packs the windowed history as 512 complex points, 8 per lane, and
// runs three radix-8 passes in registers with two exchanges through the wave's LDS tile (8 rows of 64 points, padded to kSpecTileRow
// so that both the row-wise stores and the strided loads of an exchange spread over the banks), then the split pass to the 512 bins
// with the partner bins fetched from the mirror lane.  The window and the twiddle factors a lane needs are the same for every hop:
// they live in registers, which is why the kernel is sized for kSpecResident blocks per CU (16 waves, up to 128 VGPRs each) and not
// for more: a lane's eight butterflies are independent, so the transform hides its own latencies.  Waves of a block are independent
// of each other.  No parts: the frame loop is the wave's own.
constexpr int kSpecWaves = 4;                             // waves per block, a channel each
constexpr uint32_t kSpecResident = 4;                     // blocks per CU k_spec's registers and LDS admit
constexpr uint32_t kSpecTileRow = 72;                     // complex points per tile row: 64 and 8 of padding
constexpr uint32_t kSpecTile = 8u * kSpecTileRow;         // complex points of a wave's tile
constexpr uint32_t kSpecLdsBytes = kSpecWaves * (IGDSP_SPEC_N * 2u + kSpecTile * 8u);   // a block's LDS: per wave the ring and the tile
struct SpecRoute {
    uint32_t grid = 0, threads = 0, lds = 0;
};
inline SpecRoute spec_route(uint32_t C, uint32_t F, uint32_t n)
{
    SpecRoute r;
    if ((uint64_t)C * F == 0 || (uint64_t)C * F >= 0xFFFFFFE0ull || n == 0 || n > IGDSP_MAX_PAYLOAD) return r;
    r.grid = (uint32_t)(((uint64_t)C + kSpecWaves - 1) / kSpecWaves);
    r.threads = kSpecWaves * 64;
    r.lds = kSpecLdsBytes;
    return r;
}

// ---- igdsp_tone_detect (launch_tone_detect): k_tdet<COPY, E0> (+ k_tdet_list<WRITE> and the link stage's k_link_scan for a list).
// A DPP row of 16 lanes serves one channel for all the launch's frames (the debounce is sequential in time): lanes 0..7 are the low
// group's bins, lanes 8..15 the high group's, so one three-step butterfly over eight lanes finds both groups' maxima.  A wave is four
// channels, a block kTdetWaves waves.  The block's LDS holds one plan's reference table (16 bytes per two sample pairs and lane: the
// cosine and sine values), and per channel 128 + 256 values v: the history and the frame, which the 16 lanes read as broadcasts.  The
// block walks the distinct plans of its channels one after the other (one pass when they share a plan).  E0: how evaluation 0's window
// is aligned (n % 8 == 0: 8-byte reads, n % 4 == 0: dwords, else halves).  Registers: the route is written for kTdetResident blocks per CU (80 VGPRs).
// The list: ListRoute.
constexpr int kTdetWaves = 8;                             // waves per block
constexpr uint32_t kTdetChans = kTdetWaves * 4u;          // channels per block
constexpr uint32_t kTdetResident = 3;                     // blocks per CU: 3 x 40 KiB of LDS, 6 waves per SIMD
constexpr uint32_t kTdetBuf = 128u + 256u;                // values per channel in LDS
constexpr uint32_t kTdetLdsBytes = 128u * 16u * 8u + kTdetChans * kTdetBuf * 2u + kTdetChans * 4u;   // table, buffers, the channels' plans
struct TdetRoute : ListRoute {             // the list: k_tdet_list
    uint32_t grid = 0, threads = 0, lds = 0;
    uint32_t e0 = 0;                       // k_tdet<, E0>: how evaluation 0's window is aligned in LDS (0: n % 8 == 0, 1: n % 4 == 0, 2: else)
};
inline uint64_t tdet_work_bytes(uint32_t C, uint32_t F, bool with_rec) { return list_work_bytes(C, F, with_rec, sizeof(igdsp_tdet_rec)); }
inline TdetRoute tdet_route(uint32_t C, uint32_t F, uint32_t n, bool list, bool with_rec)
{
    TdetRoute r;
    if ((uint64_t)C * F == 0 || (uint64_t)C * F >= 0xFFFFFFE0ull || n < 2u || n > IGDSP_MAX_PAYLOAD || (n & 1u)) return r;
    static_cast<ListRoute &>(r) = list_route(C, F, list, with_rec, sizeof(igdsp_tdet_rec));
    r.grid = (uint32_t)(((uint64_t)C + kTdetChans - 1u) / kTdetChans);
    r.threads = kTdetWaves * 64;
    r.lds = kTdetLdsBytes;
    r.e0 = n % 8u == 0u ? 0u : (n % 4u == 0u ? 1u : 2u);
    return r;
}

// ---- igdsp_echo_cancel (launch_echo_cancel): k_ec<NEAR_G711, L, COPY>.  A DPP row of 16 lanes owns a channel for the whole launch (the
// adaptation is sequential in time): a lane keeps L / 16 consecutive weights in registers; a wave is four channels, a block kEcWaves
// waves.  LDS per channel: kEcPad values, the shifted far history of L values and the frame of up to 256 behind it, kEcPad values
// (a block's window is read anchored at the block's END, so a short last block reads below the frame and the lowest lane below the
// history), and the near row behind kEcPad values; the output overwrites the near row in place.  Registers: the route is written for
// kEcResident blocks per CU (3 waves per SIMD, 168 VGPRs).
constexpr int kEcWaves = 4;                               // waves per block
constexpr uint32_t kEcChans = kEcWaves * 4u;              // channels per block
constexpr uint32_t kEcResident = 3;                       // blocks per CU
constexpr uint32_t kEcPad = 8;
constexpr uint32_t kEcXBuf = kEcPad + 256u + 256u + kEcPad;   // values per channel: pad, history, frame, pad
constexpr uint32_t kEcNBuf = kEcPad + 256u;                   // values per channel: pad, near row
constexpr uint32_t kEcLdsBytes = kEcChans * (kEcXBuf + kEcNBuf) * 2u;
struct EcRoute {
    uint32_t grid = 0, threads = 0, lds = 0;
    uint32_t tail = 0;                     // k_ec<, L, >
    uint32_t blocks = 0;                   // blocks of 8 (the last may be shorter) per frame
};
inline EcRoute ec_route(uint32_t C, uint32_t F, uint32_t n, uint32_t tail)
{
    EcRoute r;
    if ((uint64_t)C * F == 0 || (uint64_t)C * F >= 0xFFFFFFE0ull || n < 2u || n > IGDSP_MAX_PAYLOAD || (n & 1u) || (tail != 128u && tail != 256u)) return r;
    r.grid = (uint32_t)(((uint64_t)C + kEcChans - 1u) / kEcChans);
    r.threads = kEcWaves * 64;
    r.lds = kEcLdsBytes;
    r.tail = tail;
    r.blocks = (n + 7u) / 8u;
    return r;
}

// ---- igdsp_agc_run (launch_agc): k_agc<IN_G711, COPY>.  Half a wave, 32 lanes, owns a channel for the whole launch (the gain and the
// limiter's cap run through time): lane b owns block b of 8 samples, one load and one store per frame, and knot b + 1; a frame of n
// samples keeps n / 8 of the 32 lanes busy.  A wave is two channels, a block kAgcWaves waves.  No LDS: the lanes talk by DPP and
// ds_bpermute.  Registers: the route is written for kAgcResident blocks per CU (8 waves per SIMD, 64 VGPRs).
constexpr int kAgcWaves = 4;                              // waves per block
constexpr uint32_t kAgcLanes = 32;                        // lanes per channel
constexpr uint32_t kAgcChans = kAgcWaves * 2u;            // channels per block
constexpr uint32_t kAgcResident = 8;                      // blocks per CU
struct AgcRoute {
    uint32_t grid = 0, threads = 0, lds = 0;
    bool g711 = false, copy = false;       // k_agc<IN_G711, COPY>
    uint32_t blocks = 0;                   // blocks of 8 per frame = busy lanes per channel
};
inline AgcRoute agc_route(uint32_t C, uint32_t F, uint32_t n, bool g711, bool yardstick)
{
    AgcRoute r;
    if ((uint64_t)C * F == 0 || (uint64_t)C * F >= 0xFFFFFFE0ull || n < 8u || n > IGDSP_MAX_PAYLOAD || (n & 7u)) return r;
    r.grid = (uint32_t)(((uint64_t)C + kAgcChans - 1u) / kAgcChans);
    r.threads = kAgcWaves * 64;
    r.lds = 0;
    r.g711 = g711;
    r.copy = yardstick;
    r.blocks = n / 8u;
    return r;
}

// ---- igdsp_vad_run (launch_vad): k_vad<IN_G711, COPY> (+ k_vad_list<WRITE> and the link stage's k_link_scan for a list).  A DPP row of
// 16 lanes owns a channel for the whole launch (the floor, the hangover and the noise model run through time): lane p and lane p + 16's
// turn load a piece of 8 samples each (one 8-byte load of codes or one 16-byte load of PCM), the row goes to LDS as v = x >> 2 between
// zeros and once more one sample ahead (for the odd lags), and lane k sums lag k over the whole row (the transposed shape: 11 of 16 lanes
// busy, no reduction) and keeps A[k].  A wave is four channels, a block kVadWaves waves.  LDS: the level table times n, per channel the
// row twice and the rare path's arrays (A, R, a, the payload).  Registers: the route is written for kVadResident blocks per CU (6 waves per SIMD, 80 VGPRs: at 64 the
// PCM form spills).
// The list: ListRoute.
constexpr int kVadWaves = 4;                              // waves per block
constexpr uint32_t kVadLanes = 16;                        // lanes per channel
constexpr uint32_t kVadChans = kVadWaves * 4u;            // channels per block
constexpr uint32_t kVadResident = 6;                      // blocks per CU
constexpr uint32_t kVadPad = 16;                          // zeros in front of the row: the highest lane's lag is 15
constexpr uint32_t kVadBuf = kVadPad + 256u + 8u;         // values per channel in LDS: zeros, the row, zeros (the second copy's last pair ends in one)
constexpr uint32_t kVadLdsBytes = 128u * 8u + kVadChans * (kVadBuf * 2u + 256u * 2u + 3u * 12u * 8u + 16u);   // table; row, its second copy, A, R, a, payload
struct VadRoute : ListRoute {              // the list: k_vad_list
    uint32_t grid = 0, threads = 0, lds = 0;
    bool g711 = false, copy = false;       // k_vad<IN_G711, COPY>
    uint32_t pieces = 0;                   // pieces of 8 samples per row: lanes p and p + 16 of the 16 take them in two turns
};
inline uint64_t vad_work_bytes(uint32_t C, uint32_t F, bool with_rec) { return list_work_bytes(C, F, with_rec, sizeof(igdsp_vad_rec)); }
inline VadRoute vad_route(uint32_t C, uint32_t F, uint32_t n, bool g711, bool yardstick, bool list, bool with_rec)
{
    VadRoute r;
    if ((uint64_t)C * F == 0 || (uint64_t)C * F >= 0xFFFFFFE0ull || n < 16u || n > IGDSP_MAX_PAYLOAD || (n & 7u)) return r;
    static_cast<ListRoute &>(r) = list_route(C, F, list, with_rec, sizeof(igdsp_vad_rec));
    r.grid = (uint32_t)(((uint64_t)C + kVadChans - 1u) / kVadChans);
    r.threads = kVadWaves * 64;
    r.lds = kVadLdsBytes;
    r.g711 = g711;
    r.copy = yardstick;
    r.pieces = n / 8u;
    return r;
}

// ---- the lane-per-channel tile (k_cng, k_filt): a lane owns a channel, a block is one wave, and the frame's rows lie in LDS as a tile
// that the wave fills and stores piece by piece (16 bytes of a row; the pieces of a tile are consecutive in memory).  A row is
// n / 2 + 1 dwords apart (odd: the lanes' dword accesses of one sample pair fall into different banks); behind the rows a byte per
// row for the stage's own use.  Item i of a pass is row i / P, piece i % P, the division done by the multiplier tile_inv(P): exact
// below 2^11 items for P <= 32 (on the device: tile_item, tile_piece, igdsp_lanes.h).
constexpr uint32_t tile_row_dwords(uint32_t n) { return n / 2u + 1u; }
constexpr uint32_t tile_lds_bytes(uint32_t chans, uint32_t n) { return chans * tile_row_dwords(n) * 4u + chans; }
constexpr uint32_t tile_inv(uint32_t pieces) { return (1u << 20) / pieces + 1u; }

// ---- igdsp_cng_run (launch_cng): k_cng<IN, COPY>.  A lane owns a channel for the whole launch (the lattice is serial in the sample: the
// parallelism is across channels); a block is one wave and kCngChans channels.  LDS: the frame's kCngChans rows as the lane-per-channel tile above,
// the row's byte says who fills it.  The wave fills the voice rows and stores the whole tile.  Registers and LDS: the route is written for kCngResident blocks per CU, one wave per SIMD at 65 536 channels
// (128 VGPRs; 33 088 bytes of LDS at n = 256).
constexpr uint32_t kCngChans = 64;                        // channels per block: the lanes of its one wave
constexpr uint32_t kCngResident = 4;                      // blocks per CU
constexpr uint32_t kCngVgprs = 128;
constexpr int kCngNone = 0, kCngG711 = 1, kCngPcm = 2;    // k_cng<IN, >: the voice input
constexpr uint32_t cng_row_dwords(uint32_t n) { return tile_row_dwords(n); }   // the name the route driver checks the tile by
static_assert(kCngResident * tile_lds_bytes(kCngChans, 256) <= 160u * 1024u, "the resident blocks' tiles fit a CU's LDS");
struct CngRoute {
    uint32_t grid = 0, threads = 0, lds = 0;
    int in = kCngNone;                     // k_cng<IN, COPY>
    bool copy = false;
    uint32_t pieces = 0;                   // pieces of 8 samples per row
    uint32_t passes = 0;                   // turns of the wave per tile pass: ceil(kCngChans * pieces / 64)
    uint32_t inv = 0;                      // item / pieces == (item * inv) >> 20
};
inline CngRoute cng_route(uint32_t C, uint32_t F, uint32_t n, bool g711, bool pcm, bool yardstick)
{
    CngRoute r;
    if ((uint64_t)C * F == 0 || (uint64_t)C * F >= 0xFFFFFFE0ull || n < 16u || n > IGDSP_MAX_PAYLOAD || (n & 7u)) return r;
    r.grid = (uint32_t)(((uint64_t)C + kCngChans - 1u) / kCngChans);
    r.threads = 64;
    r.lds = tile_lds_bytes(kCngChans, n);
    r.in = g711 ? kCngG711 : (pcm ? kCngPcm : kCngNone);
    r.copy = yardstick;
    r.pieces = n / 8u;
    r.passes = (kCngChans * r.pieces + 63u) / 64u;
    r.inv = tile_inv(r.pieces);
    return r;
}

// ---- igdsp_filt_run (launch_filt): k_filt<IN, S, COPY>.  A lane owns a channel for the whole launch (the recurrence is serial in the
// sample: the parallelism is across channels); a block is one wave and kFiltChans channels.  S = 1, 2 or 4 sections run per sample: the
// entry's max_sections rounded up (a channel with fewer runs identity sections, so the lanes of a wave do not diverge); the yardstick
// runs none and is built once per input form (S = 1).  LDS: the frame's kFiltChans rows as the lane-per-channel tile above,
// filtered in place, the row's byte its law.  The wave fills the tile and stores it.  The NEXT frame's pieces are loaded into
// registers before the sample loop and written to the tile behind the store pass: the first kFiltAhead turns of 16 bytes (PCM) or 8
// (codes) per lane, 64 or 32 VGPRs; a row's turns past those (n > 128) are loaded behind the store pass.  Registers and LDS: the route is written for kFiltResident blocks per CU, one wave per SIMD at
// 65 536 channels and never more than two (kFiltVgprs = 256 of a SIMD's 512; 33 088 bytes of LDS at n = 256).
constexpr uint32_t kFiltChans = 64;                       // channels per block: the lanes of its one wave
constexpr uint32_t kFiltResident = 4;                     // blocks per CU
constexpr uint32_t kFiltVgprs = 256;
constexpr uint32_t kFiltMaxPieces = IGDSP_MAX_PAYLOAD / 8;   // pieces of 8 samples per row = turns of the wave per tile pass
constexpr uint32_t kFiltAhead = 16;                       // turns of the next frame held in registers through the sample loop
static_assert(2u * kFiltAhead == kFiltMaxPieces, "the early and the late turns cover a row");
constexpr int kFiltG711 = 1, kFiltPcm = 2;                // k_filt<IN, , >
constexpr uint32_t filt_row_dwords(uint32_t n) { return tile_row_dwords(n); }  // the name the route driver checks the tile by
static_assert(kFiltResident * tile_lds_bytes(kFiltChans, 256) <= 160u * 1024u && 2u * kFiltVgprs <= 512u, "the resident blocks' tiles fit a CU's LDS, two waves a SIMD's registers");
struct FiltRoute {
    uint32_t grid = 0, threads = 0, lds = 0;
    int in = 0, sections = 0;              // k_filt<IN, S, COPY>
    bool copy = false;
    uint32_t pieces = 0;                   // pieces of 8 samples per row = turns of the wave per tile pass
    uint32_t inv = 0;                      // item / pieces == (item * inv) >> 20
    uint32_t max_sections = 0;             // what a plan may hold and still run: 1..4
};
inline FiltRoute filt_route(uint32_t C, uint32_t F, uint32_t n, bool g711, uint32_t max_sections, bool yardstick)
{
    FiltRoute r;
    if ((uint64_t)C * F == 0 || (uint64_t)C * F >= 0xFFFFFFE0ull || n < 8u || n > IGDSP_MAX_PAYLOAD || (n & 7u) || max_sections > 4u) return r;
    r.grid = (uint32_t)(((uint64_t)C + kFiltChans - 1u) / kFiltChans);
    r.threads = 64;
    r.lds = tile_lds_bytes(kFiltChans, n);
    r.in = g711 ? kFiltG711 : kFiltPcm;
    r.max_sections = max_sections == 0u ? 4u : max_sections;
    r.sections = yardstick ? 1 : (r.max_sections <= 2u ? (int)r.max_sections : 4);
    r.copy = yardstick;
    r.pieces = n / 8u;
    r.inv = tile_inv(r.pieces);
    return r;
}

// ---- igdsp_ns_run (launch_ns): k_ns<IN, COPY>.  kNsLanes = 16 lanes own a channel for the whole launch (the state is sequential in
// time); a block is one wave and kNsChans = 4 channels.  Per channel in LDS: the state (1 072 bytes, loaded once, stored once), the
// transform's 128 complex points with the band gains and the lanes' partial sums behind them (NsWork, igdsp_ns.h), and the frame's row
// (up to 320 samples, worked in place).  The phases of a hop (igdsp_ns.h) are divided over the 16 lanes: a pass of the transform is
// four butterflies a lane, the bands two a lane; between phases stands a same-wave LDS fence, never a barrier.  A row is n / 8 pieces of
// 8 samples (16 bytes of PCM, 8 of codes): lane l of the channel takes pieces l, l + 16, l + 32 (kNsTurns = 3 turns cover 40 pieces),
// loads the NEXT frame's before the hops and stores the output's as 16-byte pieces behind them.  Registers and LDS: the route is
// written for kNsResident = 8 blocks per CU, two waves per SIMD (kNsVgprs = 256 of a SIMD's 512 each; 13 568 bytes of LDS a block at n = 320).
constexpr uint32_t kNsLanes = 16;                         // lanes per channel: a DPP row
constexpr uint32_t kNsChans = 4;                          // channels per block: the rows of its one wave
constexpr uint32_t kNsResident = 8;                       // blocks per CU
constexpr uint32_t kNsVgprs = 256;
constexpr uint32_t kNsTurns = 3;                          // pieces per lane and row
constexpr uint32_t kNsMaxN = 320;
constexpr int kNsG711 = 1, kNsPcm = 2;                    // k_ns<IN, >
constexpr uint32_t kNsStateBytes = 1072, kNsWorkBytes = 1680;   // sizeof(igdsp_ns_state), sizeof(NsWork): static_asserted in igdsp_k_ns.hip
constexpr uint32_t ns_chan_bytes(uint32_t n) { return kNsStateBytes + kNsWorkBytes + ((n * 2u + 15u) & ~15u); }
constexpr uint32_t ns_lds_bytes(uint32_t n) { return kNsChans * ns_chan_bytes(n); }
static_assert(kNsLanes * kNsChans == 64 && kNsTurns * kNsLanes * 8u >= kNsMaxN && kNsResident * ns_lds_bytes(kNsMaxN) <= 160u * 1024u &&
              (kNsResident / 4u) * kNsVgprs <= 512u && ns_chan_bytes(80) % 16u == 0u, "a wave of channels; the turns cover a row; the resident blocks fit a CU");
struct NsRoute {
    uint32_t grid = 0, threads = 0, lds = 0;
    int in = 0;                            // k_ns<IN, COPY>
    bool copy = false;
    uint32_t pieces = 0;                   // pieces of 8 samples per row
};
inline NsRoute ns_route(uint32_t C, uint32_t F, uint32_t n, bool g711, bool yardstick)
{
    NsRoute r;
    if ((uint64_t)C * F == 0 || (uint64_t)C * F >= 0xFFFFFFE0ull || n == 0u || n > kNsMaxN || n % 80u) return r;
    r.grid = (uint32_t)(((uint64_t)C + kNsChans - 1u) / kNsChans);
    r.threads = 64;
    r.lds = ns_lds_bytes(n);
    r.in = g711 ? kNsG711 : kNsPcm;
    r.copy = yardstick;
    r.pieces = n / 8u;
    return r;
}

// ---- igdsp_srtp_protect / igdsp_srtp_unprotect (launch_srtp): k_srtp<DIR, MOVE>.  A lane owns a channel for the whole launch (index
// and replay window are serial in its frames); a block is one wave and kSrtpChans = 64 channels.  A frame's packets pass through an LDS
// tile in pieces of 64 bytes (one SHA-1 block, four AES blocks) of every packet: 64 rows of 16 words at a pitch of kSrtpPitch = 17
// words, whatever the stride; a piece is four turns of 16-byte items, item i = turn * 64 + lane being quarter i & 3 of row i >> 2.
// Beside the tile: the 1 KiB AES table, the lanes' round keys as [44][64] words and two words per row (the bytes to load, the bytes to
// store whole).  LDS is static.  Registers:
// the route is written for kSrtpResident = 8 blocks per CU, two waves per SIMD (kSrtpVgprs = 256 of a SIMD's 512 each).
constexpr uint32_t kSrtpChans = 64;                       // channels per block: the lanes of its one wave
constexpr uint32_t kSrtpPitch = 17;                       // words between two rows of the tile: odd, so the lanes' reads of word i spread over the banks
constexpr uint32_t kSrtpTurns = 4;                        // 16-byte items per lane and piece
constexpr uint32_t kSrtpResident = 8;                     // blocks per CU
constexpr uint32_t kSrtpVgprs = 256;
constexpr uint32_t kSrtpMaxStride = 2048;
constexpr uint32_t kSrtpLdsBytes = 256u * 4u + kSrtpChans * kSrtpPitch * 4u + 2u * kSrtpChans * 4u + 44u * kSrtpChans * 4u;   // table, tile, two words a row, round keys [44][64]
constexpr int kSrtpDirProtect = 0, kSrtpDirUnprotect = 1; // k_srtp<DIR, >
static_assert(kSrtpTurns * 64u * 16u == kSrtpChans * 64u && (kSrtpPitch & 1u) == 1u && kSrtpPitch >= 16u && kSrtpResident * kSrtpLdsBytes <= 160u * 1024u &&
              (kSrtpResident / 4u) * kSrtpVgprs <= 512u, "the turns cover a piece of every row; the resident blocks fit a CU");
struct SrtpRoute {
    uint32_t grid = 0, threads = 0, lds = 0;
    int dir = 0;                           // k_srtp<DIR, MOVE>
    bool move = false;
    uint32_t max_pieces = 0;               // pieces of 64 bytes a slot holds: the most a pass walks
};
inline SrtpRoute srtp_route(uint32_t C, uint32_t F, uint32_t pkt_stride, uint32_t out_stride, int dir, bool yardstick)
{
    SrtpRoute r;
    if ((uint64_t)C * F == 0 || (uint64_t)C * F >= 0xFFFFFFE0ull) return r;
    if (pkt_stride < 12u || pkt_stride > kSrtpMaxStride || (pkt_stride & 3u) || out_stride < 12u || out_stride > kSrtpMaxStride || (out_stride & 3u)) return r;
    if (dir != kSrtpDirProtect && dir != kSrtpDirUnprotect) return r;
    r.grid = (uint32_t)(((uint64_t)C + kSrtpChans - 1u) / kSrtpChans);
    r.threads = 64;
    r.lds = kSrtpLdsBytes;
    r.dir = yardstick ? kSrtpDirProtect : dir;
    r.move = yardstick;
    r.max_pieces = (pkt_stride + 63u) / 64u + 1u;                           // (the hash's padding may need a block behind the data's last)
    return r;
}

// ---- igdsp_srtcp_protect / igdsp_srtcp_unprotect (launch_srtcp): k_srtcp<DIR, MOVE> has k_srtp's geometry, LDS and residency: the 14-byte
// trailer does not pass the tile, so a slot's pieces and the strides' bounds are SRTP's
inline SrtpRoute srtcp_route(uint32_t C, uint32_t F, uint32_t pkt_stride, uint32_t out_stride, int dir, bool yardstick)
{
    return srtp_route(C, F, pkt_stride, out_stride, dir, yardstick);
}

// ---- igdsp_srtp_gcm_protect / igdsp_srtp_gcm_unprotect (launch_srtp_gcm): k_srtp_gcm<DIR, MOVE> has k_srtp's geometry (a lane a leg, 64
// legs a wave and block, the 64 x 17-word tile, four turns a piece) and LDS of its own: the AES table, the tile, two words a row and
// the lanes' round keys as [60][64] words (AES-256's schedule; a leg with a 128-bit key uses 44), and for GHASH the lanes' sixteen
// multiples of H as [16][4][64] words (Shoup's 4-bit tables, 16 KiB) with sixteen reduction words.  A leg's key size is in its state, not
// in the launch, so one instantiation per direction serves both.  37 696 bytes a block: kSrtpGcmResident = 4 blocks per CU fit its
// 160 KiB and a fifth does not, so a SIMD holds one wave, which may take all of its 512 registers (kSrtpGcmVgprs).
constexpr uint32_t kSrtpGcmResident = 4;
constexpr uint32_t kSrtpGcmVgprs = 512;
constexpr uint32_t kSrtpGcmRkWords = 60;
constexpr uint32_t kSrtpGcmTabWords = 16u * 4u;
constexpr uint32_t kSrtpGcmLdsBytes = 256u * 4u + kSrtpChans * kSrtpPitch * 4u + 2u * kSrtpChans * 4u + kSrtpGcmRkWords * kSrtpChans * 4u +
                                      kSrtpGcmTabWords * kSrtpChans * 4u + 16u * 4u;   // table, tile, two words a row, round keys, multiples of H, reduction
static_assert(kSrtpGcmResident * kSrtpGcmLdsBytes <= 160u * 1024u && (kSrtpGcmResident + 1u) * kSrtpGcmLdsBytes > 160u * 1024u &&
              ((kSrtpGcmResident + 3u) / 4u) * kSrtpGcmVgprs <= 512u, "the resident blocks fit a CU, and no more do");
inline SrtpRoute srtp_gcm_route(uint32_t C, uint32_t F, uint32_t pkt_stride, uint32_t out_stride, int dir, bool yardstick)
{
    SrtpRoute r = srtp_route(C, F, pkt_stride, out_stride, dir, yardstick);   // the grid, the strides' bounds; max_pieces: the last ciphertext
    if (r.grid) r.lds = kSrtpGcmLdsBytes;                                     // block's slot may lie a piece behind the data's last
    return r;
}

// ---- igdsp_rtcp_build (launch_rtcp_build): k_rtcp_build, and igdsp_rtcp_parse (launch_rtcp_parse): k_rtcp_parse.  A lane owns a leg for
// the launch (the report's prior and the last SR heard are serial in its ticks); a block is one wave and kRtcpChans = 64 legs.  Build:
// a row of the LDS tile is a whole packet, kRtcpRowWords = 34 words at a pitch of kRtcpRowPitch = 35 (odd), stored as kRtcpRowItems = 9
// turns of 16-byte items, item i = turn * 64 + lane being sixteenth i % 9 of row i / 9.  Parse: SRTP's tile, 64 rows of one 64-byte
// piece at pitch kSrtpPitch, and a word per row for the bytes to load.  LDS is static.  Written for kRtcpResident = 8 blocks per CU,
// two waves per SIMD (kRtcpVgprs = 256 of a SIMD's 512 each).
constexpr uint32_t kRtcpChans = 64;
constexpr uint32_t kRtcpRowWords = 34;                    // IGDSP_RTCP_MAX_BUILT / 4
constexpr uint32_t kRtcpRowPitch = 35;
constexpr uint32_t kRtcpRowItems = 9;                     // 16-byte items that cover a row
constexpr uint32_t kRtcpResident = 8;
constexpr uint32_t kRtcpVgprs = 256;
constexpr uint32_t kRtcpBuildLdsBytes = kRtcpChans * kRtcpRowPitch * 4u + kRtcpChans * 4u;        // the rows, a size a row
constexpr uint32_t kRtcpParseLdsBytes = kSrtpChans * kSrtpPitch * 4u + kSrtpChans * 4u;           // the tile, a limit a row
static_assert(kRtcpRowWords * 4u == 136u && kRtcpRowItems * 16u >= kRtcpRowWords * 4u && (kRtcpRowPitch & 1u) == 1u && kRtcpRowPitch >= kRtcpRowWords &&
              kRtcpChans == kSrtpChans && kRtcpResident * kRtcpBuildLdsBytes <= 160u * 1024u && (kRtcpResident / 4u) * kRtcpVgprs <= 512u,
              "a row holds the largest packet; the items cover it; parse uses SRTP's tile; the resident blocks fit a CU");
struct RtcpRoute {
    uint32_t grid = 0, threads = 0, lds = 0;
    bool move = false;                     // k_rtcp_build<MOVE>, k_rtcp_parse<MOVE>
    uint32_t max_pieces = 0;               // parse: pieces of 64 bytes a slot holds
};
inline RtcpRoute rtcp_build_route(uint32_t C, uint32_t F, uint32_t pkt_stride, bool yardstick)
{
    RtcpRoute r;
    if ((uint64_t)C * F == 0 || (uint64_t)C * F >= 0xFFFFFFE0ull) return r;
    if (pkt_stride < kRtcpRowWords * 4u || pkt_stride > kSrtpMaxStride || (pkt_stride & 3u)) return r;
    r.grid = (uint32_t)(((uint64_t)C + kRtcpChans - 1u) / kRtcpChans);
    r.threads = 64;
    r.lds = kRtcpBuildLdsBytes;
    r.move = yardstick;
    return r;
}
inline RtcpRoute rtcp_parse_route(uint32_t C, uint32_t F, uint32_t pkt_stride, bool yardstick)
{
    RtcpRoute r;
    if ((uint64_t)C * F == 0 || (uint64_t)C * F >= 0xFFFFFFE0ull) return r;
    if (pkt_stride < 8u || pkt_stride > kSrtpMaxStride || (pkt_stride & 3u)) return r;
    r.grid = (uint32_t)(((uint64_t)C + kRtcpChans - 1u) / kRtcpChans);
    r.threads = 64;
    r.lds = kRtcpParseLdsBytes;
    r.move = yardstick;
    r.max_pieces = (pkt_stride + 63u) / 64u;
    return r;
}

// ---- igdsp_tx_flush (launch_tx_staged): a wave owns kTsLegs staged legs (runs) of the flush; lanes 0 .. kTsLegs-1 decide, the
// whole wave writes the packets.  No dynamic LDS: each wave's records (kTsLegs x IGDSP_STAGE_DEPTH) are static.
constexpr int kTsWaves = 4;
constexpr int kTsLegs = 16;
struct TxStagedRoute {
    uint32_t n_groups = 0, grid = 0, threads = 0, lds = 0;
};
inline TxStagedRoute tx_staged_route(uint32_t n_runs, uint32_t cus)
{
    TxStagedRoute r;
    r.n_groups = (n_runs + kTsLegs - 1) / kTsLegs;
    r.grid = blocks_for(r.n_groups, kTsWaves, cus * 8u);
    r.threads = kTsWaves * 64;
    return r;
}

}  // namespace igdsp
