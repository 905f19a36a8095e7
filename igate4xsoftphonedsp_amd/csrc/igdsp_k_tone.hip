// igdsp_k_tone.hip — the bridge's tone generator (igdsp_tone_generate): pjmedia's tonegen port as RoIP_ED137::init_ringTone sets it up
// (Functions.cpp:532-571), batched over ports and frames, with the rows' lengths and records.
// Semantics: include/igdsp.h, section "Tone generator"; the rules themselves: the constexpr functions of igdsp_route.h (tone_sample,
// tone_frame_sample, tone_cmd, tone_advance), which igdsp_tone_frame runs on the host; independent restatement: tests/tone_model.py.
//
// Shape (tone_route, igdsp_route.h).  A write-only stream: nothing is loaded but a port's 8-byte state, its cmd byte, its plan index
// and the plan's segment.  A wave owns kTonePorts = 16 consecutive ports for the frames of one chunk, kToneLanes = 4 lanes per port.
// Per item the lanes of a port read its facts once; per frame they step the cycle position by n (one conditional modulo), check that
// the segment in their registers still holds it (else they search the plan's <= 8 segments) and take the row's 8-sample pieces j, j + 4,
// ..: the stores of a frame cover one run of 16 consecutive rows, 64 contiguous bytes per port and instruction.
//   a piece wholly in the un-faded part of an ON period: two phases advanced by addition, two 4-byte LDS lookups per sample (the table
//       as (value, delta) pairs), the eight lookups of an oscillator issued together, then tone_interp and tone_scale1 / tone_scale2;
//   a piece wholly in an OFF period, and every piece of an EMPTY row: zeros, no oscillator;
//   every other piece (a tone's edge, a fade, the wrap of the cycle, the end of a plan that does not loop): tone_frame_sample per sample.
// The records: packed 16-bit dot products and maxima per lane, two row_shr DPP steps fold the four lanes of a port, lane j == 3 stores
// the record: the 16 records of a wave and frame are one contiguous run.  Integer sums: any order gives the same bits.
// A launch of one chunk writes the state from the lanes that read it; a launch cut into chunks leaves that to k_tone_state behind it
// (the chunks of a port read the state the kernel must not have written yet).
#include "igdsp_device.h"
#include "igdsp_pcmrec.h"

namespace igdsp {

static_assert(kToneLanes == 4u && kTonePorts == 16u && kToneWaves >= 1 && kToneWaves <= 16, "the DPP fold and the record run assume 4 lanes per port");

__device__ const int16_t d_tone_sin[1024] = {IGDSP_TONE_SIN_VALUES};

struct ToneArgs {
    const igdsp_tone_plan *plans;
    const uint16_t *plan_of;
    const uint8_t *cmd;
    igdsp_tone_state *state;
    int16_t *pcm;
    uint16_t *len;
    igdsp_frame_stats *stats;
    uint32_t n_plans, P, F, n, rpf;    // rpf: rows per frame of pcm / len
    uint32_t pieces, groups, chunk_frames, chunks;
    uint32_t write_state;              // one chunk: the kernel writes the state
};

// the segment a port's lanes keep in registers: [start, end) of the cycle, and what tone_amp / tone_fade read
struct ToneSeg {
    igdsp_tone_seg sg;
    uint32_t end;
};

template <bool VEC, int MODE>
__global__ __launch_bounds__(kToneWaves * 64) void k_tone(const ToneArgs a)
{
    constexpr bool FILL = MODE == kToneFill, PCM = MODE != kToneStats, STATS = MODE == kToneBoth || MODE == kToneStats || FILL;
    __shared__ uint32_t pairs[FILL ? 1 : 1024];
    if constexpr (!FILL) {
        for (uint32_t i = threadIdx.x; i < 1024u; i += kToneWaves * 64u) pairs[i] = tone_pair(d_tone_sin[i], d_tone_sin[(i + 1u) & 1023u]);
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, r = lane >> 2, j = lane & 3u, n = a.n;
    const uint64_t n_items = (uint64_t)a.groups * a.chunks, stride = (uint64_t)gridDim.x * kToneWaves;
    for (uint64_t item = (uint64_t)blockIdx.x * kToneWaves + w; item < n_items; item += stride) {
        const uint32_t c = (uint32_t)(item / a.groups), g = (uint32_t)(item - (uint64_t)c * a.groups);   // neighbouring waves: neighbouring ports
        const uint32_t p = g * kTonePorts + r, f0 = c * a.chunk_frames, f1 = min(a.F, f0 + a.chunk_frames);
        const bool port = p < a.P;
        // the port's facts: state after the cmd, the plan (nullptr: none), whether it plays in this launch
        igdsp_tone_state st{0u, 0u};
        const igdsp_tone_plan *pl = nullptr;
        bool hold = false, plays = false, loop = false;
        uint32_t cycle = 0;
        uint64_t q = 0;                                                            // cycle position of sample 0 of the frame (looping: < cycle + n)
        if constexpr (!FILL) {
            if (port) {
                const uint32_t cmd = a.cmd ? a.cmd[p] : 0u;
                st = tone_cmd(a.state[p], cmd);
                hold = (cmd & IGDSP_TONE_CMD_HOLD) != 0u;
                const uint32_t pi = a.plan_of ? a.plan_of[p] : 0u;
                if (pi < a.n_plans) pl = a.plans + pi;
                if (pl) {
                    cycle = pl->cycle;
                    loop = (pl->options & IGDSP_TONE_LOOP) != 0u;
                    plays = !hold && tone_plays(*pl, st);
                }
                if (plays) {
                    q = (uint64_t)st.pos + (uint64_t)f0 * n;
                    if (loop && q >= cycle) q %= cycle;
                }
            }
        }
        ToneSeg seg{};                                                             // end == 0: none yet
        for (uint32_t f = f0; f < f1; ++f) {
            bool live = false;
            if constexpr (!FILL) {
                if (loop && q >= cycle) { q -= cycle; if (q >= cycle) q %= cycle; }   // one step of n <= 256: a subtraction unless cycle < n
                live = plays && (loop || q < cycle);
                if (live && !(q >= seg.sg.start && q < seg.end)) {                 // the segment of sample 0
                    const int32_t si = tone_seg_of(*pl, (uint32_t)q);
                    if (si >= 0) { seg.sg = pl->seg[si]; seg.end = tone_seg_end(*pl, (uint32_t)si); }
                    else seg.end = 0u;
                }
            }
            const bool in_seg = live && q >= seg.sg.start && q < seg.end;
            const uint32_t k0 = (uint32_t)q - seg.sg.start;                        // offset of sample 0 in the segment (in_seg)
            const uint64_t row = (uint64_t)f * a.rpf + p;
            uint64_t sq = 0;
            v2u16_t pk2 = (v2u16_t)(0);
            for (uint32_t pc = j; pc < a.pieces; pc += kToneLanes) {
                const uint32_t s0 = pc * 8u;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if constexpr (FILL) {
                    v = make_uint4(lane, pc, f, p);
                } else if (live) {
                    const uint64_t k = (uint64_t)k0 + s0, k_end = seg.sg.start + k + 8u;                  // the piece is [k, k + 8) of the segment
                    if (in_seg && k_end <= seg.end && k >= seg.sg.fade_in && k + 8u + seg.sg.fade_out <= seg.sg.on) {   // ON, no fade
                        // (the lookups of a piece go out together: one wait for eight instead of one per sample)
                        int32_t x[8];
                        uint32_t ph[8], tw[8];
                        ph[0] = (uint32_t)k * seg.sg.step1;
#pragma unroll
                        for (int i = 1; i < 8; ++i) ph[i] = ph[i - 1] + seg.sg.step1;
#pragma unroll
                        for (int i = 0; i < 8; ++i) tw[i] = pairs[ph[i] >> 22];
#pragma unroll
                        for (int i = 0; i < 8; ++i) x[i] = tone_interp(tw[i], ph[i]);
                        if (seg.sg.step2 != 0u) {
                            ph[0] = (uint32_t)k * seg.sg.step2;
#pragma unroll
                            for (int i = 1; i < 8; ++i) ph[i] = ph[i - 1] + seg.sg.step2;
#pragma unroll
                            for (int i = 0; i < 8; ++i) tw[i] = pairs[ph[i] >> 22];
#pragma unroll
                            for (int i = 0; i < 8; ++i) x[i] = tone_scale2(seg.sg, x[i], tone_interp(tw[i], ph[i]));
                        } else {
#pragma unroll
                            for (int i = 0; i < 8; ++i) x[i] = tone_scale1(seg.sg, x[i]);
                        }
                        v.x = ((uint32_t)x[0] & 0xFFFFu) | ((uint32_t)x[1] << 16);
                        v.y = ((uint32_t)x[2] & 0xFFFFu) | ((uint32_t)x[3] << 16);
                        v.z = ((uint32_t)x[4] & 0xFFFFu) | ((uint32_t)x[5] << 16);
                        v.w = ((uint32_t)x[6] & 0xFFFFu) | ((uint32_t)x[7] << 16);
                    } else if (in_seg && k_end <= seg.end && k >= seg.sg.on) {                            // OFF: zeros
                    } else {
                        // (not unrolled: the eight samples pass through v as through a shift register, sample 0 ends in v.x's low half)
                        for (uint32_t i = 0; i < 8u; ++i) {
                            const uint32_t x = (uint32_t)tone_frame_sample(pairs, *pl, q, s0 + i);
                            v.x = (v.x >> 16) | (v.y << 16); v.y = (v.y >> 16) | (v.z << 16);
                            v.z = (v.z >> 16) | (v.w << 16); v.w = (v.w >> 16) | (x << 16);
                        }
                    }
                }
                if constexpr (!VEC) {                                              // the last piece of a row of n % 8 != 0 samples: 0 past n
                    const uint32_t valid = n - s0;
                    auto keep = [&](uint32_t first) { return valid > first + 1u ? 0xFFFFFFFFu : (valid > first ? 0xFFFFu : 0u); };
                    v.x &= keep(0u); v.y &= keep(2u); v.z &= keep(4u); v.w &= keep(6u);
                }
                if constexpr (STATS && !FILL) { pcm_acc2(v.x, sq, pk2); pcm_acc2(v.y, sq, pk2); pcm_acc2(v.z, sq, pk2); pcm_acc2(v.w, sq, pk2); }
                if constexpr (PCM) {
                    if (port) {
                        int16_t *dst = a.pcm + row * n + s0;
                        if constexpr (VEC) {
                            *reinterpret_cast<uint4 *>(dst) = v;
                        } else {
                            const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                            for (uint32_t i = 0; i < 8u; ++i) if (s0 + i < n) dst[i] = (int16_t)(uint16_t)(wd[i >> 1] >> (16u * (i & 1u)));
                        }
                    }
                }
            }
            if (a.len && port && j == 0u) a.len[row] = (uint16_t)(live || FILL ? n : 0u);
            if constexpr (STATS) {
                // every lane of the wave is here: the fold's DPP steps read the neighbours' registers
                const uint64_t sumsq = group_sum_u64<kToneLanes>(sq);              // a lane's sum is below 64 * 2^30
                const uint32_t pk = group_fold<kToneLanes>(max((uint32_t)pk2.x, (uint32_t)pk2.y), OpMax{});
                if (j == 3u && port && a.stats) {
                    uint4 rec = pcm_record_empty();                                // (as a conditional expression this schedules differently:
                    if (live) rec = pcm_record(sumsq, pk, n, 0u);                  // profiles/pcm_record_isa.md)
                    st_record_block(a.stats + (uint64_t)f * a.P + (uint64_t)g * kTonePorts, r, rec);
                }
            }
            q += n;
        }
        if constexpr (!FILL) {
            if (a.write_state && port && j == 0u) a.state[p] = pl && !hold ? tone_advance(*pl, st, (uint64_t)a.F * n) : st;
        }
    }
}

// the state of a launch that was cut into chunks: a thread per port, behind k_tone on the stream
__global__ __launch_bounds__(kToneStateThreads) void k_tone_state(const ToneArgs a)
{
    const uint32_t p = blockIdx.x * kToneStateThreads + threadIdx.x;
    if (p >= a.P) return;
    const uint32_t cmd = a.cmd ? a.cmd[p] : 0u, pi = a.plan_of ? a.plan_of[p] : 0u;
    const igdsp_tone_state st = tone_cmd(a.state[p], cmd);
    const bool moves = pi < a.n_plans && (cmd & IGDSP_TONE_CMD_HOLD) == 0u;
    a.state[p] = moves ? tone_advance(a.plans[pi], st, (uint64_t)a.F * a.n) : st;
}

hipError_t launch_tone(const LaunchCfg &cfg, const igdsp_tone_plan *plans, uint32_t n_plans, const uint16_t *plan_of, const uint8_t *cmd,
                       igdsp_tone_state *state, uint32_t P, uint32_t F, uint32_t n, uint32_t rows_per_frame, int16_t *pcm, uint16_t *len,
                       igdsp_frame_stats *stats, bool yardstick, hipStream_t s)
{
    const ToneRoute r = tone_route(P, F, n, pcm != nullptr, stats != nullptr, yardstick, reinterpret_cast<uintptr_t>(pcm), (uint32_t)cfg.compute_units);
    if (r.grid == 0) return hipSuccess;
    const ToneArgs a{plans, plan_of, cmd, state, pcm, len, stats, n_plans, P, F, n, rows_per_frame ? rows_per_frame : P,
                     r.pieces, r.groups, r.chunk_frames, r.chunks, r.chunks == 1u ? 1u : 0u};
    with_bool(r.vec != 0u, [&](auto V) { with_key(Keys<kToneBoth, kTonePcm, kToneStats, kToneFill>{}, r.mode, [&](auto M) {
        hipLaunchKernelGGL((k_tone<V, M>), dim3(r.grid), dim3(r.threads), 0, s, a); }); });
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (r.state_grid) hipLaunchKernelGGL(k_tone_state, dim3(r.state_grid), dim3(kToneStateThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace igdsp
