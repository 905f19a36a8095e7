// igdsp_io.hip — placement-aware allocation of the hot path's input / output buffers (igdsp_io_alloc, include/igdsp.h).
//
// Why it exists.  On MI355X a kernel that READS one class of device memory and WRITES another runs ~13 % faster than one
// that reads and writes the same class, and a bulk write stream spread over two classes (neither the inputs') is another
// 5-8 % faster (three classes of ~96 GB, in runs of tens of GiB of consecutive allocations — consistent with
// the three stack-ID ranks of the 12-high HBM3E stacks: write-to-read turnaround is paid inside a rank).  Which class an
// allocation lands in is not visible through any API and differs per process, so the only way to place buffers is to
// measure.  Round 1 did that in bench.py (a 200 GB arena and timed launches); a host that followed INTEGRATION.md got the
// slow case.  This file moves it into the product:
//
//   * physical memory is taken in CHUNKS (hipMemCreate, 128 MiB) and each chunk is classified by timing the bare
//     read + record-store stream (the meter kernel's traffic, k_stream_rw) reading the caller's INPUT buffers and writing
//     the chunk;
//   * buffers are virtual address ranges (hipMemAddressReserve) onto which chunks of the wanted class are mapped:
//     INPUT buffers first (their class is "A" by definition), RECORD buffers from chunks of another class, BULK buffers
//     with their first half from one non-A class and their second half from the other (the queue-driven kernels visit the
//     two halves of a bulk output alternately, spread_batch in igdsp_device.h);
//   * exploration is sparse (every 16th chunk is probed until a new class shows up, then its neighbours) and bounded by
//     `explore_limit_bytes`; everything not mapped is released before returning.
//
// When the virtual-memory API is unavailable, the inputs are too small for the probe to mean anything (< 512 MiB: the
// batch lives in the 256 MiB Infinity Cache anyway) or no second class is found inside the limit, the buffers are still
// returned — consecutive chunks / plain hipMalloc — and the report says so (placed = 0).  No CPU path is involved anywhere.
#include "igdsp_ctx.h"

#include <algorithm>
#include <chrono>
#include <thread>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

using namespace igdsp;

struct igdsp_io_set {
    // cls[i] = class label of handles[i] in the context's labelling (igdsp_ctx::io_spare; 255 = unknown), valid while epoch matches
    struct Map { void *va = nullptr; size_t bytes = 0; std::vector<hipMemGenericAllocationHandle_t> handles; std::vector<uint8_t> cls; };
    uint32_t epoch = 0;
    std::vector<Map> maps;            // VMM path: one reserved range per buffer, chunk handles mapped back to back
    std::vector<void *> plain;        // fallback path: hipMalloc'ed buffers
    size_t chunk = 0;
    int device = 0;
};

namespace {

constexpr size_t kSrcChunks = 10;     // chunks behind a probe source: 1.25 GiB streamed per probe launch, far more than the 256 MiB Infinity Cache

struct Chunk {
    hipMemGenericAllocationHandle_t h{};
    float tA = -1.f;                  // probe time as the WRITE side against source A (< 0: not timed)
    float tB = -1.f;                  // ... against source B
    bool used = false;                // handed to a buffer (not to be released)
    bool mapped = false;              // currently mapped on its scratch slot
    bool in_src = false;              // currently part of a probe source
    int cls = -1;                     // class label once established (igdsp_ctx::io_spare), -1 unknown
};

// A probe source: kSrcChunks chunks mapped back to back on an address range of their own.  A range is mapped ONCE: on this
// stack an address that was un-mapped and mapped again keeps reaching the OLD chunk (igdsp_internal_vmm_remap_check), so a new
// source always gets a new range.
struct Source { void *va = nullptr; size_t n = 0; std::vector<size_t> idx; };

struct Explorer {
    igdsp_ctx *ctx = nullptr;
    hipStream_t s = nullptr;
    size_t chunk = 0;
    size_t va_align = 0;              // alignment asked of every address reservation
    hipMemAllocationProp prop{};
    hipMemAccessDesc acc{};
    void *cand_va = nullptr;          // scratch address space for probing: slot idx belongs to chunk idx, mapped at most once
    bool debug = false;
    hipEvent_t ea = nullptr, eb = nullptr;
    std::vector<Chunk> chunks;
    std::vector<Source> sources;
    size_t limit_chunks = 0;
    size_t probe_n = 0;
    uint32_t probes = 0;

    bool open(igdsp_ctx *c, size_t n) { ctx = c; s = c->stream; probe_n = n; return hipEventCreate(&ea) == hipSuccess && hipEventCreate(&eb) == hipSuccess; }
    bool ensure(size_t idx)
    {
        while (chunks.size() <= idx) {
            if (chunks.size() >= limit_chunks) return false;
            Chunk c;
            if (hipMemCreate(&c.h, chunk, &prop, 0) != hipSuccess) { (void)hipGetLastError(); return false; }
            chunks.push_back(c);
        }
        return true;
    }
    void unmap_scratch(size_t idx)
    {
        if (chunks[idx].mapped) { (void)hipMemUnmap((char *)cand_va + idx * chunk, chunk); chunks[idx].mapped = false; }
    }
    // time the bare read(src) + record-store(dst) stream: 2 untimed + 4 timed launches
    bool time_pair(const void *rd, void *dst, float *ms)
    {
        hipError_t e = hipSuccess;
        for (int i = 0; i < 2 && e == hipSuccess; ++i) e = launch_stream_rw(cfg_of(ctx, s), rd, probe_n, dst, s);
        if (e == hipSuccess) e = hipEventRecord(ea, s);
        for (int i = 0; i < 4 && e == hipSuccess; ++i) e = launch_stream_rw(cfg_of(ctx, s), rd, probe_n, dst, s);
        if (e == hipSuccess) e = hipEventRecord(eb, s);
        if (e == hipSuccess) e = hipEventSynchronize(eb);
        float t = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, ea, eb);
        if (e != hipSuccess) { (void)hipGetLastError(); return false; }
        *ms = t / 4.f;
        ++probes;
        return true;
    }
    // time chunk idx as the write side of (source -> chunk); the chunk is mapped on its own scratch slot for that
    bool probe(size_t idx, const Source &src, float *ms, const char *tag)
    {
        char *at = (char *)cand_va + idx * chunk;
        Chunk &c = chunks[idx];
        if (c.in_src) return false;
        if (!c.mapped) {
            if (hipMemMap(at, chunk, 0, c.h, 0) != hipSuccess) { (void)hipGetLastError(); return false; }
            c.mapped = true;
            if (hipMemSetAccess(at, chunk, &acc, 1) != hipSuccess) { (void)hipGetLastError(); return false; }
        }
        const bool ok = time_pair(src.va, at, ms);
        if (debug && ok) std::fprintf(stderr, "[igdsp_io] chunk %zu vs %s: %.4f ms\n", idx, tag, *ms);
        return ok;
    }
    // a new probe source from kSrcChunks chunks (each un-mapped from its scratch slot first: one mapping per chunk at a time)
    bool make_source(const std::vector<size_t> &idx, size_t *which)
    {
        Source S;
        S.n = idx.size();
        if (hipMemAddressReserve(&S.va, S.n * chunk, va_align, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); return false; }
        sources.push_back(S);
        Source &T = sources.back();
        for (size_t k = 0; k < idx.size(); ++k) {
            unmap_scratch(idx[k]);
            if (hipMemMap((char *)T.va + k * chunk, chunk, 0, chunks[idx[k]].h, 0) != hipSuccess) { (void)hipGetLastError(); return false; }
            T.idx.push_back(idx[k]);
            chunks[idx[k]].in_src = true;
            if (hipMemSetAccess((char *)T.va + k * chunk, chunk, &acc, 1) != hipSuccess) { (void)hipGetLastError(); return false; }
        }
        *which = sources.size() - 1;
        return true;
    }
    void drop_source(size_t which)
    {
        Source &S = sources[which];
        for (size_t k = 0; k < S.idx.size(); ++k) { (void)hipMemUnmap((char *)S.va + k * chunk, chunk); chunks[S.idx[k]].in_src = false; }
        S.idx.clear();                 // the address range stays reserved until cleanup and is never mapped again
    }
    void cleanup()
    {
        for (size_t i = 0; i < chunks.size(); ++i) unmap_scratch(i);
        for (size_t w = 0; w < sources.size(); ++w) drop_source(w);
        sources.clear();
        for (auto &c : chunks) if (!c.used) (void)hipMemRelease(c.h);
        chunks.clear();
        if (ea) (void)hipEventDestroy(ea);
        if (eb) (void)hipEventDestroy(eb);
        ea = eb = nullptr; cand_va = nullptr;     // address ranges are never returned: see igdsp_io_free
        (void)hipGetLastError();
    }
};

bool map_chunks(igdsp_io_set::Map &m, size_t chunk, const std::vector<hipMemGenericAllocationHandle_t> &hs, size_t first_slot,
                const hipMemAccessDesc &acc)
{
    for (size_t i = 0; i < hs.size(); ++i) {
        char *at = (char *)m.va + (first_slot + i) * chunk;
        if (hipMemMap(at, chunk, 0, hs[i], 0) != hipSuccess) return false;
        if (hipMemSetAccess(at, chunk, &acc, 1) != hipSuccess) return false;
    }
    return true;
}

// Every IGDSP_IO_* knob, read once per call (IGDSP_IO_SPARE_CHUNKS is read once per context, by igdsp_create)
struct IoKnobs {
    bool plain = false, frac_set = false, no_spread = false, settle = true, debug = false;
    int align_mib = -1; double limit_frac = 0.0;        // align_mib < 0: one chunk; limit_frac: when frac_set
    size_t stride = 16;                                 // sparse survey: one probe per 2 GiB (classes come in runs of 3-40 GiB of consecutive chunks)
    IoKnobs()
    {
        if (const char *e = std::getenv("IGDSP_IO_PLAIN")) plain = std::atoi(e) != 0;                      // plain hipMalloc buffers
        if (const char *e = std::getenv("IGDSP_IO_ALIGN_MIB")) align_mib = std::max(0, std::atoi(e));      // of every address reservation
        if (const char *e = std::getenv("IGDSP_IO_LIMIT_FRAC")) { frac_set = true; limit_frac = std::atof(e); }   // share of free memory to explore
        if (const char *e = std::getenv("IGDSP_IO_STRIDE")) stride = std::max(1, std::atoi(e));
        no_spread = std::getenv("IGDSP_IO_NO_SPREAD") != nullptr;                                        // two classes only (experiments)
        if (const char *e = std::getenv("IGDSP_IO_SETTLE")) settle = std::atoi(e) != 0;
        debug = std::getenv("IGDSP_IO_DEBUG") != nullptr;                                                // every probe on stderr
    }
};
// a probe launch reads this much and writes 1/10 of it into the chunk under test
size_t probe_bytes(size_t chunk) { return kSrcChunks * (chunk - 4096) / 10240 * 10240; }
// The buffer set in chunks (step 4)
struct Layout {
    std::vector<size_t> nch;          // chunks per buffer
    std::vector<uint32_t> order;      // buffer indices, INPUT buffers first, then RECORD, then BULK: the order chunks are handed out in
    size_t in_chunks = 0, in_bytes = 0, rec_chunks = 0, bulk_chunks = 0;
    int in0 = -1, out0 = -1;          // the largest INPUT buffer (the first of equals), the first output buffer
};
// What the search found: chunk indices of the inputs' class (A), of the first and of the second other class (B, C), and the
// thresholds it ended with (they label the leftovers)
struct Pools {
    std::vector<size_t> a, b, c;
    float fast = 0.f, slow = 0.f, thrB = 0.f, thrC = 0.f;   // against source A: faster than `fast` = another class, slower than `slow` = the inputs'; thrB / thrC: against source B
    bool split = false;               // B and C told apart: pool B chunks are label 2, else label 1 (igdsp_ctx::io_spare)
    const std::vector<size_t> &pool(int q) const { return q == 0 ? a : (q == 1 ? b : c); }
    int label(int q) const { return q == 0 ? 0 : (q == 2 ? 3 : (split ? 2 : 1)); }
};
// The search.  Against source A (chunks of the inputs' class) a chunk of that class writes slowly and any other fast; for bulk
// outputs the fast ones are split again against a source B of one other class.  ok turns false at the first failed HIP call and
// ends every loop.
struct Search {
    Explorer &X; const Layout &L; const size_t stride; igdsp_io_report &R;
    Pools P;                                            // the result
    bool ok = true;
    // measured on MI355X: same-class 0.252 ms, other-class 0.219 ms per probe launch (ratio 1.15), spread inside a level < 1 %
    static constexpr float kBimodal = 1.08f, kPure = 1.125f, kNear = 1.035f;
    size_t srcA = 0, srcB = 0, nB = 0, nC = 0;
    float tmin = 1e30f, tmax = 0.f, tbmin = 1e30f, tbmax = 0.f;   // survey levels against source A, extremes against source B
    float cB = 0.f, cC = 0.f, thrB = 0.f, thrC = 0.f;   // levels of the pool against source B (nB / nC chunks), thresholds between them
    std::vector<size_t> surveyed; std::vector<char> taken;   // taken: chunks already collected by a walk
    bool timeA(size_t idx)                              // time chunk idx against source A (once)
    {
        Chunk &c = X.chunks[idx];
        if (c.tA >= 0.f || c.in_src) return true;
        if (!X.probe(idx, X.sources[srcA], &c.tA, "A")) return ok = false;
        return true;
    }
    bool fast_A(size_t idx) { return !X.chunks[idx].in_src && timeA(idx) && X.chunks[idx].tA < P.fast; }
    bool timeB(size_t idx)                              // chunk idx against source B (once); false: not a candidate, or a failure
    {
        Chunk &c = X.chunks[idx];
        if (c.in_src || !ok) return false;
        if (c.tB < 0.f) {
            if (!X.probe(idx, X.sources[srcB], &c.tB, "B")) return ok = false;
            tbmin = std::min(tbmin, c.tB); tbmax = std::max(tbmax, c.tB);
        }
        return true;
    }
    bool is_C(size_t idx) { return fast_A(idx) && timeB(idx) && X.chunks[idx].tB < thrC; }
    bool is_B(size_t idx) { return fast_A(idx) && timeB(idx) && X.chunks[idx].tB > thrB; }
    void survey(bool rescan)                            // every stride-th chunk until two levels are visible and three samples sit on the fast one
    {
        tmin = 1e30f; tmax = 0.f;
        std::vector<size_t> todo = rescan ? surveyed : std::vector<size_t>();
        surveyed.clear();
        size_t next = 0, seen = 0;
        for (;;) {
            const size_t idx = seen < todo.size() ? todo[seen] : next;
            if (seen >= todo.size() && !X.ensure(idx)) break;
            next = std::max(next, idx) + stride;
            ++seen;
            if (X.chunks[idx].in_src) continue;
            if (!timeA(idx)) break;
            surveyed.push_back(idx);
            tmin = std::min(tmin, X.chunks[idx].tA); tmax = std::max(tmax, X.chunks[idx].tA);
            size_t n_fast = 0;
            for (size_t k : surveyed) if (X.chunks[k].tA < kNear * tmin) ++n_fast;
            if (seen >= todo.size() && tmax > kBimodal * tmin && n_fast >= 3 && surveyed.size() >= 8) break;
        }
    }
    // The levels are closer than two pure classes give: the ten consecutive chunks of source A mix classes (a run boundary, or
    // memory that is interleaved chunk by chunk).  The SLOWEST destinations are pure chunks of the class the mixed source holds
    // most of: collect ten of them — the slowest survey sample and its neighbours, then the next slowest — and make them the
    // source.  Everything is timed again against it.  false: not enough of them.
    bool reseed_A()
    {
        std::vector<size_t> order(surveyed);
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return X.chunks[a].tA > X.chunks[b].tA; });
        std::vector<size_t> pick;
        const float near_slow = tmax / 1.015f;
        for (size_t si = 0; si < order.size() && pick.size() < kSrcChunks && ok; ++si) {
            const size_t c0 = order[si];
            if (X.chunks[c0].tA < near_slow) break;
            const size_t lo = c0 >= stride ? c0 - stride + 1 : 0;
            for (size_t k = lo; k < c0 + stride && pick.size() < kSrcChunks && ok; ++k) {
                if (!X.ensure(k) || X.chunks[k].in_src) continue;
                if (!timeA(k)) break;
                if (X.chunks[k].tA >= near_slow && std::find(pick.begin(), pick.end(), k) == pick.end()) pick.push_back(k);
            }
        }
        if (pick.size() < kSrcChunks) return false;
        if (X.debug) std::fprintf(stderr, "[igdsp_io] levels %.4f / %.4f: source A is mixed, re-seeding from the %zu slowest chunks (first %zu)\n", tmax, tmin, pick.size(), pick[0]);
        X.drop_source(srcA);
        for (auto &c : X.chunks) c.tA = -1.f;
        ok = X.make_source(pick, &srcA);
        if (ok) survey(true);
        ++R.reseeds;
        return true;
    }
    // Walk the chunk sequence from `idx` and collect `want` chunks that satisfy `pred` (which probes on demand): inside runs that
    // fail, step by `stride` (or to the next chunk that has been timed already); on a hit, walk back over the chunks skipped since
    // the last probe, then go on densely.
    template <class Pred> void walk(size_t idx, size_t want, Pred pred, std::vector<size_t> &out)
    {
        auto take = [&](size_t k) { if (taken.size() <= k) taken.resize(k + 1, 0); if (!taken[k]) { taken[k] = 1; out.push_back(k); } };
        while (ok && out.size() < want && X.ensure(idx)) {
            if (pred(idx)) {
                size_t lo = idx;
                while (ok && lo > 0 && X.chunks[lo - 1].tA < 0.f && !X.chunks[lo - 1].in_src && pred(lo - 1)) --lo;
                for (size_t k = lo; k <= idx && out.size() < want; ++k) take(k);
                ++idx;
            } else {
                size_t nxt = idx + 1;            // skip ahead through un-timed chunks, but stop at one that has been timed already
                while (nxt < idx + stride && (nxt >= X.chunks.size() || X.chunks[nxt].tA < 0.f)) ++nxt;
                idx = nxt;
            }
        }
        std::sort(out.begin(), out.end());
    }
    // Every pool chunk against a candidate source.  0: two well separated levels, or one level at the slow mark (the source is one
    // class and so is the pool).  1: two levels closer than pure classes give (a mixed source: they can interleave chunk by chunk).
    // 2: one level in the middle (the source holds the two classes evenly: separates nothing).  -1: a failure.
    int try_source(const std::vector<size_t> &sb)
    {
        for (auto &c : X.chunks) c.tB = -1.f;
        tbmin = 1e30f; tbmax = 0.f;
        ok = X.make_source(sb, &srcB);
        for (size_t k : P.b) if (ok) (void)timeB(k);
        int v = -1;
        if (ok) {
            // Levels of the pool against source B, by two-means over the measured times (robust against a stray sample, which max /
            // min are not): cC / cB = centre of the fast / slow group.  A destination is slow against a source in proportion to the
            // share of the source that is of its own class, so with a source that mixes the two classes the two groups are still
            // the two classes, only closer together.
            float lo = tbmin, hi = tbmax;
            for (int it = 0; it < 12; ++it) {
                double sl = 0, sh = 0; size_t nl = 0, nh = 0;
                for (size_t k : P.b) {
                    const float t = X.chunks[k].tB;
                    if (t < 0.f) continue;
                    if (std::fabs(t - lo) <= std::fabs(t - hi)) { sl += t; ++nl; } else { sh += t; ++nh; }
                }
                if (nl) lo = (float)(sl / (double)nl);
                if (nh) hi = (float)(sh / (double)nh);
                nC = nl; nB = nh;
            }
            cC = lo; cB = hi;
            const float sep = cB / cC;
            if (sep < 1.025f) {
                const float level = (cB * (float)nB + cC * (float)nC) / (float)std::max<size_t>(1, nB + nC);
                v = level >= tmax / 1.025f ? 0 : 2;
                cB = level; cC = level * tmin / tmax;          // all of the pool is class B: the other level is the A test's
            } else v = sep >= 1.10f ? 0 : 1;
            const float mid = 0.5f * (cB + cC), m = 0.2f * (cB - cC);
            thrB = mid + m; thrC = mid - m;
        }
        if (X.debug) std::fprintf(stderr, "[igdsp_io] source B from chunk %zu: levels %.4f (%zu) / %.4f (%zu) -> %s\n", sb[0], cB, nB, cC, nC,
                                  v == 0 ? "one class" : (v == 1 ? "mixed" : (v == 2 ? "evenly mixed" : "failed")));
        return v;
    }
    // Source B = ten pool chunks of one class.  Candidates: ten consecutive pool chunks from the start, every 2nd, every 3rd, then
    // consecutive windows further in.  0: source srcB is made and sorts the pool; anything else: no candidate did (none is left).
    int find_source_B()
    {
        const size_t picks[][2] = {{0, 1}, {0, 2}, {0, 3}, {kSrcChunks, 1}, {2 * kSrcChunks, 1}, {3 * kSrcChunks, 1}, {1, 2}};
        int verdict = -1;
        for (size_t pi = 0; pi < sizeof(picks) / sizeof(picks[0]) && ok && verdict != 0; ++pi) {
            std::vector<size_t> sb;
            for (size_t k = picks[pi][0]; k < P.b.size() && sb.size() < kSrcChunks; k += picks[pi][1]) sb.push_back(P.b[k]);
            if (sb.size() < kSrcChunks) continue;
            for (int tries = 0; ok; ++tries) {
                verdict = try_source(sb);
                if (verdict != 1 || tries == 2) break;
                // a mixed source: each group it separates is one class — re-seed from ten members of the larger group
                std::vector<size_t> gb, gc;
                for (size_t k : P.b) {
                    const Chunk &c = X.chunks[k];
                    if (c.in_src || c.tB < 0.f) continue;
                    if (c.tB > thrB) gb.push_back(k); else if (c.tB < thrC) gc.push_back(k);
                }
                std::vector<size_t> &grp = gb.size() >= gc.size() ? gb : gc;
                if (grp.size() < kSrcChunks) break;
                grp.resize(kSrcChunks);
                X.drop_source(srcB);
                sb = grp;
                ++R.reseeds;
            }
            if (verdict == 1 && cB / cC >= 1.045f) verdict = 0;      // closer than pure classes, yet clearly two groups: good enough to sort by
            if (verdict != 0) X.drop_source(srcB);
        }
        return verdict;
    }
    // 2nd split, for bulk outputs: which destinations are fast against the inputs' class AND against the first other class?  A
    // chunk that writes slowly against source B shares its class (B), a fast one belongs to the third class (C).  C usually lies
    // tens of GiB further along the allocation sequence, so the walk continues from where the pool ended until the second halves
    // of the bulk buffers are covered, or the exploration limit is reached (then B serves both halves).
    void split_BC()
    {
        if (find_source_B() != 0) return;
        const size_t need_c = L.bulk_chunks / 2, need_b = L.rec_chunks + L.bulk_chunks - need_c;
        // the pool, classified: source chunks and slow destinations are class B, fast destinations class C, anything between the
        // levels (a chunk that itself mixes classes) is left out; what is still missing is searched further along
        std::vector<size_t> cb, cc;
        for (size_t k : P.b) {
            const Chunk &c = X.chunks[k];
            if (c.in_src || c.tB > thrB) cb.push_back(k);
            else if (c.tB >= 0.f && c.tB < thrC) cc.push_back(k);
        }
        taken.assign(taken.size(), 0);
        for (size_t k : P.b) { if (taken.size() <= k) taken.resize(k + 1, 0); taken[k] = 1; }
        const size_t from = P.b.back() + 1;
        if (cc.size() < need_c) walk(from, need_c, [this](size_t i) { return is_C(i); }, cc);
        const size_t want_b = need_b + (cc.size() < need_c ? need_c - cc.size() : 0);   // B also serves what C could not
        if (ok && cb.size() < want_b) walk(from, want_b, [this](size_t i) { return is_B(i); }, cb);
        if (X.debug) std::fprintf(stderr, "[igdsp_io] split: class B %zu of %zu chunks, class C %zu of %zu\n", cb.size(), need_b, cc.size(), need_c);
        // (enough of class C: everything the second halves need, or at least four chunks and half of it.  Requiring four chunks
        // outright turned down small sets whose two or three C chunks had all been found — 80-byte frames, C 160 GB into the sequence.)
        if (ok && (cc.size() >= need_c || cc.size() >= std::max<size_t>(4, need_c / 2))) {
            R.classes_found = 3;
            P.b = cb; P.c = cc; P.split = true; P.thrB = thrB; P.thrC = thrC;
        }
        X.drop_source(srcB);
    }
    // Step 6.  A full search re-establishes the class labels: spares and older buffer sets were labelled relative to ANOTHER
    // search's inputs, which may have landed in a different class than this one's.  false: a HIP call failed.
    bool run(igdsp_ctx *ctx, igdsp_io_set *set, const IoKnobs &kn, size_t limit)
    {
        igdsp_io_drop_spares(ctx);
        { std::lock_guard<std::mutex> g(ctx->io_mu); set->epoch = ++ctx->io_epoch; ctx->io_spare_chunk = X.chunk; }
        X.limit_chunks = limit / X.chunk; X.debug = kn.debug;
        ok = hipMemAddressReserve(&X.cand_va, X.limit_chunks * X.chunk, X.va_align, nullptr, 0) == hipSuccess && X.open(ctx, probe_bytes(X.chunk));
        classify(L.bulk_chunks >= 4 && !kn.no_spread, ctx->io_spare_cap);
        R.chunks_explored = (uint32_t)X.chunks.size(); R.explored_bytes = (uint64_t)X.chunks.size() * X.chunk; R.probes = X.probes;
        (void)hipGetLastError();
        return ok;
    }
    void classify(bool want_spread, size_t spare_cap)
    {
        // source A: ten consecutive chunks; every other chunk is ranked by how fast the stream runs when it writes there
        std::vector<size_t> first;
        for (size_t k = 0; k < kSrcChunks && ok; ++k) { ok = X.ensure(k); first.push_back(k); }
        ok = ok && X.make_source(first, &srcA);
        {   // clocks: ~40 ms of the probe stream before anything is compared (the first launches after idle run ~6 % slow)
            float t = 0.f;
            if (ok && X.ensure(kSrcChunks)) { for (int k = 0; k < 28 && ok; ++k) ok = X.probe(kSrcChunks, X.sources[srcA], &t, "warm"); }
        }
        if (ok) survey(false);
        for (int attempt = 0; attempt < 2 && ok && tmax > 1.02f * tmin && tmax < kPure * tmin; ++attempt)
            if (!reseed_A()) break;
        R.probe_ms_same = tmax; R.probe_ms_other = tmin;
        if (!ok || !(tmax > kBimodal * tmin)) return;
        R.classes_found = 2;
        P.fast = kNear * tmin; P.slow = tmax / kNear;
        // inputs: the chunks of source A themselves plus chunks that write slowly against it (the same class)
        if (L.in_chunks > kSrcChunks) walk(0, L.in_chunks - kSrcChunks, [this](size_t i) { return !X.chunks[i].in_src && timeA(i) && X.chunks[i].tA > P.slow; }, P.a);
        // (with a bulk output the pool also has to yield source B and enough members of either class to re-seed it from)
        const size_t outs = L.rec_chunks + L.bulk_chunks;
        walk(0, want_spread ? std::max<size_t>(outs + kSrcChunks, 4 * kSrcChunks) : outs, [this](size_t i) { return fast_A(i); }, P.b);
        if (ok && want_spread && P.b.size() >= kSrcChunks + outs - L.bulk_chunks / 2) split_BC();
        // Spares for the NEXT set of this size: chunks the sparse survey created but never timed are classified now — about 1.5 ms of
        // probing each, no new memory — until each class has `spare_cap` of them beyond what this set takes; they stay with the context
        // (keep_spares) and a later call that they cover is served without a search.
        if (ok && !want_spread && spare_cap > 0) {
            const size_t need0 = (L.in_chunks > kSrcChunks ? L.in_chunks - kSrcChunks : 0) + spare_cap, need1 = L.rec_chunks + L.bulk_chunks + spare_cap;
            size_t cnt0 = 0, cnt1 = 0;
            for (const auto &c : X.chunks) if (!c.in_src && c.tA >= 0.f) { if (c.tA > P.slow) ++cnt0; else if (c.tA < P.fast) ++cnt1; }
            size_t budget = 4 * spare_cap;
            for (size_t k = 0; k < X.chunks.size() && ok && budget > 0 && (cnt0 < need0 || cnt1 < need1); ++k) {
                Chunk &c = X.chunks[k];
                if (c.in_src || c.tA >= 0.f) continue;
                if (!timeA(k)) break;
                --budget;
                if (c.tA > P.slow) ++cnt0; else if (c.tA < P.fast) ++cnt1;
            }
        }
        if (!ok) return;
        P.a.insert(P.a.begin(), X.sources[srcA].idx.begin(), X.sources[srcA].idx.end());   // the inputs get source A's own chunks first
        X.drop_source(srcA);
    }
};
// Step 3's fallback: consecutive hipMallocs in the order given, what a host would write itself
int plain_path(igdsp_ctx *ctx, igdsp_io_buf *bufs, uint32_t n_bufs, igdsp_io_set *set)
{
    for (uint32_t i = 0; i < n_bufs; ++i) {
        if (hipMalloc(&bufs[i].ptr, bufs[i].bytes) != hipSuccess) { (void)hipGetLastError(); bufs[i].ptr = nullptr; return fail(ctx, IGDSP_ENOMEM, "igdsp_io_alloc: hipMalloc"); }
        set->plain.push_back(bufs[i].ptr);
    }
    return IGDSP_OK;
}
// Step 4: one address range per buffer, and the set in chunks
int reserve_ranges(igdsp_ctx *ctx, const igdsp_io_buf *bufs, uint32_t n_bufs, size_t va_align, igdsp_io_set *set, Layout &L)
{
    const size_t chunk = set->chunk;
    set->maps.resize(n_bufs); L.nch.resize(n_bufs);
    for (uint32_t role = 0; role < 3; ++role)
        for (uint32_t i = 0; i < n_bufs; ++i) if (bufs[i].role == role) L.order.push_back(i);
    for (uint32_t i = 0; i < n_bufs; ++i) {
        L.nch[i] = (bufs[i].bytes + chunk - 1) / chunk;
        auto &m = set->maps[i];
        m.bytes = L.nch[i] * chunk;
        if (hipMemAddressReserve(&m.va, m.bytes, va_align, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); m.va = nullptr; return fail(ctx, IGDSP_ENOMEM, "igdsp_io_alloc: hipMemAddressReserve"); }
        if (bufs[i].role == IGDSP_IO_INPUT) { L.in_chunks += L.nch[i]; L.in_bytes += bufs[i].bytes; if (L.in0 < 0 || L.nch[i] > L.nch[L.in0]) L.in0 = (int)i; continue; }
        if (L.out0 < 0) L.out0 = (int)i;
        if (bufs[i].role == IGDSP_IO_RECORD) L.rec_chunks += L.nch[i]; else L.bulk_chunks += L.nch[i];
    }
    return IGDSP_OK;
}
// Step 11: the pointers, and the bulk buffers whose halves sit in two classes (igdsp_ctx::is_spread)
int publish(igdsp_ctx *ctx, igdsp_io_buf *bufs, uint32_t n_bufs, const igdsp_io_set *set, bool spread)
{
    for (uint32_t i = 0; i < n_bufs; ++i) bufs[i].ptr = set->maps[i].va;
    if (!spread) return IGDSP_OK;
    std::lock_guard<std::mutex> g(ctx->io_mu);
    for (uint32_t i = 0; i < n_bufs; ++i)
        if (bufs[i].role == IGDSP_IO_BULK) ctx->spread_ranges.push_back({(const char *)set->maps[i].va, set->maps[i].bytes});
    return IGDSP_OK;
}
// Step 5.  Served from what an earlier call learnt?  Spare chunks of known class (left by a search, or returned by igdsp_io_free)
// cover this set when the inputs fit class 0, the records and the bulk outputs' first halves fit the non-0 spares and the second
// halves the other non-0 class: map them, probe nothing, release nothing (so there is nothing to wait out either).  The chunks are
// taken under the context's lock and mapped after it.  kNotServed: the spares do not cover the set.
constexpr int kNotServed = 1;
int from_spares(igdsp_ctx *ctx, igdsp_io_buf *bufs, uint32_t n_bufs, const Layout &L, igdsp_io_set *set, const hipMemAccessDesc &acc, igdsp_io_report &R)
{
    const bool want_spread = L.bulk_chunks >= 4;
    const size_t second = want_spread ? L.bulk_chunks / 2 : 0, first = L.rec_chunks + L.bulk_chunks - second;
    std::unique_lock<std::mutex> g(ctx->io_mu);
    auto &S = ctx->io_spare;
    if (ctx->io_spare_chunk != set->chunk || S[0].size() < L.in_chunks || S[1].size() + S[2].size() < first || S[3].size() < second) return kNotServed;
    const uint32_t epoch = ctx->io_epoch;
    const int pref = want_spread ? 2 : 1;               // first halves: label 2 when the bulk outputs want a split, else 1; then the other
    for (uint32_t i : L.order) {
        auto &m = set->maps[i];
        const size_t h2 = (bufs[i].role == IGDSP_IO_BULK && want_spread) ? L.nch[i] / 2 : 0;
        for (size_t k = 0; k < L.nch[i]; ++k) {
            const int from = bufs[i].role == IGDSP_IO_INPUT ? 0 : (k >= L.nch[i] - h2 && !S[3].empty()) ? 3
                           : !S[pref].empty() ? pref : !S[3 - pref].empty() ? 3 - pref : 3;
            m.handles.push_back(S[from].back()); m.cls.push_back((uint8_t)from); S[from].pop_back();
        }
    }
    g.unlock();
    bool ok = true;
    for (uint32_t i : L.order) ok = ok && map_chunks(set->maps[i], set->chunk, set->maps[i].handles, 0, acc);
    if (!ok) { (void)hipGetLastError(); return fail(ctx, IGDSP_ENOMEM, "igdsp_io_alloc: mapping spare chunks"); }
    set->epoch = epoch;
    bool spread_ok = want_spread;
    for (uint32_t i = 0; i < n_bufs && spread_ok; ++i)
        if (bufs[i].role == IGDSP_IO_BULK) spread_ok = !set->maps[i].cls.empty() && set->maps[i].cls.front() != set->maps[i].cls.back();
    R.placed = 1; R.bulk_spread = (spread_ok && L.bulk_chunks > 0) ? 1u : 0u; R.classes_found = R.bulk_spread ? 3u : 2u;
    return publish(ctx, bufs, n_bufs, set, R.bulk_spread);
}
// IGDSP_IO_DEBUG: the finished set against the levels of the search, the largest INPUT -> every output buffer (before the release:
// the buffer's first three chunks; after it: the buffer, three times)
void debug_check(Explorer &E, const igdsp_io_buf *bufs, uint32_t n_bufs, const Layout &L, const igdsp_io_set *set, bool after)
{
    if (L.in0 < 0 || L.nch[L.in0] < kSrcChunks) return;
    for (uint32_t i = 0; i < n_bufs; ++i) {
        if (bufs[i].role == IGDSP_IO_INPUT) continue;
        for (size_t k = 0; k < 3 && (after || k < L.nch[i]); ++k) {
            float t = 0.f;
            if (!E.time_pair(set->maps[L.in0].va, (char *)set->maps[i].va + (after ? 0 : k * set->chunk), &t)) continue;
            if (after) std::fprintf(stderr, "[igdsp_io] after release: input -> buffer %u: %.4f ms\n", i, t);
            else std::fprintf(stderr, "[igdsp_io] final check: input -> buffer %u chunk %zu: %.4f ms\n", i, k, t);
        }
    }
}
// Step 7.  Hand the picked chunks to their buffers: INPUT buffers from pool A, RECORD buffers and the first halves of the BULK
// buffers from pool B, the second halves from pool C (from B when there is no third class); a pool that runs dry is topped up from
// the other output pool, and whatever a buffer still lacks after that comes from fresh consecutive chunks (step 10).
bool hand_out(Explorer &X, const Pools &P, const igdsp_io_buf *bufs, uint32_t n_bufs, const Layout &L, igdsp_io_set *set, igdsp_io_report &R)
{
    for (size_t i = 0; i < X.chunks.size(); ++i) X.unmap_scratch(i);
    size_t cur[3] = {0, 0, 0};
    bool ok = true, all = true, spread = !P.c.empty();
    std::vector<hipMemGenericAllocationHandle_t> hs;
    std::vector<uint8_t> labels;                        // of the chunks the current buffer pulled (igdsp_ctx::io_spare labels)
    auto pull = [&](int p, size_t n) {
        for (size_t k = 0; k < n; ++k) {
            const int q = (cur[p] >= P.pool(p).size() && p != 0) ? 3 - p : p;
            if (cur[q] >= P.pool(q).size()) return;
            Chunk &c = X.chunks[P.pool(q)[cur[q]++]]; c.used = true;
            labels.push_back((uint8_t)P.label(q));
            hs.push_back(c.h);
        }
    };
    for (size_t j = 0; j < L.order.size() && ok; ++j) {
        const uint32_t i = L.order[j];
        hs.clear(); labels.clear();
        if (bufs[i].role == IGDSP_IO_INPUT) pull(0, L.nch[i]);
        else {
            const size_t h2 = (bufs[i].role == IGDSP_IO_BULK && spread) ? L.nch[i] / 2 : 0;  // second-half chunks from class C
            pull(1, L.nch[i] - h2);
            if (hs.size() == L.nch[i] - h2) pull(2, h2);
        }
        all = all && hs.size() == L.nch[i];
        ok = map_chunks(set->maps[i], set->chunk, hs, 0, X.acc);
        set->maps[i].handles = hs; set->maps[i].cls = labels;
    }
    R.placed = (ok && all) ? 1u : 0u; R.bulk_spread = (ok && all && spread && L.bulk_chunks > 0) ? 1u : 0u;
    if (X.debug && ok) {
        std::fprintf(stderr, "[igdsp_io] pools: A %zu B %zu C %zu chunks; A:", P.a.size(), P.b.size(), P.c.size());
        for (size_t k = 0; k < P.a.size() && k < 12; ++k) std::fprintf(stderr, " %zu", P.a[k]);
        std::fprintf(stderr, "  B:");
        for (size_t k = 0; k < P.b.size() && k < 12; ++k) std::fprintf(stderr, " %zu(%.4f)", P.b[k], X.chunks[P.b[k]].tA);
        std::fprintf(stderr, "\n");
        debug_check(X, bufs, n_bufs, L, set, false);
    }
    return ok;
}
// Step 8.  Leftovers whose class the search established stay with the context as spares (up to io_spare_cap per class): the next
// call that they cover maps them without probing.  Pool members first (they were classified with the final thresholds), then any
// other timed chunk; chunks between two levels, or never timed, are released like before.
void keep_spares(igdsp_ctx *ctx, Explorer &X, const Pools &P)
{
    for (int q = 0; q < 3; ++q)
        for (size_t k : P.pool(q)) if (!X.chunks[k].used) X.chunks[k].cls = P.label(q);
    for (auto &c : X.chunks) {
        if (c.used || c.in_src || c.cls >= 0 || c.tA < 0.f) continue;
        if (c.tA > P.slow) c.cls = 0;
        else if (c.tA < P.fast) c.cls = !P.split ? 1 : (c.tB > P.thrB ? 2 : ((c.tB >= 0.f && c.tB < P.thrC) ? 3 : -1));
    }
    std::lock_guard<std::mutex> g(ctx->io_mu);
    for (auto &c : X.chunks)
        if (!c.used && !c.in_src && c.cls >= 0 && ctx->io_spare[c.cls].size() < ctx->io_spare_cap) { ctx->io_spare[c.cls].push_back(c.h); c.used = true; }
}
// Step 10: fresh consecutive chunks for what buffer m still lacks (no class wanted / known)
bool map_fresh(igdsp_io_set::Map &m, size_t nch, size_t chunk, const hipMemAllocationProp &prop, const hipMemAccessDesc &acc)
{
    const size_t have = m.handles.size();
    std::vector<hipMemGenericAllocationHandle_t> hs;
    bool ok = true;
    hipMemGenericAllocationHandle_t h;
    for (size_t k = have; k < nch && ok; ++k) if ((ok = hipMemCreate(&h, chunk, &prop, 0) == hipSuccess)) hs.push_back(h);
    ok = ok && map_chunks(m, chunk, hs, have, acc);
    m.handles.insert(m.handles.end(), hs.begin(), hs.end());      // owned by the set from here on (released by igdsp_io_free)
    m.cls.resize(m.handles.size(), 255);                          // class unknown
    return ok;
}
// Step 12.  Releasing the exploration chunks leaves the memory system busy for a while: the driver clears freed device memory in
// the background at ~30-40 GB/s (measured: 104 GB released -> the same buffers stream ~5 % slower and k_meter_chunk64 runs 1.5 %
// slower for 2-3 s; 56 GB -> 1.5-2 s; 17 GB -> ~0.5 s; then both return to the level of the search).  The call only returns when
// that is over: at least released bytes / 25 GB/s, and until the finished set streams at the speed it had BEFORE the release
// (settle_ref, taken after the hand-out; the wait follows the last mapping).  IGDSP_IO_SETTLE=0 skips the wait.
float settle_ref(Explorer &X, const Layout &L, const igdsp_io_set *set, size_t *n)
{
    if (L.in0 < 0 || L.out0 < 0) return 0.f;
    *n = std::min(X.probe_n, std::min(L.nch[L.in0] * set->chunk, 10 * (L.nch[L.out0] * set->chunk - 4096)) / 10240 * 10240);
    const size_t keep = X.probe_n; X.probe_n = *n;
    float t = 0.f, t_ref = 0.f;
    const void *rd = set->maps[L.in0].va; void *wr = set->maps[L.out0].va;
    if (*n >= ((size_t)256 << 20) && X.time_pair(rd, wr, &t) && X.time_pair(rd, wr, &t)) t_ref = t;
    X.probe_n = keep;
    return t_ref;
}
float settle(igdsp_ctx *ctx, const Layout &L, const igdsp_io_set *set, size_t n, float t_ref, size_t released_chunks, bool debug)
{
    Explorer Y;
    const auto w0 = std::chrono::steady_clock::now();
    if (Y.open(ctx, n)) {
        const float min_wait = std::min(6000.f, (float)((double)released_chunks * (double)set->chunk / 25e9 * 1e3));
        int quiet = 0;
        for (;;) {
            float t = 0.f; if (!Y.time_pair(set->maps[L.in0].va, set->maps[L.out0].va, &t)) break;
            quiet = t <= 1.012f * t_ref ? quiet + 1 : 0;
            const float waited = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
            if (debug) std::fprintf(stderr, "[igdsp_io] settle: %.4f ms against %.4f before the release (%.0f of >= %.0f ms)\n", t, t_ref, waited, min_wait);
            if ((quiet >= 2 && waited >= min_wait) || waited > 8000.f) break;
            std::this_thread::sleep_for(std::chrono::milliseconds(50));
        }
    }
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
    Y.cleanup();
    return ms;
}
// Steps 3-13 of igdsp_io_alloc; X is the call's explorer, released by the caller whatever this returns
int place(igdsp_ctx *ctx, igdsp_io_buf *bufs, uint32_t n_bufs, size_t explore_limit_bytes, const IoKnobs &kn, igdsp_io_set *set,
          Explorer &X, igdsp_io_report &R)
{
    // 3. the plain path when the virtual-memory API is missing
    int vmm = 0;
    if (hipDeviceGetAttribute(&vmm, hipDeviceAttributeVirtualMemoryManagementSupported, ctx->device) != hipSuccess) { (void)hipGetLastError(); vmm = 0; }
    if (!vmm || kn.plain) return plain_path(ctx, bufs, n_bufs, set);
    X.prop.type = hipMemAllocationTypePinned; X.prop.location.type = hipMemLocationTypeDevice; X.prop.location.id = ctx->device;
    X.acc.location = X.prop.location; X.acc.flags = hipMemAccessFlagsProtReadWrite;
    size_t gran = 0;
    if (hipMemGetAllocationGranularity(&gran, &X.prop, hipMemAllocationGranularityRecommended) != hipSuccess || gran == 0) { (void)hipGetLastError(); return plain_path(ctx, bufs, n_bufs, set); }
    // >= the 1/10 of a probe read that a probe launch writes, and small next to the class runs (3-40 GiB)
    const size_t chunk = (((size_t)128 << 20) + gran - 1) / gran * gran;
    X.chunk = set->chunk = R.chunk_bytes = chunk;
    // chunk-aligned addresses: the page tables can then map a chunk with its largest fragments
    X.va_align = kn.align_mib >= 0 ? (size_t)kn.align_mib << 20 : chunk;
    // 4. address ranges and chunk counts per buffer
    Layout L;
    if (const int rc = reserve_ranges(ctx, bufs, n_bufs, X.va_align, set, L)) return rc;
    size_t free_b = 0, total_b = 0; (void)hipMemGetInfo(&free_b, &total_b);
    // default: 50 % of what is free; 85 % when bulk outputs want a THIRD class (the allocator tends to hand that one out last).
    // That is only the ceiling: the search stops as soon as every buffer has its chunks (typically 15-50 GB explored for a
    // two-class set), and later calls are served from the spares this one leaves behind.
    const double frac = kn.frac_set ? kn.limit_frac : (L.bulk_chunks >= 4 ? 0.85 : 0.5);
    const size_t limit = std::min(explore_limit_bytes ? explore_limit_bytes : (size_t)(frac * (double)free_b), (size_t)(0.9 * (double)free_b));
    // Below 512 MiB of inputs a launch works out of the 256 MiB Infinity Cache and placement does not matter.
    // (a set of INPUT buffers only is still worth placing once it is larger than the probe source: all of it lands in ONE class)
    const bool want_place = L.in_bytes >= ((size_t)512 << 20) && ((L.rec_chunks + L.bulk_chunks) > 0 || L.in_chunks > kSrcChunks) && limit / chunk >= 4 * kSrcChunks;
    // 5. served from spares
    const int spared = want_place ? from_spares(ctx, bufs, n_bufs, L, set, X.acc, R) : kNotServed;
    if (spared != kNotServed) return spared;
    // 6. search; 7. hand out the pools
    Search S{X, L, kn.stride, R};
    bool ok = !want_place || S.run(ctx, set, kn, limit);
    if (ok && (!S.P.b.empty() || (L.rec_chunks + L.bulk_chunks == 0 && !S.P.a.empty()))) ok = hand_out(X, S.P, bufs, n_bufs, L, set, R);
    // 8. keep the leftovers as spares (the settle wait's reference is taken before anything is released)
    size_t settle_n = 0;
    const float t_ref = R.placed ? settle_ref(X, L, set, &settle_n) : 0.f;
    if (R.placed) keep_spares(ctx, X, S.P);
    // 9. release the exploration: its leftovers go back before anything else is allocated
    const size_t released_chunks = (size_t)std::count_if(X.chunks.begin(), X.chunks.end(), [](const Chunk &c) { return !c.used; });
    X.cleanup();
    // 10. fresh chunks for what is missing
    for (uint32_t i : L.order)
        if (ok && set->maps[i].handles.size() < L.nch[i]) ok = map_fresh(set->maps[i], L.nch[i], chunk, X.prop, X.acc);
    if (!ok) { (void)hipGetLastError(); return fail(ctx, IGDSP_ENOMEM, "igdsp_io_alloc: mapping chunks"); }
    // 11. publish; 12. settle
    publish(ctx, bufs, n_bufs, set, R.bulk_spread);
    if (kn.settle && t_ref > 0.f) R.settle_ms = settle(ctx, L, set, settle_n, t_ref, released_chunks, kn.debug);
    // IGDSP_IO_DEBUG: the check of step 7 once more, with every exploration chunk released
    if (kn.debug && R.placed) { Explorer Y; if (Y.open(ctx, probe_bytes(chunk))) debug_check(Y, bufs, n_bufs, L, set, true); Y.cleanup(); }
    return IGDSP_OK;
}

}  // namespace

void igdsp_io_drop_spares(igdsp_ctx *ctx)
{
    std::vector<hipMemGenericAllocationHandle_t> gone;
    std::unique_lock<std::mutex> g(ctx->io_mu);
    for (auto &v : ctx->io_spare) { gone.insert(gone.end(), v.begin(), v.end()); v.clear(); }
    g.unlock();
    for (auto h : gone) (void)hipMemRelease(h);
    (void)hipGetLastError();
}

extern "C" {

int igdsp_io_free(igdsp_ctx *ctx, igdsp_io_set *set)
{
    if (!ctx) return IGDSP_EINVAL;
    if (!set) return IGDSP_OK;
    (void)hipSetDevice(set->device);
    (void)hipDeviceSynchronize();
    // Chunks are un-mapped and released; the ADDRESS RANGES stay reserved for the life of the process.  On this stack (ROCm 7.2,
    // gfx950) an address that has been un-mapped — even freed and reserved again — and is then mapped onto another chunk keeps
    // reaching the old one (igdsp_internal_vmm_remap_check; tools/io_place.py prints it), so no address is ever handed back for
    // re-use.  Address space is the only thing this costs (<= ~0.2 TiB of 128 TiB per igdsp_io_alloc call).
    {
        std::lock_guard<std::mutex> g(ctx->io_mu);
        for (auto &m : set->maps)
            for (size_t k = 0; k < ctx->spread_ranges.size();)
                if (ctx->spread_ranges[k].base == (const char *)m.va) ctx->spread_ranges.erase(ctx->spread_ranges.begin() + (long)k); else ++k;
    }
    for (auto &m : set->maps) {
        if (!m.va) continue;
        for (size_t i = 0; i < m.handles.size(); ++i) (void)hipMemUnmap((char *)m.va + i * set->chunk, set->chunk);
        // a chunk whose class is known (and still labelled in the context's current terms) becomes a spare: the next
        // igdsp_io_alloc can map it without probing, and nothing is released for the driver to clear
        std::vector<hipMemGenericAllocationHandle_t> gone;
        std::unique_lock<std::mutex> g(ctx->io_mu);
        for (size_t i = 0; i < m.handles.size(); ++i) {
            const uint8_t c = i < m.cls.size() ? m.cls[i] : 255;
            if (c < 4 && set->epoch == ctx->io_epoch && set->chunk == ctx->io_spare_chunk && ctx->io_spare[c].size() < ctx->io_spare_cap) ctx->io_spare[c].push_back(m.handles[i]);
            else gone.push_back(m.handles[i]);
        }
        g.unlock();
        for (auto h : gone) (void)hipMemRelease(h);
    }
    for (void *p : set->plain) if (p) (void)hipFree(p);
    (void)hipGetLastError();
    delete set;
    return IGDSP_OK;
}

// Diagnostic (not in include/igdsp.h): does a device address that was un-mapped and then mapped onto ANOTHER chunk reach
// the new chunk?  Writes 0x11 through address v to chunk X, re-maps v onto chunk Y, writes 0x22 through v, then reads X and Y
// through fresh addresses: bytes[0] / bytes[1] = first byte of X / Y (expected 0x11 / 0x22; X == 0x22 means the second write
// still went to X: a stale translation).  mode 0: hipMemUnmap + hipMemMap on the same reservation; mode 1: the reservation is
// freed (hipMemAddressFree) and reserved again at the same address in between; bytes[2] = 1 when that second reservation did
// come back at the same address.  igdsp_io_alloc maps every address at most once, whatever this reports.
int igdsp_internal_vmm_remap_check(igdsp_ctx *ctx, int mode, int *bytes)
{
    if (!ctx || !bytes) return IGDSP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = ctx->device;
    hipMemAccessDesc acc{};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    size_t gran = 0;
    HIP_TRY(ctx, hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended));
    const size_t sz = std::max<size_t>(gran, (size_t)64 << 20);
    hipMemGenericAllocationHandle_t X, Y;
    void *v = nullptr, *wx = nullptr, *wy = nullptr;
    HIP_TRY(ctx, hipMemCreate(&X, sz, &prop, 0));
    HIP_TRY(ctx, hipMemCreate(&Y, sz, &prop, 0));
    HIP_TRY(ctx, hipMemAddressReserve(&v, sz, 0, nullptr, 0));
    HIP_TRY(ctx, hipMemAddressReserve(&wx, sz, 0, nullptr, 0));
    HIP_TRY(ctx, hipMemAddressReserve(&wy, sz, 0, nullptr, 0));
    HIP_TRY(ctx, hipMemMap(v, sz, 0, X, 0));
    HIP_TRY(ctx, hipMemSetAccess(v, sz, &acc, 1));
    HIP_TRY(ctx, hipMemsetAsync(v, 0x11, sz, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemUnmap(v, sz));
    bytes[2] = 1;
    if (mode == 1) {
        void *v0 = v;
        HIP_TRY(ctx, hipDeviceSynchronize());
        HIP_TRY(ctx, hipMemAddressFree(v, sz));
        HIP_TRY(ctx, hipMemAddressReserve(&v, sz, 0, v0, 0));
        bytes[2] = v == v0 ? 1 : 0;
    }
    HIP_TRY(ctx, hipMemMap(v, sz, 0, Y, 0));
    HIP_TRY(ctx, hipMemSetAccess(v, sz, &acc, 1));
    HIP_TRY(ctx, hipMemsetAsync(v, 0x22, sz, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemUnmap(v, sz));
    HIP_TRY(ctx, hipMemMap(wx, sz, 0, X, 0));
    HIP_TRY(ctx, hipMemSetAccess(wx, sz, &acc, 1));
    HIP_TRY(ctx, hipMemMap(wy, sz, 0, Y, 0));
    HIP_TRY(ctx, hipMemSetAccess(wy, sz, &acc, 1));
    unsigned char bx = 0, by = 0;
    HIP_TRY(ctx, hipMemcpy(&bx, (char *)wx + sz / 2, 1, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(&by, (char *)wy + sz / 2, 1, hipMemcpyDeviceToHost));
    bytes[0] = bx; bytes[1] = by;
    (void)hipMemUnmap(wx, sz); (void)hipMemUnmap(wy, sz);
    (void)hipMemRelease(X); (void)hipMemRelease(Y);
    // the three reservations are deliberately NOT returned: see igdsp_io_free
    return IGDSP_OK;
}

int igdsp_io_alloc(igdsp_ctx *ctx, igdsp_io_buf *bufs, uint32_t n_bufs, size_t explore_limit_bytes, igdsp_io_set **out_set,
                   igdsp_io_report *rep)
{
    // 1. validate
    if (!ctx || !bufs || !out_set || n_bufs == 0 || n_bufs > 64) return IGDSP_EINVAL;
    *out_set = nullptr;
    for (uint32_t i = 0; i < n_bufs; ++i) {
        bufs[i].ptr = nullptr;
        if (bufs[i].bytes == 0 || bufs[i].role > IGDSP_IO_BULK) return IGDSP_EINVAL;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const auto t_start = std::chrono::steady_clock::now();
    igdsp_io_set *set = new (std::nothrow) igdsp_io_set();
    if (!set) return IGDSP_ENOMEM;
    set->device = ctx->device;
    // 2. read the knobs; 3-13 (place)
    const IoKnobs kn;
    igdsp_io_report R = {};
    Explorer X; X.ctx = ctx; X.s = ctx->stream;
    const int rc = place(ctx, bufs, n_bufs, explore_limit_bytes, kn, set, X, R);
    // 13. report; the one exit
    X.cleanup();
    R.setup_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (rep) *rep = R;
    if (rc != IGDSP_OK) { igdsp_io_free(ctx, set); for (uint32_t i = 0; i < n_bufs; ++i) bufs[i].ptr = nullptr; }
    else *out_set = set;
    return rc;
}

}  // extern "C"
