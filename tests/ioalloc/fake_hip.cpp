// A CPU stand-in for the HIP calls csrc/igdsp_io.hip makes (and for igdsp::launch_stream_rw), so that the real translation unit
// runs unchanged under g++: tests/ioalloc/io_alloc_driver.cpp, tests/test_io_alloc_cpu.py.
//
// The model.  Physical memory comes in classes; the class of the n-th chunk created (hipMemCreate) comes from the scenario's
// class map, e.g. "A30 B50 A40 C*" (runs, the last one without end) or "BC200" (B and C alternating chunk by chunk for 200
// chunks).  Address ranges come from a bump allocator and are never re-used; a map is kept per 2 MiB granule.  A probe launch
// (launch_stream_rw) adds 0.219 ms x (1 + 0.15 x the share of its source chunks that are of the destination's class) x
// (1 + a deterministic jitter of at most 0.3 %) to the stream's clock: the two levels measured on MI355X (0.219 / 0.252 ms,
// igdsp_io.hip).  Events stamp that clock.
//
// The run fails (exit 3, with a message) when an address is mapped onto another handle than the first one it was ever mapped
// onto (the stale-translation rule), when a map is placed over a live mapping, when a handle is released twice
// or a launch touches an unmapped address.  IOFAKE_TRACE=1 prints one line per VMM call and per launch on stdout ("T ...").
#include "igdsp_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace iofake {

constexpr size_t kGran = (size_t)2 << 20;
constexpr uintptr_t kVaBase = (uintptr_t)1 << 44;

struct Run { std::string letters; size_t n; };      // n == 0: without end

struct State {
    std::vector<Run> runs;
    size_t free_bytes = (size_t)280 << 30, total_bytes = (size_t)288 << 30;
    int vmm = 1;
    bool trace = false;
    std::map<std::string, long> fail_at;             // call kind -> calls left until the one that fails
    std::map<std::string, long> calls;
    // handles: id -> {class, bytes, live}
    struct Handle { char cls; size_t bytes; bool live; };
    std::vector<Handle> handles{{'?', 0, false}};    // id 0 unused
    size_t live_handle_bytes = 0;
    uintptr_t va_next = kVaBase;
    std::map<uintptr_t, size_t> live;                 // granule -> handle id
    std::map<uintptr_t, size_t> first;                // granule -> first handle id ever mapped there
    double clock_ms = 0.0;
    uint64_t launches = 0;
    std::vector<double> events{0.0};
    uintptr_t malloc_next = (uintptr_t)3 << 44;
    size_t live_mallocs = 0;
} S;

[[noreturn]] void die(const char *what, uintptr_t va, size_t a, size_t b)
{
    std::fflush(stdout);
    std::fprintf(stderr, "iofake: %s at va+0x%llx (%zu, %zu)\n", what, (unsigned long long)(va - kVaBase), a, b);
    std::exit(3);
}

bool inject(const char *kind)
{
    long &n = S.calls[kind];
    ++n;
    auto it = S.fail_at.find(kind);
    if (it == S.fail_at.end()) return false;
    if (--it->second > 0) return false;
    S.fail_at.erase(it);
    if (S.trace) std::printf("T inject %s\n", kind);
    return true;
}

char class_of_index(size_t n)
{
    for (const Run &r : S.runs) {
        if (r.n == 0 || n < r.n) return r.letters[n % r.letters.size()];
        n -= r.n;
    }
    return '?';
}

size_t id_of(hipMemGenericAllocationHandle_t h) { return (size_t)reinterpret_cast<uintptr_t>(h) >> 4; }
hipMemGenericAllocationHandle_t handle_of(size_t id) { return reinterpret_cast<hipMemGenericAllocationHandle_t>((uintptr_t)id << 4); }
uintptr_t off(const void *p) { return (uintptr_t)p - kVaBase; }

// the handle behind every granule of [p, p + bytes); dies on an unmapped one
std::vector<size_t> resolve(const void *p, size_t bytes, const char *what)
{
    std::vector<size_t> ids;
    for (uintptr_t g = (uintptr_t)p / kGran * kGran; g < (uintptr_t)p + bytes; g += kGran) {
        auto it = S.live.find(g);
        if (it == S.live.end()) die(what, g, bytes, 0);
        if (ids.empty() || ids.back() != it->second) ids.push_back(it->second);
    }
    return ids;
}

}  // namespace iofake

using namespace iofake;

// ---- the scenario side (io_alloc_driver.cpp) ----
void iofake_setup(const char *classes, size_t free_bytes, int vmm)
{
    S.runs.clear();
    std::string spec(classes);
    size_t pos = 0;
    while (pos < spec.size()) {
        size_t end = spec.find(' ', pos);
        if (end == std::string::npos) end = spec.size();
        const std::string tok = spec.substr(pos, end - pos);
        pos = end + 1;
        if (tok.empty()) continue;
        size_t k = 0;
        while (k < tok.size() && tok[k] >= 'A' && tok[k] <= 'Z') ++k;
        S.runs.push_back({tok.substr(0, k), tok.substr(k) == "*" ? 0 : (size_t)std::strtoull(tok.c_str() + k, nullptr, 10)});
    }
    S.free_bytes = free_bytes;
    S.total_bytes = free_bytes + ((size_t)8 << 30);
    S.vmm = vmm;
    const char *t = std::getenv("IOFAKE_TRACE");
    S.trace = t && std::atoi(t) != 0;
}
void iofake_fail(const char *kind, long nth) { S.fail_at[kind] = nth; }
// class letter of the chunk mapped at p ('-': nothing mapped there)
char iofake_class_at(const void *p)
{
    auto it = S.live.find((uintptr_t)p / kGran * kGran);
    return it == S.live.end() ? '-' : S.handles[it->second].cls;
}
size_t iofake_live_handles()
{
    size_t n = 0;
    for (const auto &h : S.handles) n += h.live ? 1 : 0;
    return n;
}
size_t iofake_live_mappings() { return S.live.size(); }
size_t iofake_live_mallocs() { return S.live_mallocs; }

// ---- the HIP side ----
extern "C" {

hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "iofake error"; }

hipError_t hipDeviceGetAttribute(int *pi, hipDeviceAttribute_t attr, int)
{
    *pi = attr == hipDeviceAttributeVirtualMemoryManagementSupported ? S.vmm : 0;
    return hipSuccess;
}

hipError_t hipMemGetInfo(size_t *free, size_t *total)
{
    *free = S.free_bytes - S.live_handle_bytes;
    *total = S.total_bytes;
    return hipSuccess;
}

hipError_t hipMemGetAllocationGranularity(size_t *granularity, const hipMemAllocationProp *, hipMemAllocationGranularity_flags)
{
    *granularity = kGran;
    return hipSuccess;
}

hipError_t hipMemCreate(hipMemGenericAllocationHandle_t *handle, size_t size, const hipMemAllocationProp *, unsigned long long)
{
    if (inject("create") || size > S.free_bytes - S.live_handle_bytes) {
        if (S.trace) std::printf("T create fail\n");
        return hipErrorOutOfMemory;
    }
    const size_t id = S.handles.size();
    S.handles.push_back({class_of_index(id - 1), size, true});
    S.live_handle_bytes += size;
    *handle = handle_of(id);
    if (S.trace) std::printf("T create h%zu %c\n", id, S.handles[id].cls);
    return hipSuccess;
}

hipError_t hipMemRelease(hipMemGenericAllocationHandle_t handle)
{
    const size_t id = id_of(handle);
    if (id == 0 || id >= S.handles.size() || !S.handles[id].live) die("release of a dead handle", kVaBase, id, 0);
    S.handles[id].live = false;
    S.live_handle_bytes -= S.handles[id].bytes;
    if (S.trace) std::printf("T release h%zu\n", id);
    return hipSuccess;
}

hipError_t hipMemAddressReserve(void **ptr, size_t size, size_t alignment, void *, unsigned long long)
{
    if (inject("reserve")) { if (S.trace) std::printf("T reserve fail\n"); return hipErrorOutOfMemory; }
    const size_t a = alignment ? alignment : kGran;
    S.va_next = (S.va_next + a - 1) / a * a;
    *ptr = reinterpret_cast<void *>(S.va_next);
    S.va_next += (size + kGran - 1) / kGran * kGran;
    if (S.trace) std::printf("T reserve va+0x%llx %zu\n", (unsigned long long)off(*ptr), size);
    return hipSuccess;
}

hipError_t hipMemMap(void *ptr, size_t size, size_t, hipMemGenericAllocationHandle_t handle, unsigned long long)
{
    const size_t id = id_of(handle);
    if (inject("map")) { if (S.trace) std::printf("T map fail va+0x%llx h%zu\n", (unsigned long long)off(ptr), id); return hipErrorOutOfMemory; }
    if (id == 0 || id >= S.handles.size() || !S.handles[id].live) die("map of a dead handle", (uintptr_t)ptr, id, 0);
    for (uintptr_t g = (uintptr_t)ptr; g < (uintptr_t)ptr + size; g += kGran) {
        if (S.live.count(g)) die("map over a live mapping", g, id, S.live[g]);
        auto f = S.first.find(g);
        if (f != S.first.end() && f->second != id) die("address mapped onto a second handle (stale translation)", g, id, f->second);
    }
    for (uintptr_t g = (uintptr_t)ptr; g < (uintptr_t)ptr + size; g += kGran) { S.live[g] = id; S.first.emplace(g, id); }
    if (S.trace) std::printf("T map va+0x%llx h%zu\n", (unsigned long long)off(ptr), id);
    return hipSuccess;
}

hipError_t hipMemUnmap(void *ptr, size_t size)
{
    bool any = false;
    for (uintptr_t g = (uintptr_t)ptr; g < (uintptr_t)ptr + size; g += kGran) any = S.live.erase(g) > 0 || any;
    if (S.trace) std::printf("T unmap va+0x%llx%s\n", (unsigned long long)off(ptr), any ? "" : " (not mapped)");
    return any ? hipSuccess : hipErrorInvalidValue;
}

hipError_t hipMemSetAccess(void *ptr, size_t size, const hipMemAccessDesc *, size_t)
{
    if (inject("access")) { if (S.trace) std::printf("T access fail\n"); return hipErrorInvalidValue; }
    for (uintptr_t g = (uintptr_t)ptr; g < (uintptr_t)ptr + size; g += kGran)
        if (!S.live.count(g)) return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t hipMalloc(void **ptr, size_t size)
{
    if (inject("malloc")) return hipErrorOutOfMemory;
    *ptr = reinterpret_cast<void *>(S.malloc_next);
    S.malloc_next += (size + kGran - 1) / kGran * kGran;
    ++S.live_mallocs;
    if (S.trace) std::printf("T malloc %zu\n", size);
    return hipSuccess;
}

hipError_t hipFree(void *ptr)
{
    if (ptr) --S.live_mallocs;
    if (S.trace) std::printf("T free\n");
    return hipSuccess;
}

hipError_t hipEventCreate(hipEvent_t *event)
{
    S.events.push_back(0.0);
    *event = reinterpret_cast<hipEvent_t>((uintptr_t)(S.events.size() - 1) << 4);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t)
{
    S.events[(uintptr_t)event >> 4] = S.clock_ms;
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t start, hipEvent_t stop)
{
    *ms = (float)(S.events[(uintptr_t)stop >> 4] - S.events[(uintptr_t)start >> 4]);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }

// only igdsp_internal_vmm_remap_check uses these: it needs a device
hipError_t hipMemAddressFree(void *, size_t) { return hipErrorNotSupported; }
hipError_t hipMemcpy(void *, const void *, size_t, hipMemcpyKind) { return hipErrorNotSupported; }
hipError_t hipMemsetAsync(void *, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipErrorNotSupported; }

}  // extern "C"

namespace igdsp {

// k_stream_rw: reads bytes / 10240 super-rows of 10 KiB from src, writes 1 KiB of each to dst
hipError_t launch_stream_rw(const LaunchCfg &, const void *src, size_t bytes, void *dst, hipStream_t)
{
    const size_t rows = bytes / 10240u;
    if (rows == 0) return hipSuccess;
    const std::vector<size_t> srcs = resolve(src, rows * 10240u, "launch reads an unmapped address");
    const std::vector<size_t> dsts = resolve(dst, rows * 1024u, "launch writes an unmapped address");
    const char dc = S.handles[dsts[0]].cls;
    size_t same = 0;
    for (size_t id : srcs) same += S.handles[id].cls == dc ? 1 : 0;
    const uint64_t x = (++S.launches) * 0x9E3779B97F4A7C15ull;
    const double jitter = ((double)((x >> 40) % 2001) - 1000.0) * 3e-6;         // within +-0.3 %
    const double ms = 0.219 * (1.0 + 0.15 * (double)same / (double)srcs.size()) * (1.0 + jitter);
    S.clock_ms += ms;
    if (S.trace) {
        std::printf("T launch");
        for (size_t id : srcs) std::printf(" h%zu", id);
        std::printf(" -> h%zu %.6f\n", dsts[0], ms);
    }
    return hipSuccess;
}

}  // namespace igdsp
