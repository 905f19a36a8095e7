// Runs the real csrc/igdsp_io.hip on the CPU against tests/ioalloc/fake_hip.cpp: tests/test_io_alloc_cpu.py.
//
// Script on stdin, one command per line:
//   device <free GiB> <vmm 0|1> <class map...>     the fake device (fake_hip.cpp: "A30 B50 A40 C*", "BC200", ...)
//   cap <n>                                        ctx->io_spare_cap (what igdsp_create reads from IGDSP_IO_SPARE_CHUNKS)
//   fail <create|map|access|reserve|malloc> <k>    the k-th call of that kind from here on returns an error
//   alloc <name> <limit MiB> <in|rec|bulk>:<MiB>...  igdsp_io_alloc(explore_limit_bytes = limit)
//   free <name>                                    igdsp_io_free
//   drop                                           igdsp_io_drop_spares
//   live                                           live handles / mappings / plain allocations
// Output: "alloc <name> rc=.. <report fields>", "err <text>" on failure, "buf <name> <i> <role> <class runs>" per buffer (the
// class letter of every chunk behind bufs[i].ptr, run-length coded: "B9 C5"; '-' = nothing mapped), "spares <per label>".
#include "igdsp_ctx.h"

#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

void iofake_setup(const char *classes, size_t free_bytes, int vmm);
void iofake_fail(const char *kind, long nth);
char iofake_class_at(const void *p);
size_t iofake_live_handles();
size_t iofake_live_mappings();
size_t iofake_live_mallocs();

namespace {

const char *kRole[] = {"in", "rec", "bulk"};

std::string runs_of(const void *p, size_t chunks, size_t chunk)
{
    if (!p) return "null";
    std::string out;
    char cur = 0;
    size_t n = 0;
    auto flush = [&]() { if (n) out += (out.empty() ? "" : " ") + std::string(1, cur) + std::to_string(n); };
    for (size_t k = 0; k < chunks; ++k) {
        const char c = iofake_class_at((const char *)p + k * chunk);
        if (c != cur) { flush(); cur = c; n = 0; }
        ++n;
    }
    flush();
    return out;
}

}  // namespace

int main()
{
    igdsp_ctx ctx;
    ctx.device = 0;
    ctx.cus = 256;
    ctx.stream = nullptr;
    std::map<std::string, igdsp_io_set *> sets;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "device") {
            double gib = 0;
            int vmm = 1;
            in >> gib >> vmm;
            std::string rest;
            std::getline(in, rest);
            iofake_setup(rest.c_str(), (size_t)(gib * (double)(1ull << 30)), vmm);
        } else if (cmd == "cap") {
            in >> ctx.io_spare_cap;
        } else if (cmd == "fail") {
            std::string kind;
            long nth = 1;
            in >> kind >> nth;
            iofake_fail(kind.c_str(), nth);
        } else if (cmd == "alloc") {
            std::string name, tok;
            size_t limit_mib = 0;
            in >> name >> limit_mib;
            std::vector<igdsp_io_buf> bufs;
            while (in >> tok) {
                igdsp_io_buf b{};
                const std::string role = tok.substr(0, tok.find(':'));
                b.role = role == "in" ? IGDSP_IO_INPUT : (role == "rec" ? IGDSP_IO_RECORD : IGDSP_IO_BULK);
                b.bytes = (size_t)std::stoull(tok.substr(tok.find(':') + 1)) << 20;
                bufs.push_back(b);
            }
            igdsp_io_set *set = nullptr;
            igdsp_io_report r{};
            const int rc = igdsp_io_alloc(&ctx, bufs.data(), (uint32_t)bufs.size(), limit_mib << 20, &set, &r);
            std::printf("alloc %s rc=%d placed=%u bulk_spread=%u classes_found=%u chunks_explored=%u probes=%u reseeds=%u chunk_bytes=%llu "
                        "explored_bytes=%llu probe_ms_same=%.4f probe_ms_other=%.4f settle=%d\n", name.c_str(), rc, r.placed, r.bulk_spread,
                        r.classes_found, r.chunks_explored, r.probes, r.reseeds, (unsigned long long)r.chunk_bytes,
                        (unsigned long long)r.explored_bytes, r.probe_ms_same, r.probe_ms_other, r.settle_ms > 0.f ? 1 : 0);
            if (rc != IGDSP_OK) std::printf("err %s\n", ctx.err.c_str());
            const size_t chunk = r.chunk_bytes ? r.chunk_bytes : ((size_t)128 << 20);
            for (size_t i = 0; i < bufs.size(); ++i)
                std::printf("buf %s %zu %s %s\n", name.c_str(), i, kRole[bufs[i].role],
                            runs_of(bufs[i].ptr, (bufs[i].bytes + chunk - 1) / chunk, chunk).c_str());
            if (set) sets[name] = set;
            std::printf("spares %zu %zu %zu %zu\n", ctx.io_spare[0].size(), ctx.io_spare[1].size(), ctx.io_spare[2].size(), ctx.io_spare[3].size());
        } else if (cmd == "free") {
            std::string name;
            in >> name;
            std::printf("free %s rc=%d\n", name.c_str(), igdsp_io_free(&ctx, sets[name]));
            sets.erase(name);
            std::printf("spares %zu %zu %zu %zu\n", ctx.io_spare[0].size(), ctx.io_spare[1].size(), ctx.io_spare[2].size(), ctx.io_spare[3].size());
        } else if (cmd == "drop") {
            igdsp_io_drop_spares(&ctx);
            std::printf("drop\n");
        } else if (cmd == "live") {
            std::printf("live handles=%zu mappings=%zu mallocs=%zu\n", iofake_live_handles(), iofake_live_mappings(), iofake_live_mallocs());
        } else {
            std::fprintf(stderr, "unknown command: %s\n", cmd.c_str());
            return 2;
        }
        std::fflush(stdout);
    }
    return 0;
}
