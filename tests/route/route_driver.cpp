// Prints the routes of igdsp_route.h for the route tests (through tests/route_util.py).  One case per stdin line: an entry name, then key=value pairs
// (numbers in any base strtoull reads; IGDSP_* keys are set in the environment and read back through knobs_from_env, the rest
// are the route function's arguments).  One output line per case: the route's fields as key=value.  "consts" prints the
// compile-time geometry the tests derive work per wave from.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "igdsp_route.h"

using namespace igdsp;

static const char *kKnobs[] = {"IGDSP_NO_TINY", "IGDSP_NO_STRIDED", "IGDSP_IMG_WAVES", "IGDSP_RT_ORDER", "IGDSP_RT_MID", "IGDSP_RT_NSEG", "IGDSP_RT_GPB",
                               "IGDSP_RT_BLK", "IGDSP_RTB_WAVES", "IGDSP_WIN_NSEG", "IGDSP_WIN_GPB", "IGDSP_WIN_BLK", "IGDSP_WIN_WAVES"};

static const char *name(MeterFast f)
{
    switch (f) { case MeterFast::fat: return "fat"; case MeterFast::chunk: return "chunk"; case MeterFast::tiny: return "tiny";
                 case MeterFast::strided: return "strided"; default: return "none"; }
}
static const char *name(MeterRest f)
{
    switch (f) { case MeterRest::image: return "image"; case MeterRest::wave_per_frame: return "wave_per_frame"; default: return "none"; }
}
static const char *name(RtForm f)
{
    switch (f) { case RtForm::lut64: return "lut64"; case RtForm::chunk64: return "chunk64"; case RtForm::blk64: return "blk64";
                 case RtForm::strided: return "strided"; case RtForm::strided_blk: return "strided_blk"; default: return "none"; }
}
static const char *name(EncForm f)
{
    switch (f) { case EncForm::lut16: return "lut16"; case EncForm::v8_table: return "v8_table"; case EncForm::v8: return "v8";
                 case EncForm::scalar: return "scalar"; default: return "none"; }
}
static const char *tx_name(int f) { return f == kTxPcmTab ? "pcm_tab" : (f == kTxPcm ? "pcm" : "g711"); }

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string entry, kv;
        in >> entry;
        std::map<std::string, unsigned long long> a;
        for (const char *k : kKnobs) unsetenv(k);
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string key = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (key.rfind("IGDSP_", 0) == 0) setenv(key.c_str(), val.c_str(), 1);
            else a[key] = std::strtoull(val.c_str(), nullptr, 0);
        }
        const Knobs k = knobs_from_env();
        auto g = [&](const char *key, unsigned long long dflt = 0) { return a.count(key) ? a[key] : dflt; };
        const uint32_t C = (uint32_t)g("C"), F = (uint32_t)g("F"), n = (uint32_t)g("n", 160), cus = (uint32_t)g("cus", 256);
        if (entry == "meter") {
            const MeterRoute r = decode_meter_route(C, F, n, (int)g("variant"), g("len") != 0, g("payload", 0x1000), g("pcm"), g("stats", 0x1000), cus, k);
            std::printf("fast=%s store=%d key=%d grid=%u threads=%u done=%u rest=%s rest_grid=%u rest_threads=%u rest_lds=%u\n", name(r.fast), r.store,
                        r.key, r.grid, r.threads, r.done, name(r.rest), r.rest_grid, r.rest_threads, r.rest_lds);
        } else if (entry == "roundtrip") {
            const RtRoute r = roundtrip_route(C, F, n, (int)g("variant"), g("payload", 0x1000), g("out", 0x1000), g("stats", 0x1000), g("spread") != 0, cus, k);
            std::printf("form=%s key=%d grid=%u threads=%u n_groups=%u n_seg=%u order=%u gpb=%u gsh=%u mid_start=%u c_first=%u gen_grid=%u\n", name(r.form),
                        r.key, r.grid, r.threads, r.n_groups, r.n_seg, r.order, r.gpb, r.gsh, r.mid_start, r.c_first, r.gen_grid);
        } else if (entry == "encode") {
            const EncRoute r = encode_route(C, F, n, g("pcm", 0x1000), g("out", 0x1000), cus);
            std::printf("form=%s grid=%u threads=%u groups=%llu table=%d\n", name(r.form), r.grid, r.threads, (unsigned long long)r.groups,
                        encode_wants_table(r));
        } else if (entry == "window") {
            const WinRoute r = window_route(C, F, cus, k);
            std::printf("fits=%d blk=%d n_groups=%u n_seg=%u gpb=%u gsh=%u parts=%u grid=%u threads=%u\n", r.fits, r.blk, r.n_groups, r.n_seg, r.gpb,
                        r.gsh, r.parts, r.grid, r.threads);
        } else if (entry == "tx") {
            const uint64_t pcm = g("pcm"), g711 = g("g711");
            const TxRoute r = tx_route(C, F, n, pcm, g711, g("last", 0x1000), cus, g("tab_lds", 1) != 0);
            std::printf("form=%s vec=%u n_groups=%u grid=%u threads=%u lds=%u table=%d\n", tx_name(r.form), r.vec, r.n_groups, r.grid, r.threads, r.lds,
                        tx_wants_table(pcm != 0, C, F, n));
        } else if (entry == "tx_copy") {   // the yardstick of tx (launch_tx_copy_ab)
            const uint64_t pcm = g("pcm"), g711 = g("g711");
            const TxRoute r = tx_copy_route(C, F, n, pcm, g711, cus, g("tab_lds", 1) != 0);
            std::printf("form=%s vec=%u n_groups=%u grid=%u threads=%u lds=%u table=%d\n", tx_name(r.form), r.vec, r.n_groups, r.grid, r.threads, r.lds,
                        tx_wants_table(pcm != 0, C, F, n));
        } else if (entry == "bss") {   // form 0 G.711 / 1 PCM / 2 none; in, out: buffer addresses, alignment only
            const BssRoute r = bss_route((uint32_t)g("G"), F, n, (uint32_t)g("members"), (int)g("form"), g("in", 0x1000), g("out", 0x1000));
            std::printf("form=%d gpw=%u vec_in=%u vec_out=%u grid=%u threads=%u part_frames=%u parts=%u words_grid=%u\n", r.form, r.gpw, r.vec_in,
                        r.vec_out, r.grid, r.threads, r.part_frames, r.parts, r.words_grid);
        } else if (entry == "jb") {    // out: the payload output's address, alignment only
            const JbRoute r = jb_route(C, (uint32_t)g("T"), n, g("out", 0x1000));
            std::printf("vec=%u pieces=%u grid=%u threads=%u part_ticks=%u parts=%u ring=%llu\n", r.vec, r.pieces, r.grid, r.threads, r.part_ticks,
                        r.parts, (unsigned long long)jb_ring_bytes(C, n));
        } else if (entry == "plc") {   // pcm: 1 for the PCM input; in / out: the input's and the output's addresses, alignment only
            const PlcRoute r = plc_route(C, (uint32_t)g("T"), n, g("pcm") != 0, g("in", 0x1000), g("out", 0x1000));
            std::printf("vec=%u pieces=%u batch_rows=%u grid=%u threads=%u part_ticks=%u parts=%u\n", r.vec, r.pieces, r.batch_rows, r.grid,
                        r.threads, r.part_ticks, r.parts);
        } else if (entry == "consts") {
            std::printf("tiny_slot=%u super_frames=%d\n", kTinySlot, kSuperFrames);
        } else {
            std::printf("unknown entry %s\n", entry.c_str());
            return 1;
        }
    }
    return 0;
}
