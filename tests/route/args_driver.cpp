// Prints the verdicts of the argument rules (csrc/igdsp_args.h) for tests/test_args_cpu.py.  One case per stdin line: the rule's name
// (the entry without igdsp_, tx_copy for igdsp_internal_tx_copy), then key=value pairs named after the entry's C parameters.  A pointer
// is 0, a or a+k (a: a fixed 4096-aligned number, never dereferenced); a number is anything strtoull reads.  win=1 / cfg=1 pass a host
// struct built from the win.<field> / cfg.<field> keys, 0 passes NULL.  One output line per case: rc=<code> run=<0|1>.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "igdsp_args.h"

using namespace igdsp::args;

namespace {
constexpr uintptr_t kA = 0x7f0000001000ull;

struct Case {
    std::map<std::string, std::string> kv;
    const std::string &at(const char *key) const
    {
        auto it = kv.find(key);
        if (it == kv.end()) { std::fprintf(stderr, "missing key %s\n", key); std::exit(2); }
        return it->second;
    }
    uint64_t q(const char *key) const { return std::strtoull(at(key).c_str(), nullptr, 0); }
    uint32_t u(const char *key) const { return (uint32_t)q(key); }
    int i(const char *key) const { return (int)std::strtoll(at(key).c_str(), nullptr, 0); }
    const void *p(const char *key) const
    {
        const std::string &v = at(key);
        if (v[0] != 'a') return reinterpret_cast<const void *>((uintptr_t)std::strtoull(v.c_str(), nullptr, 0));
        return reinterpret_cast<const void *>(kA + (v.size() > 1 ? std::strtoull(v.c_str() + 1, nullptr, 0) : 0));
    }
};
}  // namespace

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string entry, kv;
        Case c;
        in >> entry;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            c.kv[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        igdsp_window win{};
        const igdsp_window *pwin = nullptr;
        if (c.kv.count("win") && c.u("win")) {
            win.gate_mode = c.u("win.gate_mode");
            win.probe_alarm = c.u("win.probe_alarm");
            win.d_hold = (igdsp_chan_hold *)c.p("win.d_hold");
            win.d_gate = (const uint8_t *)c.p("win.d_gate");
            win.d_probe = (igdsp_chan_probe *)c.p("win.d_probe");
            win.d_work = (void *)c.p("win.d_work");
            pwin = &win;
        }
        igdsp_jb_adapt_cfg cfg{};
        const igdsp_jb_adapt_cfg *pcfg = nullptr;
        if (c.kv.count("cfg") && c.u("cfg")) {
            cfg.min_frames = (uint8_t)c.u("cfg.min_frames");
            cfg.max_frames = (uint8_t)c.u("cfg.max_frames");
            cfg.init_frames = (uint8_t)c.u("cfg.init_frames");
            cfg.jitter_mult = (uint8_t)c.u("cfg.jitter_mult");
            cfg.late_restart = (uint8_t)c.u("cfg.late_restart");
            pcfg = &cfg;
        }
        Verdict v{};
        if (entry == "decode_meter")
            v = decode_meter(c.p("d_payload"), c.p("d_codec"), c.p("d_len"), c.u("C"), c.u("F"), c.u("n"), c.p("d_stats"), c.p("d_pcm"), c.p("d_agg"),
                             c.u("rank"));
        else if (entry == "encode")
            v = encode(c.p("d_pcm"), c.p("d_codec"), c.u("C"), c.u("F"), c.u("n"), c.p("d_out"), c.i("variant"));
        else if (entry == "roundtrip_peakhold")
            v = roundtrip_peakhold(c.p("d_payload"), c.p("d_codec"), c.u("C"), c.u("F"), c.u("n"), c.p("d_out"), c.p("d_stats"), c.p("d_hold"),
                                   c.p("d_gate"), c.i("variant"));
        else if (entry == "hold_update")
            v = hold_update(c.p("d_stats"), c.u("C"), c.u("F"), c.u("n"), c.p("d_hold"), c.p("d_gate"));
        else if (entry == "depayload")
            v = depayload(c.p("d_packets"), c.p("d_sizes"), c.p("d_radio"), c.u("C"), c.u("F"), c.u("pkt_stride"), c.u("n"), c.p("d_payload_out"),
                          c.p("d_len_out"), c.p("d_info_out"));
        else if (entry == "decode_meter_rtp")
            v = decode_meter_rtp(c.p("d_slots"), c.p("d_codec"), c.u("C"), c.u("F"), c.p("d_stats"), c.p("d_info"), c.p("d_agg"), c.u("rank"));
        else if (entry == "decode_meter_packets")
            v = decode_meter_packets(c.p("d_packets"), c.p("d_sizes"), c.p("d_codec"), c.u("C"), c.u("F"), c.u("pkt_stride"), c.u("hdr_bytes"),
                                     c.p("d_stats"), c.p("d_info"), c.p("d_agg"), c.u("rank"));
        else if (entry == "decode_meter_packets_mixed")
            v = decode_meter_packets_mixed(c.p("d_packets"), c.p("d_sizes"), c.p("d_codec"), c.p("d_radio"), c.u("C"), c.u("F"), c.u("pkt_stride"),
                                           c.p("d_stats"), c.p("d_info"), c.p("d_agg"), c.u("rank"));
        else if (entry == "window_update")
            v = window_update(c.p("d_stats"), c.p("d_info"), c.p("d_len"), c.u("C"), c.u("F"), c.u("n"), pwin);
        else if (entry == "decode_meter_window")
            v = decode_meter_window(c.u("layout"), c.p("d_packets"), c.p("d_sizes"), c.p("d_codec"), c.p("d_radio"), c.u("C"), c.u("F"),
                                    c.u("pkt_stride"), c.u("hdr_bytes"), c.p("d_stats"), c.p("d_info"), c.p("d_agg"), c.u("rank"), pwin);
        else if (entry == "wav_expand")
            v = wav_expand(c.p("d_payload"), c.u("C"), c.u("F"), c.u("n"), c.u("rate"), c.p("d_files"), c.q("file_stride"));
        else if (entry == "tx_packetize")
            v = tx_packetize(c.p("d_pcm"), c.p("d_g711"), c.p("d_ctl"), c.u("C"), c.u("F"), c.u("n"), c.q("t0_ms"), c.u("frame_ms"), c.p("d_state"),
                             c.p("d_last_payload"), c.p("d_packets"), c.u("pkt_stride"), c.p("d_sizes"), c.p("d_info"), c.i("variant"));
        else if (entry == "tx_copy")
            v = tx_copy(c.p("d_pcm"), c.p("d_g711"), c.u("C"), c.u("F"), c.u("n"), c.p("d_packets"), c.u("pkt_stride"));
        else if (entry == "g726_reorder")
            v = g726_reorder(c.p("d_in"), c.p("d_out"), c.q("n_bytes"), c.i("mode"));
        else if (entry == "conf_mix")
            v = conf_mix(c.p("d_payload"), c.p("d_codec"), c.p("d_pcm"), c.p("d_len"), c.p("d_gain"), c.p("d_port_ptr"), c.p("d_members"),
                         c.u("n_members"), c.u("C"), c.u("P"), c.u("F"), c.u("n"), c.p("d_out"), c.p("d_stats"));
        else if (entry == "bss_select")
            v = bss_select(c.p("d_info"), c.p("d_payload"), c.p("d_codec"), c.p("d_pcm"), c.p("d_len"), c.p("d_gain"), c.p("d_group_ptr"),
                           c.p("d_members"), c.u("n_members"), c.p("d_mute"), c.u("C"), c.u("G"), c.u("F"), c.u("n"), c.u("vote_frames"),
                           c.p("d_state"), c.p("d_words"), c.p("d_sel"), c.p("d_out"), c.p("d_stats"));
        else if (entry == "ptt_arbitrate")
            v = ptt_arbitrate(c.p("d_info"), c.p("d_payload"), c.p("d_codec"), c.p("d_pcm"), c.p("d_len"), c.p("d_gain"), c.p("d_group_ptr"),
                              c.p("d_members"), c.u("n_members"), c.p("d_rxonly"), c.u("C"), c.u("G"), c.u("F"), c.u("n"), c.u("release_frames"),
                              c.p("d_state"), c.p("d_slots"), c.p("d_sel"), c.p("d_tick"), c.p("d_ctl_out"), c.p("d_out"), c.p("d_stats"));
        else if (entry == "link_watch")
            v = link_watch(c.p("d_info"), c.p("d_sizes"), c.p("d_up"), c.p("d_period_ms"), c.u("C"), c.u("T"), c.u("S"), c.q("t0_ms"), c.u("tick_ms"),
                           c.u("miss_ticks"), c.u("event_mask"), c.p("d_state"), c.p("d_kind"), c.p("d_events"), c.u("event_cap"),
                           c.p("d_event_count"), c.p("d_work"));
        else if (entry == "jb_receive")
            v = jb_receive(c.p("d_packets"), c.p("d_sizes"), c.p("d_radio"), c.p("d_arrival"), c.u("C"), c.u("T"), c.u("S"), c.u("pkt_stride"), c.u("n"),
                           c.u("delay_frames"), c.p("d_state"), c.p("d_ring"), c.p("d_payload_out"), c.p("d_len_out"), c.p("d_info_out"),
                           c.p("d_tick_flags"), c.p("d_pkt_status"));
        else if (entry == "jb_receive_adaptive")
            v = jb_receive_adaptive(c.p("d_packets"), c.p("d_sizes"), c.p("d_radio"), c.p("d_arrival"), c.u("C"), c.u("T"), c.u("S"), c.u("pkt_stride"),
                                    c.u("n"), pcfg, c.p("d_state"), c.p("d_ring"), c.p("d_adapt"), c.p("d_payload_out"), c.p("d_len_out"),
                                    c.p("d_info_out"), c.p("d_tick_flags"), c.p("d_pkt_status"), c.p("d_delay_out"));
        else if (entry == "plc_conceal")
            v = plc_conceal(c.p("d_tick_flags"), c.p("d_payload"), c.p("d_codec"), c.p("d_pcm"), c.p("d_len"), c.u("C"), c.u("T"), c.u("n"),
                            c.p("d_state"), c.p("d_out"), c.p("d_len_out"), c.p("d_stats"));
        else {
            std::fprintf(stderr, "unknown entry %s\n", entry.c_str());
            return 2;
        }
        if (v.run && (v.rc != IGDSP_OK || v.why)) return 3;                // a verdict that launches carries no code and no text
        std::printf("rc=%d run=%d\n", v.rc, v.run ? 1 : 0);
    }
    return 0;
}
