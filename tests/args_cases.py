"""The argument rules of the batched C entries as one table, for tests/test_args_cpu.py (through tests/route/args_driver.cpp, which
calls csrc/igdsp_args.h with g++ alone) and tests/test_gpu_args.py (through the library, rows that launch nothing).

CASES rows are (entry, {key: value}, rc, run): the keys are the entry's C parameter names (SIG, in the C order without ctx and
stream), the values override the entry's launchable BASE; rc is the code the entry returns, run = 1 where it would launch.  Pointer
values are the tokens "0", "a", "a+1", "a+2", "a+4", "a+8": a is 4096-aligned (a fixed number in the driver, a 64 KiB device buffer
on the GPU); a pointer is only compared and masked.  The two host structs are spelt as win = 0 / 1 with win.<field>, and cfg = 0 / 1
with cfg.<field>.

Where the codes come from: rows under "from tests/test_gpu_*" are the assertions of the existing GPU argument tests; every other row
is include/igdsp.h's contract and a reading of the entry.  Rows with run = 0 are replayed against the library by test_gpu_args.py."""
EINVAL, ERANGE = -22, -34
A24 = 1 << 24

# kinds: p pointer, u uint32, q uint64, i int, win const igdsp_window *, cfg const igdsp_jb_adapt_cfg *
SIG = {
    "decode_meter": "d_payload:p d_codec:p d_len:p C:u F:u n:u d_stats:p d_pcm:p d_agg:p rank:u",
    "encode": "d_pcm:p d_codec:p C:u F:u n:u d_out:p variant:i",
    "roundtrip_peakhold": "d_payload:p d_codec:p C:u F:u n:u d_out:p d_stats:p d_hold:p d_gate:p variant:i",
    "hold_update": "d_stats:p C:u F:u n:u d_hold:p d_gate:p",
    "depayload": "d_packets:p d_sizes:p d_radio:p C:u F:u pkt_stride:u n:u d_payload_out:p d_len_out:p d_info_out:p",
    "decode_meter_rtp": "d_slots:p d_codec:p C:u F:u d_stats:p d_info:p d_agg:p rank:u",
    "decode_meter_packets": "d_packets:p d_sizes:p d_codec:p C:u F:u pkt_stride:u hdr_bytes:u d_stats:p d_info:p d_agg:p rank:u",
    "decode_meter_packets_mixed": "d_packets:p d_sizes:p d_codec:p d_radio:p C:u F:u pkt_stride:u d_stats:p d_info:p d_agg:p rank:u",
    "window_update": "d_stats:p d_info:p d_len:p C:u F:u n:u win:win",
    "decode_meter_window": "layout:u d_packets:p d_sizes:p d_codec:p d_radio:p C:u F:u pkt_stride:u hdr_bytes:u d_stats:p d_info:p d_agg:p "
                           "rank:u win:win",
    "wav_expand": "d_payload:p C:u F:u n:u rate:u d_files:p file_stride:q",
    "tx_packetize": "d_pcm:p d_g711:p d_ctl:p C:u F:u n:u t0_ms:q frame_ms:u d_state:p d_last_payload:p d_packets:p pkt_stride:u d_sizes:p "
                    "d_info:p variant:i",
    "tx_copy": "d_pcm:p d_g711:p C:u F:u n:u d_packets:p pkt_stride:u",
    "g726_reorder": "d_in:p d_out:p n_bytes:q mode:i",
    "conf_mix": "d_payload:p d_codec:p d_pcm:p d_len:p d_gain:p d_port_ptr:p d_members:p n_members:u C:u P:u F:u n:u d_out:p d_stats:p",
    "bss_select": "d_info:p d_payload:p d_codec:p d_pcm:p d_len:p d_gain:p d_group_ptr:p d_members:p n_members:u d_mute:p C:u G:u F:u n:u "
                  "vote_frames:u d_state:p d_words:p d_sel:p d_out:p d_stats:p",
    "ptt_arbitrate": "d_info:p d_payload:p d_codec:p d_pcm:p d_len:p d_gain:p d_group_ptr:p d_members:p n_members:u d_rxonly:p C:u G:u F:u n:u "
                     "release_frames:u d_state:p d_slots:p d_sel:p d_tick:p d_ctl_out:p d_out:p d_stats:p",
    "link_watch": "d_info:p d_sizes:p d_up:p d_period_ms:p C:u T:u S:u t0_ms:q tick_ms:u miss_ticks:u event_mask:u d_state:p d_kind:p "
                  "d_events:p event_cap:u d_event_count:p d_work:p",
    "jb_receive": "d_packets:p d_sizes:p d_radio:p d_arrival:p C:u T:u S:u pkt_stride:u n:u delay_frames:u d_state:p d_ring:p d_payload_out:p "
                  "d_len_out:p d_info_out:p d_tick_flags:p d_pkt_status:p",
    "jb_receive_adaptive": "d_packets:p d_sizes:p d_radio:p d_arrival:p C:u T:u S:u pkt_stride:u n:u cfg:cfg d_state:p d_ring:p d_adapt:p "
                           "d_payload_out:p d_len_out:p d_info_out:p d_tick_flags:p d_pkt_status:p d_delay_out:p",
    "plc_conceal": "d_tick_flags:p d_payload:p d_codec:p d_pcm:p d_len:p C:u T:u n:u d_state:p d_out:p d_len_out:p d_stats:p",
}
SIG = {e: [tuple(f.split(":")) for f in s.split()] for e, s in SIG.items()}
SYMBOL = {e: "igdsp_" + e for e in SIG}
SYMBOL["tx_copy"] = "igdsp_internal_tx_copy"              # the one entry here that include/igdsp.h does not declare
WIN_FIELDS = ("gate_mode", "probe_alarm", "d_hold", "d_gate", "d_probe", "d_work")      # igdsp_window, in order
CFG_FIELDS = ("min_frames", "max_frames", "init_frames", "jitter_mult", "late_restart")  # igdsp_jb_adapt_cfg, in order

_WIN = {"win": 1, "win.gate_mode": 0, "win.probe_alarm": 0, "win.d_hold": "a", "win.d_gate": "0", "win.d_probe": "0", "win.d_work": "0"}
_JB = dict(d_packets="a", d_sizes="0", d_radio="a", d_arrival="0", C=4, T=2, S=1, pkt_stride=180, n=160, d_state="a", d_ring="a",
           d_payload_out="a", d_len_out="a", d_info_out="a", d_tick_flags="0", d_pkt_status="0")
_GROUP = dict(d_info="a", d_payload="a", d_codec="a", d_pcm="0", d_len="0", d_gain="0", d_group_ptr="a", d_members="a", n_members=8, C=8, G=2,
              F=2, n=160, d_state="a", d_sel="a", d_out="a", d_stats="a")
# a launchable call of every entry (for the group and jitter-buffer entries: the calls of the GPU argument tests)
BASE = {
    "decode_meter": dict(d_payload="a", d_codec="a", d_len="0", C=4, F=2, n=160, d_stats="a", d_pcm="0", d_agg="0", rank=0),
    "encode": dict(d_pcm="a", d_codec="a", C=4, F=2, n=160, d_out="a", variant=1),
    "roundtrip_peakhold": dict(d_payload="a", d_codec="a", C=4, F=2, n=160, d_out="a", d_stats="a", d_hold="a", d_gate="0", variant=1),
    "hold_update": dict(d_stats="a", C=4, F=2, n=160, d_hold="a", d_gate="0"),
    "depayload": dict(d_packets="a", d_sizes="0", d_radio="a", C=4, F=2, pkt_stride=180, n=160, d_payload_out="a", d_len_out="a", d_info_out="a"),
    "decode_meter_rtp": dict(d_slots="a", d_codec="a", C=64, F=1, d_stats="a", d_info="0", d_agg="0", rank=0),
    "decode_meter_packets": dict(d_packets="a", d_sizes="0", d_codec="a", C=64, F=1, pkt_stride=180, hdr_bytes=20, d_stats="a", d_info="0",
                                 d_agg="0", rank=0),
    "decode_meter_packets_mixed": dict(d_packets="a", d_sizes="0", d_codec="a", d_radio="a", C=64, F=1, pkt_stride=180, d_stats="a", d_info="0",
                                       d_agg="0", rank=0),
    "window_update": dict(d_stats="a", d_info="0", d_len="0", C=4, F=2, n=160, **_WIN),
    # the fused path: C % 64 == 0 and a window with d_work
    "decode_meter_window": dict(layout=1, d_packets="a", d_sizes="0", d_codec="a", d_radio="0", C=64, F=1, pkt_stride=180, hdr_bytes=20,
                                d_stats="a", d_info="0", d_agg="0", rank=0, **{**_WIN, "win.d_work": "a"}),
    "wav_expand": dict(d_payload="a", C=4, F=2, n=160, rate=8000, d_files="a", file_stride=684),
    "tx_packetize": dict(d_pcm="a", d_g711="0", d_ctl="0", C=4, F=2, n=160, t0_ms=0, frame_ms=20, d_state="a", d_last_payload="a", d_packets="a",
                         pkt_stride=180, d_sizes="a", d_info="a", variant=1),
    "tx_copy": dict(d_pcm="a", d_g711="0", C=4, F=2, n=160, d_packets="a", pkt_stride=180),
    "g726_reorder": dict(d_in="a", d_out="a", n_bytes=30, mode=2),
    "conf_mix": dict(d_payload="a", d_codec="a", d_pcm="0", d_len="0", d_gain="a", d_port_ptr="a", d_members="a", n_members=8, C=8, P=2, F=2,
                     n=160, d_out="a", d_stats="a"),
    "bss_select": dict(_GROUP, d_mute="0", vote_frames=0, d_words="a"),
    "ptt_arbitrate": dict(_GROUP, d_rxonly="0", release_frames=0, d_slots="a", d_tick="a", d_ctl_out="a"),
    "link_watch": dict(d_info="a", d_sizes="0", d_up="0", d_period_ms="0", C=8, T=2, S=1, t0_ms=0, tick_ms=20, miss_ticks=0, event_mask=0,
                       d_state="a", d_kind="0", d_events="a", event_cap=64, d_event_count="a", d_work="a"),
    "jb_receive": dict(_JB, delay_frames=3),
    "jb_receive_adaptive": dict(_JB, cfg=0, d_adapt="a", d_delay_out="0",
                                **{"cfg.min_frames": 1, "cfg.max_frames": 12, "cfg.init_frames": 3, "cfg.jitter_mult": 4, "cfg.late_restart": 3}),
    "plc_conceal": dict(d_tick_flags="a", d_payload="a", d_codec="a", d_pcm="0", d_len="0", C=4, T=2, n=160, d_state="a", d_out="a",
                        d_len_out="0", d_stats="0"),
}

CASES = []


def _rows(entry, rows):
    CASES.extend((entry, kv, rc, run) for kv, rc, run in rows)


def _cfg(mn, mx, init, mult, late):
    return {"cfg": 1, "cfg.min_frames": mn, "cfg.max_frames": mx, "cfg.init_frames": init, "cfg.jitter_mult": mult, "cfg.late_restart": late}


BIG = dict(C=1 << 31, F=2)                                  # C * F = 2^32: past the 32-bit frame index, and a multiple of 64
RUN, NOTHING, BAD, RANGE = (0, 1), (0, 0), (EINVAL, 0), (ERANGE, 0)

_rows("decode_meter", [
    ({}, *RUN),
    (dict(C=0), *NOTHING), (dict(F=0), *NOTHING), (dict(C=0, d_payload="0", d_codec="0", d_stats="0", n=0, rank=8), *NOTHING),
    (dict(d_payload="0"), *BAD), (dict(d_codec="0"), *BAD), (dict(d_stats="0"), *BAD),
    (dict(d_len="a+1", d_pcm="a+1", d_agg="a+1"), *RUN),                                 # optional buffers: no rule
    (dict(n=0), *BAD), (dict(n=1), *RUN), (dict(n=256), *RUN), (dict(n=257), *BAD),
    (dict(C=0xFFFFFFDF, F=1), *RUN), (dict(C=0xFFFFFFE0, F=1), *RANGE), (BIG, *RANGE),
    (dict(rank=7), *RUN), (dict(rank=8), *BAD),
    (dict(BIG, rank=8), *RANGE), (dict(BIG, n=0), *BAD), (dict(BIG, d_stats="0"), *BAD),   # which code wins
])
_rows("encode", [
    ({}, *RUN), (dict(C=0), *NOTHING), (dict(F=0, d_pcm="0", variant=7, n=0), *NOTHING),
    (dict(d_pcm="0"), *BAD), (dict(d_codec="0"), *BAD), (dict(d_out="0"), *BAD),
    (dict(variant=0), *RUN), (dict(variant=2), *BAD), (dict(variant=-1), *BAD),
    (dict(n=0), *BAD), (dict(n=256), *RUN), (dict(n=257), *BAD),
    (BIG, *RANGE), (dict(BIG, variant=2), *BAD), (dict(BIG, n=0), *BAD),
    (dict(d_pcm="a+1", d_out="a+1"), *RUN),                                               # the route takes any alignment
])
_rows("roundtrip_peakhold", [
    ({}, *RUN), (dict(C=0), *NOTHING), (dict(F=0, d_hold="a+4", variant=9), *NOTHING),
    (dict(d_payload="0"), *BAD), (dict(d_codec="0"), *BAD), (dict(d_out="0"), *BAD), (dict(d_stats="0"), *BAD), (dict(d_hold="0"), *BAD),
    (dict(variant=0), *RUN), (dict(variant=2), *BAD),
    (dict(n=0), *BAD), (dict(n=256), *RUN), (dict(n=257), *BAD),
    (dict(d_stats="a+4"), *BAD), (dict(d_stats="a+8"), *RUN), (dict(d_hold="a+4"), *BAD), (dict(d_hold="a+8"), *RUN),
    (BIG, *RANGE), (dict(BIG, d_stats="a+4"), *RANGE), (dict(BIG, variant=2), *BAD),
])
_rows("hold_update", [
    ({}, *RUN), (dict(C=0), *NOTHING), (dict(F=0, d_stats="0", n=0), *NOTHING),
    (dict(d_stats="0"), *BAD), (dict(d_hold="0"), *BAD),
    (dict(n=0), *BAD), (dict(n=256), *RUN), (dict(n=257), *BAD),
    (BIG, *RANGE), (dict(BIG, d_hold="0"), *BAD),
])
_rows("depayload", [
    ({}, *RUN), (dict(C=0), *NOTHING), (dict(F=0, d_packets="0", pkt_stride=0), *NOTHING),
    (dict(d_packets="0"), *BAD), (dict(d_radio="0"), *BAD), (dict(d_payload_out="0"), *BAD), (dict(d_len_out="0"), *BAD),
    (dict(d_info_out="0"), *BAD),
    (dict(n=0), *BAD), (dict(n=256), *RUN), (dict(n=257), *BAD),
    (dict(pkt_stride=16), *BAD), (dict(pkt_stride=20), *RUN), (dict(pkt_stride=182), *BAD), (dict(pkt_stride=2048), *RUN),
    (dict(pkt_stride=2052), *BAD),
    (dict(d_packets="a+2"), *BAD), (dict(d_packets="a+4"), *RUN),
    (BIG, *RANGE), (dict(BIG, pkt_stride=182), *RANGE), (dict(BIG, d_radio="0"), *BAD),
])
_rows("decode_meter_rtp", [
    ({}, *RUN), (dict(C=0), *NOTHING), (dict(F=0, d_slots="0", rank=8), *NOTHING),
    (dict(d_slots="0"), *BAD), (dict(d_codec="0"), *BAD), (dict(d_stats="0"), *BAD),
    (dict(rank=7), *RUN), (dict(rank=8), *BAD),
    (dict(C=33), *BAD), (dict(C=32, F=2), *RUN),
    (dict(d_slots="a+8"), *BAD), (dict(d_stats="a+8"), *BAD), (dict(d_info="a+4"), *BAD), (dict(d_info="a+8"), *RUN),
    (BIG, *RANGE), (dict(BIG, d_slots="a+8"), *RANGE), (dict(BIG, rank=8), *BAD),
])
_rows("decode_meter_packets", [
    ({}, *RUN), (dict(C=0), *NOTHING), (dict(F=0, d_packets="0", hdr_bytes=0), *NOTHING),
    (dict(d_packets="0"), *BAD), (dict(d_codec="0"), *BAD), (dict(d_stats="0"), *BAD),
    (dict(rank=7), *RUN), (dict(rank=8), *BAD),
    (dict(hdr_bytes=16), *BAD), (dict(hdr_bytes=12), *RUN),
    (dict(hdr_bytes=12, pkt_stride=172), *RUN), (dict(hdr_bytes=12, pkt_stride=168), *BAD),      # the floor is hdr + 160
    (dict(pkt_stride=176), *BAD), (dict(pkt_stride=182), *BAD), (dict(pkt_stride=2048), *RUN), (dict(pkt_stride=2052), *BAD),
    (dict(C=A24, pkt_stride=1020), *RUN), (dict(C=A24, pkt_stride=1024), *BAD),                  # dword offsets stay 32-bit
    (dict(C=33), *BAD), (dict(C=32, F=2), *RUN),
    (dict(d_packets="a+2"), *BAD), (dict(d_packets="a+4"), *RUN), (dict(d_stats="a+8"), *BAD), (dict(d_info="a+4"), *BAD),
    (dict(d_info="a+8"), *RUN), (dict(d_sizes="a+1"), *BAD), (dict(d_sizes="a+2"), *RUN),
    (BIG, *RANGE), (dict(BIG, hdr_bytes=16), *BAD), (dict(BIG, pkt_stride=182), *RANGE), (dict(BIG, d_stats="a+8"), *RANGE),
])
_rows("decode_meter_packets_mixed", [
    ({}, *RUN), (dict(C=0), *NOTHING), (dict(F=0, d_radio="0", pkt_stride=0), *NOTHING),
    (dict(d_packets="0"), *BAD), (dict(d_codec="0"), *BAD), (dict(d_radio="0"), *BAD), (dict(d_stats="0"), *BAD),
    (dict(rank=7), *RUN), (dict(rank=8), *BAD),
    (dict(pkt_stride=176), *BAD), (dict(pkt_stride=182), *BAD), (dict(pkt_stride=2048), *RUN), (dict(pkt_stride=2052), *BAD),
    (dict(C=A24, pkt_stride=1020), *RUN), (dict(C=A24, pkt_stride=1024), *BAD),
    (dict(C=33), *BAD), (dict(C=32, F=2), *RUN),
    (dict(d_packets="a+2"), *BAD), (dict(d_packets="a+4"), *RUN), (dict(d_stats="a+8"), *BAD), (dict(d_info="a+4"), *BAD),
    (dict(d_info="a+8"), *RUN), (dict(d_sizes="a+1"), *BAD), (dict(d_sizes="a+2"), *RUN),
    (BIG, *RANGE), (dict(BIG, pkt_stride=176), *RANGE), (dict(BIG, rank=8), *BAD),
])
_BADWIN = [{"win": 0}, {"win.d_hold": "0"}, {"win.gate_mode": 4}, {"win.d_hold": "a+4"}, {"win.d_probe": "a+2"}, {"win.d_work": "a+8"}]
_rows("window_update", [
    ({}, *RUN), (dict(C=0), *NOTHING), (dict(F=0, d_stats="0", n=0), *NOTHING),
    *[(w, *BAD) for w in _BADWIN], *[(dict(w, C=0), *BAD) for w in _BADWIN],                  # the window is checked with nothing to do, too
    ({"win.gate_mode": 3}, *RUN), ({"win.d_hold": "a+8"}, *RUN), ({"win.d_probe": "a+4"}, *RUN), ({"win.d_work": "a"}, *RUN),
    ({"win.d_gate": "a+1"}, *RUN),
    (dict(d_stats="0"), *BAD), (dict(n=0), *BAD), (dict(n=256), *RUN), (dict(n=257), *BAD),
    (BIG, *RANGE), ({**BIG, "win.gate_mode": 4}, *BAD), (dict(BIG, d_stats="0"), *BAD),
])
_NOWORK = {"win.d_work": "0"}                                # the window of the GPU test: d_hold only
_rows("decode_meter_window", [
    # from tests/test_gpu_window.py
    (dict(_NOWORK, layout=3), *BAD), (dict(_NOWORK, hdr_bytes=16), *BAD), (dict(_NOWORK, layout=2, hdr_bytes=0), *BAD),
    (dict(_NOWORK, C=33), *BAD), (dict(_NOWORK, win=0), *BAD), ({**_NOWORK, "win.gate_mode": 7}, *BAD), ({**_NOWORK, "win.d_hold": "0"}, *BAD),
    ({**_NOWORK, "C": 96, "F": 2, "win.gate_mode": 1}, *BAD), (dict(_NOWORK, d_stats="0"), *BAD),
    # the rest
    ({}, *RUN), (dict(C=0), *NOTHING), (dict(F=0, d_packets="0", d_codec="0", hdr_bytes=0, rank=8), *NOTHING),
    (dict(layout=3), *BAD), (dict(C=0, layout=3), *BAD),
    *[(w, *BAD) for w in _BADWIN if "win.d_work" not in w], ({"win.d_work": "a+8"}, *BAD), *[(dict(w, C=0), *BAD) for w in _BADWIN],
    (dict(d_packets="0"), *BAD), (dict(d_codec="0"), *BAD), (dict(rank=7), *RUN), (dict(rank=8), *BAD),
    (dict(layout=2), *BAD), (dict(layout=2, d_radio="a"), *RUN),
    (dict(d_stats="0"), *RUN), (dict(d_stats="0", C=96, F=2, d_info="a"), *BAD),              # no records: only on the fused path
    (dict(hdr_bytes=16), *BAD), (dict(hdr_bytes=12), *RUN), (dict(hdr_bytes=12, pkt_stride=172), *RUN),
    (dict(hdr_bytes=12, pkt_stride=168), *BAD), (dict(pkt_stride=176), *BAD),
    (dict(layout=2, d_radio="a", pkt_stride=176), *BAD),                                      # MIXED: 180 whatever hdr_bytes says
    (dict(layout=2, d_radio="a", hdr_bytes=0), *RUN),
    (dict(pkt_stride=182), *BAD), (dict(pkt_stride=2048), *RUN), (dict(pkt_stride=2052), *BAD),
    (dict(C=A24, pkt_stride=1020), *RUN), (dict(C=A24, pkt_stride=1024), *BAD),
    (dict(d_packets="a+2"), *BAD), (dict(d_packets="a+4"), *RUN), (dict(d_sizes="a+1"), *BAD), (dict(d_sizes="a+2"), *RUN),
    (dict(layout=0), *RUN), (dict(layout=0, pkt_stride=0, hdr_bytes=0, d_sizes="a+1"), *RUN),  # SLOTS: no stride, header or sizes
    (dict(layout=0, d_packets="a+8"), *BAD),
    (dict(C=32, d_info="a"), *BAD), (dict(C=32, F=2, d_info="a"), *RUN),                      # C * F % 64
    (dict(d_stats="a+8"), *BAD), (dict(d_info="a+4"), *BAD), (dict(d_info="a+8"), *RUN),
    (dict(C=96, F=2), *BAD), (dict(C=96, F=2, d_info="a"), *RUN),                             # off the fused path the fold needs d_info
    (dict(_NOWORK), *BAD), (dict(_NOWORK, d_info="a"), *RUN),
    (BIG, *RANGE), (dict(BIG, hdr_bytes=16), *RANGE), (dict(BIG, pkt_stride=182), *RANGE),    # here hdr_bytes is behind the range check
    (dict(BIG, rank=8), *BAD), (dict(BIG, layout=2), *BAD), ({**BIG, "win.gate_mode": 4}, *BAD),
])
_rows("wav_expand", [
    ({}, *RUN), (dict(C=0), *NOTHING), (dict(F=0, d_files="0", file_stride=0, n=0), *NOTHING),
    (dict(d_payload="0"), *BAD), (dict(d_files="0"), *BAD),
    (dict(n=0), *BAD), (dict(n=256, file_stride=1 << 20), *RUN), (dict(n=257, file_stride=1 << 20), *BAD),
    (dict(file_stride=683), *BAD), (dict(file_stride=685), *RUN),
    (dict(C=1, F=(1 << 23) - 1, n=256, file_stride=1 << 40), *RUN), (dict(C=1, F=1 << 23, n=256, file_stride=1 << 40), *BAD),
    (BIG, *RANGE), (dict(BIG, file_stride=0), *RANGE), (dict(BIG, d_files="0"), *BAD),
])
_rows("tx_packetize", [
    ({}, *RUN), (dict(C=0), *NOTHING), (dict(F=0, d_pcm="0", d_state="0", pkt_stride=0), *NOTHING),
    (dict(d_g711="a"), *BAD), (dict(d_pcm="0"), *BAD), (dict(d_pcm="0", d_g711="a"), *RUN),
    (dict(d_state="0"), *BAD), (dict(d_last_payload="0"), *BAD), (dict(d_packets="0"), *BAD), (dict(d_sizes="0"), *BAD),
    (dict(d_info="0"), *BAD),
    (dict(variant=0), *RUN), (dict(variant=2), *BAD), (dict(variant=2, d_pcm="0", d_g711="a"), *RUN),   # the lineage matters for PCM only
    (dict(n=0), *BAD), (dict(n=256, pkt_stride=276), *RUN), (dict(n=257, pkt_stride=280), *BAD),
    (dict(pkt_stride=176), *BAD), (dict(pkt_stride=182), *BAD), (dict(pkt_stride=2048), *RUN), (dict(pkt_stride=2052), *BAD),
    (dict(n=256, pkt_stride=272), *BAD),                                                        # the floor is 20 + n
    (dict(d_packets="a+2"), *BAD), (dict(d_packets="a+4"), *RUN), (dict(d_state="a+4"), *BAD), (dict(d_state="a+8"), *RUN),
    (dict(d_info="a+2"), *BAD), (dict(d_info="a+4"), *RUN), (dict(d_sizes="a+1"), *BAD), (dict(d_sizes="a+2"), *RUN),
    (dict(d_pcm="a+1"), *BAD), (dict(d_pcm="a+2"), *RUN), (dict(d_pcm="0", d_g711="a+1"), *RUN),
    (dict(C=1, F=(1 << 23) - 1, n=256, pkt_stride=276), *RUN), (dict(C=1, F=1 << 23, n=256, pkt_stride=276), *RANGE),
    (dict(C=1, F=1 << 23, n=256, pkt_stride=278), *BAD),                                       # the stride is ahead of F * n
    (BIG, *RANGE), (dict(BIG, pkt_stride=182), *RANGE), (dict(BIG, variant=2), *BAD),
])
_rows("tx_copy", [
    ({}, *RUN), (dict(C=0), *NOTHING), (dict(F=0), *NOTHING),
    (dict(d_g711="a"), *BAD), (dict(d_pcm="0"), *BAD), (dict(d_pcm="0", d_g711="a"), *RUN),
    (dict(d_packets="0"), *BAD),
    (dict(n=0), *BAD), (dict(n=162), *BAD), (dict(n=256, pkt_stride=276), *RUN), (dict(n=260, pkt_stride=280), *BAD),
    (dict(pkt_stride=176), *BAD), (dict(pkt_stride=182), *BAD), (dict(pkt_stride=2052), *RUN),   # no upper bound here
    (dict(d_packets="a+2"), *BAD), (dict(d_packets="a+4"), *RUN), (dict(d_pcm="a+4"), *BAD), (dict(d_pcm="a+8"), *RUN),
    (dict(d_pcm="0", d_g711="a+2"), *BAD), (dict(d_pcm="0", d_g711="a+4"), *RUN),
    (dict(C=0, n=162), *BAD), (dict(F=0, d_packets="0"), *BAD), (dict(C=0, pkt_stride=176), *BAD),   # every clause with nothing to do, too
    (BIG, *RANGE), (dict(BIG, n=162), *BAD),
])
_rows("g726_reorder", [
    ({}, *RUN), (dict(n_bytes=0), *NOTHING), (dict(n_bytes=0, d_in="0", d_out="0"), *NOTHING),
    (dict(mode=0), *BAD), (dict(mode=1), *RUN), (dict(mode=4), *RUN), (dict(mode=5), *BAD), (dict(mode=-1), *BAD),
    (dict(n_bytes=0, mode=0), *BAD), (dict(n_bytes=0, mode=5), *BAD),                          # the mode is checked with nothing to do, too
    (dict(d_in="0"), *BAD), (dict(d_out="0"), *BAD),
    (dict(n_bytes=31), *BAD), (dict(n_bytes=33), *RUN), (dict(mode=4, n_bytes=31), *BAD), (dict(mode=4, n_bytes=35), *RUN),
    (dict(mode=1, n_bytes=31), *RUN), (dict(mode=3, n_bytes=31), *RUN), (dict(n_bytes=3 << 32), *RUN),
])
_rows("conf_mix", [
    # from tests/test_gpu_conf.py
    ({}, *RUN), (dict(d_pcm="a"), *BAD), (dict(d_payload="0"), *BAD), (dict(d_codec="0"), *BAD), (dict(d_out="0", d_stats="0"), *BAD),
    (dict(d_gain="0"), *BAD), (dict(d_port_ptr="0"), *BAD), (dict(d_members="0"), *BAD), (dict(n=0), *BAD), (dict(n=257), *BAD),
    (dict(d_out="a+1"), *BAD), (dict(d_stats="a+4"), *BAD), (dict(d_port_ptr="a+2"), *BAD), (dict(d_members="a+1"), *BAD),
    (dict(d_payload="0", d_codec="0", d_pcm="a+1"), *BAD), (dict(d_gain="a+1"), *BAD), (dict(d_len="a+1"), *BAD),
    (dict(C=0x10000, F=0x10000), *RANGE), (dict(P=0x10000, F=0x10000), *RANGE),
    (dict(P=0), *NOTHING), (dict(F=0), *NOTHING),
    (dict(P=0, d_payload="0", d_codec="0", d_gain="0", d_port_ptr="0", d_members="0", d_out="0", d_stats="0"), *NOTHING),
    (dict(d_members="0", n_members=0), *RUN), (dict(C=0), *RUN),
    # the rest
    (dict(d_payload="0", d_codec="0", d_pcm="a"), *RUN), (dict(d_out="0"), *RUN), (dict(d_stats="0"), *RUN),
    (dict(n=256), *RUN), (dict(d_out="a+2"), *RUN), (dict(d_stats="a+8"), *RUN), (dict(d_port_ptr="a+4"), *RUN),
    (dict(d_members="a+2"), *BAD), (dict(d_members="a+4"), *RUN), (dict(d_gain="a+2"), *RUN), (dict(d_len="a+2"), *RUN),
    (dict(d_payload="0", d_codec="0", d_pcm="a+2"), *RUN), (dict(d_payload="a+1", d_codec="a+1"), *RUN),
    (dict(C=0x10000, F=0x10000, d_out="a+1"), *RANGE), (dict(C=0x10000, F=0x10000, n=0), *BAD),
    (dict(C=0x10000, F=0x10000, d_gain="0"), *BAD),
])


def _group_rows(per_member, more):
    """the rows the vote and the arbiter share (per_member: d_words / d_slots)"""
    return [
        # from tests/test_gpu_bss.py and tests/test_gpu_ptt.py
        ({}, *RUN), (dict(d_payload="0", d_codec="0", d_pcm="a"), *RUN), (dict(d_payload="0", d_codec="0", d_out="0", d_stats="0"), *RUN),
        (dict({k: "0" for k in more}, d_sel="0", d_out="0", d_stats="0"), *RUN),
        (dict(G=0), *NOTHING), (dict(F=0), *NOTHING), (dict(G=0, d_info="0"), *NOTHING),
        (dict(d_info="0"), *BAD), (dict(d_group_ptr="0"), *BAD), (dict(d_state="0"), *BAD), (dict(d_members="0"), *BAD),
        ({per_member: "0"}, *BAD), ({"n_members": 0, "d_members": "0", per_member: "0"}, *RUN), (dict(n_members=A24 + 1), *BAD),
        (dict(d_pcm="a"), *BAD), (dict(d_codec="0"), *BAD), (dict(d_payload="0", d_codec="0"), *BAD),
        (dict(n=0), *BAD), (dict(n=257), *BAD),
        (dict(d_stats="a+4"), *BAD), (dict(d_out="a+1"), *BAD), (dict(d_sel="a+2"), *BAD), (dict(d_info="a+2"), *BAD),
        # the rest
        (dict(n_members=A24), *RUN), (dict(n=256), *RUN),
        (dict(d_payload="0", d_codec="0", d_stats="0"), *BAD), (dict(d_payload="0", d_codec="0", d_out="0"), *BAD),
        (dict(d_len="a+1"), *BAD), (dict(d_gain="a+1"), *BAD), (dict(d_payload="0", d_codec="0", d_pcm="a+1"), *BAD),
        (dict(d_group_ptr="a+2"), *BAD), (dict(d_members="a+2"), *BAD), (dict(d_state="a+2"), *BAD), ({per_member: "a+2"}, *BAD),
        ({"d_len": "a+2", "d_gain": "a+2", "d_out": "a+2", "d_stats": "a+8", "d_sel": "a+4", "d_info": "a+4", "d_group_ptr": "a+4",
          "d_members": "a+4", "d_state": "a+4", per_member: "a+4"}, *RUN),
        (dict(C=0x10000, F=0x10000), *RANGE), (dict(G=0x10000, F=0x10000), *RANGE),
        (dict(C=0x10000, F=0x10000, d_out="a+1"), *RANGE), (dict(C=0x10000, F=0x10000, d_pcm="a"), *BAD),
        (dict(C=0x10000, F=0x10000, n=0), *BAD),
    ]


_rows("bss_select", _group_rows("d_words", ()) + [
    (dict(d_mute="a+1"), *RUN),
    (dict(G=0, n=0), *NOTHING), (dict(F=0, n_members=A24 + 1), *NOTHING),                      # the vote looks at nothing when there is nothing to do
])
_rows("ptt_arbitrate", _group_rows("d_slots", ("d_tick", "d_ctl_out")) + [
    # from tests/test_gpu_ptt.py
    (dict(release_frames=1), *RUN), (dict(release_frames=255), *RUN), (dict(release_frames=256), *BAD),
    (dict(G=0, n=0), *BAD), (dict(F=0, n=257), *BAD), (dict(F=0, n_members=A24 + 1), *BAD),     # always checked
    (dict(d_tick="a+2"), *BAD), (dict(d_ctl_out="a+1"), *RUN),
    # the rest
    (dict(G=0, release_frames=256), *BAD), (dict(F=0, n_members=A24), *NOTHING), (dict(d_tick="a+4"), *RUN), (dict(d_rxonly="a+1"), *RUN),
    (dict(C=0x10000, F=0x10000, release_frames=256), *BAD),
])
_NOLIST = dict(d_event_count="0", d_work="0")
_rows("link_watch", [
    # from tests/test_gpu_link.py
    ({}, *RUN), (dict(S=0), *BAD), (dict(S=9), *BAD), (dict(S=8), *RUN), (dict(tick_ms=0), *BAD), (dict(tick_ms=1), *RUN),
    (dict(miss_ticks=65536), *BAD), (dict(miss_ticks=65535), *RUN), (dict(miss_ticks=1), *RUN),
    (dict(d_events="0"), *BAD), (dict(d_events="0", event_cap=0), *RUN),
    (dict(d_work="0"), *BAD), (dict(d_work="a+8"), *BAD), (_NOLIST, *RUN), (dict(_NOLIST, d_events="0", event_cap=0), *RUN),
    (dict(d_info="0"), *BAD), (dict(d_state="0"), *BAD),
    (dict(d_info="a+2"), *BAD), (dict(d_state="a+4"), *BAD), (dict(d_events="a+2"), *BAD), (dict(d_event_count="a+2"), *BAD),
    (dict(d_sizes="a+1"), *BAD), (dict(d_period_ms="a+1"), *BAD),
    (dict(C=0, S=0), *BAD), (dict(T=0, tick_ms=0), *BAD),
    (dict(C=0, d_info="0", d_state="0"), 0, 1), (dict(T=0, d_info="0", d_state="0"), 0, 1),    # a list and no work: the counts are written
    (dict(C=1 << 31, T=2), *RANGE),
    # the rest
    (dict(_NOLIST, C=0), *NOTHING), (dict(_NOLIST, T=0, d_info="0", d_state="0"), *NOTHING),
    (dict(_NOLIST, C=0, miss_ticks=65536), *BAD), (dict(_NOLIST, C=0, d_events="0"), *BAD), (dict(_NOLIST, T=0, d_state="a+4"), *BAD),
    (dict(C=0, d_work="0"), *BAD), (dict(C=0, d_work="a+8"), *BAD),
    (dict(d_info="a+4", d_state="a+8", d_events="a+4", d_event_count="a+4", d_sizes="a+2", d_period_ms="a+2", d_up="a+1", d_kind="a+1"), *RUN),
    (dict(C=1 << 29, T=1, S=7), *RUN), (dict(C=1 << 29, T=1, S=8), *RANGE),
    (dict(C=1 << 31, T=2, S=0), *BAD), (dict(C=1 << 31, T=2, d_info="0"), *BAD), (dict(C=1 << 31, T=2, d_state="a+4"), *BAD),
])


def _jb_rows(extra_null):
    """the rows the two jitter-buffer entries share"""
    return [
        # from tests/test_gpu_jb.py and tests/test_gpu_jb_adapt.py
        ({}, *RUN), (dict(pkt_stride=182), *BAD), (dict(pkt_stride=16), *BAD), (dict(pkt_stride=2052), *BAD), (dict(S=0), *BAD), (dict(S=9), *BAD),
        (dict(n=0), *BAD), (dict(n=257), *BAD),
        *[({k: "0"}, *BAD) for k in ("d_packets", "d_radio", "d_state", "d_ring", "d_payload_out", "d_len_out", "d_info_out")],
        (dict(d_ring="a+4"), *BAD), (dict(d_info_out="a+4"), *BAD), (dict(d_len_out="a+1"), *BAD),
        (dict({k: "0" for k in extra_null}, C=0, d_packets="0"), *NOTHING), (dict(T=0), *NOTHING),
        # the rest
        (dict(S=8), *RUN), (dict(n=256), *RUN), (dict(pkt_stride=20), *RUN), (dict(pkt_stride=2048), *RUN),
        (dict(d_ring="a+8"), *BAD), (dict(d_info_out="a+8"), *RUN), (dict(d_len_out="a+2"), *RUN), (dict(d_sizes="a+1"), *BAD),
        (dict(d_sizes="a+2"), *RUN), (dict(d_packets="a+2"), *BAD), (dict(d_packets="a+4"), *RUN), (dict(d_arrival="a+2"), *BAD),
        (dict(d_arrival="a+4"), *RUN), (dict(d_state="a+2"), *BAD), (dict(d_state="a+4"), *RUN),
        (dict(d_radio="a+1", d_payload_out="a+1", d_tick_flags="a+1", d_pkt_status="a+1"), *RUN),
        (dict(C=1 << 31, T=2), *RANGE), (dict(C=1 << 29, T=1, S=7), *RUN), (dict(C=1 << 29, T=1, S=8), *RANGE),
        (dict(C=1 << 31, T=2, pkt_stride=182), *BAD), (dict(C=1 << 31, T=2, S=9), *BAD),       # S, delay and stride are ahead of the range
        (dict(C=1 << 31, T=2, d_ring="a+8"), *RANGE), (dict(C=1 << 31, T=2, n=0), *BAD),
    ]


_rows("jb_receive", _jb_rows(()) + [
    (dict(delay_frames=16), *BAD),                                                             # from tests/test_gpu_jb.py
    (dict(delay_frames=15), *RUN), (dict(delay_frames=0), *RUN), (dict(C=0, delay_frames=16, S=0), *NOTHING),
    (dict(C=1 << 31, T=2, delay_frames=16), *BAD),
])
_rows("jb_receive_adaptive", _jb_rows(("d_adapt",)) + [
    # from tests/test_gpu_jb_adapt.py
    (_cfg(0, 15, 0, 16, 255), *RUN), (dict(d_adapt="a+4"), *RUN),
    (_cfg(2, 12, 1, 4, 3), *BAD), (_cfg(1, 12, 13, 4, 3), *BAD), (_cfg(1, 16, 3, 4, 3), *BAD), (_cfg(5, 4, 4, 4, 3), *BAD),
    (_cfg(1, 12, 3, 17, 3), *BAD),
    (dict(d_adapt="0"), *BAD), (dict(d_adapt="a+2"), *BAD), (dict(d_adapt="a+1"), *BAD),
    (dict(_cfg(9, 9, 1, 99, 0), C=0, d_packets="0", d_adapt="0"), *NOTHING),
    # the rest
    (_cfg(1, 12, 3, 4, 3), *RUN), (_cfg(3, 3, 3, 0, 0), *RUN), (dict(d_delay_out="a+1"), *RUN),
    (dict(_cfg(1, 16, 3, 4, 3), C=1 << 31, T=2), *BAD),
])
_rows("plc_conceal", [
    # from tests/test_gpu_plc.py
    ({}, *RUN), (dict(d_tick_flags="0"), *BAD), (dict(d_state="0"), *BAD), (dict(d_out="0"), *BAD),
    (dict(d_pcm="a"), *BAD), (dict(d_payload="0"), *BAD), (dict(d_codec="0"), *BAD), (dict(n=0), *BAD), (dict(n=257), *BAD),
    (dict(d_payload="0", d_codec="0", d_pcm="a"), *RUN), (dict(C=0, d_tick_flags="0"), *NOTHING), (dict(T=0, n=0), *NOTHING),
    # the rest
    (dict(n=256), *RUN), (dict(d_payload="0", d_codec="0", d_pcm="a+1"), *BAD), (dict(d_payload="0", d_codec="0", d_pcm="a+2"), *RUN),
    (dict(d_len="a+1"), *BAD), (dict(d_len="a+2"), *RUN), (dict(d_out="a+1"), *BAD), (dict(d_out="a+2"), *RUN),
    (dict(d_len_out="a+1"), *BAD), (dict(d_len_out="a+2"), *RUN), (dict(d_state="a+2"), *BAD), (dict(d_state="a+4"), *RUN),
    (dict(d_stats="a+4"), *BAD), (dict(d_stats="a+8"), *RUN), (dict(d_tick_flags="a+1", d_payload="a+1", d_codec="a+1"), *RUN),
    (dict(C=1 << 31, T=2), *RANGE), (dict(C=1 << 31, T=2, d_out="a+1"), *RANGE), (dict(C=1 << 31, T=2, d_pcm="a"), *BAD),
])


def full(entry, kv):
    """the whole argument dict of a row: the entry's BASE with the row's values over it"""
    unknown = set(kv) - set(BASE[entry])
    assert not unknown, (entry, unknown)
    return {**BASE[entry], **kv}


def line(entry, kv):
    """the driver's input line of a row"""
    return entry + "".join(f" {k}={v}" for k, v in full(entry, kv).items())


def case_id(case):
    entry, kv, rc, run = case
    return entry + "[" + ",".join(f"{k}={v}" for k, v in kv.items()) + "]"
