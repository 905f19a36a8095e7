"""-m "not gpu": the staged ED-137 send path without a device — igdsp_tx_packet's layout and the constants, header against binding;
NULL / bad-argument returns; and hand-derived transport_send_rtp sequences through tests/tx_stage_model.py (a setter between two
frames, the keep-alive boundary at exactly keepalive_ms, now going backwards, a shorter n after a longer gated frame)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import tx_stage_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "igdsp.h")


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


def test_constants_header_against_binding():
    hdr = open(HDR).read()
    for name, val in (("IGDSP_TX_MAX_N", capi.TX_MAX_N), ("IGDSP_STAGE_DEPTH", capi.STAGE_DEPTH)):
        m = re.search(rf"#define\s+{name}\s+(\d+)", hdr)
        assert m and int(m.group(1)) == val, name
    assert capi.TX_MAX_N + 20 == capi.TX_SLOT == capi.MAX_PAYLOAD       # send_pkt_buff[256]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_tx_packet_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "igdsp.h"\n'
                   "int main(void){printf(\"%zu %zu %zu %zu %zu %zu %zu\\n\", sizeof(igdsp_tx_packet), offsetof(igdsp_tx_packet, pkt),"
                   " offsetof(igdsp_tx_packet, call_id), offsetof(igdsp_tx_packet, ed137), offsetof(igdsp_tx_packet, size),"
                   " offsetof(igdsp_tx_packet, flags), offsetof(igdsp_tx_packet, level)); return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt = capi.TX_PACKET
    assert got == [dt.itemsize] + [dt.fields[f][1] for f in ("pkt", "call_id", "ed137", "size", "flags", "level")]


def test_null_and_bad_arguments_without_a_device(lib):
    pkt = sm.stream_packet(8, 1, 2, 3, bytes(160))
    assert lib.igdsp_tx_open(None, 1, b"Tx", 0, 200, 0) == -22
    assert lib.igdsp_tx_close(None, 1) == -22
    assert lib.igdsp_on_tx_frame(None, 1, pkt, len(pkt), 0) == -22
    assert lib.igdsp_tx_flush(None, None) == -22
    assert lib.igdsp_tx_results(None, None, None) == -22
    assert lib.igdsp_tx_get_chan(None, 1, None) == -22
    assert lib.igdsp_tx_counts(None, 1, None, None) == -22
    for fn, args in ((lib.igdsp_tx_set_ptt, (1, 1, 0, 0)), (lib.igdsp_tx_set_sql, (1, 1, 0, -1)), (lib.igdsp_tx_set_ptt_id, (1, 3)),
                     (lib.igdsp_tx_set_slave, (1, 1, 0)), (lib.igdsp_tx_set_recorder, (1, 1)), (lib.igdsp_tx_set_calltype, (1, b"Rx"))):
        assert fn(None, *args) == -22


# ---- hand-derived sequences through the model ----
def _leg(calltype="Tx", call_in=False, keepalive=200, now=1000):
    return sm.Legs(1), (calltype, call_in, keepalive, now)


def _one(legs, pkt, now, assign=None):
    out = legs.run([(0, pkt, now, assign)])
    return out[0]


def test_setter_between_two_frames():
    legs = sm.Legs(1)
    legs.open(0, "Tx", False, 200, 1000)
    pay1, pay2 = bytes(range(160)), bytes((i * 7) & 0xFF for i in range(160))
    # frame 1: ptt / sql off -> keep-alive, 20 bytes, pt 123; first packet: marker; debounce changing -> 0x13100, !ptt -> bit 22
    b, inf = _one(legs, sm.stream_packet(8, 0x1234, 0x01020304, 0xAABBCCDD, pay1), 1000)
    assert inf["size"] == 20 and inf["ed137"] == 0x00413100
    assert inf["flags"] == capi.TX_SENT | capi.TX_MARKER | capi.TX_KEEPALIVE_PT
    assert b == bytes([0x90, 0x80 | 123, 0x12, 0x34, 1, 2, 3, 4, 0xAA, 0xBB, 0xCC, 0xDD, 0x01, 0x67, 0x00, 0x01, 0x00, 0x41, 0x31, 0x00])
    # setAdapterPtt(true, 2, 0) between the frames: frame 2 is gated, 20 + n with the stream's pt, ptt priority 2 at bit 29
    b, inf = _one(legs, sm.stream_packet(8, 0x1235, 0x01020304 + 160, 0xAABBCCDD, pay2), 1020, sm.setter("ptt", True, 2, 0))
    assert inf["size"] == 180 and inf["ed137"] == 0x40013100
    assert inf["flags"] == capi.TX_SENT | capi.TX_LEVEL_VALID
    assert b[:2] == bytes([0x90, 8]) and b[2:4] == bytes([0x12, 0x35]) and b[20:] == pay2
    st = legs.st[0]
    assert (st["ptt"], st["pttpriority"], st["seq"], st["ts"], st["packet_cnt"], st["slave_count"]) == (1, 2, 0x1236, 0x01020304 + 320, 2, 2)
    # the level: the first n stream bytes as signed char, C division
    assert inf["level"] == sm.tm.stream_level(pay2, sm.stream_packet(8, 0x1235, 0x01020304 + 160, 0xAABBCCDD, b"")[:12], 160)


def test_keepalive_boundary_and_now_going_backwards():
    legs = sm.Legs(1)
    legs.open(0, "Tx", False, 200, 1000)
    legs.st["first_r2s"] = 0                                # past the first 30 packets
    legs.st["packet_cnt"] = 30
    pkt = lambda s: sm.stream_packet(0, s, 0, 7, bytes(160))
    sizes = [int(_one(legs, pkt(i), now)[1]["size"]) for i, now in enumerate([1199, 1200, 1399, 1400])]
    assert sizes == [0, 20, 0, 20]                          # (now - r2sSendtime) < keepAlivePeroid -> not sent; == the period -> sent
    assert legs.st["r2s_send_ms"][0] == 1400
    # now < r2sSendtime: the quint64 difference wraps to >= the period -> sent, r2sSendtime = now
    _, inf = _one(legs, pkt(4), 1399)
    assert inf["size"] == 20 and legs.st["r2s_send_ms"][0] == 1399
    _, inf = _one(legs, pkt(5), 1400)
    assert inf["size"] == 0


def test_shorter_gated_frame_leaves_old_bytes_in_a_stale_packet():
    legs = sm.Legs(1)
    legs.open(0, "Tx", False, 200, 1000)
    a, b = bytes([0x11] * 160), bytes([0x22] * 80)
    _, inf = _one(legs, sm.stream_packet(8, 1, 0, 9, a), 1000, sm.setter("ptt", True, 0, 0))
    assert inf["size"] == 180
    _, inf = _one(legs, sm.stream_packet(8, 2, 160, 9, b), 1020)
    assert inf["size"] == 100
    # ptt off, sql on, callIn false: not gated, yet 20 + n -> the send buffer's stale bytes: B over the first 80, A past them
    assign = dict(sm.setter("ptt", False, 0, 0), **sm.setter("sql", True, 0, -1))
    pk, inf = _one(legs, sm.stream_packet(8, 3, 240, 9, bytes([0x33] * 160)), 1040, assign)
    assert inf["size"] == 180 and inf["flags"] & capi.TX_STALE_PAYLOAD
    assert pk[20:] == b + a[80:]
    assert bytes(legs.buf[0, :160]) == b + a[80:] and not legs.buf[0, 160:].any()
