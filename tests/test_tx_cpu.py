"""-m "not gpu": the ED-137 TX packetizer's host side (calltype predicates, transport_adapter_create defaults, struct layouts) and
tests/tx_model.py against cases derived by hand from transport_send_rtp (TransportAdapter.cpp:635-874), one step each."""
import ctypes
import os
import re

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import tx_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 160


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


@pytest.mark.parametrize("ct,bits", [("Idle", 1), ("Rx", 2), ("Rxonly", 2), ("TRx", 4), ("Tx", 4), ("RxTx", 4), ("", 0), ("idle", 0),
                                     ("IdleRxonly", 3), ("Rx ", 0)])
def test_calltype_predicates(lib, ct, bits):
    assert capi.tx_calltype_bits(ct) == tm.calltype_bits(ct) == bits


def test_chan_init_defaults(lib):
    h = capi.tx_chan_init("TRx", True, 8, 0xDEADBEEF, 65535, 4000, 200, 1_700_000_000_123)
    ref = tm.chan_init("TRx", True, 8, 0xDEADBEEF, 65535, 4000, 200, 1_700_000_000_123)
    assert h.tobytes() == ref.tobytes()
    assert (h["first_r2s"], h["packet_cnt"], h["ptt"], h["sql"], h["call_recorder"], h["tx_slave"], h["rx_slave"]) == (1, 0, 0, 0, 0, 0, 0)
    assert h["r2s_send_ms"] == 1_700_000_000_123 and h["call_in"] == 1 and h["calltype"] == capi.TX_CT_TX
    assert lib.igdsp_tx_chan_init(None, b"Tx", 0, 0, 0, 0, 0, 200, 0) == -22
    h2 = np.zeros((), capi.TX_CHAN)
    assert lib.igdsp_tx_chan_init(h2.ctypes.data_as(ctypes.c_void_p), b"Tx", 0, 128, 0, 0, 0, 200, 0) == -22


def test_layouts_match_header(lib):
    assert capi.TX_CHAN.itemsize == 64 and capi.TX_INFO.itemsize == 8
    off = {k: capi.TX_CHAN.fields[k][1] for k in capi.TX_CHAN.names}
    assert (off["r2s_send_ms"], off["ts"], off["seq"], off["slave_count"], off["ptt"], off["pttid"], off["tx_run"], off["level"]) == (0, 8, 24, 32, 36, 40, 44, 46)
    hdr = open(os.path.join(ROOT, "include", "igdsp.h")).read()
    body = re.search(r"typedef struct igdsp_tx_chan \{(.*?)\} igdsp_tx_chan;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
    assert fields == list(capi.TX_CHAN.names)
    for name, val in (("IGDSP_TX_SENT", capi.TX_SENT), ("IGDSP_TX_LEVEL_VALID", capi.TX_LEVEL_VALID), ("IGDSP_TX_CTL_SET", capi.TX_CTL_SET),
                      ("IGDSP_TX_CT_TX", capi.TX_CT_TX), ("IGDSP_TX_STALE_PAYLOAD", capi.TX_STALE_PAYLOAD)):
        m = re.search(rf"#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)", hdr)
        assert m and int(m.group(1), 0) == val, name


def test_null_ctx_rejected_without_gpu(lib):
    assert lib.igdsp_tx_packetize(None, None, None, None, 1, 1, 160, 0, 20, None, None, None, 180, None, None, 1, None) == -22


# ---------------------------------------------------------------- model cases, one reference step each
def run(ct, call_in, F, ctl=None, g711=None, setup=None, t0=0, frame_ms=20, n=N, **kw):
    st = np.zeros((1,), capi.TX_CHAN)
    st[0] = tm.chan_init(ct, call_in, 8, 0x01020304, 100, 1000, kw.get("period", 200), kw.get("r2s", t0))
    if setup:
        setup(st)
    last = np.zeros((1, n), np.uint8)
    g = g711 if g711 is not None else (np.arange(F * n, dtype=np.int64).reshape(F, 1, n) % 251).astype(np.uint8)
    pk = np.full((F, 1, 20 + n + 4), 0xA5, np.uint8)
    c = None if ctl is None else np.asarray(ctl, np.uint8).reshape(F, 1)
    sizes, info = tm.packetize(st, last, g, pk, c, t0, frame_ms)
    return st, last, g, pk, sizes[:, 0], info[:, 0]


def S(ptt, sql):
    return capi.TX_CTL_SET | (ptt and 1) | (sql and 2)


@pytest.mark.parametrize("ct,call_in,ptt,sql,rec,size,pt", [
    # (:804) !ptt && !sql -> keep-alive header only
    ("Tx", False, 0, 0, 0, 20, 123), ("Rx", True, 0, 0, 0, 20, 123), ("Foo", False, 0, 0, 0, 20, 123),
    # (:811) Rx leg without squelch -> keep-alive
    ("Rx", False, 1, 0, 0, 20, 123), ("Rxonly", True, 1, 0, 0, 20, 123),
    # Rx leg with squelch: full size; pt 123 when !callIn (:795), the codec pt when callIn
    ("Rx", False, 0, 1, 0, 180, 123), ("Rx", True, 0, 1, 0, 180, 8),
    # (:821) Tx leg, ptt, callIn: full only with callRecorder or sql
    ("Tx", True, 1, 0, 0, 20, 123), ("Tx", True, 1, 0, 1, 180, 8), ("Tx", True, 1, 1, 0, 180, 8), ("TRx", True, 1, 0, 0, 20, 123),
    # else -> full
    ("Tx", False, 1, 0, 0, 180, 8), ("Tx", False, 0, 1, 0, 180, 8), ("Foo", True, 1, 0, 0, 180, 8), ("Foo", False, 0, 1, 0, 180, 8),
])
def test_size_pt_ladder(ct, call_in, ptt, sql, rec, size, pt):
    def setup(st):
        st["call_recorder"] = rec
    st, last, g, pk, sizes, info = run(ct, call_in, 1, ctl=[S(ptt, sql)], setup=setup)
    assert sizes[0] == size and info["size"][0] == size
    assert pk[0, 0, 1] & 0x7F == pt
    assert bool(info["flags"][0] & capi.TX_KEEPALIVE_PT) == (pt == 123)
    assert bool(info["flags"][0] & capi.TX_LEVEL_VALID) == (pt != 123)
    assert np.all(pk[0, 0, size:] == 0xA5)                     # nothing past size


def test_debounce_sequence():
    # steady 11 first, then setTxRxSlaveEnable(0, 0): the next five SENT frames carry 0x13100, then 0 (idle leg: | 1 << 22)
    def setup(st):
        st["tx_slave"] = st["rx_slave"] = st["tx_slave_changed"] = st["rx_slave_changed"] = 1
        st["slave_count"] = 5
    st, last, g, pk, sizes, info = run("Tx", False, 2, setup=setup)
    assert list(info["ed137"]) == [0x131C0 | 1 << 22] * 2
    st["tx_slave_changed"] = st["rx_slave_changed"] = 0
    st["slave_count"] = 0
    last = np.zeros((1, N), np.uint8)
    F = 8
    g = np.zeros((F, 1, N), np.uint8)
    pk = np.zeros((F, 1, 184), np.uint8)
    sizes, info = tm.packetize(st, last, g, pk, None, 40, 20)
    assert np.all(sizes[:, 0] == 20)                           # first_r2s still set: every frame goes out
    assert [int(w) for w in info["ed137"][:, 0]] == [0x13100 | 1 << 22] * 5 + [1 << 22] * 3
    assert st["slave_count"][0] == 5


def test_debounce_counts_sent_frames_only():
    def setup(st):
        st["first_r2s"], st["packet_cnt"] = 0, 30
        st["tx_slave_changed"] = 1
    st, last, g, pk, sizes, info = run("Tx", False, 40, setup=setup, t0=0, r2s=0)
    sent = np.nonzero(sizes)[0]
    assert list(sent) == [10, 20, 30]
    assert [int(info["ed137"][f]) for f in sent] == [0x13180 | 1 << 22] * 3 and st["slave_count"][0] == 3


def test_keepalive_cadence():
    st, last, g, pk, sizes, info = run("Tx", False, 100, t0=5000, r2s=5000)
    sent = np.nonzero(sizes)[0]
    assert list(sent[:31]) == list(range(31))
    assert list(sent[31:]) == list(range(40, 100, 10))
    assert np.all(sizes[sent] == 20) and np.all(info["flags"][sent] & capi.TX_KEEPALIVE_PT)
    assert st["first_r2s"][0] == 0 and st["packet_cnt"][0] == 30
    assert np.all(pk[sizes == 0] == 0xA5)                      # unsent slots untouched
    assert st["r2s_send_ms"][0] == 5000 + 90 * 20


def test_marker_only_on_first_sent_frame():
    st, last, g, pk, sizes, info = run("Tx", False, 40, ctl=[S(1, 0)] + [0] * 39)
    assert np.all(sizes == 180)
    mk = (pk[:, 0, 1] >> 7) & 1
    assert mk[0] == 1 and not mk[1:].any()
    assert list(np.nonzero(info["flags"] & capi.TX_MARKER)[0]) == [0]
    assert np.all(pk[:, 0, 0] == 0x90) and np.all(pk[:, 0, 12:16] == [1, 0x67, 0, 1])


def test_marker_skips_unsent_frames():
    def setup(st):
        st["first_r2s"], st["packet_cnt"] = 0, 0                # packetCnt 0 but the burst is over: m needs firstR2SPacket
    st, last, g, pk, sizes, info = run("Tx", False, 12, setup=setup, t0=100, r2s=0)
    assert not (info["flags"] & capi.TX_MARKER).any()


def test_quint64_wrap():
    # now < r2sSendtime: now - r2sSendtime wraps to a huge quint64 >= period -> sent, r2sSendtime = now (:688-701)
    def setup(st):
        st["first_r2s"], st["packet_cnt"] = 0, 30
    st, last, g, pk, sizes, info = run("Tx", False, 3, setup=setup, t0=1000, r2s=10_000)
    assert sizes[0] == 20 and st["r2s_send_ms"][0] == 1000 + 0        # frame 0 resets the clock to now ...
    assert sizes[1] == 0 and sizes[2] == 0                            # ... then the period applies again
    # a negative period converts to a huge quint64: nothing idle goes out once the burst is over
    def setup2(st):
        st["first_r2s"], st["packet_cnt"], st["keepalive_ms"] = 0, 30, -1
    st, last, g, pk, sizes, info = run("Tx", False, 20, setup=setup2, t0=0, r2s=0)
    assert not sizes.any()


def test_stale_payload_after_gate_close():
    # Tx leg, callIn false: ptt opens the gate for frames 0-2; from frame 3 ptt off / sql on -> size 180 but the gate is closed:
    # the packet carries frame 2's payload (:683 copies only under the gate)
    ctl = [S(1, 0)] + [0, 0] + [S(0, 1)] + [0] * 4
    st, last, g, pk, sizes, info = run("Tx", False, 8, ctl=ctl)
    assert np.all(sizes == 180)
    for f in range(3):
        assert np.array_equal(pk[f, 0, 20:180], g[f, 0]) and not info["flags"][f] & capi.TX_STALE_PAYLOAD
    for f in range(3, 8):
        assert np.array_equal(pk[f, 0, 20:180], g[2, 0]) and info["flags"][f] & capi.TX_STALE_PAYLOAD
    assert np.array_equal(last[0], g[2, 0])
    # before any copy the send buffer is zeros
    st, last, g, pk, sizes, info = run("Tx", False, 2, ctl=[S(0, 1), 0])
    assert np.all(pk[:, 0, 20:180] == 0) and np.all(info["flags"] & capi.TX_STALE_PAYLOAD)


def test_signed_level_includes_header_bytes():
    n = 16
    g = np.full((1, 1, n), 0xFF, np.uint8)                    # -1 each
    st, last, gg, pk, sizes, info = run("Tx", False, 1, ctl=[S(1, 0) | capi.TX_CTL_MARK], g711=g, n=n)
    hdr = [0x80, 0x80 | 8, 0, 100, 0, 0, 0x03, 0xE8, 1, 2, 3, 4]
    s = sum(int(np.int8(np.uint8(b))) for b in hdr) + 4 * -1     # first n = 16 stream bytes: header + 4 payload bytes
    assert s == -128 - 120 + 100 + 3 - 24 + 10 - 4 == -163
    assert info["level"][0] == ((-((-s) // n)) & 0xFF) == tm.stream_level(g[0, 0], hdr, n)
    assert st["level"][0] == info["level"][0] and info["flags"][0] & capi.TX_LEVEL_VALID


def test_idle_in_zeroing_and_silence_run():
    g = np.full((4, 1, N), 0xD5, np.uint8)
    g[2, 0, 38] = 0
    st, last, gg, pk, sizes, info = run("Idle", True, 4, ctl=[S(1, 1)] + [0] * 3, g711=g)
    assert st["ptt"][0] == 0 and st["sql"][0] == 0 and np.all(sizes == 20)   # zeroed before the gate (:675-679)
    assert st["tx_run"][0] == 1                                                # frame 2 broke the run (payload byte 38 = stream byte 50)
