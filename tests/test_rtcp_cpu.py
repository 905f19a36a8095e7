"""-m "not gpu": RTCP / SRTCP (include/igdsp.h, "RTCP / SRTCP").  The report block igdsp_rtcp_build_packet writes against the existing
igdsp_jb_report on the same state and prior; the host entries igdsp_rtcp_build_packet / igdsp_rtcp_parse_packet and
igdsp_srtcp_protect_packet / igdsp_srtcp_unprotect_packet against tests/rtcp_model.py, byte for byte: SR and RR, with and without a
block, the CNAME lengths, BYE; every truncation of a valid compound, the refusals of RFC 3550 A.2, an unknown type in the middle, a
block for somebody else in front of ours, the round-trip time of a two-peer exchange; SRTCP's packet sizes on either side of SHA-1's
padding and the 64-byte pieces, tampering, the window, E = 0, SRTP and SRTCP states swapped, states of random bytes, BYPASS / RESET,
the index wrap; the model's session keys and keystream against OpenSSL where there is one."""
import ctypes
import ctypes.util
import os
import struct

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import rtcp_model as rm
from tests import srtp_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes.fromhex("e1f97a0d3e018be0d64fa32c06de41390ec675ad498afeebb6960b3aabe6")
SRTCP_SIZES = (8, 12, 28, 48, 52, 56, 60, 64, 68, 112, 116, 120, 136, 2034)
MOVING = ("roc", "s_l", "have_s_l", "window", "n_ok", "n_auth_fail", "n_replay", "n_malformed")
FILL = 0xA5
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def lib():
    igbuild.build()
    return capi.load()


# ---- helpers: RTCP
def jb_state(rng, heard=True, **kw):
    """a seeded JB_STATE record: an A.1 source some way into its stream"""
    st = np.zeros((), capi.JB_STATE)
    base = int(rng.integers(0, 65536))
    span = int(rng.integers(1, 5000))
    st["ssrc"], st["base_seq"], st["epoch"] = int(rng.integers(0, 1 << 32)), base, int(rng.integers(0, 4))
    st["cycles"], st["max_seq"] = ((base + span) >> 16) << 16, (base + span) & 0xFFFF
    st["received"] = max(0, span + 1 - int(rng.integers(0, max(2, span // 3))))
    st["jitter"] = int(rng.integers(0, 1 << 20))
    st["flags"] = (capi.JB_HEARD if hasattr(capi, "JB_HEARD") else 1) if heard else 0
    for k, v in kw.items():
        st[k] = v
    return st


def jb_dict(st):
    return None if st is None else {k: int(st[k]) for k in ("ssrc", "cycles", "base_seq", "received", "jitter", "epoch", "max_seq", "flags")}


def src_of(ssrc, packets, rng=None):
    return np.array((ssrc, 0 if rng is None else int(rng.integers(0, 1 << 32)), packets, 160 * packets & M32), capi.RTCP_SRC)


def src_dict(s):
    return {k: int(s[k]) for k in ("ssrc", "rtp_ts", "packets", "octets")}


def same_state(st, leg, what=""):
    got = {k: int(st[k]) for k in rm.Leg.FIELDS}
    got.update({k: int(st["prior"][k]) for k in ("expected_prior", "received_prior", "epoch")})
    assert got == leg.moving(), (what, got, leg.moving())
    assert int(st["prior"]["reserved"]) == 0 and not st["reserved"].any()


def build(st, leg, ctl, src, now, jb=None, cname=None):
    """the library and the model on one tick: the packet (None for NONE), checked byte for byte with the record and the state"""
    out, n, rec = capi.rtcp_build_packet(st, ctl, src, now, jb=jb, cname=cname, fill=FILL)
    want, flags = leg.build(ctl, src_dict(src), now, jb_dict(jb), b"" if cname is None else cname)
    assert np.all(out[n:] == FILL), "bytes behind the size written"
    assert (n, int(rec["size"]), int(rec["flags"])) == (0 if want is None else len(want), n, flags) and int(rec["reserved"]) == 0 and int(rec["reserved2"]) == 0
    assert out[:n].tobytes() == (want or b"")
    same_state(st, leg)
    return want


def parse(st, leg, pkt, arrival, local):
    rec = capi.rtcp_parse_packet(st, pkt, arrival, local)
    want = leg.parse(pkt, arrival, local)
    got = {k: int(rec[k]) for k in want}
    assert got == want and int(rec["reserved"]) == 0, (got, want)
    same_state(st, leg)
    return want


def fresh():
    return np.zeros((), capi.RTCP_STATE), rm.Leg()


# ---- 1. the report block against the existing igdsp_jb_report
def test_report_block_is_jb_reports():
    rng = np.random.default_rng(3550)
    cases = [jb_state(rng) for _ in range(300)]
    cases += [jb_state(rng, heard=False), jb_state(rng, received=40000, base_seq=10, cycles=0, max_seq=20),          # negative cumulative loss
              jb_state(rng, cycles=0x7FFF0000, base_seq=0, max_seq=1, received=3),                                   # above the 24-bit clamp
              jb_state(rng, cycles=0, base_seq=5, max_seq=5, received=0x7FFFFFFF)]                                   # below it
    st, prior = np.zeros((), capi.RTCP_STATE), np.zeros((), capi.JB_PRIOR)
    seen = set()
    for i, jb in enumerate(cases):
        if i % 3 == 1:                                                      # the same source again: an interval, and every so often a new epoch
            jb = cases[i - 1].copy()
            jb["max_seq"] = (int(jb["max_seq"]) + 50) & 0xFFFF
            jb["received"] = int(jb["received"]) + int(rng.integers(0, 60))
            if i % 2:
                jb["epoch"] = int(jb["epoch"]) + 1
        out, n, rec = capi.rtcp_build_packet(st, capi.RTCP_REPORT, src_of(7, 0), 0, jb=jb)
        rr = capi.jb_report(jb, prior)
        assert bool(int(rec["flags"]) & capi.RTCP_HAS_BLOCK) == bool(rr["valid"]) and st["prior"].tobytes() == prior.tobytes(), i
        if not rr["valid"]:
            assert out[0] == 0x80 and n == 8 + 12
            continue
        ssrc, frac, cum, ext, jit, lsr, dlsr = struct.unpack(">IB3sIIII", out[8:32].tobytes())
        assert (ssrc, frac, int.from_bytes(cum, "big", signed=True), ext, jit, lsr, dlsr) == (int(rr["ssrc"]), int(rr["fraction_lost"]), int(rr["cum_lost"]),
                                                                                            int(rr["ext_max_seq"]), int(rr["jitter"]), 0, 0), i
        seen |= {"neg"} if rr["cum_lost"] < 0 else set()
        seen |= {"hi"} if rr["cum_lost"] == 0x7FFFFF else set()
        seen |= {"lo"} if rr["cum_lost"] == -0x800000 else set()
        seen |= {"frac"} if rr["fraction_lost"] else set()
    assert seen == {"neg", "hi", "lo", "frac"}, seen


# ---- 2. build against the model
@pytest.mark.parametrize("L", (None, 0, 1, 2, 5, 64, 70))
def test_build_forms_against_model(L):
    rng = np.random.default_rng(65 if L is None else L)
    cname = None if L is None else bytes(rng.integers(1, 256, L, dtype=np.uint8))
    st, leg = fresh()
    jb = jb_state(rng)
    now = (0x83AA7E80 << 32) | 0x40000000
    sizes = []
    for tick, (ctl, packets, j) in enumerate([(1, 0, None), (1, 5, None), (1, 5, jb), (1, 9, jb), (0, 11, jb), (7, 11, jb), (2, 11, jb), (2, 11, None),
                                              (1, 11, jb_state(rng, heard=False))]):
        pkt = build(st, leg, ctl, src_of(0xC0FFEE00 + tick, packets, rng), now + (tick << 32), jb=j, cname=cname)
        sizes.append(0 if pkt is None else len(pkt))
    if L in (64, 70):
        assert max(sizes) == capi.RTCP_MAX_BUILT == 136                     # SR, a block, 64 bytes of CNAME, BYE
    assert sizes[4] == sizes[5] == 0 and int(st["n_built"]) == 7
    assert capi.rtcp_build_packet(st, 1, src_of(1, 1), 0, capacity=135, raw=True) == -22


def test_build_lsr_and_dlsr_after_an_sr():
    st, leg = fresh()
    rng = np.random.default_rng(8)
    peer_st, peer = fresh()
    sr = build(peer_st, peer, 1, src_of(0xBEEF, 3, rng), (1000 << 32) | 0x12345678)
    parse(st, leg, sr, 0x03E8_2000, 0x1111)
    pkt = build(st, leg, 1, src_of(0x1111, 0), (1002 << 32) | 0x80000000, jb=jb_state(rng))
    lsr, dlsr = struct.unpack(">II", pkt[8 + 16:8 + 24])
    assert lsr == 0x03E8_1234 and dlsr == ((1002 << 16) | 0x8000) - 0x03E8_2000


# ---- 3. parse against the model
def compound(rng, local, other_first=True, bye=True):
    """SR with two blocks (another source's, then ours), SDES, an APP in the middle, BYE"""
    blk = lambda ssrc: struct.pack(">IB3sIIII", ssrc, 17, (-5 & 0xFFFFFF).to_bytes(3, "big"), 0x00012345, 99, 0x11112222, 0x00000400)
    blocks = (blk(local ^ 1) if other_first else b"") + blk(local) + blk(local)[:4] + bytes(20)
    rc = len(blocks) // 24
    sr = struct.pack(">BBHIIIIII", 0x80 | rc, 200, 6 + 6 * rc, 0xABCD0001, 0x83AA0000, 0x80000000, 1234, 77, 77 * 160) + blocks
    sdes = struct.pack(">BBHIBB", 0x81, 202, 3, 0xABCD0001, 1, 5) + b"alice\0"
    app = struct.pack(">BBHI4s", 0x80, 204, 3, 0xABCD0001, b"TEST") + bytes(4)
    out = sr + sdes + app
    if bye:
        out += struct.pack(">BBHI", 0x81, 203, 1, 0xABCD0001)
    return out


def test_parse_valid_compound_and_every_truncation():
    rng = np.random.default_rng(1)
    local = 0x5EED0001
    pkt = compound(rng, local)
    st, leg = fresh()
    rec = parse(st, leg, pkt, 0x11112222 + 0x400 + 0x3000, local)
    assert rec["flags"] == rm.PARSED | rm.GOT_SR | rm.GOT_BLOCK | rm.GOT_RTT | rm.GOT_BYE and rec["rtt"] == 0x3000 and rec["n_sub"] == 4
    assert rec["peer_cum_lost"] == -5 and rec["peer_fraction_lost"] == 17 and rec["sr_packets"] == 77 and int(st["lsr"]) == 0x00008000
    ends = {100, 116, 132, len(pkt)}                                        # where a sub-packet ends: a shorter compound that is whole
    for n in list(range(0, len(pkt) + 1, 4)) + [n + d for n in range(4, len(pkt) + 1, 4) for d in (-1, 1)]:
        st, leg = fresh()
        rec = parse(st, leg, pkt[:n] if n <= len(pkt) else pkt + b"\0", 5, local)
        want = rm.EMPTY if n == 0 else (rm.PARSED if n in ends else rm.MALFORMED)
        assert rec["flags"] & (rm.PARSED | rm.MALFORMED | rm.EMPTY) == want, n
        assert int(st["n_malformed"]) == (want == rm.MALFORMED) and int(st["n_parsed"]) == (want == rm.PARSED)


def test_parse_refusals_of_a2():
    local = 0x5EED0001
    good = compound(np.random.default_rng(2), local)

    def with_byte(at, value):
        b = bytearray(good)
        b[at] = value
        return bytes(b)

    bad = {
        "version 1 on the first": with_byte(0, 0x43),
        "version 3 on the SDES": with_byte(100, 0xC1),
        "padding on the first": with_byte(0, 0xA3),
        "padding on the SDES, not the last": with_byte(100, 0xA1),
        "first is an SDES": good[100:],
        "length past the end": with_byte(103, 200),
        "length short of the end": with_byte(119, 2),
        "SR shorter than its blocks": struct.pack(">BBHIIIIII", 0x82, 200, 6, 1, 2, 3, 4, 5, 6),
        "RR shorter than its block": struct.pack(">BBHI", 0x81, 201, 1, 1),
        "BYE shorter than its sources": struct.pack(">BBHI", 0x80, 201, 1, 1) + struct.pack(">BBHI", 0x83, 203, 1, 1),
        "four bytes": good[:4],
    }
    for what, pkt in bad.items():
        st, leg = fresh()
        st["lsr"], leg.lsr = 9, 9
        assert parse(st, leg, pkt, 5, local)["flags"] == rm.MALFORMED, what
        assert int(st["n_malformed"]) == 1 and int(st["flags"]) == 0 and int(st["lsr"]) == 9, what
    st, leg = fresh()
    ok = with_byte(132, 0xA1)                                               # padding on the last sub-packet is legal
    assert parse(st, leg, ok, 5, local)["flags"] & rm.PARSED
    assert parse(st, leg, compound(None, local, bye=False), 5, local)["flags"] == rm.PARSED | rm.GOT_SR | rm.GOT_BLOCK | rm.RTT_NEGATIVE


def test_parse_blocks_and_rtt_forms():
    local = 0x77
    blk = lambda ssrc, lsr, dlsr, cum=3: struct.pack(">IB3sIIII", ssrc, 1, (cum & 0xFFFFFF).to_bytes(3, "big"), 50, 6, lsr, dlsr)
    rr = lambda *blocks: struct.pack(">BBHI", 0x80 | len(blocks), 201, 1 + 6 * len(blocks), 0xAA) + b"".join(blocks)
    st, leg = fresh()
    assert parse(st, leg, rr(), 100, local)["flags"] == rm.PARSED                       # an empty RR
    assert parse(st, leg, rr(blk(0x78, 5, 5)), 100, local)["flags"] == rm.PARSED       # nobody reports about us
    assert parse(st, leg, rr(blk(local, 0, 44)), 100, local)["flags"] == rm.PARSED | rm.GOT_BLOCK          # LSR 0: no round trip
    r = parse(st, leg, rr(blk(0x78, 1, 1), blk(local, 60, 30, cum=0x800000), blk(local, 1, 1, cum=1)), 100, local)
    assert r["flags"] == rm.PARSED | rm.GOT_BLOCK | rm.GOT_RTT and r["rtt"] == 10 and r["peer_cum_lost"] == -0x800000
    r = parse(st, leg, rr(blk(local, 60, 50)), 100, local)
    assert r["flags"] == rm.PARSED | rm.GOT_BLOCK | rm.RTT_NEGATIVE and r["rtt"] == (100 - 110) & M32
    assert int(st["rtt_last"]) == 10 and int(st["rtt_count"]) == 1 and int(st["flags"]) == rm.PEER_VALID | rm.RTT_VALID
    two = rr(blk(0x78, 1, 1)) + rr(blk(local, 90, 4))                                 # ours in a second report of the compound
    assert parse(st, leg, two, 100, local)["rtt"] == 6
    st, leg = fresh()
    rng = np.random.default_rng(77)
    for _ in range(300):                                                               # random words behind a sound first header
        body = rng.integers(0, 256, 4 * int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
        pkt = struct.pack(">BBH", 0x80 | int(rng.integers(0, 3)), 200 + int(rng.integers(0, 2)), int(rng.integers(0, 12))) + body
        parse(st, leg, pkt, int(rng.integers(0, 1 << 32)), struct.unpack(">I", body[:4])[0] if rng.random() < 0.5 else 1)


# ---- 4. a two-peer exchange gives the round-trip time exactly
@pytest.mark.parametrize("d1,d2,hold", [(0x0123, 0x0456, 0x20000), (1, 0, 0), (0x7FFF0000, 0xFFFF, 5)])
def test_round_trip_time_is_d1_plus_d2(d1, d2, hold):
    rng = np.random.default_rng(d1)
    (a_st, a), (b_st, b) = fresh(), fresh()
    ssrc_a, ssrc_b = 0xA0A0A0A0, 0xB0B0B0B0
    jb_a, jb_b = jb_state(rng, ssrc=ssrc_b), jb_state(rng, ssrc=ssrc_a)     # what A heard of B, what B heard of A
    mid = lambda now: (now >> 16) & M32
    t0 = (0x83AA7E80 << 32) | 0x12340000
    sr = build(a_st, a, 1, src_of(ssrc_a, 10, rng), t0, jb=jb_a, cname=b"a@host")
    parse(b_st, b, sr, (mid(t0) + d1) & M32, ssrc_b)
    t1 = t0 + ((d1 + hold) << 16)
    back = build(b_st, b, 1, src_of(ssrc_b, 0), t1, jb=jb_b, cname=b"b@host")
    rec = parse(a_st, a, back, (mid(t1) + d2) & M32, ssrc_a)
    assert rec["flags"] == rm.PARSED | rm.GOT_BLOCK | rm.GOT_RTT and rec["rtt"] == d1 + d2 == int(a_st["rtt_last"])
    rr = capi.jb_report(jb_b, np.zeros((), capi.JB_PRIOR))
    assert (rec["peer_fraction_lost"], rec["peer_cum_lost"], rec["peer_ext_seq"], rec["peer_jitter"]) == (int(rr["fraction_lost"]), int(rr["cum_lost"]),
                                                                                                        int(rr["ext_max_seq"]), int(rr["jitter"]))


# ---- helpers: SRTCP
def rtcp_packet(size, seed, ssrc=None):
    rng = np.random.default_rng(seed)
    return struct.pack(">BBHI", 0x80, 201, size // 4 - 1, int(rng.integers(0, 1 << 32)) if ssrc is None else ssrc) + rng.integers(0, 256, size - 8, dtype=np.uint8).tobytes()


def run(state, pkt, unprotect=False, ctl=rm.RUN, capacity=2048, in_place=False):
    out, n, rec = capi.srtcp_packet(state, pkt, unprotect=unprotect, ctl=ctl, capacity=capacity, in_place=in_place, fill=FILL)
    assert n == int(rec["size_out"]) and int(rec["reserved"]) == 0
    if in_place and n == 0:
        assert out[:len(pkt)].tobytes() == bytes(pkt) and np.all(out[len(pkt):] == FILL), "a refused packet's slot was written"
    else:
        assert np.all(out[n:] == FILL) or in_place and np.all(out[max(n, len(pkt)):] == FILL), "bytes behind size_out written"
    return (out[:n].tobytes() if n else None), dict(flags=int(rec["flags"]), size_out=n, roc_used=int(rec["roc_used"]))


def same_moving(state, leg):
    got = {k: int(state[k]) for k in MOVING}
    assert got == leg.moving(), (got, leg.moving())


def pair(index0=0, key=KEY):
    return capi.srtcp_derive(key, index0), rm.SrtcpLeg(key, index0)


def both(st, leg, pkt, unprotect=False, **kw):
    got = run(st, pkt, unprotect=unprotect, **kw)
    mkw = {k: v for k, v in kw.items() if k == "ctl"}
    if "capacity" in kw:
        mkw["out_cap"] = kw["capacity"]
    want = (leg.unprotect if unprotect else leg.protect)(pkt, **mkw)
    assert got == want, (got[1], want[1])
    same_moving(st, leg)
    return got


# ---- 5. SRTCP against the model
def test_srtcp_derive_uses_labels_3_4_5():
    st = capi.srtcp_derive(KEY, 1)
    ke, ka, ks = rm.srtcp_keys(KEY)
    assert int(st["tag"]) == capi.SRTCP_TAG | 10 and int(st["roc"]) == 1 and st["ks"].tobytes() == ks + b"\0\0"
    assert b"".join(int(w).to_bytes(4, "big") for w in st["rk"][:4]) == ke and ke != sm.derive(KEY)[0]
    assert int(capi.srtcp_derive(KEY, 0x80000005)["roc"]) == 5


@pytest.mark.parametrize("in_place", (False, True))
def test_srtcp_sizes_round_trip_against_model(in_place):
    """The sizes cross SHA-1's padding (the hashed message is the packet and four bytes) and the 64-byte pieces.  2034 is no multiple of
    4: as a clear packet the rule refuses it, as a protected one it is the 2020-byte packet's, so it is fed to both directions."""
    (tx, txm), (rx, rxm) = pair(), pair()
    n_ok = 0
    for size in SRTCP_SIZES + (2020, 2032):
        clear = rtcp_packet(size & ~3, size)[:size] + bytes(size & 3)
        prot, rec = both(tx, txm, clear, in_place=in_place)
        if size % 4:
            assert rec == dict(flags=rm.SRTP_MALFORMED, size_out=0, roc_used=0)
            continue
        assert rec == dict(flags=rm.OK, size_out=size + 14, roc_used=0x80000000 | n_ok) and prot[:8] == clear[:8] and (size == 8 or prot[8:size] != clear[8:])
        back, rec = both(rx, rxm, prot, unprotect=True, in_place=in_place)
        assert back == clear and rec["roc_used"] == 0x80000000 | n_ok and (size != 2020 or len(prot) == 2034)
        n_ok += 1
    assert int(tx["roc"]) == n_ok == len(SRTCP_SIZES) + 1 and int(rx["window"]) == (1 << n_ok) - 1 and int(tx["n_malformed"]) == 1


def test_srtcp_tampering_window_and_clear_packets():
    (tx, txm), (rx, rxm) = pair(index0=1), pair()
    prot = [both(tx, txm, rtcp_packet(52, i))[0] for i in range(70)]
    for at in (0, 5, 9, 51, 52, 55, 56, 65):                                # header, body, index word, tag
        bad = bytearray(prot[0])
        bad[at] ^= 0x10
        fl = both(rx, rxm, bytes(bad), unprotect=True, in_place=True)[1]["flags"]
        assert fl == rm.AUTH_FAIL, at
    for i in (0, 2, 1, 1, 69, 68, 6, 5, 0, 69):                               # reorder within the window, replays, old
        both(rx, rxm, prot[i], unprotect=True)
    assert int(rx["n_ok"]) == 6 and int(rx["n_replay"]) == 4 and int(rx["n_auth_fail"]) == 8 and int(rx["roc"]) == 70
    # E = 0: authenticated, copied without decryption
    clear = rtcp_packet(60, 3)
    body = clear + (200).to_bytes(4, "big")
    got = both(rx, rxm, body + rxm.tag(body), unprotect=True)
    assert got == (clear, dict(flags=rm.OK | rm.CLEAR, size_out=60, roc_used=200))
    # the sizes' own refusals
    for pkt, kw in ((b"\x80" * 21, {}), (b"\x80" * 24, {}), (prot[3], dict(capacity=48)), (bytes(2049), {})):
        assert both(rx, rxm, pkt, unprotect=True, **kw)[1]["flags"] == rm.SRTP_MALFORMED
    for pkt, kw in ((b"\x80" * 4, {}), (b"\x80" * 10, {}), (b"\x40" + bytes(11), {}), (rtcp_packet(52, 1), dict(capacity=64)), (bytes(2049), {})):
        assert both(tx, txm, pkt, **kw)[1]["flags"] == rm.SRTP_MALFORMED
    assert both(tx, txm, b"")[1]["flags"] == rm.SRTP_EMPTY and both(rx, rxm, b"", unprotect=True)[1]["flags"] == rm.SRTP_EMPTY


def test_srtcp_and_srtp_states_are_not_each_others():
    srtp, srtcp = capi.srtp_derive(KEY, 10), capi.srtcp_derive(KEY)
    pkt = rtcp_packet(28, 1)
    for unprotect in (False, True):
        before = srtp.tobytes()
        assert run(srtp, pkt + bytes(14), unprotect=unprotect) == (None, dict(flags=rm.NO_KEY, size_out=0, roc_used=0)) and srtp.tobytes() == before
        before = srtcp.tobytes()
        out, n, rec = capi.srtp_packet(srtcp, sm.rtp(1, 2, bytes(40)), unprotect=unprotect)
        assert n == 0 and int(rec["flags"]) == capi.SRTP_NO_KEY and srtcp.tobytes() == before and np.all(out == FILL)


def test_srtcp_states_of_random_bytes():
    rng = np.random.default_rng(31)
    for i in range(40):
        st = np.array(rng.integers(0, 256, capi.SRTP_STATE.itemsize, dtype=np.uint8).view(capi.SRTP_STATE)[0])
        before = st.tobytes()
        assert run(st, rtcp_packet(28, i), unprotect=bool(i % 2))[1]["flags"] == rm.NO_KEY and st.tobytes() == before
        st["tag"] = capi.SRTCP_TAG | 10                                     # a key of random bytes: any index, window and counters are tolerated
        prot, rec = run(st, rtcp_packet(28, i))
        assert rec["flags"] == rm.OK and rec["roc_used"] >> 31 == 1 and len(prot) == 42
        run(st, prot, unprotect=True)


def test_srtcp_bypass_reset_and_index_wrap():
    (tx, txm), (rx, rxm) = pair(index0=0x7FFFFFFE), pair()
    pkt = rtcp_packet(28, 9)
    assert both(tx, txm, pkt, ctl=rm.BYPASS) == (pkt, dict(flags=rm.BYPASSED, size_out=28, roc_used=0))
    words = [both(tx, txm, pkt)[1]["roc_used"] for _ in range(3)]
    assert words == [0xFFFFFFFE, 0xFFFFFFFF, 0x80000000] and int(tx["roc"]) == 1     # the index wraps at 2^31 on protect
    p5 = [both(tx, txm, pkt)[0] for _ in range(5)]
    for p in p5:
        both(rx, rxm, p, unprotect=True)
    assert both(rx, rxm, p5[0], unprotect=True)[1]["flags"] == rm.REPLAY
    assert both(rx, rxm, p5[0], unprotect=True, ctl=rm.RESET)[1]["flags"] == rm.OK and int(rx["window"]) == 1
    assert both(tx, txm, pkt, ctl=rm.RESET)[1]["roc_used"] == 0x80000000
    assert both(tx, txm, pkt, ctl=200)[1]["roc_used"] == 0x80000001          # another value is RUN


# ---- 6. the model's SRTCP session keys and keystream against OpenSSL
def test_model_srtcp_keys_against_openssl():
    name = ctypes.util.find_library("crypto")
    if not name:
        pytest.skip("no OpenSSL libcrypto on this machine")
    ssl = ctypes.CDLL(name)
    vp = ctypes.c_void_p
    ssl.EVP_CIPHER_CTX_new.restype = vp
    ssl.EVP_aes_128_ctr.restype = vp
    ssl.EVP_EncryptInit_ex.argtypes = [vp, vp, vp, ctypes.c_char_p, ctypes.c_char_p]
    ssl.EVP_EncryptUpdate.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]
    ssl.EVP_CIPHER_CTX_free.argtypes = [vp]

    def ctr(key, iv, n):
        ctx = ssl.EVP_CIPHER_CTX_new()
        assert ssl.EVP_EncryptInit_ex(ctx, ssl.EVP_aes_128_ctr(), None, key, iv) == 1
        out, got = ctypes.create_string_buffer(n + 32), ctypes.c_int(0)
        assert ssl.EVP_EncryptUpdate(ctx, out, ctypes.byref(got), bytes(n), n) == 1 and got.value == n
        ssl.EVP_CIPHER_CTX_free(ctx)
        return out.raw[:n]

    mk, ms = KEY[:16], KEY[16:]
    want = [ctr(mk, (int.from_bytes(ms, "big") ^ (label << 48)).to_bytes(14, "big") + b"\0\0", n) for label, n in ((3, 16), (4, 20), (5, 14))]
    assert list(rm.srtcp_keys(KEY)) == want
    leg = rm.SrtcpLeg(KEY)
    for ssrc, index, n in ((0xDEADBEEF, 0, 16), (1, 0x7FFFFFFF, 2026), (0xFFFFFFFF, 0x10000, 120)):
        iv = ((int.from_bytes(leg.ks, "big") << 16) ^ (ssrc << 64) ^ (index << 16)).to_bytes(16, "big")
        assert leg.keystream(ssrc, index, n) == ctr(leg.ke, iv, n)


def test_yardstick_row_is_the_entrys():
    res, args = capi.INTERNAL_MORE["igdsp_internal_srtcp_move"]
    pub = {n: (r, a) for n, r, a in capi.PROTOTYPES}["igdsp_srtcp_protect"]
    assert (res, list(args)) == (pub[0], list(pub[1])) and capi.internal("srtcp_move") is not None


def test_host_mirror_leg_rtcp():
    """LegRtcp (host/igdsp_host.h) through its C face: two legs under SRTCP, a report each way with constructed delays, the round-trip
    time at the first; a replayed packet did not arrive; a key for one direction alone is refused"""
    host = ctypes.CDLL(os.path.join(ROOT, "igate4xsoftphonedsp_amd", "libigdsp_host.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    host.igdsp_host_rtcp_new.restype = vp
    host.igdsp_host_rtcp_new.argtypes = [u32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, u32]
    host.igdsp_host_rtcp_free.argtypes = [vp]
    host.igdsp_host_rtcp_report.argtypes = [vp, vp, u32, u32, u32, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p, u32]
    host.igdsp_host_rtcp_received.argtypes = [vp, ctypes.c_char_p, u32, u32]
    host.igdsp_host_rtcp_state.argtypes = [vp, vp]
    key_a, key_b = KEY, bytes(reversed(KEY))
    a, b = host.igdsp_host_rtcp_new(0xA1, b"a@host", key_a, key_b, 0), host.igdsp_host_rtcp_new(0xB1, b"b@host", key_b, key_a, 0)
    assert a and b and not host.igdsp_host_rtcp_new(1, b"x", key_a, None, 0)
    rng = np.random.default_rng(5)
    jb = jb_state(rng, ssrc=0xA1)                                           # what B heard of A
    out = ctypes.create_string_buffer(160)
    t0, d1, d2, hold = (0x83AA7E80 << 32) | 0x4000_0000, 0x333, 0x555, 0x10000
    n = host.igdsp_host_rtcp_report(a, None, 8000, 10, 1600, t0, 0, out, 160)
    assert n == 28 + 4 + 16 + 14 and out.raw[:2] == b"\x80\xc8"
    sr = out.raw[:n]
    assert host.igdsp_host_rtcp_received(b, sr, n, ((t0 >> 16) + d1) & M32) == 1 and host.igdsp_host_rtcp_received(b, sr, n, 0) == 0    # the second: a replay
    t1 = t0 + ((d1 + hold) << 16)
    n = host.igdsp_host_rtcp_report(b, jb.ctypes.data, 0, 0, 0, t1, 1, out, 160)
    assert n == 8 + 24 + 4 + 16 + 8 + 14 and out.raw[:2] == b"\x81\xc9"
    assert host.igdsp_host_rtcp_received(a, out.raw[:n], n, ((t1 >> 16) + d2) & M32) == 1
    st = np.zeros((), capi.RTCP_STATE)
    assert host.igdsp_host_rtcp_state(a, st.ctypes.data) == 0
    assert int(st["rtt_last"]) == d1 + d2 and int(st["flags"]) == rm.PEER_VALID | rm.RTT_VALID | rm.BYE_SEEN
    assert host.igdsp_host_rtcp_report(a, None, 0, 0, 0, t1, 0, out, 100) == -22
    clear = host.igdsp_host_rtcp_new(7, None, None, None, 0)
    assert host.igdsp_host_rtcp_report(clear, None, 0, 0, 0, t1, 0, out, 136) == 8 + 4 + 8
    for h in (a, b, clear):
        host.igdsp_host_rtcp_free(h)
