"""-m "not gpu": SRTP (include/igdsp.h, "SRTP").  tests/srtp_model.py against the standards' known answers (tests/golden/srtp_kat.json:
FIPS-197 C.1, RFC 3711 B.2 and B.3, the libsrtp packet vector) and, where there is an OpenSSL, its AES-CTR keystream against
EVP_aes_128_ctr; then the library's host entries (igdsp_srtp_derive, igdsp_srtp_protect_packet, igdsp_srtp_unprotect_packet) against the
model, byte for byte: packet sizes on either side of SHA-1's padding boundaries, CSRC counts and header extensions, both tag lengths,
the round trip, the sequence wrap, reordering / repeats / old packets against the window, one flipped bit anywhere, the malformed
packets, a state of random bytes, BYPASS and RESET, in place, and that nothing behind size_out is ever written."""
import ctypes
import ctypes.util
import json
import os

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import srtp_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "srtp_kat.json")))
SIZES = (12, 20, 33, 51, 52, 59, 60, 115, 116, 172, 180, 181, 2038)
KEY = bytes.fromhex(KAT["rfc3711_b3"]["master_key"] + KAT["rfc3711_b3"]["master_salt"])
MOVING = ("roc", "s_l", "have_s_l", "window", "n_ok", "n_auth_fail", "n_replay", "n_malformed")
FILL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def lib():
    igbuild.build()
    return capi.load()


def packet(size, seq, seed, cc=0, ext_len=None, ssrc=None, keepalive=True):
    """a seeded packet of exactly `size` bytes (size 20 without more: the PT 123 keep-alive, X set, an 8-byte header extension)"""
    rng = np.random.default_rng(seed)
    if keepalive and size == 20 and cc == 0 and ext_len is None:
        return sm.rtp(seq, 0x1234ABCD if ssrc is None else ssrc, b"", ext_len=1, pt=123)
    hdr = 12 + 4 * cc + (0 if ext_len is None else 4 + 4 * ext_len)
    assert size >= hdr, (size, hdr)
    return sm.rtp(seq, int(rng.integers(0, 1 << 32)) if ssrc is None else ssrc, rng.integers(0, 256, size - hdr, dtype=np.uint8).tobytes(), cc=cc,
                  ext_len=ext_len, ts=int(rng.integers(0, 1 << 32)))


def run(state, pkt, unprotect=False, ctl=sm.RUN, capacity=2048, in_place=False):
    """the library on one packet: (bytes out or None, dict like the model's); checks that nothing at or behind size_out was written"""
    out, n, rec = capi.srtp_packet(state, pkt, unprotect=unprotect, ctl=ctl, capacity=capacity, in_place=in_place, fill=FILL)
    assert n == int(rec["size_out"]) and int(rec["reserved"]) == 0
    if in_place and n == 0:
        assert out[:len(pkt)].tobytes() == bytes(pkt), "a refused packet's slot was written"
        assert np.all(out[len(pkt):] == FILL)
    else:
        assert np.all(out[n:] == FILL) or in_place and np.all(out[max(n, len(pkt)):] == FILL), "bytes behind size_out written"
    return (out[:n].tobytes() if n else None), dict(flags=int(rec["flags"]), size_out=n, roc_used=int(rec["roc_used"]))


def same_moving(state, leg):
    got = {k: int(state[k]) for k in MOVING}
    assert got == leg.moving(), (got, leg.moving())


def pair(tag_len=10, roc0=0, key=KEY):
    return capi.srtp_derive(key, tag_len, roc0), sm.Leg(key, tag_len, roc0)


# ---- the model against the standards
def test_model_fips197():
    f = KAT["fips197_c1"]
    assert sm.aes_encrypt(sm.aes_expand(bytes.fromhex(f["key"])), bytes.fromhex(f["plaintext"])).hex() == f["ciphertext"]


def test_model_rfc3711_keystream():
    b = KAT["rfc3711_b2"]
    leg = sm.Leg(KEY)
    leg.ke, leg.ks = bytes.fromhex(b["session_key"]), bytes.fromhex(b["session_salt"])
    ks = leg.keystream(b["ssrc"], b["index"], 48)
    for i, want in b["keystream_blocks"].items():
        assert ks[16 * int(i):16 * int(i) + 16].hex() == want, i


def test_model_rfc3711_derivation():
    d = KAT["rfc3711_b3"]
    ke, ka, ks = sm.derive(KEY)
    assert (ke.hex(), ka.hex(), ks.hex()) == (d["k_e"], d["k_a"], d["k_s"])


def test_model_packet_vector():
    p = KAT["packet_sha1_80"]
    out, rec = sm.Leg(bytes.fromhex(p["master_key"] + p["master_salt"]), p["tag_len"], p["roc"]).protect(bytes.fromhex(p["clear"]))
    assert out.hex() == p["protected"] and rec == dict(flags=sm.OK, size_out=38, roc_used=0)


def test_model_keystream_against_openssl():
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
    rng = np.random.default_rng(3711)
    for n in (1, 16, 17, 160, 2026):
        key, iv = rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), rng.integers(0, 256, 14, dtype=np.uint8).tobytes() + b"\0\0"
        ctx = ssl.EVP_CIPHER_CTX_new()
        assert ssl.EVP_EncryptInit_ex(ctx, ssl.EVP_aes_128_ctr(), None, key, iv) == 1
        out, got = ctypes.create_string_buffer(n + 32), ctypes.c_int(0)
        assert ssl.EVP_EncryptUpdate(ctx, out, ctypes.byref(got), bytes(n), n) == 1 and got.value == n
        ssl.EVP_CIPHER_CTX_free(ctx)
        assert sm.aes_ctr(key, int.from_bytes(iv, "big"), n) == out.raw[:n], n


# ---- the library against the model
def test_library_derive_and_packet_vector():
    p = KAT["packet_sha1_80"]
    st = capi.srtp_derive(bytes.fromhex(p["master_key"] + p["master_salt"]), p["tag_len"], p["roc"])
    assert int(st["tag"]) == capi.SRTP_TAG | 10 and st["ks"].tobytes() == bytes.fromhex(KAT["rfc3711_b3"]["k_s"]) + b"\0\0"
    ke = b"".join(int(w).to_bytes(4, "big") for w in st["rk"][:4])
    assert ke.hex() == KAT["rfc3711_b3"]["k_e"]                             # the schedule's first round key is k_e
    out, rec = run(st, bytes.fromhex(p["clear"]))
    assert out.hex() == p["protected"] and rec == dict(flags=sm.OK, size_out=38, roc_used=0)
    for bad in (0, 5, 9, 11, 16, 80):
        assert capi.srtp_derive(KEY, bad, raw=True) == -22
    assert capi.SRTP_STATE.itemsize == 288 and capi.SRTP_REC.itemsize == 8


@pytest.mark.parametrize("tag_len", (10, 4))
def test_sizes_round_trip_against_model(tag_len):
    """every size of the list, both directions, out of place and in place: bytes, records and the state's moving fields"""
    tx, mtx = pair(tag_len)
    rx, mrx = pair(tag_len)
    for k, size in enumerate(SIZES):
        pkt = packet(size, 1000 + k, seed=size)
        want, wrec = mtx.protect(pkt)
        got, grec = run(tx, pkt, in_place=bool(k & 1))
        assert got == want and grec == wrec and len(got) == size + tag_len, size
        same_moving(tx, mtx)
        clear, crec = mrx.unprotect(want)
        back, brec = run(rx, got, unprotect=True, in_place=not (k & 1))
        assert back == clear == pkt and brec == crec, size
        same_moving(rx, mrx)
    assert int(tx["n_ok"]) == int(rx["n_ok"]) == len(SIZES)


@pytest.mark.parametrize("cc", (0, 3, 15))
@pytest.mark.parametrize("ext_len", (None, 0, 1, 5))
def test_header_forms_against_model(cc, ext_len):
    """CSRC lists and header extensions: the header, extension included, stays in the clear and under the tag"""
    hdr = 12 + 4 * cc + (0 if ext_len is None else 4 + 4 * ext_len)
    tx, mtx = pair()
    rx, mrx = pair()
    for k, size in enumerate(s for s in SIZES + (hdr, hdr + 1) if s >= hdr):
        pkt = packet(size, 7 + k, seed=1000 * cc + size, cc=cc, ext_len=ext_len, keepalive=False)
        assert len(pkt) == size and sm.header_len(pkt) == hdr
        want, wrec = mtx.protect(pkt)
        got, grec = run(tx, pkt)
        assert got == want and grec == wrec and got[:hdr] == pkt[:hdr], (cc, ext_len, size)
        back, brec = run(rx, got, unprotect=True)
        assert back == pkt and brec == mrx.unprotect(want)[1], (cc, ext_len, size)
    same_moving(tx, mtx)
    same_moving(rx, mrx)


def test_sequence_wrap():
    """a sequence from 65 534 across the wrap: ROLLED once on each side, and the receiver follows"""
    tx, mtx = pair()
    rx, mrx = pair()
    rolled_tx = rolled_rx = 0
    for k in range(6):
        pkt = packet(172, 65534 + k, seed=k, ssrc=77)
        want, wrec = mtx.protect(pkt)
        got, grec = run(tx, pkt)
        assert got == want and grec == wrec
        back, brec = run(rx, got, unprotect=True)
        assert back == pkt and brec == mrx.unprotect(want)[1]
        rolled_tx += bool(grec["flags"] & sm.ROLLED)
        rolled_rx += bool(brec["flags"] & sm.ROLLED)
        assert grec["roc_used"] == (1 if k >= 2 else 0)
    assert rolled_tx == rolled_rx == 1 and int(tx["roc"]) == int(rx["roc"]) == 1 and int(rx["s_l"]) == 3
    same_moving(tx, mtx)
    same_moving(rx, mrx)
    # a late packet from before the wrap still authenticates with roc - 1
    old = packet(172, 65533, seed=99, ssrc=77)
    tx2, mtx2 = pair()
    want = mtx2.protect(old)[0]
    back, brec = run(rx, want, unprotect=True)
    assert back == old and brec == mrx.unprotect(want)[1] and brec["roc_used"] == 0 and int(rx["roc"]) == 1


def test_reorder_replay_and_old():
    tx, mtx = pair()
    rx, mrx = pair()
    prot = {}
    for seq in range(100, 240):
        prot[seq] = mtx.protect(packet(60, seq, seed=seq, ssrc=5))[0]
    order = [100, 103, 101, 102, 102, 110, 104, 110, 200, 199, 137, 136, 135, 200, 137, 230, 167, 166, 165, 231, 167]
    seen = []
    for seq in order:
        want, wrec = mrx.unprotect(prot[seq])
        got, grec = run(rx, prot[seq], unprotect=True, in_place=bool(seq & 1))
        assert (got, grec) == (want, wrec), seq
        same_moving(rx, mrx)
        seen.append(grec["flags"])
    f = dict(zip(range(len(order)), seen))
    assert f[4] == sm.REPLAY and f[7] == sm.REPLAY and f[13] == sm.REPLAY and f[14] == sm.REPLAY
    assert f[20] == sm.OLD                                                  # 167 was accepted, but 231 moved it out of the window: old wins over repeated
    assert f[10] == sm.OK and f[11] == sm.OLD and f[12] == sm.OLD            # 63 behind 200 is inside the window, 64 and 65 are not
    assert f[16] == sm.OK and f[17] == sm.OLD and f[18] == sm.OLD            # and again behind 230: 63, 64, 65
    assert int(rx["n_replay"]) == 9


def test_one_flipped_bit_is_an_auth_failure():
    """header, payload, tag, the SSRC, the receiver's roc: AUTH_FAIL, size 0, the output untouched, the state as before but its counter"""
    tx, mtx = pair()
    pkt = packet(180, 500, seed=1, ext_len=1)
    prot = mtx.protect(pkt)[0]
    for where in (1, 5, 8, 11, 13, 17, 25, 100, 179, 180, 185, 189):       # (bytes 0, 2 and 3 hold what the header parse and the index read)
        rx, mrx = pair()
        before = rx.tobytes()
        bad = bytearray(prot)
        bad[where] ^= 0x10
        got, grec = run(rx, bytes(bad), unprotect=True, in_place=bool(where & 1))
        assert got is None and grec == dict(flags=sm.AUTH_FAIL, size_out=0, roc_used=0) == mrx.unprotect(bytes(bad))[1], where
        after = rx.copy()
        assert int(after["n_auth_fail"]) == 1
        after["n_auth_fail"] = 0
        assert after.tobytes() == before, where
    # the sequence number's low bit: another index, so another keystream and tag
    rx, mrx = pair()
    bad = bytearray(prot)
    bad[3] ^= 1
    assert run(rx, bytes(bad), unprotect=True)[1]["flags"] == sm.AUTH_FAIL
    # the receiver's roc
    rx, mrx = pair(roc0=1)
    got, grec = run(rx, prot, unprotect=True)
    assert got is None and grec == dict(flags=sm.AUTH_FAIL, size_out=0, roc_used=1) == mrx.unprotect(prot)[1]
    same_moving(rx, mrx)
    # and the same packet is fine for the right receiver, with the 32-bit tag as well
    for tag_len in (10, 4):
        tx4, mtx4 = pair(tag_len)
        rx4, mrx4 = pair(tag_len)
        p4 = run(tx4, pkt)[0]
        bad = bytearray(p4)
        bad[-1] ^= 0x80
        assert run(rx4, bytes(bad), unprotect=True)[1]["flags"] == sm.AUTH_FAIL
        assert run(rx4, p4, unprotect=True)[0] == pkt


def test_malformed():
    good = packet(60, 9, seed=4)
    v1 = bytes([0x40 | (good[0] & 0x3F)]) + good[1:]
    short = good[:11]
    ext_past = sm.rtp(9, 1, b"", ext_len=0)[:14] + (200).to_bytes(2, "big") + bytes(40)   # ext_len 200 words in a 56-byte packet
    ext_cut = sm.rtp(9, 1, b"", ext_len=0)[:14]                                             # X set, the extension header cut off
    cc_past = bytes([0x8F]) + good[1:40]                                                    # CC 15 needs 72 bytes, the packet has 40
    for unprotect in (False, True):
        for bad in (v1, short, ext_past, ext_cut, cc_past, bytes(2049)):
            st, leg = pair()
            got, grec = run(st, bad, unprotect=unprotect, capacity=4096)
            want = (leg.unprotect if unprotect else leg.protect)(bad, out_cap=4096)
            assert got is None and grec == want[1] == dict(flags=sm.MALFORMED, size_out=0, roc_used=0), (unprotect, len(bad))
            same_moving(st, leg)
            assert int(st["n_malformed"]) == 1 and int(st["have_s_l"]) == 0
    # size + tag_len over the capacity (protect); the clear size over it (unprotect); the tag not fitting behind the header
    st, leg = pair()
    assert run(st, good, capacity=69)[1] == leg.protect(good, out_cap=69)[1] == dict(flags=sm.MALFORMED, size_out=0, roc_used=0)
    assert run(st, good, capacity=70)[1] == leg.protect(good, out_cap=70)[1] and int(st["n_ok"]) == 1
    prot = sm.Leg(KEY).protect(good)[0]
    st, leg = pair()
    assert run(st, prot, unprotect=True, capacity=59)[1] == leg.unprotect(prot, out_cap=59)[1] == dict(flags=sm.MALFORMED, size_out=0, roc_used=0)
    assert run(st, prot, unprotect=True, capacity=60)[0] == good
    st, leg = pair()
    assert run(st, good[:12 + 9], unprotect=True)[1]["flags"] == sm.MALFORMED == leg.unprotect(good[:21])[1]["flags"]


def test_empty_frames():
    for unprotect in (False, True):
        st, leg = pair()
        assert run(st, b"", unprotect=unprotect)[1] == dict(flags=sm.EMPTY, size_out=0, roc_used=0)
        same_moving(st, leg)


def test_state_of_random_bytes_is_no_key():
    rng = np.random.default_rng(8)
    pkt = packet(172, 1, seed=2)
    for i in range(50):
        raw = rng.integers(0, 256, 288, dtype=np.uint8)
        if i % 3 == 1:
            raw[:4] = np.frombuffer(np.uint32(capi.SRTP_TAG | 7).tobytes(), np.uint8)       # the constant with a tag length that is none
        if i % 3 == 2:
            raw[:4] = np.frombuffer(np.uint32((capi.SRTP_TAG ^ 0x100) | 10).tobytes(), np.uint8)
        st = np.array(raw.view(capi.SRTP_STATE)[0])
        before = st.tobytes()
        for unprotect in (False, True):
            for ctl in (sm.RUN, sm.RESET):
                got, grec = run(st, pkt, unprotect=unprotect, ctl=ctl)
                assert got is None and grec == dict(flags=sm.NO_KEY, size_out=0, roc_used=0)
                assert st.tobytes() == before


def test_bypass_and_reset():
    tx, mtx = pair()
    pkt = packet(172, 40000, seed=3)
    before = tx.tobytes()
    got, grec = run(tx, pkt, ctl=sm.BYPASS)
    assert got == pkt and grec == dict(flags=sm.BYPASSED, size_out=172, roc_used=0) == mtx.protect(pkt, ctl=sm.BYPASS)[1] and tx.tobytes() == before
    assert run(tx, pkt, unprotect=True, ctl=sm.BYPASS, in_place=True)[0] == pkt and tx.tobytes() == before
    assert run(tx, pkt, ctl=sm.BYPASS, capacity=171)[1]["flags"] == sm.MALFORMED and tx.tobytes() == before
    nokey = np.zeros((), capi.SRTP_STATE)
    assert run(nokey, pkt, ctl=sm.BYPASS)[0] == pkt                          # BYPASS needs no key
    # RESET: roc, have_s_l and the window start over, the keys stay
    rx, mrx = pair()
    prot = [mtx.protect(packet(60, 40000 + k, seed=k, ssrc=9))[0] for k in range(4)]
    for p in prot[:3]:
        assert run(rx, p, unprotect=True)[1] == mrx.unprotect(p)[1]
    assert run(rx, prot[1], unprotect=True)[1]["flags"] == sm.REPLAY == mrx.unprotect(prot[1])[1]["flags"]
    got, grec = run(rx, prot[1], unprotect=True, ctl=sm.RESET)
    assert grec == mrx.unprotect(prot[1], ctl=sm.RESET)[1] and grec["flags"] == sm.OK and int(rx["window"]) == 1 and int(rx["s_l"]) == 40001
    same_moving(rx, mrx)
    got, grec = run(rx, b"", unprotect=True, ctl=sm.RESET)                    # before the frame, whatever the frame is
    assert grec["flags"] == sm.EMPTY and int(rx["have_s_l"]) == 0 and int(rx["window"]) == 0
    mrx.unprotect(b"", ctl=sm.RESET)
    same_moving(rx, mrx)
    assert run(rx, prot[3], unprotect=True, ctl=77)[1] == mrx.unprotect(prot[3])[1]   # another value is RUN


def test_yardstick_row_is_the_entrys():
    """igdsp_internal_srtp_move takes igdsp_srtp_protect's arguments: capi.INTERNAL_MORE is that list and capi.internal finds it"""
    res, args = capi.INTERNAL_MORE["igdsp_internal_srtp_move"]
    pub = {n: (r, a) for n, r, a in capi.PROTOTYPES}["igdsp_srtp_protect"]
    assert (res, list(args)) == (pub[0], list(pub[1])) and capi.INTERNAL_MORE_TWIN["igdsp_internal_srtp_move"] == "igdsp_srtp_protect"
    assert capi.internal("srtp_move") is not None and "igdsp_internal_srtp_move" not in capi.INTERNAL
    text = open(os.path.join(ROOT, "tools", "srtp_bench.py")).read()
    assert 'capi.internal("igdsp_internal_srtp_move")' in text and ".argtypes" not in text


def test_host_mirror_leg_srtp():
    """LegSrtp (host/igdsp_host.h) through its C face: a sender and a receiver from one key, the packet vector, a replay"""
    host = ctypes.CDLL(os.path.join(ROOT, "igate4xsoftphonedsp_amd", "libigdsp_host.so"))
    vp = ctypes.c_void_p
    host.igdsp_host_srtp_new.restype = vp
    host.igdsp_host_srtp_new.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]
    host.igdsp_host_srtp_free.argtypes = [vp]
    for fn in (host.igdsp_host_srtp_protect, host.igdsp_host_srtp_unprotect):
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32]
    p = KAT["packet_sha1_80"]
    tx, rx = host.igdsp_host_srtp_new(KEY, 10, 0), host.igdsp_host_srtp_new(KEY, 10, 0)
    assert tx and rx and not host.igdsp_host_srtp_new(KEY, 7, 0)
    out, back = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    clear = bytes.fromhex(p["clear"])
    assert host.igdsp_host_srtp_protect(tx, clear, len(clear), out, 64) == 38 and out.raw[:38].hex() == p["protected"]
    assert host.igdsp_host_srtp_unprotect(rx, out.raw[:38], 38, back, 64) == 28 and back.raw[:28] == clear
    assert host.igdsp_host_srtp_unprotect(rx, out.raw[:38], 38, back, 64) == 0       # a replay: the packet did not arrive
    host.igdsp_host_srtp_free(tx)
    host.igdsp_host_srtp_free(rx)
