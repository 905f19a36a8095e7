"""-m "not gpu": SRTP with AES-GCM (include/igdsp.h, "SRTP with AES-GCM").  tests/srtp_gcm_model.py against the standards' known answers
and the packets recorded from OpenSSL (tests/golden/srtp_gcm_kat.json: FIPS-197 C.3, the GCM specification's test cases 1, 2 and 14,
thirty whole packets) and, where there is an OpenSSL, against its GCM on seeded random packets and its AES-CTR under the model's key
derivation; then the library's host entries (igdsp_srtp_gcm_derive, igdsp_srtp_gcm_protect_packet, igdsp_srtp_gcm_unprotect_packet)
against the model, byte for byte: payload lengths on either side of a block, headers of 12, 20, 24 bytes and one that reaches into the
packet's second 64 bytes, both key sizes, the round trip, the sequence wrap (the rollover counter enters the IV), reordering / repeats /
old packets against the window, one flipped bit anywhere, the malformed packets, a state of random bytes, the states of the other suites
(both directions), BYPASS and RESET, in place, and that nothing behind size_out is ever written; LegSrtpGcm through its C face."""
import ctypes
import ctypes.util
import json
import os

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import srtp_gcm_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "srtp_gcm_kat.json")))
PAYLOADS = (0, 1, 15, 16, 17, 31, 32, 33, 160)
HEADERS = ((0, None), (0, 1), (3, None), (15, 2))                           # (CSRCs, extension words): 12, 20, 24 and 12 + 60 + 4 + 8 = 84 bytes
KEYS = {16: bytes(range(0x40, 0x40 + 28)), 32: bytes(range(0x80, 0x80 + 44))}
MOVING = ("roc", "s_l", "have_s_l", "window", "n_ok", "n_auth_fail", "n_replay", "n_malformed")
FILL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def lib():
    igbuild.build()
    return capi.load()


def packet(pay, seq, seed, cc=0, ext_len=None, ssrc=None):
    rng = np.random.default_rng(seed)
    return gm.rtp(seq, int(rng.integers(0, 1 << 32)) if ssrc is None else ssrc, rng.integers(0, 256, pay, dtype=np.uint8).tobytes(), cc=cc, ext_len=ext_len,
                  ts=int(rng.integers(0, 1 << 32)))


def run(state, pkt, unprotect=False, ctl=gm.RUN, capacity=2048, in_place=False, fn=None):
    """the library on one packet: (bytes out or None, dict like the model's); checks that nothing at or behind size_out was written"""
    out, n, rec = (fn or capi.srtp_gcm_packet)(state, pkt, unprotect=unprotect, ctl=ctl, capacity=capacity, in_place=in_place, fill=FILL)
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


def pair(kb=16, roc0=0):
    return capi.srtp_gcm_derive(KEYS[kb], roc0=roc0), gm.Leg(KEYS[kb], roc0)


def openssl():
    name = ctypes.util.find_library("crypto")
    if not name:
        pytest.skip("no OpenSSL libcrypto on this machine")
    ssl = ctypes.CDLL(name)
    vp = ctypes.c_void_p
    ssl.EVP_CIPHER_CTX_new.restype = vp
    for n in ("EVP_aes_128_ctr", "EVP_aes_256_ctr", "EVP_aes_128_gcm", "EVP_aes_256_gcm"):
        getattr(ssl, n).restype = vp
    ssl.EVP_EncryptInit_ex.argtypes = [vp, vp, vp, ctypes.c_char_p, ctypes.c_char_p]
    ssl.EVP_EncryptUpdate.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]
    ssl.EVP_EncryptFinal_ex.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    ssl.EVP_CIPHER_CTX_ctrl.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
    ssl.EVP_CIPHER_CTX_free.argtypes = [vp]
    return ssl


# ---- the model against the standards and the recorded packets
def test_model_fips197_c3():
    f = KAT["fips197_c3"]
    rks = gm.aes_expand(bytes.fromhex(f["key"]))
    assert len(rks) == 15 and gm.aes_encrypt(rks, bytes.fromhex(f["plaintext"])).hex() == f["ciphertext"]


@pytest.mark.parametrize("case", ("1", "2", "14"))
def test_model_gcm_specification(case):
    g = KAT["gcm_spec_case_" + case]
    ct, tag = gm.gcm_encrypt(bytes.fromhex(g["key"]), bytes.fromhex(g["iv"]), bytes.fromhex(g["aad"]), bytes.fromhex(g["plaintext"]))
    assert (ct.hex(), tag.hex()) == (g["ciphertext"], g["tag"])


def test_model_and_library_recorded_packets():
    """thirty packets recorded from OpenSSL: both key sizes, 12-, 20- and 24-byte headers, payloads of 0, 1, 16, 17 and 160 bytes"""
    pk = KAT["packets"]["list"]
    assert {(p["key_bytes"], p["header"], p["payload"]) for p in pk} == {(k, h, n) for k in (16, 32) for h in (12, 20, 24) for n in (0, 1, 16, 17, 160)}
    for p in pk:
        ks, clear, what = bytes.fromhex(p["master_key_salt"]), bytes.fromhex(p["clear"]), (p["key_bytes"], p["header"], p["payload"])
        leg = gm.Leg(ks, p["roc"])
        assert (leg.ke.hex(), leg.ks.hex()) == (p["k_e"], p["k_s"]), what
        out, rec = leg.protect(clear)
        assert out.hex() == p["protected"] and rec == dict(flags=gm.OK, size_out=len(clear) + 16, roc_used=p["roc"]), what
        st = capi.srtp_gcm_derive(ks, roc0=p["roc"])
        assert int(st["tag"]) == capi.SRTP_GCM_TAG | p["key_bytes"] and st["salt"].tobytes().hex() == p["k_s"]
        assert b"".join(int(w).to_bytes(4, "big") for w in st["rk"][:p["key_bytes"] // 4]).hex() == p["k_e"]   # the schedule's first words are k_e
        got, grec = run(st, clear)
        assert got.hex() == p["protected"] and grec == rec, what
        back, brec = run(capi.srtp_gcm_derive(ks, roc0=p["roc"]), got, unprotect=True)
        assert back == clear and brec["flags"] == gm.OK, what


def test_model_gcm_against_openssl():
    ssl = openssl()
    rng = np.random.default_rng(7714)
    for i in range(24):
        kb, aad_n, n = (16, 32)[i & 1], (12, 20, 24, 84, 13, 0)[i % 6], (0, 1, 15, 16, 17, 160, 333, 2000)[i % 8]
        key, iv = rng.integers(0, 256, kb, dtype=np.uint8).tobytes(), rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
        aad, plain = rng.integers(0, 256, aad_n, dtype=np.uint8).tobytes(), rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        c = ssl.EVP_CIPHER_CTX_new()
        assert ssl.EVP_EncryptInit_ex(c, ssl.EVP_aes_128_gcm() if kb == 16 else ssl.EVP_aes_256_gcm(), None, None, None) == 1
        assert ssl.EVP_CIPHER_CTX_ctrl(c, 0x9, 12, None) == 1 and ssl.EVP_EncryptInit_ex(c, None, None, key, iv) == 1     # EVP_CTRL_AEAD_SET_IVLEN
        got, out, fin, tag = ctypes.c_int(0), ctypes.create_string_buffer(n + 32), ctypes.create_string_buffer(32), ctypes.create_string_buffer(16)
        assert not aad or ssl.EVP_EncryptUpdate(c, None, ctypes.byref(got), aad, len(aad)) == 1
        assert not plain or (ssl.EVP_EncryptUpdate(c, out, ctypes.byref(got), plain, n) == 1 and got.value == n)
        assert ssl.EVP_EncryptFinal_ex(c, fin, ctypes.byref(got)) == 1 and ssl.EVP_CIPHER_CTX_ctrl(c, 0x10, 16, ctypes.cast(tag, ctypes.c_void_p)) == 1   # _GET_TAG
        ssl.EVP_CIPHER_CTX_free(c)
        assert gm.gcm_encrypt(key, iv, aad, plain) == (out.raw[:n], tag.raw), (kb, aad_n, n)


def test_model_kdf_keystream_against_openssl():
    """the model's key derivation is AES-CM of the master key's own size over (salt || 00 00) xor label 2^48, times 2^16"""
    ssl = openssl()
    rng = np.random.default_rng(3711)
    for kb in (16, 32):
        for label, n in ((0, kb), (2, 12), (0, 100)):
            mk, ms = rng.integers(0, 256, kb, dtype=np.uint8).tobytes(), rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
            x = bytearray(ms + b"\0\0")
            x[7] ^= label
            c = ssl.EVP_CIPHER_CTX_new()
            assert ssl.EVP_EncryptInit_ex(c, ssl.EVP_aes_128_ctr() if kb == 16 else ssl.EVP_aes_256_ctr(), None, mk, bytes(x) + b"\0\0") == 1
            out, got = ctypes.create_string_buffer(n + 32), ctypes.c_int(0)
            assert ssl.EVP_EncryptUpdate(c, out, ctypes.byref(got), bytes(n), n) == 1 and got.value == n
            ssl.EVP_CIPHER_CTX_free(c)
            assert gm.kdf(mk, ms, label, n) == out.raw[:n], (kb, label, n)


# ---- the library against the model
def test_library_derive():
    for kb in (16, 32):
        st, leg = pair(kb, roc0=7)
        assert int(st["tag"]) == capi.SRTP_GCM_TAG | kb and int(st["roc"]) == 7 and st["salt"].tobytes() == leg.ks
        nw = 4 * (kb // 4 + 7)
        assert b"".join(int(w).to_bytes(4, "big") for w in st["rk"][:nw]) == b"".join(gm.aes_expand(leg.ke)) and not st["rk"][nw:].any()
        assert st["h"].tobytes() == gm.aes_encrypt(gm.aes_expand(leg.ke), bytes(16))
    for bad in (0, 8, 15, 17, 24, 31, 33, 64):
        assert capi.srtp_gcm_derive(bytes(76), bad, raw=True) == -22
    assert capi.SRTP_GCM_STATE.itemsize == 320
    assert len({capi.SRTP_GCM_TAG >> 8, capi.SRTP_TAG >> 8, 0x53524300 >> 8}) == 3


@pytest.mark.parametrize("kb", (16, 32))
@pytest.mark.parametrize("cc,ext_len", HEADERS)
def test_payloads_and_headers_round_trip_against_model(kb, cc, ext_len):
    """every payload length under every header, both directions, out of place and in place: bytes, records, the state's moving fields"""
    hdr = 12 + 4 * cc + (0 if ext_len is None else 4 + 4 * ext_len)
    tx, mtx = pair(kb)
    rx, mrx = pair(kb)
    for k, pay in enumerate(PAYLOADS):
        pkt = packet(pay, 1000 + k, seed=100 * hdr + pay, cc=cc, ext_len=ext_len)
        assert len(pkt) == hdr + pay and gm.header_len(pkt) == hdr
        want, wrec = mtx.protect(pkt)
        got, grec = run(tx, pkt, in_place=bool(k & 1))
        assert got == want and grec == wrec and len(got) == hdr + pay + 16 and got[:hdr] == pkt[:hdr], (hdr, pay)
        same_moving(tx, mtx)
        clear, crec = mrx.unprotect(want)
        back, brec = run(rx, got, unprotect=True, in_place=not (k & 1))
        assert back == clear == pkt and brec == crec, (hdr, pay)
        same_moving(rx, mrx)
    assert int(tx["n_ok"]) == int(rx["n_ok"]) == len(PAYLOADS)


def test_largest_packet():
    tx, mtx = pair(32)
    pkt = packet(2032 - 12, 5, seed=9)
    want, wrec = mtx.protect(pkt)
    got, grec = run(tx, pkt)
    assert got == want and grec == wrec and len(got) == 2048
    assert run(pair(32)[0], got, unprotect=True)[0] == pkt
    assert run(pair(32)[0], packet(2033 - 12, 5, seed=9))[1]["flags"] == gm.MALFORMED     # the tag would pass 2048


def test_sequence_wrap_and_roc_in_the_iv():
    tx, mtx = pair()
    rx, mrx = pair()
    rolled_tx = rolled_rx = 0
    for k in range(6):
        pkt = packet(160, 65534 + k, seed=k, ssrc=77)
        want, wrec = mtx.protect(pkt)
        got, grec = run(tx, pkt)
        assert got == want and grec == wrec
        back, brec = run(rx, got, unprotect=True)
        assert back == pkt and brec == mrx.unprotect(want)[1]
        rolled_tx += bool(grec["flags"] & gm.ROLLED)
        rolled_rx += bool(brec["flags"] & gm.ROLLED)
        assert grec["roc_used"] == (1 if k >= 2 else 0)
    assert rolled_tx == rolled_rx == 1 and int(tx["roc"]) == int(rx["roc"]) == 1 and int(rx["s_l"]) == 3
    same_moving(tx, mtx)
    same_moving(rx, mrx)
    # a packet protected at roc 1 fails under roc 0, and passes under roc 1
    pkt = packet(40, 9, seed=1, ssrc=77)
    prot = gm.Leg(KEYS[16], roc0=1).protect(pkt)[0]
    rx0, mrx0 = pair(roc0=0)
    got, grec = run(rx0, prot, unprotect=True)
    assert got is None and grec == dict(flags=gm.AUTH_FAIL, size_out=0, roc_used=0) == mrx0.unprotect(prot)[1]
    assert run(pair(roc0=1)[0], prot, unprotect=True)[0] == pkt


def test_reorder_replay_and_old():
    rx, mrx = pair(32)
    mtx = gm.Leg(KEYS[32])
    prot = {seq: mtx.protect(packet(24, seq, seed=seq, ssrc=5))[0] for seq in range(100, 240)}
    order = [100, 103, 101, 102, 102, 110, 104, 110, 200, 199, 137, 136, 135, 200, 137, 230, 167, 166, 165, 231, 167]
    seen = []
    for seq in order:
        want, wrec = mrx.unprotect(prot[seq])
        got, grec = run(rx, prot[seq], unprotect=True, in_place=bool(seq & 1))
        assert (got, grec) == (want, wrec), seq
        same_moving(rx, mrx)
        seen.append(grec["flags"])
    assert [seen[i] for i in (4, 7, 13, 14)] == [gm.REPLAY] * 4 and seen[20] == gm.OLD
    assert seen[10:13] == [gm.OK, gm.OLD, gm.OLD] and seen[16:19] == [gm.OK, gm.OLD, gm.OLD]
    assert int(rx["n_replay"]) == 9


@pytest.mark.parametrize("kb", (16, 32))
def test_one_flipped_bit_is_an_auth_failure(kb):
    """header (the AAD), payload, tag: AUTH_FAIL, size 0, the output untouched, the state as before but its counter"""
    mtx = gm.Leg(KEYS[kb])
    pkt = packet(160, 500, seed=1, ext_len=1)                               # 20-byte header, 196 bytes protected
    prot = mtx.protect(pkt)[0]
    for where in (1, 4, 5, 8, 11, 12, 13, 17, 19, 20, 25, 100, 179, 180, 185, 195):   # (bytes 0, 2, 3 and 14, 15 hold what the header parse and the index read)
        rx, mrx = pair(kb)
        before = rx.tobytes()
        bad = bytearray(prot)
        bad[where] ^= 0x10
        got, grec = run(rx, bytes(bad), unprotect=True, in_place=bool(where & 1))
        assert got is None and grec == dict(flags=gm.AUTH_FAIL, size_out=0, roc_used=0) == mrx.unprotect(bytes(bad))[1], where
        after = rx.copy()
        assert int(after["n_auth_fail"]) == 1
        after["n_auth_fail"] = 0
        assert after.tobytes() == before, where
    rx, mrx = pair(kb)
    bad = bytearray(prot)
    bad[3] ^= 1                                                            # the sequence number's low bit: another IV, and another AAD
    assert run(rx, bytes(bad), unprotect=True)[1]["flags"] == gm.AUTH_FAIL
    assert run(rx, prot, unprotect=True)[0] == pkt


def test_malformed():
    good = packet(48, 9, seed=4)
    v1 = bytes([0x40 | (good[0] & 0x3F)]) + good[1:]
    short = good[:11]
    ext_past = gm.rtp(9, 1, b"", ext_len=0)[:14] + (200).to_bytes(2, "big") + bytes(40)   # ext_len 200 words in a 56-byte packet
    ext_cut = gm.rtp(9, 1, b"", ext_len=0)[:14]                                             # X set, the extension header cut off
    cc_past = bytes([0x8F]) + good[1:40]                                                    # CC 15 needs 72 bytes, the packet has 40
    for unprotect in (False, True):
        for bad in (v1, short, ext_past, ext_cut, cc_past, bytes(2049)):
            st, leg = pair()
            got, grec = run(st, bad, unprotect=unprotect, capacity=4096)
            want = (leg.unprotect if unprotect else leg.protect)(bad, out_cap=4096)
            assert got is None and grec == want[1] == dict(flags=gm.MALFORMED, size_out=0, roc_used=0), (unprotect, len(bad))
            same_moving(st, leg)
            assert int(st["n_malformed"]) == 1 and int(st["have_s_l"]) == 0
    # size + 16 over the capacity (protect); the clear size over it (unprotect); the tag not fitting behind the header
    st, leg = pair()
    assert run(st, good, capacity=75)[1] == leg.protect(good, out_cap=75)[1] == dict(flags=gm.MALFORMED, size_out=0, roc_used=0)
    assert run(st, good, capacity=76)[1] == leg.protect(good, out_cap=76)[1] and int(st["n_ok"]) == 1
    prot = gm.Leg(KEYS[16]).protect(good)[0]
    st, leg = pair()
    assert run(st, prot, unprotect=True, capacity=59)[1] == leg.unprotect(prot, out_cap=59)[1] == dict(flags=gm.MALFORMED, size_out=0, roc_used=0)
    assert run(st, prot, unprotect=True, capacity=60)[0] == good
    st, leg = pair()
    assert run(st, good[:12 + 15], unprotect=True)[1]["flags"] == gm.MALFORMED == leg.unprotect(good[:27])[1]["flags"]
    # an empty payload is legal: the tag alone behind the header
    st, leg = pair()
    bare = leg.protect(good[:12])[0]
    assert len(bare) == 28 and run(st, bare, unprotect=True)[0] == good[:12]


def test_empty_frames():
    for unprotect in (False, True):
        st, leg = pair()
        assert run(st, b"", unprotect=unprotect)[1] == dict(flags=gm.EMPTY, size_out=0, roc_used=0)
        same_moving(st, leg)


def test_state_of_random_bytes_is_no_key():
    rng = np.random.default_rng(8)
    pkt = packet(160, 1, seed=2)
    for i in range(50):
        raw = rng.integers(0, 256, 320, dtype=np.uint8)
        if i % 3 == 1:
            raw[:4] = np.frombuffer(np.uint32(capi.SRTP_GCM_TAG | 24).tobytes(), np.uint8)       # the constant with a key size that is none
        if i % 3 == 2:
            raw[:4] = np.frombuffer(np.uint32((capi.SRTP_GCM_TAG ^ 0x100) | 16).tobytes(), np.uint8)
        st = np.array(raw.view(capi.SRTP_GCM_STATE)[0])
        before = st.tobytes()
        for unprotect in (False, True):
            for ctl in (gm.RUN, gm.RESET):
                got, grec = run(st, pkt, unprotect=unprotect, ctl=ctl)
                assert got is None and grec == dict(flags=gm.NO_KEY, size_out=0, roc_used=0)
                assert st.tobytes() == before


def test_cross_suite_states_are_no_key_both_directions():
    """a state of one suite is NO_KEY to the other suites' entries: the GCM entries refuse SRTP and SRTCP states, the SRTP and SRTCP
    entries refuse a GCM state, whatever the key size; nothing is written and the state stays as it was"""
    pkt = packet(160, 1, seed=2)
    key30 = bytes(range(30))
    for foreign in (capi.srtp_derive(key30, 10), capi.srtp_derive(key30, 4), capi.srtcp_derive(key30)):
        raw = np.zeros(320, np.uint8)
        raw[:288] = np.frombuffer(foreign.tobytes(), np.uint8)
        st = np.array(raw.view(capi.SRTP_GCM_STATE)[0])
        before = st.tobytes()
        for unprotect in (False, True):
            assert run(st, pkt, unprotect=unprotect) == (None, dict(flags=gm.NO_KEY, size_out=0, roc_used=0)) and st.tobytes() == before
    rtcp = bytes([0x80, 200, 0, 6]) + bytes(24)
    for kb in (16, 32):
        gcm = capi.srtp_gcm_derive(KEYS[kb])
        st = np.frombuffer(gcm.tobytes()[:288], capi.SRTP_STATE).copy().reshape(())
        before = st.tobytes()
        for unprotect in (False, True):
            assert run(st, pkt, unprotect=unprotect, fn=capi.srtp_packet) == (None, dict(flags=gm.NO_KEY, size_out=0, roc_used=0)) and st.tobytes() == before
            assert run(st, rtcp + bytes(14) * unprotect, unprotect=unprotect, fn=capi.srtcp_packet) == (None, dict(flags=gm.NO_KEY, size_out=0, roc_used=0))
            assert st.tobytes() == before


def test_bypass_and_reset():
    tx, mtx = pair()
    pkt = packet(160, 40000, seed=3)
    before = tx.tobytes()
    got, grec = run(tx, pkt, ctl=gm.BYPASS)
    assert got == pkt and grec == dict(flags=gm.BYPASSED, size_out=172, roc_used=0) == mtx.protect(pkt, ctl=gm.BYPASS)[1] and tx.tobytes() == before
    assert run(tx, pkt, unprotect=True, ctl=gm.BYPASS, in_place=True)[0] == pkt and tx.tobytes() == before
    assert run(tx, pkt, ctl=gm.BYPASS, capacity=171)[1]["flags"] == gm.MALFORMED and tx.tobytes() == before
    nokey = np.zeros((), capi.SRTP_GCM_STATE)
    assert run(nokey, pkt, ctl=gm.BYPASS)[0] == pkt                          # BYPASS needs no key
    # RESET: roc, have_s_l and the window start over, the keys stay
    rx, mrx = pair()
    prot = [mtx.protect(packet(48, 40000 + k, seed=k, ssrc=9))[0] for k in range(4)]
    for p in prot[:3]:
        assert run(rx, p, unprotect=True)[1] == mrx.unprotect(p)[1]
    assert run(rx, prot[1], unprotect=True)[1]["flags"] == gm.REPLAY == mrx.unprotect(prot[1])[1]["flags"]
    got, grec = run(rx, prot[1], unprotect=True, ctl=gm.RESET)
    assert grec == mrx.unprotect(prot[1], ctl=gm.RESET)[1] and grec["flags"] == gm.OK and int(rx["window"]) == 1 and int(rx["s_l"]) == 40001
    same_moving(rx, mrx)
    got, grec = run(rx, b"", unprotect=True, ctl=gm.RESET)                    # before the frame, whatever the frame is
    assert grec["flags"] == gm.EMPTY and int(rx["have_s_l"]) == 0 and int(rx["window"]) == 0
    mrx.unprotect(b"", ctl=gm.RESET)
    same_moving(rx, mrx)
    assert run(rx, prot[3], unprotect=True, ctl=77)[1] == mrx.unprotect(prot[3])[1]   # another value is RUN


def test_yardstick_row_is_the_entrys():
    """igdsp_internal_srtp_gcm_move takes igdsp_srtp_gcm_protect's arguments: capi.INTERNAL_MORE is that list and capi.internal finds it"""
    res, args = capi.INTERNAL_MORE["igdsp_internal_srtp_gcm_move"]
    pub = {n: (r, a) for n, r, a in capi.PROTOTYPES}["igdsp_srtp_gcm_protect"]
    assert (res, list(args)) == (pub[0], list(pub[1])) and capi.INTERNAL_MORE_TWIN["igdsp_internal_srtp_gcm_move"] == "igdsp_srtp_gcm_protect"
    assert capi.internal("srtp_gcm_move") is not None and "igdsp_internal_srtp_gcm_move" not in capi.INTERNAL
    text = open(os.path.join(ROOT, "tools", "srtp_gcm_bench.py")).read()
    assert 'capi.internal("igdsp_internal_srtp_gcm_move")' in text and ".argtypes" not in text


def test_host_mirror_leg_srtp_gcm():
    """LegSrtpGcm (host/igdsp_host.h) through its C face: a sender and a receiver from one key, a recorded packet, a replay"""
    host = ctypes.CDLL(os.path.join(ROOT, "igate4xsoftphonedsp_amd", "libigdsp_host.so"))
    vp = ctypes.c_void_p
    host.igdsp_host_srtp_gcm_new.restype = vp
    host.igdsp_host_srtp_gcm_new.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]
    host.igdsp_host_srtp_gcm_free.argtypes = [vp]
    for fn in (host.igdsp_host_srtp_gcm_protect, host.igdsp_host_srtp_gcm_unprotect):
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32]
    host.igdsp_host_srtp_gcm_rec.argtypes = [vp, vp]
    for kb in (16, 32):
        p = next(q for q in KAT["packets"]["list"] if (q["key_bytes"], q["header"], q["payload"]) == (kb, 20, 160))
        ks, clear, n = bytes.fromhex(p["master_key_salt"]), bytes.fromhex(p["clear"]), 196
        tx, rx = host.igdsp_host_srtp_gcm_new(ks, kb, p["roc"]), host.igdsp_host_srtp_gcm_new(ks, kb, p["roc"])
        assert tx and rx and not host.igdsp_host_srtp_gcm_new(ks, 24, 0) and not host.igdsp_host_srtp_gcm_new(None, kb, 0)
        out, back = ctypes.create_string_buffer(256), ctypes.create_string_buffer(256)
        assert host.igdsp_host_srtp_gcm_protect(tx, clear, len(clear), out, 256) == n and out.raw[:n].hex() == p["protected"]
        assert host.igdsp_host_srtp_gcm_unprotect(rx, out.raw[:n], n, back, 256) == 180 and back.raw[:180] == clear
        assert host.igdsp_host_srtp_gcm_unprotect(rx, out.raw[:n], n, back, 256) == 0   # a replay: the packet did not arrive
        rec = np.zeros((), capi.SRTP_REC)
        assert host.igdsp_host_srtp_gcm_rec(rx, rec.ctypes.data_as(vp)) == 0 and int(rec["flags"]) == gm.REPLAY
        host.igdsp_host_srtp_gcm_free(tx)
        host.igdsp_host_srtp_gcm_free(rx)
