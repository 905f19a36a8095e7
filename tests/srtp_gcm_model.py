"""A plain Python model of the AES-GCM SRTP rule (include/igdsp.h, "SRTP with AES-GCM"): RFC 7714 with AEAD_AES_128_GCM / AEAD_AES_256_GCM
for RTP.  Independent of csrc/igdsp_srtp_gcm.h: AES-128 and AES-256 encryption are written out byte-wise from FIPS-197 (the S-box from
the field's inverse and the affine map, ShiftRows, MixColumns, the key expansion for Nk = 4 and 8), GHASH is the GCM specification's
bit-by-bit multiply on Python integers, the counter and the index are Python integers.  The header's length, the index estimate, the
window and the record's flags are tests/srtp_model.py's, imported.  tests/test_srtp_gcm_cpu.py holds this model against the standards'
known answers and packets recorded from OpenSSL (tests/golden/srtp_gcm_kat.json), against OpenSSL itself where there is one, and holds
the library's host entries against it."""
from tests import srtp_model as sm
from tests.srtp_model import (AUTH_FAIL, BYPASS, BYPASSED, EMPTY, MALFORMED, MAX_PACKET, NO_KEY, OK, OLD, REPLAY, RESET, ROLLED, RUN, WINDOW,  # noqa: F401
                              estimate, header_len, rtp)

TAG_LEN = 16
_gmul, SBOX = sm._gmul, sm._make_sbox()


# ---- AES, FIPS-197, Nk = 4 or 8
def aes_expand(key):
    """the Nr + 1 round keys of a 16- or 32-byte key, 16 bytes each"""
    nk = len(key) // 4
    assert nk in (4, 8)
    w = [list(key[4 * i:4 * i + 4]) for i in range(nk)]
    rcon = 1
    for i in range(nk, 4 * (nk + 7)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = [SBOX[t[1]] ^ rcon, SBOX[t[2]], SBOX[t[3]], SBOX[t[0]]]
            rcon = _gmul(rcon, 2)
        elif nk > 6 and i % nk == 4:
            t = [SBOX[b] for b in t]
        w.append([a ^ b for a, b in zip(w[i - nk], t)])
    return [bytes(sum(w[4 * r:4 * r + 4], [])) for r in range(nk + 7)]


def aes_encrypt(rks, block):
    """one block under len(rks) - 1 rounds; the state is column-major: byte 4 c + r is row r of column c"""
    nr = len(rks) - 1
    s = [a ^ b for a, b in zip(block, rks[0])]
    for rnd in range(1, nr + 1):
        s = [SBOX[v] for v in s]
        s = [s[4 * ((c + r) % 4) + r] for c in range(4) for r in range(4)]                       # ShiftRows
        if rnd < nr:
            m = []
            for c in range(4):
                a = s[4 * c:4 * c + 4]
                m += [_gmul(a[0], 2) ^ _gmul(a[1], 3) ^ a[2] ^ a[3], a[0] ^ _gmul(a[1], 2) ^ _gmul(a[2], 3) ^ a[3],
                      a[0] ^ a[1] ^ _gmul(a[2], 2) ^ _gmul(a[3], 3), _gmul(a[0], 3) ^ a[1] ^ a[2] ^ _gmul(a[3], 2)]
            s = m
        s = [a ^ b for a, b in zip(s, rks[rnd])]
    return bytes(s)


def aes_ctr(key, iv, n):
    """n bytes of keystream: AES_key(iv + j) for j = 0, 1, ..., iv a 128-bit integer"""
    rks = aes_expand(key)
    out = b""
    j = 0
    while len(out) < n:
        out += aes_encrypt(rks, ((iv + j) % (1 << 128)).to_bytes(16, "big"))
        j += 1
    return out[:n]


# ---- GCM: a block is a 128-bit big-endian number whose bit 0 is the most significant
R = 0xE1 << 120


def gf_mul(x, y):
    z, v = 0, y
    for i in range(128):
        if (x >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ R if v & 1 else v >> 1
    return z


def ghash(h, aad, ct):
    def blocks(b):
        b = bytes(b) + bytes(-len(b) % 16)
        return [int.from_bytes(b[i:i + 16], "big") for i in range(0, len(b), 16)]
    y = 0
    for x in blocks(aad) + blocks(ct) + [(8 * len(aad) << 64) | (8 * len(ct))]:
        y = gf_mul(y ^ x, h)
    return y


def gcm_encrypt(key, iv12, aad, plain):
    """(ciphertext, the 16-byte tag) with a 96-bit IV"""
    rks = aes_expand(key)
    h = int.from_bytes(aes_encrypt(rks, bytes(16)), "big")
    j0 = int.from_bytes(bytes(iv12) + b"\0\0\0\1", "big")
    stream = b"".join(aes_encrypt(rks, (j0 + 1 + j).to_bytes(16, "big")) for j in range(-(-len(plain) // 16)))   # (never past 2^32 blocks here)
    ct = bytes(a ^ b for a, b in zip(plain, stream))
    tag = ghash(h, aad, ct) ^ int.from_bytes(aes_encrypt(rks, j0.to_bytes(16, "big")), "big")
    return ct, tag.to_bytes(16, "big")


# ---- RFC 3711 4.3.1 at key derivation rate 0 with AES of the master key's size; the 96-bit salt times 2^16 (RFC 7714 11)
def kdf(master_key, master_salt12, label, n):
    x = (int.from_bytes(master_salt12, "big") << 16) ^ (label << 48)
    return aes_ctr(master_key, x << 16, n)


def derive(key_salt):
    """(k_e, k_s 12 bytes) from the master key (16 or 32 bytes) and the 12 bytes of master salt"""
    nk = len(key_salt) - 12
    assert nk in (16, 32)
    mk, ms = bytes(key_salt[:nk]), bytes(key_salt[nk:])
    return kdf(mk, ms, 0, nk), kdf(mk, ms, 2, 12)


class Leg(sm.Leg):
    """one leg and direction: the session keys and what moves (the index, the window, the counters and the controls are srtp_model's)"""

    def __init__(self, key_salt, roc0=0):
        self.ke, self.ks = derive(key_salt)
        self.tag_len, self.roc, self.s_l, self.have, self.window = TAG_LEN, roc0, 0, 0, 0
        self.n_ok = self.n_auth_fail = self.n_replay = self.n_malformed = 0

    def iv(self, ssrc, v, seq):
        return (int.from_bytes(self.ks, "big") ^ (ssrc << 48) ^ (v << 16) ^ seq).to_bytes(12, "big")

    def protect(self, pkt, ctl=RUN, in_cap=MAX_PACKET, out_cap=MAX_PACKET):
        pkt = bytes(pkt)
        done, h = self._open(pkt, ctl, in_cap, out_cap)
        if done is not None:
            return done
        if len(pkt) + TAG_LEN > out_cap:
            return self._refuse(MALFORMED)
        seq, s_l, v, index, top = self._index(pkt)
        ct, tag = gcm_encrypt(self.ke, self.iv(int.from_bytes(pkt[8:12], "big"), v, seq), pkt[:h], pkt[h:])
        out = pkt[:h] + ct + tag
        flags = OK
        self.n_ok += 1
        if not self.have or index > top:
            if v != self.roc:
                flags |= ROLLED
            self.roc, self.s_l, self.have = v, seq, 1
        return out, dict(flags=flags, size_out=len(out), roc_used=v)

    def unprotect(self, pkt, ctl=RUN, in_cap=MAX_PACKET, out_cap=MAX_PACKET):
        pkt = bytes(pkt)
        done, h = self._open(pkt, ctl, in_cap, out_cap)
        if done is not None:
            return done
        if len(pkt) < h + TAG_LEN or len(pkt) - TAG_LEN > out_cap:
            return self._refuse(MALFORMED)
        end = len(pkt) - TAG_LEN
        seq, s_l, v, index, top = self._index(pkt)
        ahead = not self.have or index > top
        if not ahead:
            if top - index >= WINDOW:
                return self._refuse(OLD, v)
            if (self.window >> (top - index)) & 1:
                return self._refuse(REPLAY, v)
        iv = self.iv(int.from_bytes(pkt[8:12], "big"), v, seq)
        rks = aes_expand(self.ke)
        hkey = int.from_bytes(aes_encrypt(rks, bytes(16)), "big")
        want = ghash(hkey, pkt[:h], pkt[h:end]) ^ int.from_bytes(aes_encrypt(rks, iv + b"\0\0\0\1"), "big")
        if want.to_bytes(16, "big") != pkt[end:]:
            return self._refuse(AUTH_FAIL, v)
        clear, _ = gcm_encrypt(self.ke, iv, b"", pkt[h:end])              # counter mode is its own inverse
        out = pkt[:h] + clear
        flags = OK
        self.n_ok += 1
        if ahead:
            d = index - top
            self.window = ((0 if (not self.have or d >= WINDOW) else (self.window << d)) | 1) % (1 << 64)
            if v != self.roc:
                flags |= ROLLED
            self.roc, self.s_l, self.have = v, seq, 1
        else:
            self.window |= 1 << (top - index)
        return out, dict(flags=flags, size_out=len(out), roc_used=v)
