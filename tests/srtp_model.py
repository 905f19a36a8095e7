"""A plain Python model of the SRTP rule (include/igdsp.h, "SRTP"): RFC 3711 with AES_CM_128_HMAC_SHA1_80 / _32 for RTP.  Independent of
csrc/igdsp_srtp.h: AES-128 encryption is written out byte-wise from FIPS-197 (S-box from the field's inverse and the affine map,
ShiftRows, MixColumns, the key expansion), the tag comes from the standard library's hmac / hashlib, the counter and the index are
Python integers.  tests/test_srtp_cpu.py holds it against the standards' known answers (tests/golden/srtp_kat.json), against OpenSSL
where there is one, and holds the library's host entries against it."""
import hashlib
import hmac

RUN, BYPASS, RESET = 0, 1, 2
NO_KEY, OK, AUTH_FAIL, REPLAY, OLD, MALFORMED, EMPTY, ROLLED, BYPASSED = 0, 1, 2, 4, 8, 16, 32, 64, 128
MAX_PACKET, WINDOW = 2048, 64


# ---- AES-128, FIPS-197
def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = ((a << 1) ^ 0x11B) if a & 0x80 else a << 1
        b >>= 1
    return r


def _make_sbox():
    box = []
    for x in range(256):
        inv = next((y for y in range(1, 256) if _gmul(x, y) == 1), 0)
        s = inv
        for k in range(1, 5):
            s ^= ((inv << k) | (inv >> (8 - k))) & 0xFF
        box.append(s ^ 0x63)
    return box


SBOX = _make_sbox()


def aes_expand(key):
    """the 11 round keys of a 16-byte key, 16 bytes each"""
    w = [list(key[4 * i:4 * i + 4]) for i in range(4)]
    rcon = 1
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [SBOX[t[1]] ^ rcon, SBOX[t[2]], SBOX[t[3]], SBOX[t[0]]]
            rcon = _gmul(rcon, 2)
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    return [bytes(sum(w[4 * r:4 * r + 4], [])) for r in range(11)]


def aes_encrypt(rks, block):
    """one block; the state is column-major: byte 4 c + r is row r of column c"""
    s = [a ^ b for a, b in zip(block, rks[0])]
    for rnd in range(1, 11):
        s = [SBOX[v] for v in s]
        s = [s[4 * ((c + r) % 4) + r] for c in range(4) for r in range(4)]                       # ShiftRows
        if rnd < 10:
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


# ---- RFC 3711 4.3.1 at key derivation rate 0
def kdf(master_key, master_salt, label, n):
    x = int.from_bytes(master_salt, "big") ^ (label << 48)
    return aes_ctr(master_key, x << 16, n)


def derive(key_salt):
    """(k_e 16 bytes, k_a 20, k_s 14) from the 30 bytes of master key and salt"""
    mk, ms = bytes(key_salt[:16]), bytes(key_salt[16:30])
    return kdf(mk, ms, 0, 16), kdf(mk, ms, 1, 20), kdf(mk, ms, 2, 14)


def header_len(pkt):
    """h, or None for a malformed packet (the checks of the size against 12 and the caps are the caller's)"""
    size = len(pkt)
    if size < 12 or pkt[0] >> 6 != 2:
        return None
    h = 12 + 4 * (pkt[0] & 15)
    if h > size:
        return None
    if pkt[0] & 0x10:
        if h + 4 > size:
            return None
        h += 4 + 4 * int.from_bytes(pkt[h + 2:h + 4], "big")
        if h > size:
            return None
    return h


def estimate(roc, s_l, seq):
    """RFC 3711 Appendix A, as written"""
    if s_l < 32768:
        v = roc - 1 if seq - s_l > 32768 else roc
    else:
        v = roc + 1 if s_l - 32768 > seq else roc
    return v % (1 << 32)


class Leg:
    """one leg and direction: the session keys and what moves"""

    def __init__(self, key_salt, tag_len=10, roc0=0):
        assert tag_len in (4, 10)
        self.ke, self.ka, self.ks = derive(key_salt)
        self.tag_len, self.roc, self.s_l, self.have, self.window = tag_len, roc0, 0, 0, 0
        self.n_ok = self.n_auth_fail = self.n_replay = self.n_malformed = 0

    def moving(self):
        return dict(roc=self.roc, s_l=self.s_l, have_s_l=self.have, window=self.window, n_ok=self.n_ok, n_auth_fail=self.n_auth_fail,
                    n_replay=self.n_replay, n_malformed=self.n_malformed)

    def keystream(self, ssrc, index, n):
        iv = (int.from_bytes(self.ks, "big") << 16) ^ (ssrc << 64) ^ (index << 16)
        return aes_ctr(self.ke, iv, n)

    def tag(self, data, v):
        return hmac.new(self.ka, bytes(data) + v.to_bytes(4, "big"), hashlib.sha1).digest()[:self.tag_len]

    def _refuse(self, flags, v=0):
        if flags & AUTH_FAIL:
            self.n_auth_fail += 1
        elif flags & (REPLAY | OLD):
            self.n_replay += 1
        elif flags & MALFORMED:
            self.n_malformed += 1
        return None, dict(flags=flags, size_out=0, roc_used=v)

    def _open(self, pkt, ctl, in_cap, out_cap):
        """what both directions do first: (result or None, h)"""
        size = len(pkt)
        fits = size <= MAX_PACKET and size <= in_cap
        if ctl == BYPASS:
            if size == 0:
                return (None, dict(flags=EMPTY, size_out=0, roc_used=0)), None
            if not fits or size > out_cap:
                return (None, dict(flags=MALFORMED, size_out=0, roc_used=0)), None
            return (bytes(pkt), dict(flags=BYPASSED, size_out=size, roc_used=0)), None
        if ctl == RESET:
            self.roc, self.have, self.window = 0, 0, 0
        if size == 0:
            return (None, dict(flags=EMPTY, size_out=0, roc_used=0)), None
        h = header_len(pkt) if fits else None
        if h is None:
            return self._refuse(MALFORMED), None
        return None, h

    def _index(self, pkt):
        seq = int.from_bytes(pkt[2:4], "big")
        s_l = self.s_l if self.have else seq
        v = estimate(self.roc, s_l, seq)
        return seq, s_l, v, (v << 16) | seq, (self.roc << 16) | s_l

    def protect(self, pkt, ctl=RUN, in_cap=MAX_PACKET, out_cap=MAX_PACKET):
        """-> (the protected packet or None, dict(flags, size_out, roc_used))"""
        pkt = bytes(pkt)
        done, h = self._open(pkt, ctl, in_cap, out_cap)
        if done is not None:
            return done
        if len(pkt) + self.tag_len > out_cap:
            return self._refuse(MALFORMED)
        seq, s_l, v, index, top = self._index(pkt)
        ssrc = int.from_bytes(pkt[8:12], "big")
        body = pkt[:h] + bytes(a ^ b for a, b in zip(pkt[h:], self.keystream(ssrc, index, len(pkt) - h)))
        out = body + self.tag(body, v)
        flags = OK
        self.n_ok += 1
        if not self.have or index > top:
            if v != self.roc:
                flags |= ROLLED
            self.roc, self.s_l, self.have = v, seq, 1
        return out, dict(flags=flags, size_out=len(out), roc_used=v)

    def unprotect(self, pkt, ctl=RUN, in_cap=MAX_PACKET, out_cap=MAX_PACKET):
        """-> (the clear packet or None, dict(flags, size_out, roc_used))"""
        pkt = bytes(pkt)
        done, h = self._open(pkt, ctl, in_cap, out_cap)
        if done is not None:
            return done
        if len(pkt) < h + self.tag_len or len(pkt) - self.tag_len > out_cap:
            return self._refuse(MALFORMED)
        end = len(pkt) - self.tag_len
        seq, s_l, v, index, top = self._index(pkt)
        ahead = not self.have or index > top
        if not ahead:
            if top - index >= WINDOW:
                return self._refuse(OLD, v)
            if (self.window >> (top - index)) & 1:
                return self._refuse(REPLAY, v)
        if not hmac.compare_digest(self.tag(pkt[:end], v), pkt[end:]):
            return self._refuse(AUTH_FAIL, v)
        ssrc = int.from_bytes(pkt[8:12], "big")
        out = pkt[:h] + bytes(a ^ b for a, b in zip(pkt[h:end], self.keystream(ssrc, index, end - h)))
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


def rtp(seq, ssrc, payload, cc=0, ext_len=None, pt=8, ts=0, version=2, ext_words=None):
    """an RTP packet: cc CSRCs, with ext_len not None a header extension of ext_len words (ext_words: its bytes, default a counting pattern)"""
    b0 = (version << 6) | (0x10 if ext_len is not None else 0) | cc
    out = bytes([b0, pt]) + (seq % 65536).to_bytes(2, "big") + (ts % (1 << 32)).to_bytes(4, "big") + (ssrc % (1 << 32)).to_bytes(4, "big")
    out += bytes((7 * i + 1) % 256 for i in range(4 * cc))
    if ext_len is not None:
        body = bytes((5 * i + 3) % 256 for i in range(4 * ext_len)) if ext_words is None else bytes(ext_words)
        out += b"\x01\x67" + ext_len.to_bytes(2, "big") + body
    return out + bytes(payload)
