"""A plain Python model of the RTCP / SRTCP rule (include/igdsp.h, "RTCP / SRTCP").  Independent of csrc/igdsp_rtcp.h: packets are built
and taken apart with struct from RFC 3550's figures (6.4.1 SR, 6.4.2 RR, 6.5 SDES, 6.6 BYE) by offsets and slices, not a word at a
time; the report block is RFC 3550 A.3 in Python integers; SRTCP (RFC 3711 3.4) uses tests/srtp_model.py's byte-wise AES and the
standard library's hmac.  tests/test_rtcp_cpu.py holds the library's host entries against it."""
import hashlib
import hmac
import struct

from tests import srtp_model as sm

NONE, REPORT, BYE = 0, 1, 2
SR, RR, HAS_BLOCK, BYE_SENT = 1, 2, 4, 8
HAVE_SR, PEER_VALID, RTT_VALID, BYE_SEEN = 1, 2, 4, 8
PARSED, MALFORMED, EMPTY, GOT_SR, GOT_BLOCK, GOT_RTT, RTT_NEGATIVE, GOT_BYE = 1, 2, 4, 8, 16, 32, 64, 128
JB_HEARD = 1
M32 = 0xFFFFFFFF


class Leg:
    """one leg's igdsp_rtcp_state as attributes"""

    FIELDS = ("sent_prior", "n_built", "lsr", "lsr_arrival", "flags", "n_parsed", "n_malformed", "rtt_last", "rtt_count", "peer_fraction_lost",
              "peer_cum_lost", "peer_ext_seq", "peer_jitter")

    def __init__(self):
        self.prior = dict(expected_prior=0, received_prior=0, epoch=0)
        for k in self.FIELDS:
            setattr(self, k, 0)

    def moving(self):
        d = {k: getattr(self, k) for k in self.FIELDS}
        d.update(self.prior)
        return d

    # ---- RFC 3550 A.3
    def block(self, jb, now):
        ext = (jb["cycles"] + jb["max_seq"]) & M32
        expected = (ext - jb["base_seq"] + 1) & M32
        lost = expected - jb["received"]
        same = self.prior["epoch"] == jb["epoch"]
        exp_int = (expected - (self.prior["expected_prior"] if same else 0)) & M32
        rec_int = (jb["received"] - (self.prior["received_prior"] if same else 0)) & M32
        lost_int = exp_int - rec_int
        frac = 0 if exp_int == 0 or lost_int <= 0 else min((lost_int << 8) // exp_int, 255)
        cum = max(-0x800000, min(0x7FFFFF, lost))
        have = self.flags & HAVE_SR
        lsr = self.lsr if have else 0
        dlsr = (((now >> 16) & M32) - self.lsr_arrival) & M32 if have else 0
        self.prior = dict(expected_prior=expected, received_prior=jb["received"], epoch=jb["epoch"])
        return struct.pack(">IB3sIIII", jb["ssrc"], frac, (cum & 0xFFFFFF).to_bytes(3, "big"), ext, jb["jitter"] >> 4, lsr, dlsr)

    def build(self, ctl, src, now, jb=None, cname=b""):
        """-> (the packet or None, flags).  src: dict(ssrc, rtp_ts, packets, octets); jb: dict of igdsp_jb_state's fields or None"""
        if ctl not in (REPORT, BYE):
            return None, 0
        sr = src["packets"] != self.sent_prior
        blocks = self.block(jb, now) if jb is not None and jb["flags"] & JB_HEARD else b""
        rc = len(blocks) // 24
        body = struct.pack(">I", src["ssrc"])
        if sr:
            body += struct.pack(">IIIII", (now >> 32) & M32, now & M32, src["rtp_ts"], src["packets"], src["octets"])
        body += blocks
        pkt = struct.pack(">BBH", 0x80 | rc, 200 if sr else 201, len(body) // 4) + body
        text = bytes(cname)[:64]
        chunk = struct.pack(">IBB", src["ssrc"], 1, len(text)) + text + b"\0"
        chunk += b"\0" * (-len(chunk) % 4)
        pkt += struct.pack(">BBH", 0x81, 202, len(chunk) // 4) + chunk
        if ctl == BYE:
            pkt += struct.pack(">BBHI", 0x81, 203, 1, src["ssrc"])
        self.sent_prior = src["packets"]
        self.n_built = (self.n_built + 1) & M32
        return pkt, (SR if sr else RR) | (HAS_BLOCK if rc else 0) | (BYE_SENT if ctl == BYE else 0)

    # ---- RFC 3550 A.2 and what a valid packet gives
    def parse(self, pkt, arrival, local_ssrc, slot=2048):
        """-> dict of igdsp_rtcp_seen's fields"""
        pkt = bytes(pkt)
        rec = dict(flags=0, n_sub=0, peer_fraction_lost=0, sender_ssrc=0, rtt=0, peer_cum_lost=0, peer_ext_seq=0, peer_jitter=0, sr_packets=0, sr_octets=0)
        if len(pkt) == 0:
            rec["flags"] = EMPTY
            return rec
        subs = self._split(pkt) if len(pkt) >= 8 and len(pkt) % 4 == 0 and len(pkt) <= slot else None
        if subs is None:
            self.n_malformed = (self.n_malformed + 1) & M32
            rec["flags"] = MALFORMED
            return rec
        flags, ours = PARSED, None
        rec["n_sub"] = min(len(subs), 255)
        rec["sender_ssrc"] = struct.unpack(">I", subs[0][2][4:8])[0]
        for pt, count, sub in subs:
            if pt == 200:
                msw, lsw, _, packets, octets = struct.unpack(">IIIII", sub[8:28])
                self.lsr, self.lsr_arrival = ((msw << 16) | (lsw >> 16)) & M32, arrival
                self.flags |= HAVE_SR
                rec["sr_packets"], rec["sr_octets"] = packets, octets
                flags |= GOT_SR
            if pt in (200, 201):
                at = 28 if pt == 200 else 8
                for b in range(count):
                    blk = sub[at + 24 * b:at + 24 * b + 24]
                    if ours is None and struct.unpack(">I", blk[:4])[0] == local_ssrc:
                        ours = blk
            if pt == 203:
                self.flags |= BYE_SEEN
                flags |= GOT_BYE
        if ours is not None:
            _, frac, cum, ext, jit, lsr, dlsr = struct.unpack(">IB3sIIII", ours)
            cum = int.from_bytes(cum, "big", signed=True)
            self.peer_fraction_lost, self.peer_cum_lost, self.peer_ext_seq, self.peer_jitter = frac, cum, ext, jit
            self.flags |= PEER_VALID
            rec.update(peer_fraction_lost=frac, peer_cum_lost=cum, peer_ext_seq=ext, peer_jitter=jit)
            flags |= GOT_BLOCK
            if lsr != 0:
                rtt = (arrival - lsr - dlsr) & M32
                rec["rtt"] = rtt
                if rtt < 1 << 31:
                    self.rtt_last, self.rtt_count = rtt, (self.rtt_count + 1) & M32
                    self.flags |= RTT_VALID
                    flags |= GOT_RTT
                else:
                    flags |= RTT_NEGATIVE
        self.n_parsed = (self.n_parsed + 1) & M32
        rec["flags"] = flags
        return rec

    @staticmethod
    def _split(pkt):
        """the sub-packets as (pt, count, bytes), or None where A.2 refuses the compound"""
        subs, at = [], 0
        while at < len(pkt):
            b0, pt, length = struct.unpack(">BBH", pkt[at:at + 4])
            n = 4 * (length + 1)
            if b0 >> 6 != 2 or at + n > len(pkt):
                return None
            if subs and subs[-1][3]:
                return None                                                # padding on a sub-packet that is not the last
            count, pad = b0 & 31, (b0 >> 5) & 1
            if not subs and (pad or pt not in (200, 201)):
                return None
            if (pt == 200 and n < 28 + 24 * count) or (pt == 201 and n < 8 + 24 * count) or (pt == 203 and n < 4 + 4 * count):
                return None
            subs.append((pt, count, pkt[at:at + n], pad))
            at += n
        return [(pt, count, sub) for pt, count, sub, _ in subs]


# ---- SRTCP, RFC 3711 3.4
RUN, BYPASS, RESET = sm.RUN, sm.BYPASS, sm.RESET
NO_KEY, OK, AUTH_FAIL, REPLAY, OLD, SRTP_MALFORMED, SRTP_EMPTY, CLEAR, BYPASSED = 0, 1, 2, 4, 8, 16, 32, 64, 128
TRAILER, WINDOW, MAX_PACKET = 14, 64, 2048


def srtcp_keys(key_salt):
    """(k_e 16 bytes, k_a 20, k_s 14): labels 3, 4, 5"""
    mk, ms = bytes(key_salt[:16]), bytes(key_salt[16:30])
    return sm.kdf(mk, ms, 3, 16), sm.kdf(mk, ms, 4, 20), sm.kdf(mk, ms, 5, 14)


class SrtcpLeg:
    def __init__(self, key_salt, index0=0):
        self.ke, self.ka, self.ks = srtcp_keys(key_salt)
        self.index, self.have, self.window = index0 & 0x7FFFFFFF, 0, 0
        self.n_ok = self.n_auth_fail = self.n_replay = self.n_malformed = 0

    def moving(self):
        return dict(roc=self.index, s_l=0, have_s_l=self.have, window=self.window, n_ok=self.n_ok, n_auth_fail=self.n_auth_fail, n_replay=self.n_replay,
                    n_malformed=self.n_malformed)

    def keystream(self, ssrc, index, n):
        iv = (int.from_bytes(self.ks, "big") << 16) ^ (ssrc << 64) ^ (index << 16)
        return sm.aes_ctr(self.ke, iv, n)

    def tag(self, data):
        return hmac.new(self.ka, bytes(data), hashlib.sha1).digest()[:10]

    def _refuse(self, flags, v=0):
        if flags & AUTH_FAIL:
            self.n_auth_fail += 1
        elif flags & (REPLAY | OLD):
            self.n_replay += 1
        else:
            self.n_malformed += 1
        return None, dict(flags=flags, size_out=0, roc_used=v)

    def _open(self, pkt, ctl, in_cap, out_cap):
        size = len(pkt)
        if ctl == BYPASS:
            if size == 0:
                return None, dict(flags=SRTP_EMPTY, size_out=0, roc_used=0)
            if size > MAX_PACKET or size > in_cap or size > out_cap:
                return None, dict(flags=SRTP_MALFORMED, size_out=0, roc_used=0)
            return pkt, dict(flags=BYPASSED, size_out=size, roc_used=0)
        if ctl == RESET:
            self.index, self.have, self.window = 0, 0, 0
        if size == 0:
            return None, dict(flags=SRTP_EMPTY, size_out=0, roc_used=0)
        if size > MAX_PACKET or size > in_cap:
            return self._refuse(SRTP_MALFORMED)
        return False

    def protect(self, pkt, ctl=RUN, in_cap=MAX_PACKET, out_cap=MAX_PACKET):
        pkt = bytes(pkt)
        done = self._open(pkt, ctl, in_cap, out_cap)
        if done is not False:
            return done
        if len(pkt) < 8 or len(pkt) % 4 or len(pkt) + TRAILER > out_cap or pkt[0] >> 6 != 2:
            return self._refuse(SRTP_MALFORMED)
        word = (1 << 31) | self.index
        ssrc = int.from_bytes(pkt[4:8], "big")
        body = pkt[:8] + bytes(a ^ b for a, b in zip(pkt[8:], self.keystream(ssrc, self.index, len(pkt) - 8))) + word.to_bytes(4, "big")
        self.index = (self.index + 1) % (1 << 31)
        self.n_ok += 1
        return body + self.tag(body), dict(flags=OK, size_out=len(body) + 10, roc_used=word)

    def unprotect(self, pkt, ctl=RUN, in_cap=MAX_PACKET, out_cap=MAX_PACKET):
        pkt = bytes(pkt)
        done = self._open(pkt, ctl, in_cap, out_cap)
        if done is not False:
            return done
        if len(pkt) < 22 or (len(pkt) - TRAILER) % 4 or len(pkt) - TRAILER > out_cap:
            return self._refuse(SRTP_MALFORMED)
        end = len(pkt) - TRAILER
        word = int.from_bytes(pkt[end:end + 4], "big")
        index, e = word & 0x7FFFFFFF, word >> 31
        ahead = not self.have or index > self.index
        if not ahead:
            if self.index - index >= WINDOW:
                return self._refuse(OLD, word)
            if (self.window >> (self.index - index)) & 1:
                return self._refuse(REPLAY, word)
        if not hmac.compare_digest(self.tag(pkt[:end + 4]), pkt[end + 4:]):
            return self._refuse(AUTH_FAIL, word)
        ssrc = int.from_bytes(pkt[4:8], "big")
        out = pkt[:end] if not e else pkt[:8] + bytes(a ^ b for a, b in zip(pkt[8:end], self.keystream(ssrc, index, end - 8)))
        self.n_ok += 1
        if ahead:
            d = index - self.index
            self.window = ((0 if (not self.have or d >= WINDOW) else (self.window << d)) | 1) % (1 << 64)
            self.index, self.have = index, 1
        else:
            self.window |= 1 << (self.index - index)
        return out, dict(flags=OK | (0 if e else CLEAR), size_out=end, roc_used=word)
