"""The comfort-noise generator's rule (include/igdsp.h, "Comfort noise") in Python integers, written from the interface text: an
independent restatement of csrc/igdsp_cng.h for tests/test_cng_cpu.py and tests/test_gpu_cng.py.  Nothing here imports the library.
run() walks the frames of C channels at once (numpy int64 vectors over the channels, every step an exact integer operation); the
rare step 2 of a payload is plain Python integers."""
from __future__ import annotations

import math

import numpy as np

from tests import record_model
from tests.vad_model import T8

TAG = 0xC4610001
RUN, FREEZE, BYPASS, RESET = 0, 1, 2, 3
NONE, VOICE, SID = 0, 1, 2
F_GENERATED, F_SID, F_NO_MODEL, F_VOICE, F_CLIPPED, F_SID_EMPTY, F_FROZEN, F_BYPASSED = 1, 2, 4, 8, 16, 32, 64, 128
BMAX, KQMAX, GMAX = 131071, 16383, 3632640
M32 = 0xFFFFFFFF
STATE = np.dtype([("tag", "<u4"), ("seed", "<u4"), ("ctr", "<u4"), ("g", "<u4"), ("g_tgt", "<u4"), ("b", "<i4", 10), ("kq", "<i2", 10),
                  ("since_sid", "<u2"), ("level", "u1"), ("order", "u1"), ("have", "u1"), ("flags", "u1"), ("reserved", "u1", 10)])
REC = np.dtype([("g", "<u4"), ("g_tgt", "<u4"), ("since_sid", "<u2"), ("flags", "u1"), ("level", "u1"), ("order", "u1"), ("reserved", "u1", 3)])
assert STATE.itemsize == 96 and REC.itemsize == 16

G = [math.isqrt(int(t)) for t in T8]


def mix(x):
    """mix() on uint32, for an int or an int64 vector"""
    x = x & M32
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def exc(q, hs):
    """e(q) for the stream's sample index q and hs = mix(seed)"""
    r = mix((q & M32) ^ hs)
    return (r & 255) + ((r >> 8) & 255) + ((r >> 16) & 255) + (r >> 24) - 510


def cdiv2(d):
    """d / 2, C division, for an int or a vector"""
    return np.where(d < 0, -((-d) // 2), d // 2) if isinstance(d, np.ndarray) else (-((-d) // 2) if d < 0 else d // 2)


def clamp(v, m=BMAX):
    return np.clip(v, -m, m) if isinstance(v, np.ndarray) else min(m, max(-m, v))


def sid_decode(payload, ln: int):
    """igdsp_sid_decode: (level, k[10] in Q15)"""
    return int(payload[0]), [258 * (min(int(payload[i + 1]), 254) - 127) if i + 1 < ln else 0 for i in range(10)]


def gain(payload, ln: int):
    """Step 2 of a payload of ln = 1..11 bytes: (g_tgt, kq[10], level, order)"""
    level, k = sid_decode(payload, ln)
    p = 1 << 30
    for ki in k:
        p = (p * ((1 << 30) - ki * ki)) >> 30
    sp = math.isqrt(p)
    return (G[min(level, 127)] * sp * 7095) >> 23, [cdiv2(ki) for ki in k], level, ln - 1


def lattice(e, g, b, kq):
    """Step 5's samples for the channels of the vectors: e [n][K] the excitation, g [K], b [10][K] (updated in place), kq [10][K].
    Returns out [n][K] and whether a sample of magnitude >= 32767 was made [K]"""
    n = e.shape[0]
    out = np.empty(e.shape, np.int64)
    for j in range(n):
        f = clamp((e[j] * g + 2048) >> 12)
        for i in range(10, 0, -1):
            f = clamp(f - ((kq[i - 1] * b[i - 1] + 8192) >> 14))
            if i < 10:
                b[i] = clamp(b[i - 1] + ((kq[i - 1] * f + 8192) >> 14))
        b[0] = f
        out[j] = np.clip((f + 2) >> 2, -32768, 32767)
    return out, (np.abs(out) >= 32767).any(axis=0)


def run(kind, sid, n, sid_len=None, voice=None, ctl=None, seed=None, state=None):
    """kind [F][C], sid [F][C][16], sid_len [F][C] or None (11), voice [F][C][n] (the decoded rows) or None, ctl [C] or None (RUN), seed
    [C] or None, state [C] STATE or None (all-zero: the RESET state).  Returns (out [F][C][n] int16, len_out [F][C] uint16, rec [F][C]
    REC, stats [F][C] record_model.STATS, state [C] STATE)."""
    kind = np.asarray(kind).astype(np.int64)
    F_, C_ = kind.shape
    sid = np.asarray(sid, np.uint8).reshape(F_, C_, 16)
    sid_len = np.full((F_, C_), 11, np.int64) if sid_len is None else np.asarray(sid_len).astype(np.int64)
    ctl = np.zeros(C_, np.int64) if ctl is None else np.asarray(ctl).astype(np.int64)
    ctl = np.where(ctl > 3, RUN, ctl)
    seed = np.zeros(C_, np.int64) if seed is None else np.asarray(seed).astype(np.int64)
    st0 = np.zeros(C_, STATE) if state is None else np.asarray(state, STATE).copy()
    i64 = lambda k: st0[k].astype(np.int64)
    z = (i64("tag") != TAG) | (ctl == RESET)                               # the RESET state
    zi = lambda v: np.where(z if v.ndim == 1 else z[:, None], 0, v)
    s_seed, ctr = np.where(z, seed, i64("seed")), zi(i64("ctr"))
    g, g_tgt = zi(np.minimum(i64("g"), GMAX)), zi(np.minimum(i64("g_tgt"), GMAX))
    b, kq = zi(clamp(i64("b"))).T.copy(), zi(clamp(i64("kq"), KQMAX)).T.copy()     # [10][C]
    since, level, order, have = zi(i64("since_sid")), zi(i64("level")), zi(i64("order")), zi(i64("have") & 1)
    last = zi(i64("flags"))
    bypass, frozen = ctl == BYPASS, ctl == FREEZE
    hs = mix(s_seed)

    out = np.zeros((F_, C_, n), np.int16)
    len_out = np.zeros((F_, C_), np.uint16)
    rec = np.zeros((F_, C_), REC)
    for f in range(F_):
        ln = np.minimum(sid_len[f], 11)
        is_sid = kind[f] == SID
        is_voice = ~is_sid & (kind[f] != NONE)
        take = is_sid & ~frozen & (ln > 0) & ~bypass
        flags = np.where(frozen, F_FROZEN, 0) | np.where(is_sid & (ln == 0), F_SID_EMPTY, 0) | np.where(is_voice, F_VOICE, 0)
        for c in np.nonzero(take)[0]:                                      # step 2
            g_tgt[c], k, level[c], order[c] = gain(sid[f, c], int(ln[c]))
            kq[:, c] = k
            if not have[c]:
                g[c], have[c] = g_tgt[c], 1
        flags |= np.where(take, F_SID, 0)
        since = np.where(bypass, since, np.where(take, 0, np.minimum(since + 1, 65535)))
        silent = ~bypass & ~is_voice
        gen = silent & (have == 1)
        flags |= np.where(silent & (have == 0), F_NO_MODEL, 0) | np.where(gen, F_GENERATED, 0)
        d = g_tgt - g
        g = np.where(gen, g + d - cdiv2(d), g)
        idx = np.nonzero(gen)[0]
        if len(idx):                                                       # step 5
            q = ctr[idx][None, :] + np.arange(n, dtype=np.int64)[:, None]
            bb = b[:, idx]
            o, clip = lattice(exc(q, hs[idx][None, :]), g[idx], bb, kq[:, idx])
            b[:, idx] = bb
            out[f, idx] = o.T
            len_out[f, idx] = n
            flags[idx] |= np.where(clip, F_CLIPPED, 0)
        if voice is not None:                                              # step 3, and a bypass
            vi = np.nonzero(is_voice)[0]
            out[f, vi] = np.asarray(voice)[f, vi]
            len_out[f, vi] = n
        ctr = np.where(bypass, ctr, (ctr + n) & M32)
        flags = np.where(bypass, F_BYPASSED, flags)
        last = np.where(bypass, last, flags)
        for k, v in (("g", g), ("g_tgt", g_tgt), ("since_sid", since), ("flags", flags), ("level", level), ("order", order)):
            rec[k][f] = v
    st = np.zeros(C_, STATE)
    for k, v in (("tag", np.full(C_, TAG)), ("seed", s_seed), ("ctr", ctr), ("g", g), ("g_tgt", g_tgt), ("b", b.T), ("kq", kq.T), ("since_sid", since),
                 ("level", level), ("order", order), ("have", have), ("flags", last)):
        st[k] = v
    st[bypass] = st0[bypass]                                               # a bypass leaves the state's bytes alone
    stats = record_model.records(out, live=len_out != 0)
    return out, len_out, rec, stats, st


def yardstick_state(state, seed=None):
    """the state igdsp_internal_cng_move leaves: as read, clamped, with the tag, flags as read, reserved 0"""
    C_ = len(state)
    k0 = np.zeros((0, C_), np.int64)
    return run(k0, np.zeros((0, C_, 16), np.uint8), 16, seed=seed, state=state)[4]


def garbage_state(C_, seed, tagged=True):
    """states of random bytes, under the tag or not"""
    rng = np.random.default_rng(seed)
    st = np.frombuffer(rng.integers(0, 256, C_ * STATE.itemsize, dtype=np.uint8).tobytes(), STATE).copy()
    if tagged:
        st["tag"] = TAG
    else:
        st["tag"][st["tag"] == TAG] = 0
    return st


def payload(level, ns=()):
    """sixteen bytes: the level, the coefficient bytes ns, zeros"""
    p = np.zeros(16, np.uint8)
    p[0] = level
    p[1:1 + len(ns)] = ns
    return p
