"""The voice detector (include/igdsp.h, "Voice activity") restated from the interface text with Python integers and numpy: the oracle
of tests/test_vad_cpu.py and tests/test_gpu_vad.py.  Nothing here is taken from csrc/igdsp_vad.h: a frame is a dict of Python ints
stepped clause by clause, the level table comes from decimal arithmetic, the sums from numpy int64.  UNVERIFIED against RFC 3389 and
G.711 Appendix II, as the rule itself is."""
from decimal import Decimal, getcontext

import numpy as np

TAG = 0x7AD10001
RUN, FREEZE, BYPASS, RESET = 0, 1, 2, 3
NONE, VOICE, SID = 0, 1, 2
F_RAW, F_VOICE, F_ONSET, F_OFFSET, F_SID, F_QUIET, F_FROZEN, F_BYPASSED = 1, 2, 4, 8, 16, 32, 64, 128
EVENT_DEFAULT = F_ONSET | F_OFFSET
M = 10
KMAX = 32508
AMAX = 1 << 40
CFG = np.dtype([("thr_abs", "<u4"), ("nf_min", "<u4"), ("nf_max", "<u4"), ("sid_every", "<u2"), ("ratio_on_q4", "u1"), ("ratio_off_q4", "u1"),
                ("dn", "u1"), ("up", "u1"), ("up_v", "u1"), ("asm_shift", "u1"), ("burst", "u1"), ("hang_long", "u1"), ("hang_short", "u1"),
                ("order", "u1"), ("dtx", "u1"), ("sid_delta", "u1"), ("sid_gap", "u1"), ("vox_on", "u1"), ("vox_off", "u1"), ("reserved", "u1", 3)])
STATE = np.dtype([("tag", "<u4"), ("nf", "<u4"), ("A", "<i8", 11), ("since_sid", "<u2"), ("run", "<u2"), ("hang", "u1"), ("voice", "u1"),
                  ("avalid", "u1"), ("last_level", "u1"), ("sid_sent", "u1"), ("flags", "u1"), ("reserved", "u1", 22)])
REC = np.dtype([("ms", "<u4"), ("nf", "<u4"), ("run", "<u2"), ("flags", "u1"), ("kind", "u1"), ("level", "u1"), ("hang", "u1"), ("sid_len", "u1"),
                ("reserved", "u1")])
EVENT = np.dtype([("channel", "<u4"), ("frame", "<u4"), ("ms", "<u4"), ("run", "<u2"), ("flags", "u1"), ("level", "u1")])
assert (CFG.itemsize, STATE.itemsize, REC.itemsize, EVENT.itemsize) == (32, 128, 16, 16)
DEFAULTS = dict(thr_abs=212, nf_min=8, nf_max=1 << 20, sid_every=0, ratio_on_q4=80, ratio_off_q4=40, dn=2, up=5, up_v=7, asm_shift=2, burst=5,
                hang_long=10, hang_short=2, order=10, dtx=1, sid_delta=2, sid_gap=2, vox_on=0x81, vox_off=0x80)
CFG_KEYS = tuple(DEFAULTS)


def cfg_default(**kw):
    c = np.zeros((), CFG)
    for k, v in {**DEFAULTS, **kw}.items():
        c[k] = v
    return c


def cfg_valid(c):
    g = lambda k: int(c[k])
    return (1 <= g("nf_min") <= g("nf_max") <= 1 << 24 and 16 <= g("ratio_off_q4") <= g("ratio_on_q4") <= 255 and
            all(g(k) <= 15 for k in ("dn", "up", "up_v", "asm_shift")) and g("order") <= 10 and g("hang_short") <= g("hang_long"))


def t8():
    """T8[d] = floor(2^34 * 10^(-d / 10) + 1/2), d = 0..127, by decimal arithmetic"""
    getcontext().prec = 80
    return [int((Decimal(2) ** 34 * Decimal(10) ** (Decimal(-d) / Decimal(10)) + Decimal(1) / 2).to_integral_value(rounding="ROUND_FLOOR")) for d in range(128)]


T8 = t8()


def level(e, n):
    if e <= 0:
        return 127
    for d in range(127):
        if (e << 8) >= n * T8[d]:
            return d
    return 127


def tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def quant(k):
    m = (abs(k) + 129) // 258
    return 127 + (m if k >= 0 else -m)


def reflection(A, order):
    """the k_i (Q15) of step 7, order of them"""
    k = [0] * order
    A0 = A[0]
    if A0 <= 0 or order == 0:
        return k
    R0 = A0 + (A0 >> 10) + 1
    sh = R0.bit_length() - 30
    shift = lambda v: v >> sh if sh >= 0 else v << -sh
    R = [shift(R0)] + [shift(max(-A0, min(A0, A[i]))) for i in range(1, order + 1)]
    a = [0] * (order + 1)
    err = R[0]
    for i in range(1, order + 1):
        acc = (R[i] << 15) + sum(a[j] * R[i - j] for j in range(1, i))
        ki = max(-KMAX, min(KMAX, tdiv(-acc, err)))
        a = [a[j] + ((ki * a[i - j] + 16384) >> 15) if 1 <= j < i else a[j] for j in range(order + 1)]
        a[i] = ki
        k[i - 1] = ki
        err -= (((ki * ki) >> 15) * err) >> 15
        if err <= 0:
            break
    return k


def sid_payload(A, lvl, order):
    return [lvl] + [quant(k) for k in reflection(A, order)]


def sid_decode(payload):
    """(level, k[10]) of a payload: the inverse of quant; index 255 reads as 254, coefficients past the payload are 0"""
    k = [258 * (min(int(N), 254) - 127) for N in payload[1:11]]
    return int(payload[0]), k + [0] * (10 - len(k))


def autocorr(x):
    """r[0..10] of one row (int samples), exact"""
    v = np.asarray(x, np.int64) >> 2
    n = len(v)
    return [int(np.dot(v[k:], v[:n - k])) for k in range(M + 1)]


def reset_state():
    return dict(nf=0, A=[0] * 11, since_sid=0, run=0, hang=0, voice=0, avalid=0, last_level=0, sid_sent=0)


def read_state(rec, cfg, reset):
    if reset or int(rec["tag"]) != TAG:
        return reset_state()
    nf = int(rec["nf"])
    return dict(nf=0 if nf == 0 else max(int(cfg["nf_min"]), min(int(cfg["nf_max"]), nf)), A=[max(-AMAX, min(AMAX, int(a))) for a in rec["A"]],
                since_sid=int(rec["since_sid"]), run=int(rec["run"]), hang=int(rec["hang"]), voice=int(rec["voice"]) & 1, avalid=int(rec["avalid"]) & 1,
                last_level=int(rec["last_level"]), sid_sent=int(rec["sid_sent"]) & 1)


def write_state(s, flags):
    o = np.zeros((), STATE)
    o["tag"], o["nf"], o["A"], o["flags"] = TAG, s["nf"], s["A"], flags
    for k in ("since_sid", "run", "hang", "voice", "avalid", "last_level", "sid_sent"):
        o[k] = s[k]
    return o


def frame(c, s, x, ctl):
    """one frame of one channel: s (a dict, updated unless bypassed), x the row -> (kind, rec fields dict, sid bytes list of 16)"""
    g = lambda k: int(c[k])
    n = len(x)
    r = autocorr(x)
    E = r[0]
    ms = E // n
    lvl_e = level(E, n)
    if ctl == BYPASS:
        return VOICE, dict(ms=ms, nf=s["nf"], run=s["run"], flags=F_BYPASSED, kind=VOICE, level=lvl_e, hang=s["hang"], sid_len=0), [0] * 16
    frozen = ctl == FREEZE
    # 2
    if s["nf"] == 0:
        s["nf"] = max(g("nf_min"), min(g("nf_max"), ms))
    ratio = g("ratio_off_q4") if s["voice"] else g("ratio_on_q4")
    raw = ms >= g("thr_abs") and ms * 16 > s["nf"] * ratio
    quiet = ms < g("nf_min")
    flags = (F_RAW if raw else 0) | (F_QUIET if quiet else 0) | (F_FROZEN if frozen else 0)
    # 3
    if not frozen and not quiet:
        nf = s["nf"]
        if ms <= nf:
            nf -= (nf - ms) >> g("dn")
        else:
            nf = min(ms, nf + max(1, nf >> (g("up_v") if raw else g("up"))))
        s["nf"] = max(g("nf_min"), min(g("nf_max"), nf))
    # 4
    was = s["voice"]
    if raw:
        s["run"] = min(s["run"] + 1, 65535)
        s["hang"] = g("hang_long") if s["run"] >= g("burst") else max(s["hang"], g("hang_short"))
        s["voice"] = 1
    else:
        s["run"] = 0
        if s["hang"] > 0:
            s["hang"] -= 1
        else:
            s["voice"] = 0
    if s["voice"]:
        flags |= F_VOICE | (0 if was else F_ONSET)
    elif was:
        flags |= F_OFFSET
    # 5
    if not frozen and not raw:
        s["A"] = [A + ((rk - A) >> g("asm_shift")) for A, rk in zip(s["A"], r)] if s["avalid"] else list(r)
        s["avalid"] = 1
    # 6, 7
    kind, sid = VOICE, [0] * 16
    if g("dtx") and not s["voice"]:
        lvl = level(s["A"][0], n)
        due = (bool(flags & F_OFFSET) or not s["sid_sent"] or (g("sid_every") > 0 and s["since_sid"] >= g("sid_every")) or
               (abs(lvl - s["last_level"]) >= g("sid_delta") and s["since_sid"] >= g("sid_gap")))
        if due:
            kind, s["since_sid"], s["last_level"], s["sid_sent"] = SID, 0, lvl, 1
            flags |= F_SID
            p = sid_payload(s["A"], lvl, g("order"))
            sid = p + [0] * (16 - len(p))
        else:
            kind, s["since_sid"] = NONE, min(s["since_sid"] + 1, 65535)
    return kind, dict(ms=ms, nf=s["nf"], run=s["run"], flags=flags, kind=kind, level=lvl_e, hang=s["hang"], sid_len=1 + g("order") if kind == SID else 0), sid


def run(cfg, x, ctl=None, state=None):
    """x [F][C][n] ints; ctl [C] or None; state [C] STATE or None (all-zero) -> kind [F][C] u8, rec [F][C] REC, sid [F][C][16] u8,
    txctl [F][C] u8, state [C] STATE (a bypassed channel's bytes as they were)"""
    c = cfg_default() if cfg is None else cfg
    x = np.asarray(x)
    F_, C_, n = x.shape
    kind, rec, sid, tx = np.zeros((F_, C_), np.uint8), np.zeros((F_, C_), REC), np.zeros((F_, C_, 16), np.uint8), np.zeros((F_, C_), np.uint8)
    st = np.zeros(C_, STATE) if state is None else np.array(state, STATE)
    for ch in range(C_):
        ct = int(ctl[ch]) if ctl is not None else RUN
        ct = ct if ct <= 3 else RUN
        s = read_state(st[ch], c, ct == RESET)
        ct = RUN if ct == RESET else ct
        flags = 0
        for f in range(F_):
            k, fields, sb = frame(c, s, x[f, ch], ct)
            flags = fields["flags"]
            kind[f, ch], sid[f, ch] = k, sb
            for key, v in fields.items():
                rec[f, ch][key] = v
            tx[f, ch] = int(c["vox_on"]) if (flags & (F_VOICE | F_BYPASSED)) else int(c["vox_off"])
        if ct != BYPASS and F_:
            st[ch] = write_state(s, flags)
    return kind, rec, sid, tx, st


def events(rec, mask=0, cap=None):
    """the event list of records [F][C]: (events, total)"""
    mask = mask or EVENT_DEFAULT
    ev = []
    for f in range(rec.shape[0]):
        for ch in range(rec.shape[1]):
            r = rec[f, ch]
            if int(r["flags"]) & mask:
                ev.append((ch, f, int(r["ms"]), int(r["run"]), int(r["flags"]), int(r["level"])))
    out = np.array(ev if cap is None else ev[:cap], EVENT) if ev else np.zeros(0, EVENT)
    return out, len(ev)


def garbage_state(C_, seed, tagged=True):
    rng = np.random.default_rng(seed)
    st = rng.integers(0, 256, C_ * STATE.itemsize, dtype=np.uint8).view(STATE).copy()
    sel = rng.integers(0, 3, C_)
    A = st["A"].copy()
    A[sel == 1] >>= 24                                                     # within +-2^40: kept as they are
    A[sel == 2] >>= 30
    st["A"] = A
    st["tag"] = TAG if tagged else rng.integers(0, TAG, C_)
    return st


def noise(F_, C_, n, seed, rms):
    return np.clip(np.rint(np.random.default_rng(seed).normal(0.0, rms, (F_, C_, n))), -32768, 32767).astype(np.int64)


def ar_noise(F_, n, seed, rms, poles):
    """one channel [F][n] of an all-pole process 1 / prod (1 - p z^-1), scaled to rms"""
    rng = np.random.default_rng(seed)
    a = np.real(np.poly(poles)) if len(poles) else np.array([1.0])
    e = rng.normal(0.0, 1.0, F_ * n + 512)
    y = np.zeros_like(e)
    for i in range(len(e)):
        y[i] = e[i] - sum(a[j] * y[i - j] for j in range(1, len(a)) if i - j >= 0)
    y = y[512:]
    y *= rms / np.sqrt(np.mean(y * y))
    return np.clip(np.rint(y), -32768, 32767).astype(np.int64).reshape(F_, n)


def scene(F_, C_, n, seed, rms=100, burst=(4, 8), gain=12.0):
    """noise, a burst in frames [burst[0], burst[1]) of every channel, noise: ONSET, OFFSET and SID on every channel once F is long enough"""
    x = noise(F_, C_, n, seed, rms).astype(np.float64)
    x[burst[0]:burst[1]] *= gain
    return np.clip(np.rint(x), -32768, 32767).astype(np.int64)
