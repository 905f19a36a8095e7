"""The numpy statement of the level control (include/igdsp.h, "Level control"): the integer rule restated independently of
csrc/igdsp_agc.h (run: every channel at once, frames and knots in sequence), the same rule in float64 without rounding and without
Q12 (run_f64: the reference of the fidelity test), and the scenes the property tests and the GPU tests share.  The model asserts on
every sample that no clamp could fire: |x t| <= ceil << 12.  The rule is the library's own, UNVERIFIED against ITU-T G.169."""
import numpy as np

from tests import record_model

BLOCK, UNITY, CAP, TAG = 8, 4096, 65535, 0xA6C10001
RUN, FREEZE, BYPASS, RESET = 0, 1, 2, 3
ACTIVE, LIMITED, AT_MAX, AT_MIN, ATTACKED, FROZEN, BYPASSED = 1, 2, 4, 8, 16, 32, 64
CFG = np.dtype([("target", "<u2"), ("ceil", "<u2"), ("gate", "<u2"), ("gmin", "<u2"), ("gmax", "<u2"), ("att", "u1"), ("rel", "u1"), ("up", "u1"),
                ("down", "u1"), ("lrel", "u1"), ("reserved", "u1")])
STATE = np.dtype([("tag", "<u4"), ("env", "<u2"), ("gain", "<u2"), ("cap", "<u2"), ("flags", "<u2"), ("reserved", "<u4")])
REC = np.dtype([("gain", "<u2"), ("tmin", "<u2"), ("in_peak", "<u2"), ("out_peak", "<u2"), ("env", "<u2"), ("flags", "u1"), ("n_limited", "u1"),
                ("reserved", "<u4")])
assert CFG.itemsize == 16 and STATE.itemsize == 16 and REC.itemsize == 16
DEFAULTS = dict(target=8192, ceil=23170, gate=256, gmin=1024, gmax=32768, att=1, rel=5, up=5, down=2, lrel=6)


def cfg_default(**kw):
    c = np.zeros((), CFG)
    for k, v in {**DEFAULTS, **kw}.items():
        c[k] = v
    return c


def cfg_valid(c):
    g = lambda k: int(c[k])
    return (1 <= g("gate") and 1 <= g("target") <= g("ceil") <= 32767 and 1 <= g("gmin") <= 4096 <= g("gmax") <= 65535
            and all(g(k) <= 15 for k in ("att", "rel", "up", "down")) and 1 <= g("lrel") <= 15)


def tdiv(a, b):
    """C division, toward zero"""
    a = np.asarray(a, np.int64)
    return np.sign(a) * (np.abs(a) // b)


def garbage_state(C_, seed, tagged=True):
    rng = np.random.default_rng(seed)
    st = np.frombuffer(rng.integers(0, 256, C_ * STATE.itemsize, dtype=np.uint8).tobytes(), STATE).copy()
    if tagged:
        st["tag"] = TAG
    else:
        st["tag"][st["tag"] == TAG] = 0
    return st


def run(cfg, x, ctl=None, state=None, want_gains=False):
    """x [F][C][n] integers in int16's range; ctl [C] or None (RUN); state [C] STATE or None (all-zero: the RESET state).
    Returns (out int16 [F][C][n], rec REC [F][C], stats record_model.STATS [F][C], state STATE [C]) and, with want_gains, the
    per-sample gains t [F][C][n] and the knots T [F][C][B + 1] behind them."""
    assert cfg_valid(cfg)
    g = {k: int(cfg[k]) for k in DEFAULTS}
    x = np.asarray(x).astype(np.int64)
    F_, C_, n = x.shape
    assert n % 8 == 0 and 8 <= n <= 256
    B = n // 8
    ctl = np.zeros(C_, np.int64) if ctl is None else np.asarray(ctl).astype(np.int64)
    ctl = np.where(ctl > 3, RUN, ctl)
    st0 = np.zeros(C_, STATE) if state is None else np.array(state, STATE)
    keep = (st0["tag"] == TAG) & (ctl != RESET)
    env = np.where(keep, st0["env"], 0).astype(np.int64)
    G = np.where(keep, np.clip(st0["gain"].astype(np.int64), g["gmin"], g["gmax"]), UNITY)
    cap = np.where(keep, st0["cap"], CAP).astype(np.int64)
    byp, frz = ctl == BYPASS, ctl == FREEZE
    out = np.zeros((F_, C_, n), np.int16)
    rec = np.zeros((F_, C_), REC)
    gains = np.zeros((F_, C_, n), np.int64)
    knots = np.zeros((F_, C_, B + 1), np.int64)
    flags = np.zeros(C_, np.int64)
    ks, ii = np.arange(B + 1), np.arange(8)
    for f in range(F_):
        xb = x[f].reshape(C_, B, 8)
        p = np.abs(xb).max(axis=2)                                          # [C][B]
        pk = p.max(axis=1)
        active = pk >= g["gate"]
        moves = active & ~frz & ~byp
        flags = np.where(active, ACTIVE, 0) | np.where(frz, FROZEN, 0)
        # step 2
        e_new = np.where(env == 0, pk, np.where(pk > env, env + ((pk - env + (1 << g["att"]) - 1) >> g["att"]), env - ((env - pk) >> g["rel"])))
        env_n = np.where(moves, e_new, env)
        q = (g["target"] << 12) // np.maximum(env_n, 1)
        Gt = np.clip(q, g["gmin"], g["gmax"])
        flags |= np.where(moves & (q > g["gmax"]), AT_MAX, 0) | np.where(moves & (q < g["gmin"]), AT_MIN, 0)
        d = Gt - G
        Gn = np.where(d >= 0, G + ((d + (1 << g["up"]) - 1) >> g["up"]), G - ((-d + (1 << g["down"]) - 1) >> g["down"]))
        Gn = np.where(moves, Gn, G)
        A = G[:, None] + tdiv((Gn - G)[:, None] * ks[None, :], B)           # [C][B + 1]
        # step 3
        r = np.where(p == 0, CAP, np.minimum(CAP, (g["ceil"] << 12) // np.maximum(p, 1)))
        rp = np.concatenate([np.full((C_, 1), CAP), r, np.full((C_, 1), CAP)], axis=1)
        m = np.minimum(rp[:, :-1], rp[:, 1:])                               # m_k = min(r_(k-1), r_k)
        flags |= np.where(m[:, 0] < cap, ATTACKED, 0)
        c = np.zeros((C_, B + 1), np.int64)
        c[:, 0] = np.minimum(m[:, 0], cap)
        for k in range(1, B + 1):
            prev = c[:, k - 1]
            c[:, k] = np.minimum(m[:, k], np.minimum(CAP, prev + np.maximum(1, prev >> g["lrel"])))
        # step 4
        T = np.minimum(A, c)
        n_lim = (c < A).sum(axis=1)
        flags |= np.where(n_lim > 0, LIMITED, 0)
        t = T[:, :-1, None] + tdiv((T[:, 1:] - T[:, :-1])[:, :, None] * ii[None, None, :], 8)       # [C][B][8]
        prod = xb * t
        assert np.all(np.abs(prod)[~byp] <= g["ceil"] << 12), "a clamp would have fired"
        o = (prod + 2048) >> 12
        o = np.where(byp[:, None, None], xb, o)
        assert np.all(np.abs(o)[~byp] <= g["ceil"])
        out[f] = o.reshape(C_, n)
        gains[f], knots[f] = t.reshape(C_, n), T
        opk = np.abs(o).max(axis=(1, 2))
        flags = np.where(byp, BYPASSED, flags)
        rec["gain"][f] = np.where(byp, G, Gn)
        rec["tmin"][f] = np.where(byp, UNITY, T.min(axis=1))
        rec["in_peak"][f], rec["out_peak"][f] = pk, opk
        rec["env"][f] = np.where(byp, env, env_n)
        rec["flags"][f], rec["n_limited"][f] = flags, np.where(byp, 0, n_lim)
        env, G, cap = np.where(byp, env, env_n), np.where(byp, G, Gn), np.where(byp, cap, c[:, B])
    st = np.zeros(C_, STATE)
    st["tag"], st["env"], st["gain"], st["cap"], st["flags"] = TAG, env, G, cap, flags
    if F_ == 0:
        st = st0.copy()
    st[byp] = st0[byp]                                                      # a bypass does not touch the state's bytes
    res = (out, rec, record_model.records(out), st)
    return res + (gains, knots) if want_gains else res


def run_f64(cfg, x):
    """The same rule in float64 from the RESET state under RUN: no rounding anywhere, gains as plain factors.  x [F][C][n].
    Returns (out float [F][C][n], Gn [F][C], active [F][C])."""
    g = {k: float(cfg[k]) for k in DEFAULTS}
    x = np.asarray(x).astype(np.float64)
    F_, C_, n = x.shape
    B = n // 8
    env, G, cap = np.zeros(C_), np.ones(C_), np.full(C_, CAP / 4096.0)
    out, gain, act = np.zeros(x.shape), np.zeros((F_, C_)), np.zeros((F_, C_), bool)
    ks, ii = np.arange(B + 1) / B, np.arange(8) / 8.0
    for f in range(F_):
        xb = x[f].reshape(C_, B, 8)
        p = np.abs(xb).max(axis=2)
        pk = p.max(axis=1)
        active = pk >= g["gate"]
        e_new = np.where(env == 0, pk, np.where(pk > env, env + (pk - env) / 2 ** g["att"], env - (env - pk) / 2 ** g["rel"]))
        env = np.where(active, e_new, env)
        Gt = np.clip(g["target"] / np.maximum(env, 1e-9), g["gmin"] / 4096.0, g["gmax"] / 4096.0)
        d = Gt - G
        Gn = np.where(active, np.where(d >= 0, G + d / 2 ** g["up"], G + d / 2 ** g["down"]), G)
        A = G[:, None] + (Gn - G)[:, None] * ks[None, :]
        r = np.minimum(CAP / 4096.0, g["ceil"] / np.maximum(p, 1e-9))
        rp = np.concatenate([np.full((C_, 1), CAP / 4096.0), r, np.full((C_, 1), CAP / 4096.0)], axis=1)
        m = np.minimum(rp[:, :-1], rp[:, 1:])
        c = np.zeros((C_, B + 1))
        c[:, 0] = np.minimum(m[:, 0], cap)
        for k in range(1, B + 1):
            c[:, k] = np.minimum(m[:, k], np.minimum(CAP / 4096.0, c[:, k - 1] * (1 + 2.0 ** -g["lrel"])))
        T = np.minimum(A, c)
        t = T[:, :-1, None] + (T[:, 1:] - T[:, :-1])[:, :, None] * ii[None, None, :]
        out[f] = (xb * t).reshape(C_, n)
        gain[f], act[f] = Gn, active
        G, cap = Gn, c[:, B]
    return out, gain, act


# ---- the scenes
def tone(amp, F_, n, freq=440.0, rate=8000.0, phase=0.0):
    """[F][1][n]: round(amp sin): at 440 Hz every 160-sample frame holds a sample of the full amplitude"""
    i = np.arange(F_ * n)
    return np.rint(amp * np.sin(2 * np.pi * freq * i / rate + phase)).astype(np.int64).clip(-32768, 32767).reshape(F_, 1, n)


def step_scene(F_, n, at, lo=300, hi=32767):
    """a quiet tone that becomes a full-scale one at sample `at` of the whole scene"""
    i = np.arange(F_ * n)
    a = np.where(i < at, lo, hi)
    return np.rint(a * np.sin(2 * np.pi * 440.0 * i / 8000.0)).astype(np.int64).reshape(F_, 1, n)


def noise(F_, C_, n, seed, lo=-32768, hi=32767):
    return np.random.default_rng(seed).integers(lo, hi + 1, (F_, C_, n)).astype(np.int64)


def mixed_scene(F_, C_, n, seed):
    """per channel another kind of row: tones of levels 20 dB apart, bursts that start at any sample (first blocks included), noise at
    full scale, silence, -32768 runs: what drives every branch of the rule within a few frames"""
    rng = np.random.default_rng(seed)
    i = np.arange(F_ * n)
    x = np.zeros((C_, F_ * n), np.int64)
    for c in range(C_):
        kind = (c + seed) % 6
        amp = int(rng.choice([120, 300, 1000, 3000, 8000, 30000]))
        base = np.rint(amp * np.sin(2 * np.pi * (300 + 37 * (c % 40)) * i / 8000.0 + c)).astype(np.int64)
        if kind == 0:
            x[c] = base
        elif kind == 1:                                                    # bursts to full scale from a quiet tone
            x[c] = base
            for _ in range(2):
                a = int(rng.integers(0, F_ * n))
                a = a - a % n if rng.integers(0, 3) == 0 else a              # a third of them in a frame's first block
                ln = int(rng.integers(1, 40))
                x[c, a:a + ln] = rng.integers(-32768, 32768, len(x[c, a:a + ln]))
        elif kind == 2:
            x[c] = rng.integers(-32768, 32768, F_ * n)
        elif kind == 3:
            x[c] = np.where((i // (3 * n // 2)) % 2 == 0, 0, base)           # silence and tone in turn
        elif kind == 4:
            x[c] = np.where(rng.integers(0, 50, F_ * n) == 0, -32768, base // 4)
        else:
            x[c] = np.clip(np.rint(rng.normal(0, amp, F_ * n)), -32768, 32767)
    return np.ascontiguousarray(x.reshape(C_, F_, n).transpose(1, 0, 2))
