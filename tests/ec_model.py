"""The numpy statement of the echo canceller (include/igdsp.h, "Echo canceller"): the integer rule restated independently of
csrc/igdsp_ec.h (cancel / frame), the same algorithm in float64 without any truncation (frame_f64: the reference of the integer-loss
test), and the generator of the echo scenes the property tests and the GPU tests share.  The rule is the library's own, UNVERIFIED
against ITU-T G.168 and against any other canceller."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from tests import record_model

MAX_TAIL, BLOCK, TAG = 256, 8, 0xEC010000
RUN, FREEZE, BYPASS, RESET = 0, 1, 2, 3
ADAPTED, DOUBLETALK, FAR_ACTIVE, W_SATURATED, BYPASSED = 1, 2, 4, 8, 16
CFG = np.dtype([("tail", "<u2"), ("mu_shift", "u1"), ("reserved", "u1"), ("pmin", "<u4"), ("hang", "<u2"), ("dmin", "<u2")])
STATE = np.dtype([("w", "<i4", (MAX_TAIL,)), ("hist", "<i2", (MAX_TAIL,)), ("hang", "<u4"), ("flags", "<u4"), ("tag", "<u4"), ("reserved", "<u4")])
REC = np.dtype([("near_e", "<u4"), ("out_e", "<u4"), ("flags", "u1"), ("n_adapt", "u1"), ("n_dt", "u1"), ("reserved", "u1"), ("wmax", "<u2"),
                ("reserved2", "<u2")])
assert CFG.itemsize == 12 and STATE.itemsize == 1552 and REC.itemsize == 16


def cfg_default(tail=128, **kw):
    c = np.zeros((), CFG)
    c["tail"], c["mu_shift"], c["pmin"], c["hang"], c["dmin"] = tail, 2, 1 << 16, 80, 256
    for k, v in kw.items():
        c[k] = v
    return c


def fresh(C_=None):
    return np.zeros((), STATE) if C_ is None else np.zeros(C_, STATE)


def _tdiv4(e):
    """C division by 4, toward zero"""
    return np.where(e < 0, -((-e) // 4), e // 4)


def frame(cfg, st, near, far, ctl=RUN):
    """One frame of one channel: st a STATE record (updated in place), near int16 [n], far int16 [n] or None (no far end).
    Returns (out int16 [n], REC record)."""
    L, mu, pmin, hang_cfg, dmin = int(cfg["tail"]), int(cfg["mu_shift"]), int(cfg["pmin"]), int(cfg["hang"]), int(cfg["dmin"])
    near = np.asarray(near).astype(np.int64)
    n = len(near)
    assert L in (128, 256) and n % 2 == 0 and 2 <= n <= 256
    ctl = ctl if ctl <= 3 else RUN
    if ctl != RESET and int(st["tag"]) == (TAG | L):
        w = st["w"][:L].astype(np.int64)
        hist = np.clip(st["hist"][:L].astype(np.int64), -8192, 8191)
        hang, sflags = int(st["hang"]), int(st["flags"]) & W_SATURATED
    else:
        w, hist, hang, sflags = np.zeros(L, np.int64), np.zeros(L, np.int64), 0, 0
    if ctl == RESET:
        ctl = RUN
    if far is None:
        ctl = BYPASS
    xs = np.zeros(n, np.int64) if far is None else np.asarray(far).astype(np.int64) >> 2
    buf = np.concatenate([hist, xs])
    win = sliding_window_view(buf, L)                                      # win[i] = buf[i .. i + L)
    out = near.copy()
    flags, n_adapt, n_dt = (BYPASSED if ctl == BYPASS else 0), 0, 0
    if ctl != BYPASS:
        for s in range(0, n, BLOCK):
            b = min(BLOCK, n - s)
            M = win[s + 1:s + 1 + b, ::-1]                                 # M[j][k] = xs[j - k] of the block's sample j
            wh = w >> 18
            acc = M @ wh
            yhat = np.clip((acc + 1024) >> 11, -32768, 32767)
            e = np.clip(near[s:s + b] - yhat, -32768, 32767)
            out[s:s + b] = e
            end = L + s + b
            P = int((buf[end - L:end] ** 2).sum())
            xmax = 4 * int(np.abs(buf[end - L - b:end]).max())
            dmax = int(np.abs(near[s:s + b]).max())
            if 2 * dmax > xmax and dmax >= dmin:
                hang = hang_cfg
            elif hang > 0:
                hang -= 1
            if hang > 0:
                n_dt += 1
                flags |= DOUBLETALK
            if P >= pmin:
                flags |= FAR_ACTIVE
            if hang == 0 and P >= pmin and ctl != FREEZE:
                g = M.T @ _tdiv4(e)
                sh = 31 - mu - P.bit_length()
                nw = w + (g << sh if sh >= 0 else g >> -sh)                # |g| <= 2^29, sh <= 31: inside int64
                cl = np.clip(nw, -(1 << 31), (1 << 31) - 1)
                if np.any(cl != nw):
                    flags |= W_SATURATED
                    sflags |= W_SATURATED
                w = cl.astype(np.int64)
                n_adapt += 1
                flags |= ADAPTED
    st["w"] = 0
    st["hist"] = 0
    st["w"][:L] = w
    st["hist"][:L] = buf[n:n + L]
    st["hang"], st["flags"], st["tag"], st["reserved"] = hang, sflags, TAG | L, 0
    rec = np.zeros((), REC)
    rec["near_e"], rec["out_e"] = int((near ** 2).sum()) >> 8, int((out ** 2).sum()) >> 8
    rec["flags"], rec["n_adapt"], rec["n_dt"], rec["wmax"] = flags, n_adapt, n_dt, int(np.abs(w >> 18).max())
    return out.astype(np.int16), rec


def cancel(cfg, near, far, far_of=None, ctl=None, state=None):
    """near [F][C][n] int16, far [F][P][n] int16 (P may be 0), far_of [C] or None (row c), ctl [C] or None (RUN: holds for the first frame
    as given; RESET applies to the first frame only, as one launch does), state [C] STATE or None (all-zero).
    Returns (out [F][C][n] int16, rec [F][C], stats [F][C] record_model.STATS, state [C])."""
    near = np.asarray(near)
    F_, C_, n = near.shape
    P_ = 0 if far is None else np.asarray(far).shape[1]
    st = fresh(C_) if state is None else np.array(state, STATE)
    out = np.zeros((F_, C_, n), np.int16)
    rec = np.zeros((F_, C_), REC)
    for c in range(C_):
        r = c if far_of is None else int(far_of[c])
        k = RUN if ctl is None else int(ctl[c])
        for f in range(F_):
            out[f, c], rec[f, c] = frame(cfg, st[c], near[f, c], far[f, r] if r < P_ else None, k)
            if k == RESET or k > 3:
                k = RUN
    return out, rec, record_model.records(out), st


# ---- the same algorithm in float64, nothing truncated: taps t = w / 2^31, the far end unshifted
def frame_f64(cfg, st, near, far, detector=True):
    """st: dict(t float64 [L], hist float64 [L] (far values), hang int).  Returns the output (float64 [n])."""
    L, mu, pmin, hang_cfg, dmin = int(cfg["tail"]), int(cfg["mu_shift"]), int(cfg["pmin"]), int(cfg["hang"]), int(cfg["dmin"])
    near = np.asarray(near, np.float64)
    n = len(near)
    buf = np.concatenate([st["hist"], np.asarray(far, np.float64)])
    win = sliding_window_view(buf, L)
    out = near.copy()
    t, hang = st["t"], st["hang"]
    for s in range(0, n, BLOCK):
        b = min(BLOCK, n - s)
        M = win[s + 1:s + 1 + b, ::-1]
        e = near[s:s + b] - M @ t
        out[s:s + b] = e
        end = L + s + b
        P = float((buf[end - L:end] ** 2).sum()) / 16.0                    # of far / 4, as the rule counts it
        xmax = float(np.abs(buf[end - L - b:end]).max())                   # 4 * max |far / 4|
        dmax = float(np.abs(near[s:s + b]).max())
        if detector and 2 * dmax > xmax and dmax >= dmin:
            hang = hang_cfg
        elif hang > 0:
            hang -= 1
        if hang == 0 and P >= pmin:
            q = int(P).bit_length()
            t = t + (M.T @ e) / 16.0 * 2.0 ** (-mu - q)                    # g 2^(31 - mu - q) / 2^31
    st["t"], st["hang"], st["hist"] = t, hang, buf[n:n + L]
    return out


def fresh_f64(L):
    return dict(t=np.zeros(L), hist=np.zeros(L), hang=0)


# ---- scenes
def _law_trip(x, law):
    """int16 [S] through a G.711 round trip (law 0: mu-law, 8: A-law)"""
    from tests import tdet_model
    codec = np.array([law], np.uint8)
    return tdet_model.decode(tdet_model.encode(x.reshape(1, 1, -1), codec), codec)[0, 0]


def speech_like(rng, S, amp=6000.0, rate=8000, phase=0.0):
    """noise through the resonator y = w + 1.6 y1 - 0.8 y2 under a squared 4 Hz envelope (sin^2, starting at `phase`), scaled so that three
    standard deviations of the resonator's output reach amp"""
    w = rng.normal(0.0, 1.0, S)
    y = np.zeros(S)
    y1 = y2 = 0.0
    for i in range(S):
        y[i] = w[i] + 1.6 * y1 - 0.8 * y2
        y2, y1 = y1, y[i]
    env = np.sin(2 * np.pi * 4.0 * np.arange(S) / rate + phase) ** 2
    return amp * env * y / (3.0 * y.std())


def echo_path(rng, loss_db=6.0):
    """12 zeros, then 100 Gaussian taps under exp(-k / 25), scaled to loss_db of loss"""
    h = np.concatenate([np.zeros(12), rng.normal(0.0, 1.0, 100) * np.exp(-np.arange(100) / 25.0)])
    return h * np.sqrt(10.0 ** (-loss_db / 10.0) / (h ** 2).sum())


def echo_scene(seed, seconds=8, law=0, talk=None, rate=8000):
    """One channel: (far int16 [S], near int16 [S], talker float64 [S]).  far: speech-like, through the law; near: the far end through
    the echo path, noise of sigma 20 and the talker (talk = (from_second, to_second): speech-like of the same level there), through
    the law.  Every seed has its own signal and echo path."""
    rng = np.random.default_rng(1000 + seed)
    S = seconds * rate
    far = _law_trip(np.clip(np.rint(speech_like(rng, S)), -32768, 32767).astype(np.int16), law)
    h = echo_path(rng)
    echo = np.convolve(far.astype(np.float64), h)[:S]
    talker = np.zeros(S)
    if talk:
        a, b = int(talk[0] * rate), int(talk[1] * rate)
        talker[a:b] = speech_like(rng, b - a, phase=np.pi / 2)               # its syllables fall into the far end's pauses
    near = echo + rng.normal(0.0, 20.0, S) + talker
    return far, _law_trip(np.clip(np.rint(near), -32768, 32767).astype(np.int16), law), talker


def erle_db(near, out, rate=8000):
    """per whole second: 10 log10(sum near^2 / sum out^2)"""
    S = len(near) // rate * rate
    a = (np.asarray(near[:S], np.float64) ** 2).reshape(-1, rate).sum(axis=1)
    b = (np.asarray(out[:S], np.float64) ** 2).reshape(-1, rate).sum(axis=1)
    return 10.0 * np.log10(np.maximum(a, 1.0) / np.maximum(b, 1.0))


def small_scene(C_, F_, n, seed=0, P_=None):
    """The GPU tests' and the bit-for-bit tests' input: near [F][C][n], far [F][P][n] int16.  Far row p: speech-like noise at its own
    level (every fifth row silent, every seventh full scale); channel c hears row c % P through a short decaying path plus, on every
    third channel, a loud talker in frames 1, 4, 7, .. (so the detector fires and the hang runs out again)."""
    P_ = C_ if P_ is None else P_
    rng = np.random.default_rng(77 + seed)
    S = F_ * n
    far = np.zeros((max(P_, 1), S))
    for p in range(max(P_, 1)):
        x = rng.normal(0.0, 1.0, S + 2)
        x = x[2:] + 0.9 * x[1:-1] + 0.5 * x[:-2]
        far[p] = 0.0 if p % 5 == 4 else x * (30000.0 if p % 7 == 6 else 1500.0 + 700.0 * (p % 4))
    far = np.clip(np.rint(far), -32768, 32767)
    near = np.zeros((C_, S))
    for c in range(C_):
        h = rng.normal(0.0, 0.12, 24) * np.exp(-np.arange(24) / 8.0)
        near[c] = np.convolve(far[c % max(P_, 1)], h)[:S] + rng.normal(0.0, 12.0, S)
        if c % 3 == 2:
            for f in range(1, F_, 3):
                near[c, f * n:(f + 1) * n] += rng.normal(0.0, 9000.0, n)
    near = np.clip(np.rint(near), -32768, 32767)
    cut = lambda a: np.ascontiguousarray(a.astype(np.int16).reshape(a.shape[0], F_, n).transpose(1, 0, 2))
    return cut(near), cut(far)[:, :P_]


def garbage_state(C_, L, seed=0, saturated=False):
    """STATE [C] with the right tag and arbitrary bytes everywhere else (saturated: every weight at an end of int32, the history at the
    ends of int16, which the rule reads clamped)"""
    rng = np.random.default_rng(5 + seed)
    st = np.frombuffer(rng.integers(0, 256, C_ * STATE.itemsize, dtype=np.uint8).tobytes(), STATE).copy()
    if saturated:
        st["w"] = np.where(rng.integers(0, 2, st["w"].shape) == 1, (1 << 31) - 1, -(1 << 31))
        st["hist"] = np.where(rng.integers(0, 2, st["hist"].shape) == 1, 32767, -32768)
    st["tag"] = TAG | L
    st["hang"][::2] %= 3                                                   # every other channel adapts within a few blocks
    return st
