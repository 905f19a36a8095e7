"""The numpy statement of the noise suppressor (include/igdsp.h, "Noise suppression"), written from the header's text, not from
csrc/igdsp_ns.h: the rule in exact integers, transform included, step for step as the header has it (every channel of a launch walks
together: the hop loop is Python, each step an int64 array over the channels; every value of the transform is checked against int32),
and beside it the same rule in float64 with no rounding (run_float), for the quality figures.  The tables are made here from their
float64 formulas.  Also here: the scenes of tests/test_ns_cpu.py and the level measures."""
import numpy as np

from tests import record_model

TAG, HOP, BANDS, UNITY, POINTS = 0x4E530001, 80, 32, 32768, 128
RUN, FREEZE, BYPASS, RESET = 0, 1, 2, 3
LEARNING, SUPPRESSING, CLIPPED, FROZEN, BYPASSED, WAS_RESET = 1, 2, 4, 8, 16, 32
LEVEL_MASK = (1 << 56) - 1
CFG = np.dtype([("floor_q15", "<u4"), ("over_q4", "<u2"), ("init_hops", "<u2"), ("track_shift", "<u2"), ("rise_shift", "<u2"), ("reserved", "<u4")])
STATE = np.dtype([("tag", "<u4"), ("hops", "<u2"), ("flags", "<u2"), ("reserved", "<u4", (2,)), ("prev", "<i2", (80,)), ("ola", "<i4", (80,)),
                  ("S", "<u8", (32,)), ("N", "<u8", (32,)), ("Gt", "<u2", (32,))])
REC = np.dtype([("in_energy", "<u4"), ("out_energy", "<u4"), ("min_gain_q15", "<u2"), ("n_clipped", "<u2"), ("noise_idx", "u1"), ("flags", "u1"),
                ("reserved", "u1", (2,))])
assert CFG.itemsize == 16 and STATE.itemsize == 1072 and REC.itemsize == 16
DEFAULTS = dict(floor_q15=5827, over_q4=24, init_hops=16, track_shift=4, rise_shift=9)
RANGES = dict(floor_q15=(1, 32768), over_q4=(16, 64), init_hops=(1, 255), track_shift=(1, 8), rise_shift=(4, 12))

WIN_REAL = 32768.0 * np.sin(np.pi * (np.arange(2 * HOP) + 0.5) / (2 * HOP))
WIN = np.rint(WIN_REAL).astype(np.int64)
_A = 2.0 * np.pi * np.arange(POINTS) / (2 * POINTS)
TW = np.rint(np.stack([np.cos(_A), np.sin(_A)], axis=1) * float(1 << 30)).astype(np.int64)    # [128][2], Q30
REV = np.array([int(format(k, "07b")[::-1], 2) for k in range(POINTS)])
BAND_OF = np.concatenate([[0], (np.arange(1, POINTS + 1) - 1) >> 2])                            # bins 0 .. 128


def cfg_of(**kw):
    c = np.zeros((), CFG)
    for k, v in {**DEFAULTS, **kw}.items():
        c[k] = v
    return c


def cfg_ok(c):
    return all(RANGES[k][0] <= int(c[k]) <= RANGES[k][1] for k in RANGES)


def garbage_state(C_, seed, tagged=True):
    rng = np.random.default_rng(seed)
    st = rng.integers(0, 256, C_ * STATE.itemsize, dtype=np.uint8).view(STATE).copy()
    if tagged:
        st["tag"] = TAG
    else:
        st["tag"][st["tag"] == TAG] = 0
    return st


def _i32(*arrays):
    for a in arrays:
        assert (np.abs(a) < 1 << 31).all()


def _passes(zr, zi, inverse):
    """seven radix-2 passes in place over [C][128]: forward decimation in frequency (natural in, bit-reversed out), inverse decimation in
    time with a halving per pass (bit-reversed in, natural out)"""
    b = np.arange(POINTS // 2)
    for sh in (range(7) if inverse else range(6, -1, -1)):
        half = 1 << sh
        pos = b & (half - 1)
        i = ((b >> sh) << (sh + 1)) + pos
        j = i + half
        c, s = TW[pos << (7 - sh), 0], TW[pos << (7 - sh), 1]
        pr, pi, qr, qi = zr[:, i], zi[:, i], zr[:, j], zi[:, j]
        if inverse:
            tr, ti = qr * c - qi * s, qi * c + qr * s
            zr[:, i], zi[:, i] = ((pr << 30) + tr + (1 << 30)) >> 31, ((pi << 30) + ti + (1 << 30)) >> 31
            zr[:, j], zi[:, j] = ((pr << 30) - tr + (1 << 30)) >> 31, ((pi << 30) - ti + (1 << 30)) >> 31
        else:
            dr, di = pr - qr, pi - qi
            zr[:, i], zi[:, i] = pr + qr, pi + qi
            zr[:, j], zi[:, j] = (dr * c + di * s + (1 << 29)) >> 30, (di * c - dr * s + (1 << 29)) >> 30
        _i32(zr, zi)


def forward(xw):
    """xw [C][160] Q7 -> bins 0 .. 128 as (re [C][129], im [C][129])"""
    C_ = xw.shape[0]
    pad = np.zeros((C_, 2 * POINTS), np.int64)
    pad[:, :2 * HOP] = xw
    zr, zi = pad[:, 0::2].copy(), pad[:, 1::2].copy()
    _passes(zr, zi, False)
    Zr, Zi = zr[:, REV], zi[:, REV]                                         # bin k of the 128-point transform
    k = np.arange(1, POINTS)
    c, s = TW[k, 0], TW[k, 1]
    Ar, Ai, Br, Bi = Zr[:, k], Zi[:, k], Zr[:, POINTS - k], -Zi[:, POINTS - k]
    Er, Ei, Or, Oi = Ar + Br, Ai + Bi, Ar - Br, Ai - Bi
    Xr, Xi = np.zeros((C_, POINTS + 1), np.int64), np.zeros((C_, POINTS + 1), np.int64)
    Xr[:, k] = ((Er << 30) - s * Or + c * Oi + (1 << 30)) >> 31
    Xi[:, k] = ((Ei << 30) - s * Oi - c * Or + (1 << 30)) >> 31
    Xr[:, 0], Xr[:, POINTS] = Zr[:, 0] + Zi[:, 0], Zr[:, 0] - Zi[:, 0]
    _i32(Xr, Xi)
    return Xr, Xi


def inverse(Yr, Yi):
    """bins 0 .. 128 -> y [C][160] Q7, the 1/256 inside"""
    C_ = Yr.shape[0]
    k = np.arange(1, POINTS)
    c, s = TW[k, 0], TW[k, 1]
    Ar, Ai, Br, Bi = Yr[:, k], Yi[:, k], Yr[:, POINTS - k], -Yi[:, POINTS - k]
    Er, Ei, Or, Oi = Ar + Br, Ai + Bi, Ar - Br, Ai - Bi
    Zr, Zi = np.zeros((C_, POINTS), np.int64), np.zeros((C_, POINTS), np.int64)
    Zr[:, k] = ((Er << 30) - s * Or - c * Oi + (1 << 30)) >> 31
    Zi[:, k] = ((Ei << 30) - s * Oi + c * Or + (1 << 30)) >> 31
    Zr[:, 0], Zi[:, 0] = (Yr[:, 0] + Yr[:, POINTS] + 1) >> 1, (Yr[:, 0] - Yr[:, POINTS] + 1) >> 1
    _i32(Zr, Zi)
    zr, zi = np.zeros_like(Zr), np.zeros_like(Zi)
    zr[:, REV], zi[:, REV] = Zr, Zi
    _passes(zr, zi, True)
    y = np.zeros((C_, 2 * POINTS), np.int64)
    y[:, 0::2], y[:, 1::2] = zr, zi
    return y[:, :2 * HOP]


def bitlen(v):
    """bit length of non-negative integers below 2^63, exact: frexp of each 32-bit half, which a float64 holds exactly"""
    v = np.asarray(v, np.int64)
    hi, lo = v >> 32, v & 0xFFFFFFFF
    return np.where(hi > 0, 32 + np.frexp(hi.astype(np.float64))[1], np.frexp(lo.astype(np.float64))[1]).astype(np.int64)


def run(x, cfg=None, ctl=None, state=None, trace=None):
    """x [F][C][n] integers in int16 (n = 80, 160, 240 or 320), cfg a CFG record or None (the defaults), ctl [C] or None, state [C] STATE or
    None (all-zero).  Returns (out [F][C][n] int16, rec [F][C] REC, stats [F][C] record_model.STATS, state [C] STATE).  trace: a dict that
    gets "N", "S" and "Gt" as lists of [C][32] arrays, one per hop."""
    x = np.asarray(x).astype(np.int64)
    F_, C_, n = x.shape
    assert n in (80, 160, 240, 320)
    cfg = cfg_of() if cfg is None else cfg
    assert cfg_ok(cfg)
    floor, over, init, track, rise = (int(cfg[k]) for k in ("floor_q15", "over_q4", "init_hops", "track_shift", "rise_shift"))
    ctl = np.zeros(C_, np.int64) if ctl is None else np.asarray(ctl).astype(np.int64)
    ctl = np.where(ctl > 3, RUN, ctl)
    st = np.zeros(C_, STATE) if state is None else np.array(state, STATE)
    fresh = (st["tag"] != TAG) | (ctl == RESET)
    bypass, frozen = ctl == BYPASS, ctl == FREEZE
    live = ~bypass                                                          # channels that run the hop
    hops = np.where(fresh, 0, st["hops"].astype(np.int64))
    prev = np.where(fresh[:, None], 0, st["prev"].astype(np.int64))
    ola = np.where(fresh[:, None], 0, st["ola"].astype(np.int64))
    S = np.where(fresh[:, None], 0, (st["S"] & np.uint64(LEVEL_MASK)).astype(np.int64))
    N = np.where(fresh[:, None], 0, (st["N"] & np.uint64(LEVEL_MASK)).astype(np.int64))
    Gt = np.where(fresh[:, None], UNITY, np.minimum(st["Gt"].astype(np.int64), UNITY))
    out = np.zeros((F_, C_, n), np.int64)
    rec = np.zeros((F_, C_), REC)
    for f in range(F_):
        clipped, learning, min_gain = np.zeros(C_, np.int64), np.zeros(C_, bool), np.full(C_, UNITY, np.int64)
        for h in range(0, n, HOP):
            cur = x[f, :, h:h + HOP]
            win = np.concatenate([prev, cur], axis=1)
            xw = (win * WIN + 128) >> 8
            Xr, Xi = forward(xw)
            P = Xr * Xr + Xi * Xi                                           # < 2^61
            E = P[:, 1:].reshape(C_, BANDS, 4).sum(axis=2) >> 14
            S1 = np.where((hops == 0)[:, None], E, S + ((E - S) >> 2))
            first = (hops < init)[:, None]
            N1 = np.where(first, N + ((S1 - N) >> 2), np.where(S1 < 4 * N, N + ((S1 - N) >> track), N + (N >> rise) + 1))
            hold = (frozen | bypass)[:, None]
            N1 = np.where(hold, N, N1)
            learning |= live & ~frozen & (hops < init)
            d = S1 - ((over * N1) >> 4)
            t = np.maximum(0, bitlen(S1) - 16)
            G = np.minimum(UNITY, ((d >> t) << 15) // np.maximum(1, S1 >> t))
            G = np.maximum(np.where((d <= 0) | (S1 == 0), 0, G), floor)
            Ge = np.concatenate([G[:, :1], G, G[:, -1:]], axis=1)
            Gs = (Ge[:, :-2] + 2 * Ge[:, 1:-1] + Ge[:, 2:] + 2) >> 2
            Gt1 = np.where(Gs >= Gt, Gs, Gt + ((Gs - Gt) >> 1))
            gb = Gt1[:, BAND_OF]
            y = inverse((Xr * gb + 16384) >> 15, (Xi * gb + 16384) >> 15)
            yw = (y * WIN + 16384) >> 15
            o = (ola + yw[:, :HOP] + 64) >> 7
            oc = np.clip(o, -32768, 32767)
            # a bypassed channel: the input through the same delay; ola as unity gains would leave it
            xb = (cur * WIN[HOP:] + 128) >> 8
            ola_b = (xb * WIN[HOP:] + 16384) >> 15
            out[f, :, h:h + HOP] = np.where(bypass[:, None], prev, oc)
            clipped += np.where(live, (oc != o).sum(axis=1), 0)
            ola = np.where(bypass[:, None], ola_b, yw[:, HOP:])
            prev = cur.copy()
            S = np.where(hold, S, S1)
            N = N1
            Gt = np.where(bypass[:, None], Gt, Gt1)
            min_gain = np.where(live, np.minimum(min_gain, Gt1.min(axis=1)), min_gain)
            hops = np.where(hold[:, 0], hops, np.minimum(hops + 1, 65535))
            if trace is not None:
                for k, v in (("N", N), ("S", S), ("Gt", Gt)):
                    trace.setdefault(k, []).append(v.copy())
        rec["in_energy"][f] = (x[f] * x[f]).sum(axis=1) >> 8
        rec["out_energy"][f] = (out[f] * out[f]).sum(axis=1) >> 8
        rec["min_gain_q15"][f] = min_gain
        rec["n_clipped"][f] = np.minimum(clipped, 65535)
        rec["noise_idx"][f] = bitlen(N.sum(axis=1))                # 32 values below 2^56
        fl = (np.where(learning, LEARNING, 0) | np.where(min_gain < UNITY, SUPPRESSING, 0) | np.where(clipped > 0, CLIPPED, 0) | np.where(frozen, FROZEN, 0) |
              (np.where(fresh, WAS_RESET, 0) if f == 0 else 0))
        rec["flags"][f] = np.where(bypass, BYPASSED, fl)
    new = np.array(st)
    if F_:
        new["tag"], new["hops"], new["flags"], new["reserved"] = TAG, hops, rec["flags"][-1], 0
        new["prev"], new["ola"], new["S"], new["N"], new["Gt"] = prev, ola, S.astype(np.uint64), N.astype(np.uint64), Gt
    return out.astype(np.int16), rec, record_model.records(out), new


def run_float(x, cfg=None):
    """the same rule in float64 with no rounding and no saturation, RUN from a fresh state: x [F][C][n] -> out [F][C][n] float64"""
    x = np.asarray(x, np.float64)
    F_, C_, n = x.shape
    cfg = cfg_of() if cfg is None else cfg
    floor, over, init, track, rise = (float(cfg[k]) for k in ("floor_q15", "over_q4", "init_hops", "track_shift", "rise_shift"))
    prev, ola = np.zeros((C_, HOP)), np.zeros((C_, HOP))
    S, N, Gt = np.zeros((C_, BANDS)), np.zeros((C_, BANDS)), np.full((C_, BANDS), float(UNITY))
    out = np.zeros((F_, C_, n))
    hops = 0
    for f in range(F_):
        for h in range(0, n, HOP):
            cur = x[f, :, h:h + HOP]
            xw = np.concatenate([prev, cur], axis=1) * WIN_REAL / 256.0
            X = np.fft.rfft(xw, 2 * POINTS, axis=1)
            E = (np.abs(X[:, 1:]) ** 2).reshape(C_, BANDS, 4).sum(axis=2) / 16384.0
            S = E if hops == 0 else S + (E - S) / 4.0
            if hops < init:
                N = N + (S - N) / 4.0
            else:
                N = np.where(S < 4 * N, N + (S - N) / 2.0 ** track, N + N / 2.0 ** rise)
            d = S - over * N / 16.0
            G = np.where((d <= 0) | (S == 0), 0.0, np.minimum(1.0, d / np.maximum(S, 1e-300))) * UNITY
            G = np.maximum(G, floor)
            Ge = np.concatenate([G[:, :1], G, G[:, -1:]], axis=1)
            Gs = (Ge[:, :-2] + 2 * Ge[:, 1:-1] + Ge[:, 2:]) / 4.0
            Gt = np.where(Gs >= Gt, Gs, Gt + (Gs - Gt) / 2.0)
            y = np.fft.irfft(X * Gt[:, BAND_OF] / UNITY, 2 * POINTS, axis=1)[:, :2 * HOP]
            yw = y * WIN_REAL / 32768.0
            out[f, :, h:h + HOP] = (ola + yw[:, :HOP]) / 128.0
            ola, prev = yw[:, HOP:], cur.copy()
            hops += 1
    return out


# ---- scenes and measures (8 kHz)
def noise(sigma, count, seed):
    return np.clip(np.rint(np.random.default_rng(seed).normal(0.0, sigma, count)), -32768, 32767).astype(np.int16)


def bursts(count, seed, rms=4000.0, on=0.4, off=0.3, lead=1.0, rate=8000):
    """harmonic bursts: 19 harmonics at 1/k of a fundamental drawn from 110 - 170 Hz per burst, RMS `rms` over a burst, `on` seconds on and
    `off` seconds off, nothing in the first `lead` seconds.  Returns (signal float64 [count], mask bool [count]: inside a burst)"""
    rng = np.random.default_rng(seed)
    sig, mask = np.zeros(count), np.zeros(count, bool)
    a, n_on, n_off = int(lead * rate), int(on * rate), int(off * rate)
    while a < count:
        m = min(n_on, count - a)
        t = np.arange(m) / rate
        f0 = rng.uniform(110.0, 170.0)
        b = sum(np.sin(2 * np.pi * k * f0 * t + rng.uniform(0, 2 * np.pi)) / k for k in range(1, 20))
        sig[a:a + m] = b * rms / np.sqrt(np.mean(b * b))
        mask[a:a + m] = True
        a += n_on + n_off
    return sig, mask


def frames_of(x, n=160):
    """a signal [count] (count a multiple of n) as one channel's rows [F][1][n]"""
    x = np.asarray(x)
    return x.reshape(-1, 1, n)


def level_db(x):
    x = np.asarray(x, np.float64)
    return 10 * np.log10(max(np.mean(x * x), 1e-30))
