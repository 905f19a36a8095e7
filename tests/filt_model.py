"""The numpy statement of the filter (include/igdsp.h, "Filter"): chains of second-order sections in Q13 with first-order error
feedback, written from the header's text, not from csrc/igdsp_filt.h.  Every channel of a launch walks together: the sample loop is
Python, each step an int64 array over the channels, and a section that does not run is simply skipped (the library runs an identity in
its place).  Every accumulator is checked against int32.  Also here: the float64 RBJ designs and presets the library's
igdsp_filt_design / igdsp_filt_plan_preset are tested against, the float64 response of quantised coefficients, and the PCM record."""
import numpy as np

from tests import record_model

TAG, UNITY, EMASK, SUM_MAX = 0xF1170001, 8192, 8191, 65535
RUN, BYPASS, RESET = 0, 1, 2
CLIPPED, NO_PLAN, BAD_PLAN, BYPASSED, WAS_RESET = 1, 2, 4, 8, 16
LOWPASS, HIGHPASS, BANDPASS, NOTCH, PEAK, LOWSHELF, HIGHSHELF, LP1, HP1 = range(9)
VOICE_BAND, CTCSS_HP, DEEMPH, PREEMPH, DC_BLOCK = range(5)
PRESETS = (VOICE_BAND, CTCSS_HP, DEEMPH, PREEMPH, DC_BLOCK)
SECTION = np.dtype([("c", "<i2", (5,))])                                   # b0 b1 b2 a1 a2
PLAN = np.dtype([("n_sections", "<u2"), ("reserved", "<u2"), ("clock_rate", "<u4"), ("c", "<i2", (4, 5))])
STATE = np.dtype([("tag", "<u4"), ("h", "<u2", (4, 5)), ("flags", "<u2"), ("reserved", "<u2")])   # h: x1 x2 y1 y2 e as their 16 bits
REC = np.dtype([("in_peak", "<u2"), ("out_peak", "<u2"), ("n_clipped", "<u2"), ("plan", "<u2"), ("flags", "u1"), ("n_sections", "u1"), ("reserved", "u1", (6,))])
assert PLAN.itemsize == 48 and STATE.itemsize == 48 and REC.itemsize == 16
IDENTITY = (UNITY, 0, 0, 0, 0)


def plan_of_sections(sections, clock_rate=8000, n_sections=None):
    """a PLAN record from up to four (b0, b1, b2, a1, a2); the rest identity"""
    p = np.zeros((), PLAN)
    p["n_sections"] = len(sections) if n_sections is None else n_sections
    p["clock_rate"] = clock_rate
    for i in range(4):
        p["c"][i] = sections[i] if i < len(sections) else IDENTITY
    return p


def valid(c):
    return sum(abs(int(v)) for v in c) <= SUM_MAX


def garbage_state(C_, seed, tagged=True):
    rng = np.random.default_rng(seed)
    st = rng.integers(0, 256, C_ * STATE.itemsize, dtype=np.uint8).view(STATE).copy()
    if tagged:
        st["tag"] = TAG
    else:
        st["tag"][st["tag"] == TAG] = 0
    return st


def run(plans, x, plan_of=None, ctl=None, state=None, max_sections=0):
    """plans [n_plans] PLAN (any bytes), x [F][C][n] integers in int16, plan_of [C] or None, ctl [C] or None, state [C] STATE or None
    (all-zero).  Returns (out [F][C][n] int16, rec [F][C] REC, stats [F][C] record_model.STATS, state [C] STATE)."""
    x = np.asarray(x).astype(np.int64)
    F_, C_, n = x.shape
    plans = np.atleast_1d(np.asarray(plans, PLAN))
    pi = np.zeros(C_, np.int64) if plan_of is None else np.asarray(plan_of).astype(np.int64)
    ctl = np.zeros(C_, np.int64) if ctl is None else np.asarray(ctl).astype(np.int64)
    ctl = np.where(ctl > 2, RUN, ctl)
    st = np.zeros(C_, STATE) if state is None else np.array(state, STATE)
    max_s = 4 if max_sections == 0 else max_sections
    have = pi < len(plans)
    mine = plans[np.where(have, pi, 0)]
    ns = np.where(have, np.minimum(mine["n_sections"].astype(np.int64), 4), 0)
    coef = mine["c"].astype(np.int64)                                      # [C][4][5]
    pflags = np.where(ns == 0, NO_PLAN, np.where(ns > max_s, NO_PLAN | BAD_PLAN, 0))
    bypass = ctl == BYPASS
    passes = bypass | ((pflags & NO_PLAN) != 0)
    wanted = (np.arange(4)[None, :] < ns[:, None]) & ~passes[:, None]      # [C][4]
    ok = np.abs(coef).sum(axis=2) <= SUM_MAX
    runs = wanted & ok
    base = np.where(bypass, BYPASSED, pflags | np.where((wanted & ~ok).any(axis=1), BAD_PLAN, 0))
    zeroed = (st["tag"] != TAG) | (ctl == RESET)
    h = st["h"].astype(np.uint16).view(np.int16).astype(np.int64).reshape(C_, 4, 5)
    h[:, :, 4] &= 0xFFFF
    h[:, :, 4] &= EMASK
    h[zeroed] = 0
    out = np.zeros((F_, C_, n), np.int64)
    rec = np.zeros((F_, C_), REC)
    for f in range(F_):
        clipped = np.zeros(C_, np.int64)
        for j in range(n):
            v = x[f, :, j].copy()
            for s in range(4):
                r = runs[:, s]
                if not r.any():
                    continue
                c = coef[:, s]
                acc = c[:, 0] * v + c[:, 1] * h[:, s, 0] + c[:, 2] * h[:, s, 1] - c[:, 3] * h[:, s, 2] - c[:, 4] * h[:, s, 3] + h[:, s, 4]
                assert (np.abs(acc[r]) < 1 << 31).all()
                y = acc >> 13
                e = acc & EMASK
                hi, lo = y > 32767, y < -32768
                y = np.clip(y, -32768, 32767)
                e[hi | lo] = 0
                clipped += (r & (hi | lo))
                new = np.stack([v, h[:, s, 0], y, h[:, s, 2], e], axis=1)
                h[:, s] = np.where(r[:, None], new, h[:, s])
                v = np.where(r, y, v)
            out[f, :, j] = v
        rec["in_peak"][f] = np.abs(x[f]).max(axis=1)
        rec["out_peak"][f] = np.abs(out[f]).max(axis=1)
        rec["n_clipped"][f] = np.minimum(clipped, 65535)
        rec["plan"][f] = pi & 0xFFFF
        rec["n_sections"][f] = ns
        rec["flags"][f] = base | np.where(clipped > 0, CLIPPED, 0) | (np.where(zeroed & ~passes, WAS_RESET, 0) if f == 0 else 0)
    new = np.array(st)
    if F_:
        keep = passes
        hw = h.copy()
        nh = (hw & 0xFFFF).astype(np.uint16)
        new["tag"] = np.where(keep, st["tag"], TAG)
        new["h"] = np.where(keep[:, None, None], st["h"], nh)
        new["flags"] = np.where(keep, st["flags"], rec["flags"][-1])
        new["reserved"] = np.where(keep, st["reserved"], 0)
    return out.astype(np.int16), rec, record_model.records(out), new


def yardstick_state(state):
    """the state igdsp_internal_filt_move leaves: as read (e masked; another tag: zero histories), with the tag, flags as read, reserved 0"""
    st = np.array(state, STATE)
    bad = st["tag"] != TAG
    st["h"][:, :, 4] &= EMASK
    st["h"][bad] = 0
    st["flags"][bad] = 0
    st["tag"] = TAG
    st["reserved"] = 0
    return st


# ---- float64: the designs, the presets, the response
def design_real(kind, rate, f0, q=np.sqrt(0.5), gain_db=0.0):
    """(b0, b1, b2, a1, a2) over a0 = 1 in float64: the RBJ cookbook, first-order LP1 / HP1 by the bilinear transform"""
    if kind in (LP1, HP1):
        K = np.tan(np.pi * f0 / rate)
        a1 = (K - 1) / (K + 1)
        return (K / (1 + K), K / (1 + K), 0.0, a1, 0.0) if kind == LP1 else (1 / (1 + K), -1 / (1 + K), 0.0, a1, 0.0)
    w0 = 2 * np.pi * f0 / rate
    cs, al, A = np.cos(w0), np.sin(w0) / (2 * q), 10 ** (gain_db / 40)
    if kind == LOWPASS:
        b, a = ((1 - cs) / 2, 1 - cs, (1 - cs) / 2), (1 + al, -2 * cs, 1 - al)
    elif kind == HIGHPASS:
        b, a = ((1 + cs) / 2, -(1 + cs), (1 + cs) / 2), (1 + al, -2 * cs, 1 - al)
    elif kind == BANDPASS:
        b, a = (al, 0.0, -al), (1 + al, -2 * cs, 1 - al)
    elif kind == NOTCH:
        b, a = (1.0, -2 * cs, 1.0), (1 + al, -2 * cs, 1 - al)
    elif kind == PEAK:
        b, a = (1 + al * A, -2 * cs, 1 - al * A), (1 + al / A, -2 * cs, 1 - al / A)
    elif kind == LOWSHELF:
        r = 2 * np.sqrt(A) * al
        b = (A * ((A + 1) - (A - 1) * cs + r), 2 * A * ((A - 1) - (A + 1) * cs), A * ((A + 1) - (A - 1) * cs - r))
        a = ((A + 1) + (A - 1) * cs + r, -2 * ((A - 1) + (A + 1) * cs), (A + 1) + (A - 1) * cs - r)
    elif kind == HIGHSHELF:
        r = 2 * np.sqrt(A) * al
        b = (A * ((A + 1) + (A - 1) * cs + r), -2 * A * ((A - 1) + (A + 1) * cs), A * ((A + 1) + (A - 1) * cs - r))
        a = ((A + 1) - (A - 1) * cs + r, 2 * ((A - 1) - (A + 1) * cs), (A + 1) - (A - 1) * cs - r)
    else:
        raise ValueError(kind)
    return (b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0])


def response(c, f, rate, unity=1.0):
    """|H| at f Hz (scalar or array) of one section (b0, b1, b2, a1, a2) whose 1.0 is `unity` (8192 for quantised coefficients)"""
    c = np.asarray(c, np.float64) / unity
    z = np.exp(-2j * np.pi * np.asarray(f, np.float64) / rate)
    return np.abs((c[0] + c[1] * z + c[2] * z * z) / (1 + c[3] * z + c[4] * z * z))


def quantise(c):
    """to the nearest Q13; None when a coefficient leaves int16, the section is invalid or the quantised poles are not strictly inside"""
    q = [int(np.rint(v * UNITY)) for v in c]
    if any(v < -32768 or v > 32767 for v in q) or not valid(q) or not (abs(q[4]) < UNITY and abs(q[3]) < UNITY + q[4]):
        return None
    return tuple(q)


def preset_sections(preset, rate):
    """the preset's quantised sections, or None where the library returns IGDSP_EINVAL"""
    if not 8000 <= rate <= 48000:
        return None
    bw = np.sqrt(0.5)
    if preset == VOICE_BAND:
        real = [design_real(HIGHPASS, rate, 300.0, bw), design_real(LOWPASS, rate, 3400.0, bw)] if 3400 < rate / 2 else None
    elif preset == CTCSS_HP:
        real = [design_real(HIGHPASS, rate, 300.0, 1 / (2 * np.cos(np.pi / 8))), design_real(HIGHPASS, rate, 300.0, 1 / (2 * np.cos(3 * np.pi / 8)))]
    elif preset in (DEEMPH, PREEMPH):
        if not 3400 < rate / 2:
            return None
        za, zp = np.exp(-2 * np.pi * 300.0 / rate), np.exp(-2 * np.pi * 3400.0 / rate)
        c = (1.0, -za, 0.0, -zp, 0.0) if preset == PREEMPH else (1.0, -zp, 0.0, -za, 0.0)
        g = 1 / response(c, 1000.0, rate)
        real = [(c[0] * g, c[1] * g, 0.0, c[3], 0.0)]
    elif preset == DC_BLOCK:
        real = [design_real(HP1, rate, 20.0)]
    else:
        return None
    if real is None:
        return None
    q = [quantise(c) for c in real]
    return None if any(v is None for v in q) else q


def plan_response(sections, f, rate):
    """the float64 response of a chain of quantised sections"""
    r = np.ones_like(np.asarray(f, np.float64))
    for c in sections:
        r = r * response(c, f, rate, UNITY)
    return r


def sine(amp, freq, rate, count):
    return np.rint(amp * np.sin(2 * np.pi * freq * np.arange(count) / rate)).astype(np.int16)


def rms_db(x):
    x = np.asarray(x, np.float64)
    return 10 * np.log10(max(np.mean(x * x), 1e-30))
