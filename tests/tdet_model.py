"""The tone detector of include/igdsp.h ("Tone detector"), restated in numpy from the header's text: plan, table, the two evaluations
per frame, the hit rule with its shifts, the debounce, the records, the event list.  Vectorised over channels (a frame's evaluation is
one integer matrix product), sequential over evaluations.  The CPU tests compare igdsp_tdet_frame with it, the GPU tests
igdsp_tone_detect; the detection properties (digits, twist, offset, talk-off, noise, duration) are measured with it as well."""
import math

import numpy as np

T = np.array([math.floor(32767 * math.sin(2 * math.pi * i / 1024) + 0.5) for i in range(1024)], np.int64)
DTMF_LO, DTMF_HI = (697, 770, 852, 941), (1209, 1336, 1477, 1633)
DIGITS = "123A456B789C*0#D"
DEFAULT_THR = dict(min_amp=400, rel_q8=1024, fwd_q8=673, rev_q8=1615, frac_q8=150, min_on=3, min_off=2)
ON0, OFF0, ON1, OFF1 = 1, 2, 4, 8

THR = np.dtype([("min_amp", "<u2"), ("rel_q8", "<u2"), ("fwd_q8", "<u2"), ("rev_q8", "<u2"), ("frac_q8", "<u2"), ("min_on", "u1"), ("min_off", "u1")])
PLAN = np.dtype([("clock_rate", "<u4"), ("n_lo", "u1"), ("n_hi", "u1"), ("reserved", "u1", (2,)), ("thr", THR), ("step", "<u4", (16,))])
STATE = np.dtype([("hist", "<i2", (128,)), ("cur", "u1"), ("cand", "u1"), ("run", "u1"), ("off", "u1"), ("len", "<u2"), ("reserved", "<u2")])
REC = np.dtype([("hit", "u1", (2,)), ("cur", "u1"), ("flags", "u1"), ("len", "<u2"), ("code", "u1"), ("reserved", "u1")])
EVENT = np.dtype([("channel", "<u4"), ("frame", "<u4"), ("rec", REC)])
assert (THR.itemsize, PLAN.itemsize, STATE.itemsize, REC.itemsize, EVENT.itemsize) == (12, 84, 264, 8, 16)


def step_of(freq, clock_rate):
    return ((freq << 32) + clock_rate // 2) // clock_rate


def plan_build(lo, hi=(), clock_rate=8000, **thr):
    """one PLAN record; thr: fields of DEFAULT_THR to change"""
    t = dict(DEFAULT_THR, **thr)
    p = np.zeros((), PLAN)
    p["clock_rate"], p["n_lo"], p["n_hi"] = clock_rate, len(lo), len(hi)
    for k, v in t.items():
        p["thr"][k] = v
    for k, f in enumerate(list(lo) + list(hi)):
        assert 1 <= f <= clock_rate // 2 - 1
        p["step"][k] = step_of(int(f), clock_rate)
    return p


def plan_dtmf(clock_rate=8000, **thr):
    return plan_build(DTMF_LO, DTMF_HI, clock_rate, **thr)


def digit(code):
    return DIGITS[code - 1] if 1 <= code <= 16 else ""


def osc(ph):
    ph = np.asarray(ph, np.int64) & 0xFFFFFFFF
    i, fr = ph >> 22, (ph >> 6) & 0xFFFF
    return T[i] + (((T[(i + 1) & 1023] - T[i]) * fr) >> 16)


def tdiv16(a):
    return np.sign(a) * (np.abs(a) // 16)


def table(plan, n):
    """int64 [n_lo + n_hi][2][n]: the cosine column, then the sine column"""
    nf = min(int(plan["n_lo"]), 8) + min(int(plan["n_hi"]), 8)
    i = np.arange(n, dtype=np.int64)
    out = np.zeros((nf, 2, n), np.int64)
    for k in range(nf):
        ph = i * int(plan["step"][k])
        out[k, 0] = tdiv16(osc(ph + 0x40000000))
        out[k, 1] = tdiv16(osc(ph))
    return out


def _wrap32(a):
    return ((a + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def evaluate(plan, tab, w):
    """w int64 [C][n]: the windows' values v -> the hit codes [C]"""
    C_, n = w.shape
    nlo, nhi = min(int(plan["n_lo"]), 8), min(int(plan["n_hi"]), 8)
    thr = {k: int(plan["thr"][k]) for k in THR.names}
    I = _wrap32(w @ tab[:, 0].T)
    Q = _wrap32(w @ tab[:, 1].T)
    P = np.abs(I).astype(np.uint64) ** 2 + np.abs(Q).astype(np.uint64) ** 2                 # [C][nf]
    E = (w * w).sum(1).astype(np.uint64)
    eref = (E * np.uint64(n // 2) * np.uint64(2047 * 2047)) >> np.uint64(16)
    floor = np.uint64(((thr["min_amp"] >> 3) * 2047 * (n // 2)) ** 2)
    u = np.uint64

    def group(first, count):
        if count == 0:
            return np.zeros(C_, bool), np.zeros(C_, np.int64), np.zeros(C_, np.uint64)
        g = P[:, first:first + count]
        idx = np.argmax(g, 1)                                                               # the first of the largest
        pw = g[np.arange(C_), idx]
        ok = pw >= floor
        S, Sb = g >> u(16), (pw >> u(16))[:, None]
        fails = (Sb * u(256) < u(thr["rel_q8"]) * S) & (np.arange(count)[None, :] != idx[:, None])
        return ok & ~fails.any(1), idx, pw

    ok_lo, i_lo, p_lo = group(0, nlo)
    ok_hi, i_hi, p_hi = group(nlo, nhi)
    s_lo, s_hi = p_lo >> u(16), p_hi >> u(16)
    hit = ok_lo
    if nhi:
        hit = hit & ok_hi & (s_hi * u(256) <= u(thr["fwd_q8"]) * s_lo) & (s_lo * u(256) <= u(thr["rev_q8"]) * s_hi)
        code = 1 + i_lo * nhi + i_hi
    else:
        s_hi = np.zeros_like(s_lo)
        code = i_lo + 1
    hit = hit & ((s_lo + s_hi) * u(256) >= u(thr["frac_q8"]) * eref)
    return np.where(hit, code, 0).astype(np.int64)


def debounce(d, h, min_on, min_off):
    """d: dict of int64 arrays cur, cand, run, off, len, code; h [C] -> the flags (ON0 / OFF0 bits) [C]"""
    cur, cand, run, off, ln = d["cur"], d["cand"], d["run"], d["off"], d["len"]
    up = cur != 0
    ln = np.where(up, np.minimum(ln + 1, 65535), ln)
    off = np.where(up, np.where(h == cur, 0, np.minimum(off + 1, 255)), off)
    same = up & (h == cur)
    grow = ~same & (h != 0) & (h == cand)
    new = ~same & ~grow
    run = np.where(same, 0, np.where(grow, np.minimum(run + 1, 255), np.where(h != 0, 1, 0)))
    cand = np.where(same, 0, np.where(new, h, cand))
    ends = up & (off >= min_off)
    code = np.where(ends, cur, d["code"])
    ln = np.where(ends, np.where(ln > off, ln - off, 0), ln)
    cur = np.where(ends, 0, cur)
    off = np.where(ends, 0, off)
    starts = (cur == 0) & (cand != 0) & (run >= min_on)
    cur = np.where(starts, cand, cur)
    code = np.where(starts, cur, code)
    ln = np.where(starts, run, ln)
    off = np.where(starts, 0, off)
    cand = np.where(starts, 0, cand)
    run = np.where(starts, 0, run)
    d.update(cur=cur, cand=cand, run=run, off=off, len=ln, code=code)
    return ends * OFF0 + starts * ON0


def detect(plans, pcm, state=None, plan_of=None):
    """plans: a PLAN record or a list of them; pcm int16 [F][C][n]; state [C] STATE or None (reset); plan_of [C] or None (plan 0).
    Returns (rec [F][C] REC, the state after [C] STATE).  A channel whose plan index is out of range: zero records, state untouched."""
    plans = [plans] if isinstance(plans, np.ndarray) and plans.shape == () else list(plans)
    pcm = np.asarray(pcm, np.int16)
    F_, C_, n = pcm.shape
    assert n % 2 == 0 and 2 <= n <= 256
    h = n // 2
    state = np.zeros(C_, STATE) if state is None else state.copy()
    rec = np.zeros((F_, C_), REC)
    plan_of = np.zeros(C_, np.int64) if plan_of is None else np.asarray(plan_of, np.int64)
    for pi, plan in enumerate(plans):
        ch = np.nonzero(plan_of == pi)[0]
        if not len(ch):
            continue
        tab = table(plan, n)
        min_on, min_off = int(plan["thr"]["min_on"]), int(plan["thr"]["min_off"])
        buf = np.zeros((len(ch), 128 + n), np.int64)
        buf[:, :128] = state["hist"][ch]
        d = {k: state[k][ch].astype(np.int64) for k in ("cur", "cand", "run", "off", "len")}
        for f in range(F_):
            buf[:, 128:] = pcm[f, ch].astype(np.int64) >> 3
            d["code"] = np.zeros(len(ch), np.int64)
            h0 = evaluate(plan, tab, buf[:, 128 - h:128 - h + n])
            fl = debounce(d, h0, min_on, min_off)
            h1 = evaluate(plan, tab, buf[:, 128:])
            fl = fl + debounce(d, h1, min_on, min_off) * 4
            r = rec[f]
            r["hit"][ch, 0], r["hit"][ch, 1] = h0, h1
            r["cur"][ch], r["flags"][ch], r["len"][ch], r["code"][ch] = d["cur"], fl, d["len"], d["code"]
            buf[:, :128] = buf[:, n:n + 128].copy()
        state["hist"][ch] = buf[:, :128]
        for k in ("cur", "cand", "run", "off", "len"):
            state[k][ch] = d[k]
        state["reserved"][ch] = 0
    return rec, state


def events(rec, mask=0, cap=None):
    """the event list of a launch's records: (EVENT array of the stored events, [total, stored])"""
    mask = mask or 15
    F_, C_ = rec.shape
    f, c = np.nonzero(rec["flags"] & mask)                                                  # row-major: frame-major, ascending channel
    ev = np.zeros(len(f), EVENT)
    ev["channel"], ev["frame"], ev["rec"] = c, f, rec[f, c]
    stored = len(ev) if cap is None else min(len(ev), cap)
    return ev[:stored], np.array([len(ev), stored], np.uint32)


def on_off(rec):
    """one channel's records [F] -> [(kind, code, evaluation index, len)] in time order, kind "on" / "off" """
    out = []
    for f in np.nonzero(rec["flags"])[0]:
        r = rec[f]
        for e in range(2):
            fl = (int(r["flags"]) >> (2 * e)) & 3
            # within one evaluation an OFF comes before an ON; the record's code is the frame's last, so a frame with several events
            # reports that code for each (the tests that look at codes use digits with silence between them)
            if fl & OFF0:
                out.append(("off", int(r["code"]), 2 * int(f) + e, int(r["len"])))
            if fl & ON0:
                out.append(("on", int(r["code"]), 2 * int(f) + e, int(r["len"])))
    return out


def digits_of(rec):
    """the digit string of one channel's ON events (DTMF plan)"""
    return "".join(digit(c) for k, c, _, _ in on_off(rec) if k == "on")


# ---- signals
def dtmf(digit_char, n_samples, amp_lo, amp_hi=None, phase=(0.0, 0.0), rate=8000, f_scale=1.0):
    i = DIGITS.index(digit_char)
    flo, fhi = DTMF_LO[i // 4] * f_scale, DTMF_HI[i % 4] * f_scale
    t = np.arange(n_samples) / rate
    amp_hi = amp_lo if amp_hi is None else amp_hi
    return amp_lo * np.sin(2 * np.pi * flo * t + phase[0]) + amp_hi * np.sin(2 * np.pi * fhi * t + phase[1])


def to_pcm(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def frames(x, n):
    """a signal [S] or [C][S] -> int16 [F][C][n], zero-padded to whole frames"""
    x = np.atleast_2d(x)
    F_ = -(-x.shape[1] // n)
    out = np.zeros((x.shape[0], F_ * n), np.int16)
    out[:, :x.shape[1]] = to_pcm(x)
    return out.reshape(x.shape[0], F_, n).transpose(1, 0, 2).copy()


# ---- G.711 for the tests' inputs, and a scene with something for every plan
LO8, HI8 = (350, 440, 480, 620) + DTMF_LO, DTMF_HI + (1800, 2000, 2200, 2400)


def plan_8x8(**thr):
    return plan_build(LO8, HI8, 8000, **thr)


def plan_single(freq=1000, **thr):
    return plan_build((freq,), (), 8000, **thr)


def decode(codes, codec):
    """[F][C][n] G.711 codes -> int16 (codec[c] 8: A-law, anything else mu-law)"""
    from tests import rs_model
    return rs_model.decode(codes, codec).astype(np.int16)


def encode(pcm, codec):
    """[F][C][n] int16 -> for every sample a code whose decoded value is the nearest the law has (a test input, not an encoder's rule)"""
    pcm = np.asarray(pcm, np.int16)
    out = np.zeros(pcm.shape, np.uint8)
    all_codes = np.arange(256, dtype=np.uint8).reshape(1, 1, 256)
    for law in (0, 8):
        ch = np.nonzero((np.asarray(codec) == 8) == (law == 8))[0]
        if not len(ch):
            continue
        vals = decode(all_codes, np.array([law], np.uint8))[0, 0].astype(np.int64)
        order = np.argsort(vals, kind="stable")
        sv = vals[order]
        x = pcm[:, ch].astype(np.int64)
        hi = np.clip(np.searchsorted(sv, x), 1, 255)
        pick = np.where(np.abs(sv[hi] - x) < np.abs(sv[hi - 1] - x), hi, hi - 1)
        out[:, ch] = order[pick].astype(np.uint8)
    return out


def scene(C_, F_, n, seed=0, amp=3000, tones=()):
    """int16 [F][C][n]: channel c plays a two-tone (one of LO8 with one of HI8: DTMF digits among them), every fifth (and every channel of `tones`) a 1 000 Hz tone, every
    seventh noise; each tone starts at its own sample of one of the first four frames, lasts 60 % of the scene and is followed by silence"""
    rng = np.random.default_rng(seed)
    S = F_ * n
    t = np.arange(S) / 8000.0
    x = np.zeros((C_, S))
    for c in range(C_):
        s0 = min((c * 37) % n + (c % 4) * n, S - 2)
        s1 = min(S, s0 + max(2, (S * 3) // 5))
        if c % 7 == 6:
            x[c] = rng.normal(0, amp, S)
        elif c % 5 == 4 or c in tones:
            x[c, s0:s1] = amp * np.sin(2 * np.pi * 1000 * t[:s1 - s0])
        else:
            lo, hi = LO8[4 + c % 4] if c % 3 else LO8[c % 8], HI8[(c // 4) % 4] if c % 3 else HI8[(c // 2) % 8]
            twist = 10 ** ((((c * 5) % 17) - 10) / 20) if c % 2 else 1.0                          # every other two-tone: -10 .. +6 dB, around both limits
            x[c, s0:s1] = amp * np.sin(2 * np.pi * lo * t[:s1 - s0] + c) + amp * twist * np.sin(2 * np.pi * hi * t[:s1 - s0] + 2 * c)
    return frames(x, n)
