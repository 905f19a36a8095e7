"""The numpy / Python-integer statement of the tone generator (include/igdsp.h, "Tone generator"): the plan, the oscillator, the
port-frame rule, the records and the state.  Independent of the kernels, of igdsp_route.h and of the host mirror: the table comes from
math.sin, a plan's whole cycle is synthesised once as an array and rows are read out of it by index."""
import math

import numpy as np

from tests import record_model
from tests.record_model import FLAG_EMPTY, FLAG_SILENT, STATS  # noqa: F401  (re-exported)

TONE_MAX, VOLUME = 8, 12288
LOOP, NO_FADE = 1, 2
PLAYING = 1
REWIND, STOP, HOLD = 1, 2, 4
TABLE = np.array([math.floor(32767 * math.sin(2 * math.pi * i / 1024) + 0.5) for i in range(1024)], np.int64)


def step_of(freq, clock_rate):
    return ((freq << 32) + clock_rate // 2) // clock_rate


def plan_build(tones, clock_rate=8000, options=LOOP):
    """tones: (freq1, freq2, on_msec, off_msec[, volume[, reserved]]) each.  Returns a dict, or None where the entry returns EINVAL."""
    if not 1 <= len(tones) <= TONE_MAX or clock_rate % 1000 or not 8000 <= clock_rate <= 48000 or options & ~(LOOP | NO_FADE):
        return None
    segs, at = [], 0
    for t in tones:
        f1, f2, on_ms, off_ms = t[:4]
        vol = t[4] if len(t) > 4 else 0
        if len(t) > 5 and t[5]:
            return None
        top = clock_rate // 2 - 1
        if not 1 <= f1 <= top or not 0 <= f2 <= top or not 0 <= vol <= 32767:
            return None
        on, off = on_ms * clock_rate // 1000, off_ms * clock_rate // 1000
        fi, fo = clock_rate // 1000, clock_rate // 500
        if options & NO_FADE or on < fi + fo:
            fi = fo = 0
        segs.append(dict(start=at, on=on, off=off, step1=step_of(f1, clock_rate), step2=step_of(f2, clock_rate) if f2 else 0,
                         vol=vol or VOLUME, fade_in=fi, fade_out=fo))
        at += on + off
    if at < 1:
        return None
    return dict(n_tones=len(tones), options=options, cycle=at, clock_rate=clock_rate, seg=segs)


def osc(ph):
    """the interpolated table at phases ph (int64 array of 32-bit values)"""
    i, fr = ph >> 22, (ph >> 6) & 0xFFFF
    return TABLE[i] + (((TABLE[(i + 1) & 1023] - TABLE[i]) * fr) >> 16)          # >> of a negative int64: floor


def tdiv(a, d):
    """C division, toward zero"""
    return np.sign(a) * (np.abs(a) // d)


def seg_on(sg):
    """the ON period of one tone: int64 [on]"""
    k = np.arange(sg["on"], dtype=np.int64)
    o1 = osc((k * sg["step1"]) & 0xFFFFFFFF)
    if sg["step2"]:
        a = ((o1 + osc((k * sg["step2"]) & 0xFFFFFFFF)) * sg["vol"]) >> 16
    else:
        a = (o1 * sg["vol"]) >> 15
    if sg["fade_in"]:
        a = np.where(k < sg["fade_in"], tdiv(a * k, sg["fade_in"]), a)
    if sg["fade_out"]:
        a = np.where(k >= sg["on"] - sg["fade_out"], tdiv(a * (sg["on"] - 1 - k), sg["fade_out"]), a)
    return a


def cycle_wave(plan):
    """one whole cycle of a plan: int16 [cycle]"""
    w = plan.get("_wave")
    if w is None:
        w = np.zeros(plan["cycle"], np.int64)
        for sg in plan["seg"]:
            w[sg["start"]:sg["start"] + sg["on"]] = seg_on(sg)
        assert np.abs(w).max() <= 32767
        w = plan["_wave"] = w.astype(np.int16)
    return w


def records(pcm, live):
    """records over rows pcm [..][n] with live [..] bool: a live row's sumsq / rms / peak / SILENT, an EMPTY row's len-0 record"""
    return record_model.records(pcm, live=live)


def apply_cmd(pos, flags, cmd):
    if cmd & STOP:
        flags &= ~PLAYING
    elif cmd & REWIND:
        pos, flags = 0, flags | PLAYING
    return pos, flags


def generate(plans, plan_of, cmd, pos, flags, F, n):
    """One launch.  plans: list of plan_build dicts; plan_of [P] (an index >= len(plans): no plan) or None; cmd [P] or None; pos, flags [P].
    Returns pcm [F][P][n] int16, len [F][P] u16, stats [F][P], pos' [P], flags' [P]."""
    P = len(pos)
    pcm = np.zeros((F, P, n), np.int16)
    ln = np.zeros((F, P), np.uint16)
    pos2, flags2 = np.array(pos, np.int64), np.array(flags, np.int64)
    plan_of = np.zeros(P, np.int64) if plan_of is None else np.asarray(plan_of, np.int64)
    cmd = np.zeros(P, np.int64) if cmd is None else np.asarray(cmd, np.int64)
    stop, rewind = (cmd & STOP) != 0, ((cmd & REWIND) != 0) & ((cmd & STOP) == 0)
    flags2[stop] &= ~PLAYING
    pos2[rewind] = 0
    flags2[rewind] |= PLAYING
    f_n = np.arange(F, dtype=np.int64)[:, None] * n
    s = np.arange(n, dtype=np.int64)
    for pi, plan in enumerate(plans):
        sel = np.nonzero((plan_of == pi) & ((cmd & HOLD) == 0) & ((flags2 & PLAYING) != 0))[0]
        if not len(sel):
            continue
        wave, cycle = cycle_wave(plan), plan["cycle"]
        q0 = pos2[sel][None, :] + f_n                                          # [F][sel]
        if plan["options"] & LOOP:
            live = np.ones(q0.shape, bool)
            for f in range(F):
                pcm[f, sel] = wave[(q0[f][:, None] + s) % cycle]
            pos2[sel] = (pos2[sel] + F * n) % cycle
        else:
            live = q0 < cycle
            for f in range(F):
                q = q0[f][:, None] + s
                pcm[f, sel] = np.where(live[f][:, None] & (q < cycle), wave[np.minimum(q, cycle - 1)], 0)
            pos2[sel] = np.minimum(pos2[sel] + F * n, cycle)
            flags2[sel[pos2[sel] >= cycle]] &= ~PLAYING
        ln[:, sel] = np.where(live, n, 0)
    return pcm, ln, records(pcm, ln != 0), pos2.astype(np.uint32), flags2.astype(np.uint32)


def plan_record(plan, dtype):
    """a plan_build dict as one record of the binding's TONE_PLAN dtype"""
    r = np.zeros((), dtype)
    for k in ("n_tones", "options", "cycle", "clock_rate"):
        r[k] = plan[k]
    for i, sg in enumerate(plan["seg"]):
        for k in ("start", "on", "step1", "step2", "vol", "fade_in", "fade_out"):
            r["seg"][i][k] = sg[k]
    return r
