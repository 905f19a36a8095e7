"""The delay buffer's rule (include/igdsp.h, section "Delay buffer") in numpy and Python integers, written from the header's text:
the independent statement igdsp_dbuf_step (tests/test_dbuf_cpu.py) and igdsp_dbuf_run (tests/test_gpu_dbuf.py) are compared with.  A
state is a plain dict: the ring as an int array and the scalars as Python ints; records through tests/record_model.py."""
import numpy as np

from tests import record_model

CAP, WIN, RECALC = 1024, 280, 200
PUT, GET = 1, 2
PMIN, PMAX, SPAN = 40, 120, 160
IDLE, PLAYED, LOST = 1, 2, 3
SCALARS = ("head", "len", "eff", "level", "max_level", "since", "last_op")
COUNTERS = ("underruns", "shrinks", "shrunk", "dropped", "puts", "gets")


def new_state():
    st = {k: 0 for k in SCALARS + COUNTERS}
    st["ring"] = np.zeros(CAP, np.int64)
    return st


def from_record(rec):
    """a state from one record of capi.DBUF_STATE (or anything indexable by the field names)"""
    st = {k: int(rec[k]) for k in SCALARS + COUNTERS}
    st["ring"] = np.asarray(rec["ring"]).astype(np.int64).copy()
    return st


def read(st, M):
    """the state as a launch reads it (in place)"""
    st["head"] %= CAP
    if st["len"] > M:
        st["head"] = (st["head"] + st["len"] - M) % CAP
        st["len"] = M
    st["eff"] = M >> 1 if st["eff"] == 0 else min(st["eff"], M)
    if st["last_op"] not in (PUT, GET):
        st["last_op"] = 0
    st["since"] = min(st["since"], RECALC - 1)
    return st


def _idx(st, k0, count):
    return (st["head"] + k0 + np.arange(count)) % CAP


def live(st):
    """the buffered samples y[0 .. len), oldest first"""
    return st["ring"][_idx(st, 0, st["len"])].copy()


def scalars(st):
    return tuple(st[k] for k in SCALARS) + tuple(st[k] & 0xFFFFFFFF for k in COUNTERS)


def update(st, op, n, M):
    if st["last_op"] == op:
        st["level"] = min(st["level"] + 1, 65535)
        return
    if st["last_op"] != 0:
        st["max_level"] = max(st["max_level"], st["level"])
        st["since"] += st["level"]
    st["last_op"] = op
    st["level"] = 1
    if st["since"] >= RECALC:
        st["eff"] = (3 * st["eff"] + min(M, (st["max_level"] + 1) * n)) >> 2
        st["max_level"] = 0
        st["since"] = 0


def pitch(z):
    """the lag of the smallest D, the smallest lag on ties"""
    best = None
    for p in range(PMIN, PMAX + 1):
        d = int(np.abs(z[PMAX:PMAX + SPAN] - z[PMAX - p:PMAX + SPAN - p]).sum())
        if best is None or d < best[0]:
            best = (d, p)
    return best[1]


def shrink(st):
    """drop one pitch period of the newest audio by overlap-add; returns p"""
    ln = st["len"]
    z = st["ring"][_idx(st, ln - WIN, WIN)]
    p = pitch(z)
    i = np.arange(p)
    w = ((i + 1) << 15) // (p + 1)
    b = (z[WIN - 2 * p + i] * (32768 - w) + z[WIN - p + i] * w + 16384) >> 15
    st["ring"][_idx(st, ln - 2 * p, p)] = b
    st["len"] -= p
    st["shrinks"] += 1
    st["shrunk"] += p
    return p


def put(st, x, n, M):
    update(st, PUT, n, M)
    st["puts"] += 1
    if (st["len"] > n + st["eff"] or st["len"] + n > M) and st["len"] >= WIN:
        shrink(st)
    d = st["len"] + n - M
    if d > 0:
        st["head"] = (st["head"] + d) % CAP
        st["len"] -= d
        st["dropped"] += d
    st["ring"][_idx(st, st["len"], n)] = np.asarray(x).astype(np.int64)
    st["len"] += n


def get(st, n, M):
    update(st, GET, n, M)
    st["gets"] += 1
    if st["len"] < n:
        out = np.zeros(n, np.int64)
        st["head"] = (st["head"] + st["len"]) % CAP
        st["len"] = 0
        st["underruns"] += 1
        return out, LOST
    out = st["ring"][_idx(st, 0, n)].copy()
    st["head"] = (st["head"] + n) % CAP
    st["len"] -= n
    return out, PLAYED


def step(st, op, x, n, M):
    """one step of one channel: (the row or None, the flag).  The state is read by the rule first, as every launch does."""
    assert 1 <= n <= 256 and 2 * n <= M <= CAP
    read(st, M)
    op &= 3
    out, flag = None, IDLE
    if op & PUT:
        put(st, x, n, M)
    if op & GET:
        out, flag = get(st, n, M)
    return out, flag


def run(states, ops, x, n, M):
    """T steps of C channels: ops [T][C], x [T][C][n], states a list of C states (advanced in place).  Returns a dict: out [T][C][n]
    int16 (rows without a GET: 0, and got [T][C] False), flags, length, fill [T][C], stats [T][C] record_model.STATS."""
    ops = np.asarray(ops)
    T, C = ops.shape
    out = np.zeros((T, C, n), np.int16)
    got = np.zeros((T, C), bool)
    flags = np.zeros((T, C), np.uint8)
    fill = np.zeros((T, C), np.uint16)
    for c in range(C):
        st = states[c]
        for t in range(T):
            row, flags[t, c] = step(st, int(ops[t, c]), x[t, c], n, M)
            if row is not None:
                out[t, c] = row
                got[t, c] = True
            fill[t, c] = st["len"]
    return dict(out=out, got=got, flags=flags, length=np.where(got, n, 0).astype(np.uint16), fill=fill,
                stats=record_model.records(out, live=got))


# ---- inputs the tests share
def speech(rng, T, n, f0):
    """T rows of a harmonic series on the fundamental f0 (Hz at 8 kHz) plus small noise: D(p) has a clear minimum near 8000 / f0"""
    k = np.arange(T * n)
    s = sum(a * np.sin(2 * np.pi * f0 * h * k / 8000.0 + ph) for h, a, ph in ((1, 6000, 0.3), (2, 3000, 1.1), (3, 1500, 2.0), (4, 700, 0.7)))
    return np.clip(np.rint(s + rng.normal(0, 40, T * n)), -32768, 32767).astype(np.int16).reshape(T, n)


def square(T, n, period=50):
    """a full-scale +-32768 / 32767 square: the blend's extremes"""
    k = np.arange(T * n)
    return np.where((k // (period // 2)) % 2 == 0, 32767, -32768).astype(np.int16).reshape(T, n)


def clocked_ops(T, rate, phase=0.0):
    """ops of T steps for a consumer that takes one frame per tick and a producer that delivers `rate` frames per tick (1.01: 1 % fast):
    a tick in which the producer delivered one frame is one PUT|GET step, none a GET step, two a PUT step and a PUT|GET step"""
    ops, tick = [], 0
    while len(ops) < T:
        k = int(np.floor((tick + 1) * rate + phase)) - int(np.floor(tick * rate + phase))
        ops += [PUT] * max(k - 1, 0) + [(PUT if k else 0) | GET]
        tick += 1
    return np.array(ops[:T], np.uint8)
