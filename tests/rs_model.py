"""The numpy statement of the rate converter (include/igdsp.h, "Rate converter"): the tables from the float64 formula itself, the two
sample rules over a channel's whole stream as windowed dot products in int64, the layouts, d_len, the G.711 expansion, the records and
the state.  Independent of the kernels, of igdsp_route.h and of the host mirror."""
import hashlib

import numpy as np

from tests import record_model
from tests.record_model import FLAG_SATURATED, FLAG_SILENT, STATS  # noqa: F401  (re-exported)

FACTORS, TAPS, HIST = (2, 3, 4, 6), 24, 144
UP, DOWN = 0, 1
ROWS, SUBFRAMES = 0, 1
TABLE_SHA256 = "20df89a0d30511f925cf8aa5795c080719080cd53bce42bbfb503114f68608dc"


def prototype(R):
    N = TAPS * R
    c = np.arange(N, dtype=np.float64) - (N - 1) / 2.0
    return np.sinc(0.95 * c / R) * np.kaiser(N, 6.0)


def fix(v):
    q = np.floor(16384.0 * v / np.sum(v) + 0.5).astype(np.int64)
    big = np.flatnonzero(np.abs(q) == np.abs(q).max())[0]                 # the largest |q|, the lowest index on a tie
    q[big] += 16384 - q.sum()
    return q


def up_table(R):
    h = prototype(R)
    return np.stack([fix(h[p::R]) for p in range(R)])                     # [R][24]


def down_table(R):
    return fix(prototype(R))                                              # [24 R]


def table_digest():
    d = hashlib.sha256()
    for R in FACTORS:
        d.update(up_table(R).astype("<i2").tobytes())
        d.update(down_table(R).astype("<i2").tobytes())
    return d.hexdigest()


def g711_expand(codes, alaw):
    """ITU-T G.711 expansion of uint8 codes (any shape) to int64; alaw broadcasts against codes."""
    c = np.asarray(codes, np.int64)
    u = ~c & 0x7F
    mu = ((((u & 15) * 2 + 33) << (u >> 4)) - 33) << 2
    a = (c ^ 0x55) & 0x7F
    s, q = a >> 4, a & 15
    al = np.where(s == 0, q * 2 + 1, (q * 2 + 33) << np.maximum(s - 1, 0)) << 3
    m = np.where(alaw, al, mu)
    return np.where(c & 0x80, m, -m)


def decode(payload, codec):
    """[F][C][n] G.711 -> int64, the law from codec[c] (8 A-law, anything else mu-law)"""
    return g711_expand(payload, (np.asarray(codec) == 8)[None, :, None])


def mask(rows, length):
    """rows [..][n] with samples at and past length [..] zeroed (d_len: laid out as the rows are)"""
    if length is None:
        return np.asarray(rows, np.int64)
    rows = np.asarray(rows, np.int64)
    return np.where(np.arange(rows.shape[-1]) < np.asarray(length, np.int64)[..., None], rows, 0)


def sub_to_rows(sub, R):
    """the wide side [F R][C][n] -> [F][C][n R]: wide sample q of (f, c) is sample q % n of frame f R + q / n"""
    FR, C_, n = sub.shape
    return sub.reshape(FR // R, R, C_, n).transpose(0, 2, 1, 3).reshape(FR // R, C_, R * n)


def rows_to_sub(rows, R):
    F_, C_, nR = rows.shape
    return rows.reshape(F_, C_, R, nR // R).transpose(0, 2, 1, 3).reshape(F_ * R, C_, nR // R)


def convert(direction, R, x, hist=None):
    """x [C][L]: every channel's input stream of a launch (after decode and d_len), hist [C][144] or None (silence).
    Returns (raw [C][L_out] int64 BEFORE the clamp, the new hist [C][144])."""
    x = np.asarray(x, np.int64)
    C_, L = x.shape
    hist = np.zeros((C_, HIST), np.int64) if hist is None else np.asarray(hist, np.int64)
    xs = np.concatenate([hist, x], axis=1)                               # x[g] is xs[:, 144 + g]
    win = np.lib.stride_tricks.sliding_window_view
    if direction == UP:
        U = up_table(R)
        w = win(xs[:, HIST - (TAPS - 1):], TAPS, axis=1)                 # w[c][g][t] = x[g - 23 + t]: tap k = 23 - t
        acc = np.einsum("cgt,pt->cgp", w, U[:, ::-1])                    # [C][L][R]
        raw = ((acc + 8192) >> 14).reshape(C_, L * R)
    else:
        assert L % R == 0
        D, N = down_table(R), TAPS * R
        w = win(xs[:, HIST - (N - R):], N, axis=1)[:, ::R]               # w[c][g][t] = x[g R + R - 1 - (N - 1) + t]: tap j = N - 1 - t
        raw = (np.einsum("cgt,t->cg", w, D[::-1]) + 8192) >> 14
    return raw, xs[:, L:L + HIST]


def clamp(raw):
    return np.clip(raw, -32768, 32767)


def records(raw):
    """raw [..][count] before the clamp -> STATS [..] over each row"""
    return record_model.records(clamp(raw), raw=raw)


def launch(direction, R, layout, rows, hist=None, length=None):
    """A launch as the entry sees it.  rows: the input as laid out, decoded: UP [F][C][n]; DOWN [F][C][n R] (ROWS) or [F R][C][n]
    (SUBFRAMES); length laid out as the input rows.  Returns (out as laid out int16, STATS per output row as laid out, new hist)."""
    x = mask(rows, length)
    if direction == DOWN and layout == SUBFRAMES:
        x = sub_to_rows(x, R)
    F_, C_, n_in = x.shape
    raw, new_hist = convert(direction, R, x.transpose(1, 0, 2).reshape(C_, F_ * n_in), hist)
    n_out = n_in * R if direction == UP else n_in // R
    raw = raw.reshape(C_, F_, n_out).transpose(1, 0, 2)                  # [F][C][n_out]
    if direction == UP and layout == SUBFRAMES:
        raw = rows_to_sub(raw, R)
    return clamp(raw).astype(np.int16), records(raw), new_hist.astype(np.int16)
