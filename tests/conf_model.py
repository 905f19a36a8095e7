"""Independent numpy restatement of igdsp_conf_mix (include/igdsp.h, section "Conference mix"), decoding with the oracle's G.711
tables.  All arithmetic in int64; the Q7 scale truncates toward zero explicitly (C integer division), never floors."""
import numpy as np

from tests import record_model
from tests.record_model import FLAG_EMPTY, FLAG_SATURATED, FLAG_SILENT  # noqa: F401  (re-exported)


def trunc_div(a, d):
    """C integer division a / d (toward zero) of int64 arrays by a positive d."""
    a = np.asarray(a, np.int64)
    q = np.abs(a) // d
    return np.where(a < 0, -q, q)


def scale(x, g):
    """(clamp16(trunc(x * g / 128)), clamp fired) for int64 x, g (broadcast)."""
    a = trunc_div(np.asarray(x, np.int64) * np.asarray(g, np.int64), 128)
    c = np.clip(a, -32768, 32767)
    return c, c != a


def decode(payload, codec, orc):
    """G.711 [F][C][n] -> int64 samples, law from codec[c] (8 A-law, else mu-law)."""
    tab = np.stack([orc.decode_table(0).astype(np.int64), orc.decode_table(8).astype(np.int64)])
    law = (np.asarray(codec) == 8).astype(np.int64)
    return tab[law[None, :, None], payload.astype(np.int64)]


def mix(x, gain, port_ptr, members, n_members, n_ports, length=None):
    """x: decoded int64 samples [F][C][n].  Returns (out int16 [F][P][n], stats dict of arrays [F][P])."""
    F_, C_, n = x.shape
    ln = np.full((F_, C_), n, np.int64) if length is None else np.minimum(np.asarray(length, np.int64), n)
    s_idx = np.arange(n)
    out = np.zeros((F_, n_ports, n), np.int16)
    st = {k: np.zeros((F_, n_ports), t) for k, t in (("sumsq", np.uint64), ("rms", np.float32), ("peak", np.uint16),
                                                      ("byte_mean", np.uint8), ("flags", np.uint8))}
    ptr = np.minimum(np.asarray(port_ptr, np.int64), n_members)
    mem = np.asarray(members, np.int64)[:n_members]
    for p in range(n_ports):
        b, e = int(ptr[p]), int(ptr[p + 1])
        ms = mem[b:e] if e > b else mem[:0]
        ms = ms[ms < C_]                                   # members >= C: nothing
        S = np.zeros((F_, n), np.int64)
        sat = np.zeros(F_, bool)
        live = np.zeros(F_, bool)
        for m in ms:
            valid = s_idx[None, :] < ln[:, m, None]        # [F][n]
            a, fired = scale(np.where(valid, x[:, m, :], 0), int(gain[m]))
            S += a
            sat |= fired.any(axis=1)
            live |= ln[:, m] > 0
        o = np.clip(S, -32768, 32767)
        sat |= (o != S).any(axis=1)
        o = np.where(live[:, None], o, 0)
        out[:, p, :] = o
        rec = record_model.records(o, live=live, extra=np.where(sat, FLAG_SATURATED, 0))
        for k in st:
            st[k][:, p] = rec[k]                           # (rms rounded to float32)
    return out, st


def level_q7(level):
    """pjsua's float -> Q7 mapping in float32: 128 + (int)((level - 1) * 128); None where igdsp_conf_level_q7 returns IGDSP_EINVAL."""
    l32 = np.float32(level)
    if not np.isfinite(l32):
        return None
    adj = (l32 - np.float32(1.0)) * np.float32(128.0)
    if not -1e6 < adj < 1e6:
        return None
    q = 128 + int(np.trunc(adj))
    return q if 0 <= q <= 65535 else None


def build(channel, port, n_channels, n_ports):
    """CSR of a connection list: sorted by (port, channel), duplicates removed."""
    pairs = sorted(set(zip((int(p) for p in port), (int(c) for c in channel))))
    ptr = np.zeros(n_ports + 1, np.uint32)
    for p, _ in pairs:
        ptr[p + 1] += 1
    return np.cumsum(ptr).astype(np.uint32), np.array([c for _, c in pairs], np.uint32)
