"""Two independent restatements of igdsp_plc_conceal (include/igdsp.h, section "Packet loss concealment"): `run_scalar`, sample by
sample in plain Python ints, and `run`, vectorised in numpy int64 over channels (and over lags in the pitch search).  Both take the
decoded input; `decode` gives it from G.711 with the oracle's tables (igdsp_decode_meter's).

All arithmetic is integer: Q15 weights, `>> 15` a floor shift (Python's and numpy's >> on signed ints), w(i) = ((i + 1) << 15) // (q + 1)
of positive numbers.  The state is read as head % 280, pitch clamped to [40, 120] and pos % pitch, and written back so."""
import numpy as np

from tests import record_model
from tests.record_model import FLAG_CONCEALED, FLAG_EMPTY, FLAG_SILENT  # noqa: F401  (re-exported)

HIST, PMIN, PMAX, SPAN, FLAT, STEP = 280, 40, 120, 160, 80, 82
IDLE, PLAYED, LOST = 1, 2, 3
U32 = 0xFFFFFFFF


def decode(payload, codec, orc):
    """G.711 [T][C][n] -> int64 samples, law from codec[c] (8 A-law, else mu-law)."""
    tab = np.stack([orc.decode_table(0).astype(np.int64), orc.decode_table(8).astype(np.int64)])
    law = (np.asarray(codec) == 8).astype(np.int64)
    return tab[law[None, :, None], np.asarray(payload).astype(np.int64)]


def state_dtype():
    from igate4xsoftphonedsp_amd import capi

    return capi.PLC_STATE


def w(i, q):
    return ((i + 1) << 15) // (q + 1)


def gain(m):
    return max(0, 32768 - max(0, m - FLAT) * STEP)


# ---------------------------------------------------------------------------------------------------------- scalar restatement
class Chan:
    """one channel's state in Python ints"""

    def __init__(self, rec=None):
        if rec is None:
            self.hist, self.cycle = [0] * HIST, [0] * PMAX
            self.head = self.pitch = self.pos = self.missing = self.runs = self.concealed = 0
            self.reserved = [0] * 4
        else:
            self.hist = [int(v) for v in rec["hist"]]
            self.cycle = [int(v) for v in rec["cycle"]]
            self.head, self.pitch, self.pos, self.missing = int(rec["head"]), int(rec["pitch"]), int(rec["pos"]), int(rec["missing"])
            self.runs, self.concealed = int(rec["runs"]), int(rec["concealed"])
            self.reserved = [int(v) for v in rec["reserved"]]
        self.head %= HIST
        self.pitch = min(max(self.pitch, PMIN), PMAX)
        self.pos %= self.pitch

    def record(self, dtype=None):
        r = np.zeros((), dtype or state_dtype())
        r["hist"], r["cycle"] = self.hist, self.cycle
        for k in ("head", "pitch", "pos", "missing", "runs", "concealed"):
            r[k] = getattr(self, k)
        r["reserved"] = self.reserved
        return r

    def y(self, k):
        return self.hist[(self.head + k) % HIST]

    def S(self, m):
        v = (self.cycle[self.pos] * gain(m) + 16384) >> 15
        self.pos = (self.pos + 1) % self.pitch
        return v

    def tick(self, flag, x, ln, n):
        """x: the tick's n input samples; ln: its len.  Returns (out list of n ints, kind) with kind 'good' / 'concealed' / 'idle'."""
        x = [x[s] if s < min(ln, n) else 0 for s in range(n)]
        if flag == PLAYED and ln > 0:
            kind = "good"
            if self.missing == 0:
                out = list(x)
            else:
                q = self.pitch >> 2
                out = []
                for i in range(n):
                    if i < q:
                        wi = w(i, q)
                        out.append((self.S(self.missing + i) * (32768 - wi) + x[i] * wi + 16384) >> 15)
                    else:
                        out.append(x[i])
                self.missing = 0
        elif flag == LOST or flag == PLAYED:
            kind = "concealed"
            if self.missing == 0:
                y = [self.y(k) for k in range(HIST)]
                best = None
                for p in range(PMIN, PMAX + 1):
                    D = sum(abs(y[120 + i] - y[120 + i - p]) for i in range(SPAN))
                    key = (D << 7) | p
                    best = key if best is None else min(best, key)
                p = best & 127
                q = p >> 2
                for i in range(p):
                    if i < p - q:
                        self.cycle[i] = y[280 - p + i]
                    else:
                        j = i - (p - q)
                        self.cycle[i] = (y[280 - p + i] * (32768 - w(j, q)) + y[280 - 2 * p + i] * w(j, q) + 16384) >> 15
                self.pitch, self.pos = p, 0
                self.runs = (self.runs + 1) & U32
                out = []
                for i in range(n):
                    s = self.S(i)
                    out.append((y[279 - i] * (32768 - w(i, q)) + s * w(i, q) + 16384) >> 15 if i < q else s)
            else:
                out = [self.S(self.missing + i) for i in range(n)]
            self.missing = min(self.missing + n, 65535)
            self.concealed = (self.concealed + 1) & U32
        else:
            kind = "idle"
            out = [0] * n
            self.missing = 0
        for i in range(n):
            self.hist[(self.head + i) % HIST] = out[i]
        self.head = (self.head + n) % HIST
        return out, kind


def record_of(out, kind, n):
    """the igdsp_frame_stats fields of one output row: (sumsq, rms, peak, byte_mean, flags)"""
    if kind == "idle":
        return 0, 0.0, 0, 0, FLAG_EMPTY
    sq = sum(v * v for v in out)
    peak = max(abs(v) for v in out)
    fl = (FLAG_SILENT if peak <= 8 else 0) | (FLAG_CONCEALED if kind == "concealed" else 0)
    return sq, float(np.sqrt(sq / n)), peak, 0, fl


def _stats_arrays(T, C_):
    return {k: np.zeros((T, C_), t) for k, t in (("sumsq", np.uint64), ("rms", np.float32), ("peak", np.uint16), ("byte_mean", np.uint8),
                                                   ("flags", np.uint8))}


def run_scalar(flags, x, length=None, state=None):
    """flags [T][C], x [T][C][n] decoded input, length [T][C] or None, state [C] PLC_STATE or None (reset).
    Returns (out int16 [T][C][n], len_out u16 [T][C], stats dict of [T][C] arrays, state [C] PLC_STATE)."""
    T, C_, n = np.asarray(x).shape
    chans = [Chan(None if state is None else state[c]) for c in range(C_)]
    out = np.zeros((T, C_, n), np.int16)
    lo = np.zeros((T, C_), np.uint16)
    st = _stats_arrays(T, C_)
    for c in range(C_):
        ch = chans[c]
        for t in range(T):
            ln = n if length is None else int(length[t][c])
            o, kind = ch.tick(int(flags[t][c]), [int(v) for v in x[t][c]], ln, n)
            out[t, c] = o
            lo[t, c] = 0 if kind == "idle" else n
            for k, v in zip(("sumsq", "rms", "peak", "byte_mean", "flags"), record_of(o, kind, n)):
                st[k][t, c] = v
    rec = np.zeros(C_, state_dtype())
    for c in range(C_):
        rec[c] = chans[c].record()
    return out, lo, st, rec


# ---------------------------------------------------------------------------------------------------------- vectorised restatement
def _w(i, q):
    return ((i + 1) << 15) // (q + 1)


def _gain(m):
    return np.maximum(0, 32768 - np.maximum(0, m - FLAT) * STEP)


def run(flags, x, length=None, state=None):
    """As run_scalar, in numpy int64 over channels."""
    x = np.asarray(x, np.int64)
    T, C_, n = x.shape
    flags = np.asarray(flags)
    dt = state_dtype()
    st0 = np.zeros(C_, dt) if state is None else np.array(state, dt).reshape(C_)
    hist = st0["hist"].astype(np.int64)
    cycle = st0["cycle"].astype(np.int64)
    head = st0["head"].astype(np.int64) % HIST
    pitch = np.clip(st0["pitch"].astype(np.int64), PMIN, PMAX)
    pos = st0["pos"].astype(np.int64) % pitch
    missing = st0["missing"].astype(np.int64)
    runs = st0["runs"].astype(np.int64)
    conc = st0["concealed"].astype(np.int64)
    rows = np.arange(C_)
    i_n = np.arange(n)
    out = np.zeros((T, C_, n), np.int64)
    lo = np.zeros((T, C_), np.uint16)
    st = _stats_arrays(T, C_)

    def synth(sel, m0, count):
        """S(m0 + i) for i < count on channels sel (bool [C]); advances pos.  Returns [C][count] (0 off sel)."""
        i = np.arange(count)
        idx = (pos[:, None] + i[None, :]) % pitch[:, None]
        v = (cycle[rows[:, None], idx] * _gain(m0[:, None] + i[None, :]) + 16384) >> 15
        pos[sel] = (pos[sel] + count) % pitch[sel]
        return np.where(sel[:, None], v, 0)

    for t in range(T):
        f = flags[t].astype(np.int64)
        ln = np.full(C_, n, np.int64) if length is None else np.minimum(np.asarray(length[t], np.int64), n)
        xt = np.where(i_n[None, :] < ln[:, None], x[t], 0)
        good = (f == PLAYED) & (ln > 0)
        lost = (f == LOST) | ((f == PLAYED) & (ln == 0))
        idle = ~(good | lost)
        o = np.zeros((C_, n), np.int64)
        # good
        o[good & (missing == 0)] = xt[good & (missing == 0)]
        rec = good & (missing > 0)
        if rec.any():
            q = pitch >> 2
            qm = np.minimum(q, n)
            s = np.zeros((C_, n), np.int64)
            for c in np.nonzero(rec)[0]:                     # a per-channel count: pos advances by min(q, n)
                one = np.zeros(C_, bool)
                one[c] = True
                s[c, :qm[c]] = synth(one, missing, int(qm[c]))[c]
            wi = _w(i_n[None, :], q[:, None])
            blend = (s * (32768 - wi) + xt * wi + 16384) >> 15
            o[rec] = np.where(i_n[None, :] < q[:, None], blend, xt)[rec]
        # run starts
        start = lost & (missing == 0)
        if start.any():
            y = hist[rows[:, None], (head[:, None] + np.arange(HIST)[None, :]) % HIST]
            D = np.stack([np.abs(y[:, 120:280] - y[:, 120 - p:280 - p]).sum(axis=1) for p in range(PMIN, PMAX + 1)], axis=1)
            key = (D << 7) | np.arange(PMIN, PMAX + 1)[None, :]
            p = key.min(axis=1) & 127
            q = p >> 2
            i = np.arange(PMAX)[None, :]
            src = y[rows[:, None], np.clip(HIST - p[:, None] + i, 0, HIST - 1)]
            j = i - (p - q)[:, None]
            src2 = y[rows[:, None], np.clip(HIST - 2 * p[:, None] + i, 0, HIST - 1)]
            wj = _w(np.maximum(j, 0), q[:, None])
            cyc = np.where(j >= 0, (src * (32768 - wj) + src2 * wj + 16384) >> 15, src)
            cycle[start] = np.where(i < p[:, None], cyc, cycle)[start]
            pitch[start], pos[start] = p[start], 0
            runs[start] += 1
            s = synth(start, np.zeros(C_, np.int64), n)
            wi = _w(i_n[None, :], q[:, None])
            fade = (y[:, HIST - 1 - np.minimum(i_n, HIST - 1)] * (32768 - wi) + s * wi + 16384) >> 15
            o[start] = np.where(i_n[None, :] < q[:, None], fade, s)[start]
        cont = lost & (missing > 0)
        if cont.any():
            o[cont] = synth(cont, missing, n)[cont]
        missing = np.where(lost, np.minimum(missing + n, 65535), np.where(good | idle, 0, missing))
        conc += lost
        # ring, outputs
        hist[rows[:, None], (head[:, None] + i_n[None, :]) % HIST] = o
        head = (head + n) % HIST
        out[t] = o
        lo[t] = np.where(idle, 0, n)
        rows_rec = record_model.records(o, live=~idle, extra=np.where(lost, FLAG_CONCEALED, 0))
        for k in st:
            st[k][t] = rows_rec[k]                           # (rms rounded to float32)
    rec = st0.copy()
    rec["hist"], rec["cycle"] = hist, cycle
    rec["head"], rec["pitch"], rec["pos"], rec["missing"] = head, pitch, pos, missing
    rec["runs"], rec["concealed"] = runs & U32, conc & U32
    return out.astype(np.int16), lo, st, rec
