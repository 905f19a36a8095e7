"""The numpy statement of the PCM record (include/igdsp.h: "the record as igdsp_conf_mix writes it"): the 16-byte igdsp_frame_stats over
a row of n int16 samples, as the conference mix, best signal selection, PTT arbitration, loss concealment, the sound-card splitter /
combiner, the tone generator and the rate converter write it.  The stage models (conf_model, bss_model, plc_model's array form,
snd_model, tone_model, rs_model) all end here; plc_model.record_of is the scalar restatement test_plc_cpu checks this one against."""
import numpy as np

FLAG_SILENT, FLAG_EMPTY, FLAG_SATURATED, FLAG_CONCEALED = 0x01, 0x08, 0x10, 0x20
STATS = np.dtype([("sumsq", "<u8"), ("rms", "<f8"), ("peak", "<u2"), ("byte_mean", "u1"), ("flags", "u1")])   # rms in float64: the reference value


def records(rows, n=None, live=None, raw=None, extra=0):
    """STATS [..] over the rows [..][n] (integers).  sumsq exact, rms = sqrt(sumsq / n) in float64, peak = max |x| (32768 for -32768),
    byte_mean 0, flags SILENT when peak <= 8.
    n: the divisor, where it is not the rows' length.  live [..] bool: a row that is not live gets the len-0 record, all 0 with EMPTY.
    raw [..][n]: the values before the clamp to int16 that gave the rows; SATURATED where the clamp fired.
    extra: flags of the stage's own (int or [..]), ORed into the live rows'."""
    x = np.asarray(rows).astype(np.int64)
    n = x.shape[-1] if n is None else n
    live = np.ones(x.shape[:-1], bool) if live is None else np.asarray(live, bool)
    sq = (x * x).sum(axis=-1)
    peak = np.abs(x).max(axis=-1)
    flags = np.where(peak <= 8, FLAG_SILENT, 0) | extra
    if raw is not None:
        flags = flags | np.where((x != np.asarray(raw)).any(axis=-1), FLAG_SATURATED, 0)
    st = np.zeros(x.shape[:-1], STATS)
    st["sumsq"] = np.where(live, sq, 0).astype(np.uint64)
    st["rms"] = np.where(live, np.sqrt(sq.astype(np.float64) / n), 0.0)
    st["peak"] = np.where(live, peak, 0)
    st["flags"] = np.where(live, flags, FLAG_EMPTY)
    return st


def known_rows(n):
    """(rows [7][n] int16, live [7], the records' (sumsq, peak, flags)): rows whose records are known in closed form"""
    rows = np.zeros((7, n), np.int16)
    rows[0] = -32768
    rows[1] = 8
    rows[2] = -8
    rows[3, n // 2] = 9
    rows[5] = 1234                                         # not live: what it holds does not matter
    rows[6, ::2] = 32767
    live = np.array([1, 1, 1, 1, 1, 0, 1], bool)
    want = [(n << 30, 32768, 0), (64 * n, 8, FLAG_SILENT), (64 * n, 8, FLAG_SILENT), (81, 9, 0), (0, 0, FLAG_SILENT),
            (0, 0, FLAG_EMPTY), (32767 * 32767 * ((n + 1) // 2), 32767, 0)]
    return rows, live, want
