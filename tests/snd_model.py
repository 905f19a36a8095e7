"""The numpy statement of the sound-card splitter / combiner (include/igdsp.h, "Sound-card splitter / combiner"): both directions, the
per-row records and igdsp_snd_vu.  Independent of the kernels and of the host mirror: reshapes, integer sums, float64 roots."""
import math

import numpy as np

FLAG_SILENT = 0x01
MAX_CHANNELS = 8
DB_FLOOR = -100.0
STATS = np.dtype([("sumsq", "<u8"), ("rms", "<f8"), ("peak", "<u2"), ("byte_mean", "u1"), ("flags", "u1")])   # rms in float64: the reference value


def combine(pcm, D, K):
    """pcm [F][D * K][n] int16 -> frames [F][D][n][K]: frames[f][d][s][k] = pcm[f][d * K + k][s]"""
    F, rows, n = pcm.shape
    assert rows == D * K
    return np.ascontiguousarray(pcm.reshape(F, D, K, n).transpose(0, 1, 3, 2))


def split(frames):
    """frames [F][D][n][K] int16 -> pcm [F][D * K][n]: pcm[f][d * K + k][s] = frames[f][d][s][k]"""
    F, D, n, K = frames.shape
    return np.ascontiguousarray(frames.transpose(0, 1, 3, 2)).reshape(F, D * K, n)


def records(pcm):
    """the records [F][D * K] over the mono rows pcm [F][D * K][n]: integer sumsq and peak, float64 rms, SILENT when peak <= 8"""
    x = pcm.astype(np.int64)
    st = np.zeros(pcm.shape[:2], STATS)
    st["sumsq"] = (x * x).sum(axis=2).astype(np.uint64)
    st["rms"] = np.sqrt(st["sumsq"].astype(np.float64) / pcm.shape[2])
    peak = np.abs(x).max(axis=2)
    st["peak"] = peak
    st["flags"] = np.where(peak <= 8, FLAG_SILENT, 0)
    return st


def snd_vu(rms):
    """(percent, db) of a record's float32 rms: int(float(rms * 100.0 / 30000.0)) and 20 log10(rms / 32768), DB_FLOOR at 0"""
    r = float(np.float32(rms))
    percent = int(np.float32(r * 100.0 / 30000.0))
    return percent, (20.0 * math.log10(r / 32768.0) if r > 0 else DB_FLOOR)
