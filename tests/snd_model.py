"""The numpy statement of the sound-card splitter / combiner (include/igdsp.h, "Sound-card splitter / combiner"): both directions, the
per-row records and igdsp_snd_vu.  Independent of the kernels and of the host mirror: reshapes, integer sums, float64 roots."""
import math

import numpy as np

from tests import record_model
from tests.record_model import FLAG_SILENT, STATS  # noqa: F401  (re-exported)

MAX_CHANNELS = 8
DB_FLOOR = -100.0


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
    return record_model.records(pcm)


def snd_vu(rms):
    """(percent, db) of a record's float32 rms: int(float(rms * 100.0 / 30000.0)) and 20 log10(rms / 32768), DB_FLOOR at 0"""
    r = float(np.float32(rms))
    percent = int(np.float32(r * 100.0 / 30000.0))
    return percent, (20.0 * math.log10(r / 32768.0) if r > 0 else DB_FLOOR)
