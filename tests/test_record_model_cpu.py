"""tests/record_model.py, the one statement of the PCM record the stage models share, on rows whose records are known in closed form."""
import numpy as np
import pytest

from tests import record_model as rec

NS = (160, 21)


def fields(st):
    return int(st["sumsq"]), float(st["rms"]), int(st["peak"]), int(st["byte_mean"]), int(st["flags"])


@pytest.mark.parametrize("n", NS)
def test_closed_form_rows(n):
    rows, live, want = rec.known_rows(n)
    st = rec.records(rows, live=live)
    assert st.dtype == rec.STATS and st.shape == (7,)
    for i, (sq, pk, fl) in enumerate(want):
        rms = 0.0 if fl == rec.FLAG_EMPTY else (sq / n) ** 0.5
        assert fields(st[i]) == (sq, rms, pk, 0, fl), i
    assert int(st["sumsq"][0]) > 2 ** 32                   # the sum needs its high word


@pytest.mark.parametrize("n", NS)
def test_full_scale_negative(n):
    st = rec.records(np.full((1, n), -32768, np.int16))[0]
    assert fields(st) == (n * 2 ** 30, 32768.0, 32768, 0, 0)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("v", (8, -8))
def test_silent_threshold(n, v):
    st = rec.records(np.full((2, 3, n), v, np.int16))
    assert st.shape == (2, 3) and np.all(st["flags"] == rec.FLAG_SILENT) and np.all(st["peak"] == 8) and np.all(st["sumsq"] == 64 * n)
    one = np.zeros((1, n), np.int16)
    one[0, n - 1] = 9 if v > 0 else -9
    assert fields(rec.records(one)[0]) == (81, (81 / n) ** 0.5, 9, 0, 0)


@pytest.mark.parametrize("n", NS)
def test_zero_live_and_not_live(n):
    z = np.zeros((2, n), np.int16)
    st = rec.records(z, live=np.array([True, False]))
    assert fields(st[0]) == (0, 0.0, 0, 0, rec.FLAG_SILENT)
    assert fields(st[1]) == (0, 0.0, 0, 0, rec.FLAG_EMPTY)
    loud = rec.records(np.full((1, n), 5000, np.int16), live=np.array([False]), extra=rec.FLAG_CONCEALED)[0]
    assert fields(loud) == (0, 0.0, 0, 0, rec.FLAG_EMPTY)  # a row that does not exist has no stage flag either


@pytest.mark.parametrize("n", NS)
def test_raw_saturates(n):
    raw = np.zeros((2, n), np.int64)
    raw[0, 3] = 32768
    raw[1, 3] = 32767
    st = rec.records(np.clip(raw, -32768, 32767), raw=raw)
    assert fields(st[0]) == (32767 ** 2, (32767 ** 2 / n) ** 0.5, 32767, 0, rec.FLAG_SATURATED)
    assert fields(st[1]) == (32767 ** 2, (32767 ** 2 / n) ** 0.5, 32767, 0, 0)
    low = rec.records(np.full((1, n), -32768, np.int64), raw=np.full((1, n), -32769, np.int64))[0]
    assert fields(low) == (n * 2 ** 30, 32768.0, 32768, 0, rec.FLAG_SATURATED)


def test_extra_and_divisor():
    rows = np.array([[3, -4, 0, 0], [100, 0, 0, 0]], np.int16)
    st = rec.records(rows, extra=np.array([rec.FLAG_CONCEALED, 0]))
    assert fields(st[0]) == (25, 2.5, 4, 0, rec.FLAG_SILENT | rec.FLAG_CONCEALED)
    assert fields(st[1]) == (10000, 50.0, 100, 0, 0)
    assert fields(rec.records(rows, n=1)[1]) == (10000, 100.0, 100, 0, 0)
