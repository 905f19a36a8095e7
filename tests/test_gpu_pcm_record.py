"""-m gpu: the PCM record (csrc/igdsp_pcmrec.h) through three of the entries that write it, on the same rows as PCM: igdsp_conf_mix with
one-member ports at unity gain, igdsp_plc_conceal with every tick PLAIN, igdsp_snd_combine with and without frames.  The three record
arrays are byte-equal, rms included (the same correctly rounded expression in each), and equal tests/record_model.py; the EMPTY record
of a memberless port and of an IDLE tick are byte-equal.  F = 2, 80 rows (five waves of plc, ten items of snd), n = 160 (the vector
forms) and n = 21 (no multiple of 4 or 8: every kernel's non-vector form)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import plc_model as pm  # noqa: E402
from tests import record_model as rec  # noqa: E402

F, ROWS, D, K = 2, 80, 10, 8


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def make_rows(n):
    """[F][ROWS][n] int16: seeded random rows (full range, and some at the SILENT threshold), the closed-form live rows planted at the
    start of frame 0 and at the end of frame 1"""
    rng = np.random.default_rng(1000 + n)
    rows = rng.integers(-32768, 32768, (F, ROWS, n)).astype(np.int16)
    rows[:, 40:48] = rng.integers(-9, 10, (F, 8, n))
    known, live, _ = rec.known_rows(n)
    known = known[live]
    rows[0, :len(known)] = known
    rows[1, ROWS - len(known):] = known[::-1]
    return rows


def stats_of(d_st, shape):
    return gu.to_host(d_st, capi.FRAME_STATS, shape).copy()


def conf_records(ctx, rows, ptr):
    """igdsp_conf_mix over rows [F][C][n] as PCM, unity gain, ports ptr over members 0, 1, .."""
    F_, C_, n = rows.shape
    P_ = len(ptr) - 1
    d_st = gu.dev_zeros(F_ * P_ * 16, 0x5A)
    mem = np.arange(max(int(ptr[-1]), 1), dtype=np.uint32)
    ctx.conf_mix(gu.to_dev(np.full(C_, 128, np.uint16)), gu.to_dev(np.asarray(ptr, np.uint32)), gu.to_dev(mem), int(ptr[-1]), C_, P_, F_, n,
                 stats=d_st, pcm=gu.to_dev(rows))
    gu.torch_cuda().cuda.synchronize()
    return stats_of(d_st, (F_, P_))


def plc_records(ctx, rows, flags):
    """igdsp_plc_conceal over rows [T][C][n] as PCM from a reset state"""
    T, C_, n = rows.shape
    d_st = gu.dev_zeros(T * C_ * 16, 0x5A)
    d_out = gu.dev_zeros(T * C_ * n * 2)
    ctx.plc_conceal(gu.to_dev(np.asarray(flags, np.uint8)), gu.dev_zeros(C_ * capi.PLC_STATE.itemsize), d_out, C_, T, n, pcm=gu.to_dev(rows),
                    stats=d_st)
    gu.torch_cuda().cuda.synchronize()
    assert np.array_equal(gu.to_host(d_out, "<i2", rows.shape)[flags == pm.PLAYED], rows[flags == pm.PLAYED])
    return stats_of(d_st, (T, C_))


def snd_records(ctx, rows, frames):
    F_, _, n = rows.shape
    d_st = gu.dev_zeros(F_ * D * K * 16, 0x5A)
    d_fr = gu.dev_zeros(rows.nbytes) if frames else None
    ctx.snd_combine(gu.to_dev(rows), D, K, F_, n, frames=d_fr, stats=d_st)
    gu.torch_cuda().cuda.synchronize()
    return stats_of(d_st, (F_, D * K))


@pytest.mark.parametrize("n", (160, 21))
def test_three_entries_one_record(ctx, n):
    rows = make_rows(n)
    want = rec.records(rows)
    assert (want["flags"] == rec.FLAG_SILENT).any() and (want["flags"] == 0).any() and (want["sumsq"] > 2 ** 32).any()
    got = {"conf": conf_records(ctx, rows, np.arange(ROWS + 1)),
           "plc": plc_records(ctx, rows, np.full((F, ROWS), pm.PLAYED, np.uint8)),
           "snd records": snd_records(ctx, rows, frames=False),
           "snd both": snd_records(ctx, rows, frames=True)}
    for name, st in got.items():
        gu.assert_stats_equal(st, want)
        assert st.tobytes() == got["conf"].tobytes(), f"{name} differs from conf in {np.argwhere(st != got['conf'])[:5].tolist()}"


@pytest.mark.parametrize("n", (160, 21))
def test_empty_records_equal(ctx, n):
    rows = make_rows(n)[:, :2]
    conf = conf_records(ctx, rows, np.array([0, 1, 1]))              # port 1 has no member
    flags = np.array([[pm.PLAYED, pm.IDLE], [pm.PLAYED, pm.IDLE]], np.uint8)
    plc = plc_records(ctx, rows, flags)
    want = rec.records(rows, live=np.array([[True, False]] * F))
    gu.assert_stats_equal(conf, want)
    gu.assert_stats_equal(plc, want)
    assert conf[:, 1].tobytes() == plc[:, 1].tobytes() == (bytes(15) + bytes([rec.FLAG_EMPTY])) * F
    assert conf[:, 1].tobytes() != conf[:, 0].tobytes()
