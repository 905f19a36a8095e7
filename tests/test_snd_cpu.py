"""-m "not gpu": the sound-card splitter / combiner without a device: properties of tests/snd_model.py, the host mirror's SplitComb and
VU (libigdsp_host.so) against the model for every channel count, the host-only igdsp_snd_vu against Python, and the NULL-context paths
of the two device entries."""
import ctypes
import math

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import snd_model as sm

EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


@pytest.fixture(scope="module")
def host(lib):
    H = ctypes.CDLL(igbuild.HOST_LIB)
    vp, i = ctypes.c_void_p, ctypes.c_int
    for name, res, args in (("igdsp_host_sc_new", vp, [i, i]), ("igdsp_host_sc_free", None, [vp]), ("igdsp_host_sc_combine", i, [vp, vp, vp]),
                            ("igdsp_host_sc_split", i, [vp, vp, vp]), ("igdsp_host_sc_vu", i, [vp, vp, vp])):
        getattr(H, name).restype = res
        getattr(H, name).argtypes = args
    return H


def rand_pcm(rng, F, rows, n):
    pcm = rng.integers(-32768, 32768, (F, rows, n)).astype(np.int16)
    pcm[0, 0] = -32768
    if rows > 1:
        pcm[0, 1] = np.where(np.arange(n) & 1, -8, 8)
    return pcm


def test_model_round_trip_and_layout():
    rng = np.random.default_rng(1)
    for K in range(1, 9):
        for n in (1, 7, 160, 256):
            pcm = rand_pcm(rng, 3, 5 * K, n)
            fr = sm.combine(pcm, 5, K)
            assert fr.shape == (3, 5, n, K)
            np.testing.assert_array_equal(sm.split(fr), pcm)
            f, d, s, k = 2, 4, n - 1, K - 1
            assert fr[f, d, s, k] == pcm[f, d * K + k, s] and fr[0, 0, 0, 0] == pcm[0, 0, 0]
            assert fr.reshape(3, 5, n * K)[1, 2, (n // 2) * K + K // 2] == pcm[1, 2 * K + K // 2, n // 2]   # s * K + k


def test_model_one_channel_is_the_identity():
    rng = np.random.default_rng(2)
    pcm = rand_pcm(rng, 4, 9, 160)
    assert sm.combine(pcm, 9, 1).tobytes() == pcm.tobytes()
    assert sm.split(pcm.reshape(4, 9, 160, 1)).tobytes() == pcm.tobytes()


def test_model_records():
    n = 160
    pcm = np.zeros((1, 4, n), np.int16)
    pcm[0, 0] = -32768
    pcm[0, 1] = np.where(np.arange(n) & 1, -8, 8)
    pcm[0, 2, 5] = 9
    st = sm.records(pcm)
    assert st["peak"].tolist() == [[32768, 8, 9, 0]]
    assert st["sumsq"].tolist() == [[n * 32768 ** 2, n * 64, 81, 0]]
    assert st["flags"].tolist() == [[0, sm.FLAG_SILENT, 0, sm.FLAG_SILENT]]
    assert st["rms"][0, 0] == 32768.0 and st["rms"][0, 3] == 0.0 and np.all(st["byte_mean"] == 0)
    # the records of both sides of a card frame are the same rows
    rng = np.random.default_rng(3)
    x = rand_pcm(rng, 2, 12, 80)
    assert sm.records(sm.split(sm.combine(x, 2, 6))).tobytes() == sm.records(x).tobytes()


@pytest.mark.parametrize("K", range(1, 9))
def test_host_splitcomb_and_vu_vs_model(host, K):
    rng = np.random.default_rng(10 + K)
    for n in (1, 7, 160, 256):
        pcm = rand_pcm(rng, 1, K, n)
        want = sm.combine(pcm, 1, K)[0, 0]                               # [n][K]
        sc = host.igdsp_host_sc_new(K, n)
        assert sc
        try:
            rows = [np.ascontiguousarray(pcm[0, k]) for k in range(K)]
            ptrs = (ctypes.c_void_p * K)(*[r.ctypes.data for r in rows])
            frame = np.full(n * K + 8, 0x5A5A, np.int16)
            assert host.igdsp_host_sc_combine(sc, ptrs, frame.ctypes.data) == 0
            np.testing.assert_array_equal(frame[:n * K].reshape(n, K), want)
            assert np.all(frame[n * K:] == 0x5A5A)
            back = [np.full(n + 8, 0x5A5A, np.int16) for _ in range(K)]
            bptrs = (ctypes.c_void_p * K)(*[b.ctypes.data for b in back])
            assert host.igdsp_host_sc_split(sc, frame.ctypes.data, bptrs) == 0
            for k in range(K):
                np.testing.assert_array_equal(back[k][:n], pcm[0, k])
                assert np.all(back[k][n:] == 0x5A5A)
            vu = np.zeros(K + 1, capi.FRAME_STATS)
            vu[K]["sumsq"] = 0xDEAD
            assert host.igdsp_host_sc_vu(sc, frame.ctypes.data, vu.ctypes.data) == 0
            es = sm.records(pcm)[0]
            for f in ("sumsq", "peak", "byte_mean", "flags"):
                np.testing.assert_array_equal(vu[f][:K], es[f], err_msg=f)
            np.testing.assert_array_equal(vu["rms"][:K], np.sqrt(es["sumsq"].astype(np.float32) / np.float32(n)))   # sqrtf((float)sumsq / n)
            assert np.all(np.abs(vu["rms"][:K] - es["rms"]) <= 1e-5 * es["rms"]) and vu[K]["sumsq"] == 0xDEAD
            assert host.igdsp_host_sc_combine(sc, None, frame.ctypes.data) == EINVAL and host.igdsp_host_sc_vu(sc, None, vu.ctypes.data) == EINVAL
        finally:
            host.igdsp_host_sc_free(sc)
    assert host.igdsp_host_sc_combine(None, None, None) == EINVAL
    for bad in ((0, 160), (9, 160), (6, 0), (6, 257)):
        assert not host.igdsp_host_sc_new(*bad)


def test_snd_vu_vs_python(lib):
    rng = np.random.default_rng(5)
    rms = np.concatenate([[0.0, 1.0, 8.0, 299.99, 300.0, 29999.9, 30000.0, 32767.0, 32768.0, 1e-3],
                          rng.uniform(0, 32768, 500), 10.0 ** rng.uniform(-6, 4.5, 500)]).astype(np.float32)
    for r in rms:
        st = np.zeros((), capi.FRAME_STATS)
        st["rms"] = r
        vu = capi.snd_vu(st)
        p, db = sm.snd_vu(r)
        assert vu["percent"] == p, r                                     # exact
        assert abs(vu["db"] - db) <= 1e-9, r                             # libm's log10 against Python's, no more
    st = np.zeros((), capi.FRAME_STATS)
    assert capi.snd_vu(st) == {"percent": 0, "db": capi.SND_DB_FLOOR} and capi.SND_DB_FLOOR == sm.DB_FLOOR == -100.0
    st["rms"] = 32768.0
    assert capi.snd_vu(st) == {"percent": 109, "db": 0.0}
    st["rms"] = 30000.0
    assert capi.snd_vu(st)["percent"] == 100 and abs(capi.snd_vu(st)["db"] - 20 * math.log10(30000 / 32768)) <= 1e-9
    out = np.zeros((), capi.SND_VU)
    assert lib.igdsp_snd_vu(None, out.ctypes.data) == EINVAL and lib.igdsp_snd_vu(st.ctypes.data, None) == EINVAL
    assert capi.SND_VU.itemsize == 16 and capi.SND_MAX_CHANNELS == sm.MAX_CHANNELS == 8


def test_null_context_is_rejected_not_computed(lib):
    assert lib.igdsp_snd_combine(None, None, 1, 6, 1, 160, None, None, None) == EINVAL
    assert lib.igdsp_snd_split(None, None, 1, 6, 1, 160, None, None, None) == EINVAL
    assert lib.igdsp_snd_combine(None, None, 0, 6, 0, 160, None, None, None) == EINVAL      # even with nothing to do
