"""-m "not gpu": the conference mix's host side — igdsp_conf_level_q7 (pjsua's float -> Q7 mapping), igdsp_conf_build (the CSR of a
connection list), the host mirror's SLOT_VOLUME stepping (setSlotVolume / setvolumeSiteTone, no context) — and tests/conf_model.py on
hand cases where truncation and floor differ, both clamp stages and the EMPTY rules."""
import ctypes

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import conf_model as cm


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


@pytest.fixture(scope="module")
def host(lib):
    H = ctypes.CDLL(igbuild.HOST_LIB)
    vp, i, u32, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_float
    for name, res, args in (("igdsp_host_levels_new", vp, [u32]), ("igdsp_host_levels_free", None, [vp]),
                            ("igdsp_host_levels_map_call", i, [vp, i, u32]), ("igdsp_host_levels_bind_radio", i, [vp, i, i]),
                            ("igdsp_host_levels_set", i, [vp, f, f]), ("igdsp_host_levels_slot_volume", f, [vp]),
                            ("igdsp_host_set_slot_volume", i, [vp, i, i, i]), ("igdsp_host_set_volume_sidetone", i, [vp, i]),
                            ("igdsp_host_levels_gains", ctypes.POINTER(ctypes.c_uint16), [vp])):
        getattr(H, name).restype = res
        getattr(H, name).argtypes = args
    return H


# ---------------------------------------------------------------- igdsp_conf_level_q7
@pytest.mark.parametrize("level,q", [(0.0, 0), (np.float32(0.1), 13), (0.5, 64), (1.0, 128), (2.0, 256), (np.float32(1.9), 243)])
def test_level_q7_examples(lib, level, q):
    assert capi.conf_level_q7(float(level)) == q == cm.level_q7(level)


def test_level_q7_agrees_with_float32_expression(lib):
    levels = np.random.default_rng(1).uniform(0.0, 2.0, 10000).astype(np.float32)
    levels[:3] = (0.0, 2.0, 1.0)
    got = np.array([lib.igdsp_conf_level_q7(float(v)) for v in levels])
    adj = (levels - np.float32(1.0)) * np.float32(128.0)
    assert adj.dtype == np.float32
    np.testing.assert_array_equal(got, 128 + np.trunc(adj).astype(np.int64))


@pytest.mark.parametrize("level", [float("nan"), -0.01, -1.0, float("-inf"), float("inf"), 513.0, 1e30])
def test_level_q7_errors(lib, level):
    assert lib.igdsp_conf_level_q7(level) == -22
    assert cm.level_q7(level) is None
    with pytest.raises(capi.IgdspError):
        capi.conf_level_q7(level)


def test_level_q7_range_ends(lib):
    assert lib.igdsp_conf_level_q7(0.0) == 0                       # adj = -128: the lowest pjmedia accepts
    assert lib.igdsp_conf_level_q7(511.9921875) == 65535           # 128 + 65 407: the highest Q7 level
    assert lib.igdsp_conf_level_q7(512.0) == -22                   # 65 536
    assert lib.igdsp_conf_level_q7(-0.0078) == 0                   # (int)(-128.998) = -128


# ---------------------------------------------------------------- igdsp_conf_build
def test_build_sorts_and_dedups(lib):
    ch = [5, 1, 3, 1, 0, 5, 2, 2]
    pt = [2, 0, 2, 0, 2, 2, 0, 0]
    ptr, mem = capi.conf_build(ch, pt, 6, 4)
    assert ptr.tolist() == [0, 2, 2, 5, 5]                         # ports 1 and 3 empty
    assert mem.tolist() == [1, 2, 0, 3, 5]
    eptr, emem = cm.build(ch, pt, 6, 4)
    assert np.array_equal(ptr, eptr) and np.array_equal(mem, emem)


def test_build_random_against_model(lib):
    rng = np.random.default_rng(4)
    ch, pt = rng.integers(0, 300, 5000), rng.integers(0, 70, 5000)
    ptr, mem = capi.conf_build(ch, pt, 300, 70)
    eptr, emem = cm.build(ch, pt, 300, 70)
    assert np.array_equal(ptr, eptr) and np.array_equal(mem, emem)


def test_build_empty_and_errors(lib):
    ptr, mem = capi.conf_build([], [], 4, 3)
    assert ptr.tolist() == [0, 0, 0, 0] and mem.size == 0
    for ch, pt in (([4], [0]), ([0], [3]), ([0, 1, 9], [0, 0, 0])):
        with pytest.raises(capi.IgdspError):
            capi.conf_build(ch, pt, 4, 3)
    ptr = np.full(4, 7, np.uint32)
    nm = ctypes.c_uint32(99)
    a = np.array([0, 4], np.uint32)
    assert lib.igdsp_conf_build(a.ctypes.data, a.ctypes.data, 2, 4, 3, ptr.ctypes.data, a.ctypes.data, ctypes.byref(nm)) == -22
    assert ptr.tolist() == [7, 7, 7, 7] and nm.value == 99         # nothing written on error
    assert lib.igdsp_conf_build(None, None, 0, 4, 3, None, None, ctypes.byref(nm)) == -22
    assert lib.igdsp_conf_build(None, None, 1, 4, 3, ptr.ctypes.data, None, ctypes.byref(nm)) == -22


def test_mix_entry_rejects_null_ctx_without_gpu(lib):
    assert lib.igdsp_conf_mix(None, None, None, None, None, None, None, None, 0, 1, 1, 1, 160, None, None, None) == -22


# ---------------------------------------------------------------- the model on hand cases
def _mix1(xs, gains, length=None, n_ports=1, ptr=None, mem=None):
    x = np.asarray(xs, np.int64)[None]                             # [1][C][n]
    C_ = x.shape[1]
    ptr = np.array([0, C_], np.uint32) if ptr is None else np.asarray(ptr, np.uint32)
    mem = np.arange(C_, dtype=np.uint32) if mem is None else np.asarray(mem, np.uint32)
    return cm.mix(x, np.asarray(gains), ptr, mem, len(mem), n_ports, length)


def test_truncation_not_floor():
    assert cm.trunc_div(-3 * 13, 128) == 0 and (-3 * 13) // 128 == -1
    assert cm.trunc_div(-129 * 1, 128) == -1 and (-129 * 1) // 128 == -2
    o, st = _mix1([[-3, 3, -129, 129]], [13])
    assert o[0, 0].tolist() == [0, 0, -13, 13]
    o, st = _mix1([[-3, 3, -129, 129]], [1])
    assert o[0, 0].tolist() == [0, 0, -1, 1]


def test_both_clamp_stages():
    o, st = _mix1([[32767] * 4, [32767] * 4], [256, 256])         # per member: 65 534 -> 32 767; sum 65 534 -> 32 767
    assert o[0, 0].tolist() == [32767] * 4 and st["flags"][0, 0] & cm.FLAG_SATURATED
    o, st = _mix1([[-32768] * 2, [-32768] * 2], [128, 128])       # only the final clamp
    assert o[0, 0].tolist() == [-32768] * 2 and st["flags"][0, 0] & cm.FLAG_SATURATED and st["peak"][0, 0] == 32768
    o, st = _mix1([[32767, -32768], [-32767, 32767]], [256, 256])  # both members clamp, the sum does not
    assert o[0, 0].tolist() == [-1, -1] and st["flags"][0, 0] & cm.FLAG_SATURATED
    o, st = _mix1([[20000, -20000], [-100, 100]], [128, 128])
    assert o[0, 0].tolist() == [19900, -19900] and not st["flags"][0, 0] & cm.FLAG_SATURATED


def test_empty_rules():
    x = [[1000] * 4, [2000] * 4]
    # no members; members >= C only; every member len 0
    o, st = _mix1(x, [128, 128], n_ports=2, ptr=[0, 0, 1], mem=[7])
    assert st["flags"][0].tolist() == [cm.FLAG_EMPTY, cm.FLAG_EMPTY] and not o.any()
    o, st = _mix1(x, [128, 128], length=[[0, 0]])
    assert st["flags"][0, 0] == cm.FLAG_EMPTY and st["sumsq"][0, 0] == 0 and not o.any()
    # a muted member keeps the frame live: silent, not empty
    o, st = _mix1(x, [0, 0])
    assert st["flags"][0, 0] == cm.FLAG_SILENT
    # a descending port_ptr is empty; port_ptr past n_members is clamped
    o, st = _mix1(x, [128, 128], n_ports=2, ptr=[2, 1, 9], mem=[0, 1])
    assert st["flags"][0, 0] == cm.FLAG_EMPTY and o[0, 1].tolist() == [2000] * 4
    # a duplicate member is mixed twice; len cuts a member's samples
    o, st = _mix1(x, [128, 128], ptr=[0, 3], mem=[1, 1, 0], length=[[2, 4]])
    assert o[0, 0].tolist() == [5000, 5000, 4000, 4000]


# ---------------------------------------------------------------- host mirror: SLOT_VOLUME (roip_ed137.cpp:5190-5233, 6869-6878)
def _steps(start, k, up):
    v, out = np.float32(start), []
    for _ in range(k):
        v = np.float32(v + np.float32(0.1)) if up else np.float32(v - np.float32(0.1))
        v = min(v, np.float32(2.0)) if up else max(v, np.float32(0.0))
        out.append(v)
    return out


def test_slot_volume_stepping(host):
    L = host.igdsp_host_levels_new(8)
    try:
        assert host.igdsp_host_levels_slot_volume(L) == np.float32(2.0)          # roip_ed137.cpp:210
        assert host.igdsp_host_levels_gains(L)[3] == 256
        assert host.igdsp_host_set_slot_volume(L, 42, 0, 0) == 0                 # no such call: nothing stepped
        assert host.igdsp_host_levels_slot_volume(L) == np.float32(2.0)
        host.igdsp_host_levels_map_call(L, 42, 3)
        for want in _steps(2.0, 20, False):
            assert host.igdsp_host_set_slot_volume(L, 42, 0, 0) == 1
            assert host.igdsp_host_levels_slot_volume(L) == want
            assert host.igdsp_host_levels_gains(L)[3] == cm.level_q7(want)
        assert host.igdsp_host_levels_slot_volume(L) == 0.0 and host.igdsp_host_levels_gains(L)[3] == 0
        for want in _steps(0.0, 5, True):
            assert host.igdsp_host_set_slot_volume(L, 42, 1, 0) == 1
            assert host.igdsp_host_levels_slot_volume(L) == want
        assert [cm.level_q7(v) for v in _steps(0.0, 5, True)] == [13, 26, 39, 52, 64]
        assert host.igdsp_host_levels_gains(L)[3] == 64
        assert host.igdsp_host_levels_gains(L)[2] == 256                        # other channels untouched
    finally:
        host.igdsp_host_levels_free(L)


def test_slot_volume_sidetone_and_current(host):
    L = host.igdsp_host_levels_new(8)
    try:
        for call, ch in ((10, 0), (11, 2), (12, 4)):
            host.igdsp_host_levels_map_call(L, call, ch)
        host.igdsp_host_levels_bind_radio(L, 1, 11)
        host.igdsp_host_levels_set(L, 2.0, 0.3)
        host.igdsp_host_set_volume_sidetone(L, 11)                               # a bound radio: the sidetone level
        assert host.igdsp_host_levels_slot_volume(L) == np.float32(0.3) and host.igdsp_host_levels_gains(L)[2] == cm.level_q7(np.float32(0.3))
        host.igdsp_host_set_volume_sidetone(L, 12)                               # any other call: 0.5
        assert host.igdsp_host_levels_gains(L)[4] == 64
        host.igdsp_host_levels_set(L, 0.0, 0.3)                                  # setvolume's mute: SLOT_VOLUME = 0, current
        assert host.igdsp_host_set_slot_volume(L, 10, 0, 1) == 1 and host.igdsp_host_levels_gains(L)[0] == 0
        host.igdsp_host_levels_set(L, -0.5, 0.3)                                 # a level pjsua_conf_adjust_rx_level rejects
        assert host.igdsp_host_set_slot_volume(L, 10, 0, 1) == 0 and host.igdsp_host_levels_gains(L)[0] == 0
    finally:
        host.igdsp_host_levels_free(L)
