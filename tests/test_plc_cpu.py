"""-m "not gpu": tests/plc_model.py against itself and against the header: the scalar and the vectorised restatements agree on a fuzz;
lossless input passes through; a periodic history gives its period and its true continuation; the envelope; a reset state; IDLE;
recovery by hand; extreme inputs; split launches; and the state layout, constants and flag value of include/igdsp.h."""
import os
import re

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import capi
from tests import plc_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rand_state(rng, C_, garbage=False):
    st = np.zeros(C_, capi.PLC_STATE)
    st["hist"] = rng.integers(-32768, 32768, (C_, pm.HIST))
    st["cycle"] = rng.integers(-32768, 32768, (C_, pm.PMAX))
    if garbage:
        for k in ("head", "pitch", "pos", "missing"):
            st[k] = rng.integers(0, 65536, C_)
        st["runs"] = rng.integers(0, 1 << 32, C_)
        st["concealed"] = rng.integers(0, 1 << 32, C_)
        st["reserved"] = rng.integers(0, 1 << 32, (C_, 4))
    return st


def rand_ticks(rng, T, C_, n):
    fl = rng.choice(np.array([pm.IDLE, pm.PLAYED, pm.PLAYED, pm.PLAYED, pm.LOST, pm.LOST, 0, 9], np.uint8), (T, C_))
    ln = np.where(rng.random((T, C_)) < 0.2, rng.integers(0, n + 5, (T, C_)), n).astype(np.uint16)
    return fl, ln


def same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k
    assert a[3].tobytes() == b[3].tobytes()


@pytest.mark.parametrize("n", [1, 24, 80, 160, 164, 256])
def test_restatements_agree(n):
    rng = np.random.default_rng(n)
    C_, T = 4, 14
    fl, ln = rand_ticks(rng, T, C_, n)
    x = rng.integers(-32768, 32768, (T, C_, n))
    st = rand_state(rng, C_, garbage=n % 2 == 0)
    same(pm.run(fl, x, ln, st), pm.run_scalar(fl, x, ln, st))


def test_lossless_passes_through_and_ring_is_the_tail():
    rng = np.random.default_rng(1)
    C_, T, n = 3, 5, 160
    x = rng.integers(-32768, 32768, (T, C_, n))
    out, lo, st, rec = pm.run(np.full((T, C_), pm.PLAYED), x)
    assert np.array_equal(out, x) and np.all(lo == n)
    assert np.all(rec["head"] == (T * n) % pm.HIST) and np.all(rec["runs"] == 0) and np.all(rec["missing"] == 0)
    tail = x.transpose(1, 0, 2).reshape(C_, T * n)[:, -pm.HIST:]
    y = np.stack([np.roll(rec["hist"][c], -int(rec["head"][c])) for c in range(C_)])
    assert np.array_equal(y, tail)
    assert np.array_equal(st["sumsq"], (x * x).sum(axis=2).astype(np.uint64)) and not (st["flags"] & pm.FLAG_CONCEALED).any()


@pytest.mark.parametrize("P", [40, 57, 80, 113, 120])
def test_periodic_history_gives_its_period(P):
    rng = np.random.default_rng(P)
    n = 160
    pat = rng.integers(-20000, 20000, P)
    sig = np.tile(pat, 4 * 160 // P + 1)                        # 3 good ticks, then 6 lost ones
    T = 9
    x = np.zeros((T, 1, n), np.int64)
    x[:3, 0] = sig[:3 * n].reshape(3, n)
    fl = np.array([pm.PLAYED] * 3 + [pm.LOST] * 6, np.uint8)[:, None]
    out, lo, st, rec = pm.run(fl, x)
    assert rec["pitch"][0] == P and rec["runs"][0] == 1 and rec["concealed"][0] == 6
    q = P >> 2
    conceal = out[3:, 0].reshape(-1)
    truth = sig[3 * n:3 * n + 80]
    assert np.array_equal(conceal[q:80], truth[q:80])          # past the fade-in, full gain: the true continuation
    same(pm.run(fl, x), pm.run_scalar(fl, x))


def test_envelope():
    """full gain for 80 samples, then -82 / 32768 per sample: the last nonzero synthetic sample is run index 479, silence from 480"""
    n = 160
    x = np.zeros((8, 1, n), np.int64)
    x[0, 0] = 32767
    x[1, 0] = 32767                                            # a constant history: any lag matches, the cycle is constant 32767
    fl = np.array([pm.PLAYED, pm.PLAYED] + [pm.LOST] * 6, np.uint8)[:, None]
    out, _, st, rec = pm.run(fl, x)
    run = out[2:, 0].reshape(-1).astype(np.int64)
    assert np.all(run[:80] == 32767)
    assert run[479] != 0 and np.all(run[480:] == 0)
    assert np.all(np.diff(run[80:480]) <= 0)
    assert rec["missing"][0] == 6 * n and (st["flags"][2:, 0] & pm.FLAG_CONCEALED).all()
    assert st["flags"][-1, 0] == pm.FLAG_SILENT | pm.FLAG_CONCEALED


def test_reset_state_conceals_to_silence():
    fl = np.full((4, 2), pm.LOST, np.uint8)
    out, lo, st, rec = pm.run(fl, np.zeros((4, 2, 160), np.int64))
    assert not out.any() and np.all(lo == 160) and np.all(rec["runs"] == 1) and np.all(rec["pitch"] == pm.PMIN)
    assert np.all(st["flags"] == pm.FLAG_SILENT | pm.FLAG_CONCEALED)


def test_idle_resets_the_run():
    rng = np.random.default_rng(3)
    n = 80
    x = rng.integers(-9000, 9000, (7, 1, n))
    fl = np.array([pm.PLAYED, pm.PLAYED, pm.PLAYED, pm.LOST, pm.IDLE, pm.PLAYED, pm.LOST], np.uint8)[:, None]
    out, lo, st, rec = pm.run(fl, x)
    assert not out[4].any() and lo[4, 0] == 0 and st["flags"][4, 0] == pm.FLAG_EMPTY
    assert np.array_equal(out[5], x[5])                        # no recovery fade after IDLE
    assert rec["runs"][0] == 2                                 # the LOST tick after it starts a new run
    same(pm.run(fl, x), pm.run_scalar(fl, x))


def test_recovery_by_hand():
    """the first good tick after a run: q = pitch >> 2 samples cross-faded from the cycle into the input, pos advancing by q"""
    ch = pm.Chan()
    ch.pitch, ch.pos, ch.missing = 40, 37, 100
    ch.cycle[:40] = list(range(1000, 1040))
    x = [5000] * 24
    out, kind = ch.tick(pm.PLAYED, x, 24, 24)
    q = 10
    exp = []
    for i in range(24):
        if i < q:
            s = ((1000 + (37 + i) % 40) * (32768 - (100 + i - 80) * 82) + 16384) >> 15
            w = ((i + 1) << 15) // (q + 1)
            exp.append((s * (32768 - w) + 5000 * w + 16384) >> 15)
        else:
            exp.append(5000)
    assert kind == "good" and out == exp and ch.missing == 0 and ch.pos == (37 + q) % 40
    # q beyond the tick: only n samples blended, pos advances by n
    ch = pm.Chan()
    ch.pitch, ch.pos, ch.missing = 120, 0, 1
    out, _ = ch.tick(pm.PLAYED, [0] * 8, 8, 8)
    assert ch.pos == 8 and ch.missing == 0
    # PLAYED with len 0 is a loss, not a recovery
    ch = pm.Chan()
    ch.missing = 5
    _, kind = ch.tick(pm.PLAYED, [1] * 8, 0, 8)
    assert kind == "concealed" and ch.missing == 13 and ch.runs == 0


def test_extreme_inputs_stay_in_int32():
    for v in (-32768, 32767):
        n = 160
        x = np.full((6, 1, n), v, np.int64)
        x[1, 0, ::2] = -32768
        fl = np.array([pm.PLAYED, pm.PLAYED, pm.LOST, pm.LOST, pm.PLAYED, pm.LOST], np.uint8)[:, None]
        ch = pm.Chan()
        biggest = 0
        for t in range(6):
            y = [ch.y(k) for k in range(pm.HIST)]
            biggest = max(biggest, max(abs(a) for a in y) * 32768 + 16384)
            out, _ = ch.tick(int(fl[t, 0]), [int(a) for a in x[t, 0]], n, n)
            assert all(-32768 <= a <= 32767 for a in out)
        assert biggest < 2 ** 31
        same(pm.run(fl, x), pm.run_scalar(fl, x))


def test_split_launches_identical():
    rng = np.random.default_rng(8)
    C_, T, n = 5, 40, 24
    fl, ln = rand_ticks(rng, T, C_, n)
    x = rng.integers(-32768, 32768, (T, C_, n))
    st = rand_state(rng, C_)
    whole = pm.run(fl, x, ln, st)
    cur, outs = st, []
    for a, b in ((0, 1), (1, 17), (17, 18), (18, 40)):
        r = pm.run(fl[a:b], x[a:b], ln[a:b], cur)
        outs.append(r)
        cur = r[3]
    assert np.array_equal(np.concatenate([o[0] for o in outs]), whole[0])
    assert np.array_equal(np.concatenate([o[1] for o in outs]), whole[1])
    assert cur.tobytes() == whole[3].tobytes()


def test_layouts_agree():
    assert capi.PLC_STATE.itemsize == 832
    hdr = open(os.path.join(ROOT, "include", "igdsp.h")).read()
    body = re.search(r"typedef struct igdsp_plc_state \{(.*?)\} igdsp_plc_state;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", x).strip() for x in decl.split(None, 1)[1].split(",")]
    assert names == list(capi.PLC_STATE.names)
    for name, val in (("IGDSP_PLC_PMIN", capi.PLC_PMIN), ("IGDSP_PLC_PMAX", capi.PLC_PMAX), ("IGDSP_PLC_SPAN", capi.PLC_SPAN),
                      ("IGDSP_PLC_HIST", capi.PLC_HIST), ("IGDSP_PLC_FLAT", capi.PLC_FLAT), ("IGDSP_PLC_STEP", capi.PLC_STEP)):
        m = re.search(rf"#define\s+{name}\s+(\d+)", hdr)
        assert m and int(m.group(1)) == val, name
    m = re.search(r"#define\s+IGDSP_FLAG_CONCEALED\s+(0x[0-9A-Fa-f]+)", hdr)
    assert m and int(m.group(1), 16) == capi.FLAG_CONCEALED == pm.FLAG_CONCEALED
    assert (capi.PLC_PMIN, capi.PLC_PMAX, capi.PLC_SPAN, capi.PLC_HIST, capi.PLC_FLAT, capi.PLC_STEP) == (
        pm.PMIN, pm.PMAX, pm.SPAN, pm.HIST, pm.FLAT, pm.STEP)
    assert capi.PLC_HIST == capi.PLC_SPAN + capi.PLC_PMAX
    assert (capi.JB_IDLE, capi.JB_PLAYED, capi.JB_LOST) == (pm.IDLE, pm.PLAYED, pm.LOST)
    assert capi.PLC_STATE["hist"].shape == (280,) and capi.PLC_STATE.fields["cycle"][1] == 560 and capi.PLC_STATE.fields["runs"][1] == 808
