"""-m "not gpu": the noise suppressor's rule on the host (include/igdsp.h, "Noise suppression") against tests/ns_model.py, bit for bit.
The rule runs three times: as a program of its own, tests/route/ns_rule_driver.cpp, which compiles csrc/igdsp_ns.h with g++ alone and
calls ns_frame_run (what igdsp_ns_frame calls) with one lane, the same program with the kernel's walk (16 threads as the 16 lanes of a
channel, a barrier where the kernel has its fence), and through the library's host-only entries.  Out, record and state at every
samples_per_frame from fresh, garbage-under-tag and wrong-tag states, any split of the frames, every ctl value and switches between
RUN, BYPASS and FREEZE in mid stream, cfg at its range ends and rejected cfgs, full-scale random, full-scale square and silent rows;
the tables against float64 numpy with their SHA-256 pinned; the conditions the rule was written to (delay, silence, noise, speech-like
bursts, a noise step with the estimate's trace, tones) and the integer rule against the float64 rule."""
import hashlib
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import ns_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL = -22
NS = (80, 160, 240, 320)
R, DELAY = 8000, 80
TABLES_SHA256 = "68d58791823583749b7fb3d0718238d591088b58405e502fec277feeeef9f539"
# Measured with tests/ns_model.py: the largest error of the unity-gain path against the delayed input is 1 LSB (the
# bound is 2), and the largest difference in output level between the integer rule and the float64 rule over scenes 3 (noise at sigma 8, 300, 3000)
# and 4 (bursts in noise): 0.1645 dB, at sigma = 8, where the output is +-1 LSB and its rounding is the difference; 0.0002 dB elsewhere.
# The bound is twice that
FLOAT_DEV_DB = 0.1645
FLOAT_BOUND_DB = 2 * FLOAT_DEV_DB
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
         os.path.join(ROOT, "tests", "route", "ns_rule_driver.cpp")]


def asker(exe, clean=False):
    def ask(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and (not clean or not r.stderr), r.stdout[-300:] + r.stderr[-2000:]
        return r.stdout.splitlines()
    return ask


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("ns_rule") / "ns_rule_driver")
    subprocess.run(["g++", *FLAGS, "-o", exe], check=True, capture_output=True, timeout=300)
    return asker(exe)


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


def hexs(rec):
    return " ".join(f"{int(w):x}" for w in np.frombuffer(np.asarray(rec).tobytes(), "<u8"))


def cfg_words(cfg):
    return " ".join(str(int(cfg[k])) for k in ("floor_q15", "over_q4", "init_hops", "track_shift", "rise_shift"))


def host(driver, cases):
    """cases: (cfg, state STATE record, x [F][n], ctl, lanes) -> per case (out [F][n] int16, rec [F] REC, state record)"""
    lines = []
    for cfg, st, x, ctl, lanes in cases:
        x = np.asarray(x)
        lines.append(f"{x.shape[1]} {x.shape[0]} {ctl} {lanes} {cfg_words(cfg)} {hexs(st)} " + " ".join(map(str, x.reshape(-1).tolist())))
    outs = driver("\n".join(lines) + "\n")
    assert len(outs) == len(cases)
    res = []
    for (cfg, st, x, ctl, lanes), line in zip(cases, outs):
        F_, n = np.asarray(x).shape
        tok = line.split()
        out, rec = np.zeros((F_, n), np.int16), np.zeros(F_, nm.REC)
        for f in range(F_):
            t = tok[f * (n + 2):(f + 1) * (n + 2)]
            rec[f] = np.frombuffer(np.array([int(t[0], 16), int(t[1], 16)], "<u8").tobytes(), nm.REC)[0]
            out[f] = np.array(t[2:], np.int64)
        sw = np.array([int(v, 16) for v in tok[F_ * (n + 2):]], "<u8")
        assert len(sw) == nm.STATE.itemsize // 8
        res.append((out, rec, np.frombuffer(sw.tobytes(), nm.STATE)[0]))
    return res


def rows(F_, n, seed):
    """[4][F][n]: full-scale random, +-full-scale square, silent, quiet noise"""
    rng = np.random.default_rng(seed)
    x = np.zeros((4, F_, n), np.int16)
    x[0] = rng.integers(-32768, 32768, (F_, n))
    x[1] = np.where(rng.integers(0, 2, (F_, n)) == 1, 32767, -32768)
    x[3] = rng.integers(-40, 41, (F_, n))
    return x


def states(seed):
    """fresh, garbage under the tag, garbage under a wrong tag"""
    return [np.zeros((), nm.STATE), nm.garbage_state(1, seed)[0], nm.garbage_state(1, seed + 1, tagged=False)[0]]


def check_against_model(driver, cfg, chans):
    """chans: (state, x [F][n], ctl, lanes): the driver's bytes equal the model's, channel by channel"""
    got = host(driver, [(cfg, st, x, ctl, lanes) for st, x, ctl, lanes in chans])
    x = np.stack([c[1] for c in chans], axis=1)
    out, rec, _, st = nm.run(x, cfg, ctl=[c[2] for c in chans], state=np.array([c[0] for c in chans], nm.STATE))
    for i, (o, r, s) in enumerate(got):
        assert np.array_equal(o, out[:, i]), (i, np.argwhere(o != out[:, i])[:4])
        assert r.tobytes() == rec[:, i].tobytes(), (i, r, rec[:, i])
        assert s.tobytes() == st[i].tobytes(), (i, [k for k in s.dtype.names if not np.array_equal(s[k], st[i][k])])
    return out, rec, st


def flat(o):
    return np.asarray(o).reshape(-1)


# ---- 1. every frame length, every kind of row over every kind of state, every ctl value, with one lane and with sixteen
@pytest.mark.parametrize("n", NS)
def test_host_equals_model(driver, n):
    F_ = 10
    x = rows(F_, n, 100 + n)
    chans = []
    for k in range(4):
        for j, st in enumerate(states(7 * n + k)):
            for ctl in (nm.RUN, nm.FREEZE, nm.BYPASS, nm.RESET, 200):
                if (k + j + ctl) % 2 == 0 or ctl == nm.RUN:
                    chans.append((st, x[k], ctl, 16 if (k + j + ctl) % 3 == 0 else 1))
    _, rec, st = check_against_model(driver, nm.cfg_of(), chans)
    fl = rec["flags"]
    assert (fl & nm.CLIPPED).any() and (fl[0] & nm.WAS_RESET).any() and not (fl[1:] & nm.WAS_RESET).any() and (fl & nm.LEARNING).any()
    assert (st["tag"] == nm.TAG).all() and not st["reserved"].any() and (st["Gt"] <= nm.UNITY).all() and (st["S"] <= nm.LEVEL_MASK).all()


def test_lanes_do_not_matter(driver):
    """the kernel's walk (16 lanes, a barrier per phase) and the host's (one lane) give the same bytes"""
    n, F_ = 240, 8
    x = rows(F_, n, 5)
    cfg = nm.cfg_of()
    for k in range(4):
        for st in states(k):
            for ctl in (nm.RUN, nm.FREEZE, nm.BYPASS):
                a, b = host(driver, [(cfg, st, x[k], ctl, 1), (cfg, st, x[k], ctl, 16)])
                assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_any_split_of_the_frames(driver):
    n, F_ = 160, 9
    x = rows(F_, n, 9)[0] // 8
    cfg = nm.cfg_of()
    for st in states(3):
        whole = host(driver, [(cfg, st, x, nm.RUN, 1)])[0]
        for cuts in ((1, 4, 9), tuple(range(1, 10))):
            s, a, outs, recs = st, 0, [], []
            for b in cuts:
                o, r, s = host(driver, [(cfg, s, x[a:b], nm.RUN, 1)])[0]
                outs.append(o), recs.append(r)
                a = b
            assert np.array_equal(np.concatenate(outs), whole[0]) and np.concatenate(recs).tobytes() == whole[1].tobytes() and s.tobytes() == whole[2].tobytes()


def test_switches_in_mid_stream(driver):
    """RUN <-> BYPASS <-> FREEZE between launches: driver and model agree; a bypassed stretch is the input through the delay bit for bit,
    and no switch clicks: around every switch the output stays within the unity path's error of the delayed input (floor_q15 = 32768)"""
    n, F_ = 160, 30
    rng = np.random.default_rng(12)
    x = (8000 * np.sin(2 * np.pi * 440 * np.arange(F_ * n) / R) + rng.normal(0, 200, F_ * n)).astype(np.int16).reshape(F_, n)
    plan = [(0, 5, nm.RUN), (5, 9, nm.BYPASS), (9, 14, nm.RUN), (14, 18, nm.FREEZE), (18, 22, nm.BYPASS), (22, 26, nm.FREEZE), (26, 30, nm.RUN)]
    for cfg in (nm.cfg_of(), nm.cfg_of(floor_q15=32768)):
        s_d, s_m, outs = np.zeros((), nm.STATE), np.zeros(1, nm.STATE), []
        for a, b, ctl in plan:
            o, r, s_d = host(driver, [(cfg, s_d, x[a:b], ctl, 16 if a % 2 else 1)])[0]
            mo, mr, _, s_m = nm.run(x[a:b, None, :], cfg, ctl=[ctl], state=s_m)
            assert np.array_equal(o, mo[:, 0]) and r.tobytes() == mr[:, 0].tobytes() and s_d.tobytes() == s_m[0].tobytes(), (a, b, ctl)
            assert (r["flags"] == nm.BYPASSED).all() if ctl == nm.BYPASS else (r["flags"] & nm.FROZEN).astype(bool).all() == (ctl == nm.FREEZE)
            outs.append(o)
        out = np.concatenate(outs).reshape(-1).astype(int)
        for a, b, ctl in plan:
            if ctl == nm.BYPASS:
                assert np.array_equal(out[a * n + DELAY:b * n], flat(x)[a * n:b * n - DELAY])
        if int(cfg["floor_q15"]) == nm.UNITY:
            assert np.abs(out[DELAY:] - flat(x).astype(int)[:-DELAY]).max() <= 2


def test_cfg_range_ends_and_rejected(driver, lib):
    n, F_ = 160, 20
    x = rows(F_, n, 2)[3] * 20
    ends = [nm.cfg_of(**{k: v}) for k, r in nm.RANGES.items() for v in r]
    ends += [nm.cfg_of(**{k: r[0] for k, r in nm.RANGES.items()}), nm.cfg_of(**{k: r[1] for k, r in nm.RANGES.items()})]
    for i, cfg in enumerate(ends):
        assert nm.cfg_ok(cfg)
        check_against_model(driver, cfg, [(st, x, nm.RUN, 16 if i % 2 else 1) for st in states(i)])
    st, zero = np.zeros((), nm.STATE), np.zeros(n, np.int16)
    for k, (lo, hi) in nm.RANGES.items():
        for v in (lo - 1, hi + 1):
            bad = nm.cfg_of(**{k: v})
            assert driver(f"{n} 1 0 1 {cfg_words(bad)} {hexs(st)} " + " ".join(["0"] * n) + "\n") == [str(EINVAL)]
            s = np.zeros((), capi.NS_STATE)
            assert capi.ns_frame(np.frombuffer(bad.tobytes(), capi.NS_CFG)[0], s, zero, raw=True) == EINVAL and not s.tobytes().strip(b"\0")
    good = capi.ns_cfg_default()
    assert good.tobytes() == nm.cfg_of().tobytes()
    for bad_n in (0, 8, 79, 81, 256, 400):
        assert capi.ns_frame(good, np.zeros((), capi.NS_STATE), np.zeros(bad_n, np.int16), raw=True) == EINVAL
    L = capi.load()
    s = np.zeros((), capi.NS_STATE)
    assert L.igdsp_ns_frame(None, s.ctypes.data, zero.ctypes.data, n, 0, None, None) == EINVAL
    assert L.igdsp_ns_frame(good.ctypes.data, None, zero.ctypes.data, n, 0, None, None) == EINVAL
    assert L.igdsp_ns_frame(good.ctypes.data, s.ctypes.data, None, n, 0, None, None) == EINVAL
    assert L.igdsp_ns_frame(good.ctypes.data, s.ctypes.data, zero.ctypes.data, n, 0, None, None) == 0 and s["tag"] == nm.TAG   # out and rec optional


def test_library_entry_is_the_rule(driver, lib):
    """igdsp_ns_frame through the library returns what the driver's ns_frame_run returns"""
    n, F_ = 320, 6
    x = rows(F_, n, 8)
    cfg = nm.cfg_of(over_q4=32, init_hops=5)
    for k in range(4):
        for st in states(60 + k):
            for ctl in (nm.RUN, nm.FREEZE, nm.BYPASS, nm.RESET):
                want = host(driver, [(cfg, st, x[k], ctl, 1)])[0]
                s = np.frombuffer(st.tobytes(), capi.NS_STATE).copy().reshape(())
                for f in range(F_):
                    o, r = capi.ns_frame(np.frombuffer(cfg.tobytes(), capi.NS_CFG)[0], s, x[k, f], ctl if f == 0 or ctl != nm.RESET else nm.RUN)
                    assert np.array_equal(o, want[0][f]) and r.tobytes() == want[1][f].tobytes(), (k, ctl, f)
                assert s.tobytes() == want[2].tobytes()


# ---- 2. the tables
def test_tables(driver, lib):
    tok = np.array(driver("T\n")[0].split(), np.int64)
    win, tw = tok[:160], tok[160:].reshape(128, 2)
    assert len(tok) == 160 + 256
    assert np.array_equal(win, nm.WIN) and np.array_equal(tw, nm.TW)
    lw, lt = capi.ns_tables()
    assert lw.dtype == np.int16 and lt.dtype == np.int32 and np.array_equal(lw, win) and np.array_equal(lt, tw)
    assert hashlib.sha256(win.astype("<i2").tobytes() + tw.astype("<i4").tobytes()).hexdigest() == TABLES_SHA256
    assert win.max() < 32768 and np.abs(win[:80] ** 2 + win[80:] ** 2 - (1 << 30)).max() <= 2 * 32768      # w[i]^2 + w[i+80]^2 = 2^30 up to rounding
    assert np.abs(tw[:, 0].astype(np.float64) ** 2 + tw[:, 1].astype(np.float64) ** 2 - 2.0 ** 60).max() <= 2.0 ** 32
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ns_tables.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and TABLES_SHA256 in r.stdout and "matches" in r.stdout, r.stdout + r.stderr


def test_header_constants():
    hdr = open(os.path.join(ROOT, "include", "igdsp.h")).read()
    for name, val in dict(TAG=nm.TAG, HOP=nm.HOP, BANDS=nm.BANDS, UNITY=nm.UNITY, RUN=nm.RUN, FREEZE=nm.FREEZE, BYPASS=nm.BYPASS, RESET=nm.RESET,
                          LEARNING=nm.LEARNING, SUPPRESSING=nm.SUPPRESSING, CLIPPED=nm.CLIPPED, FROZEN=nm.FROZEN, BYPASSED=nm.BYPASSED,
                          WAS_RESET=nm.WAS_RESET).items():
        m = re.search(rf"#define\s+IGDSP_NS_{name}\s+(0x[0-9A-Fa-f]+|\d+)", hdr)
        assert m and int(m.group(1), 0) == val == getattr(capi, "NS_" + name), name
    assert "#define IGDSP_ABI_VERSION 3" in hdr
    for a, b in ((capi.NS_CFG, nm.CFG), (capi.NS_STATE, nm.STATE), (capi.NS_REC, nm.REC)):
        assert a.itemsize == b.itemsize and [a.fields[k][1] for k in a.names] == [b.fields[k][1] for k in b.names]


# ---- 3. the conditions
@pytest.mark.parametrize("kind", (0, 1))
def test_condition_1_unity_gains_are_a_delay(driver, kind):
    """floor_q15 = 32768 forces every gain to unity: out = the input delayed by 80 samples within 2 LSB on full-scale random and
    +-full-scale square rows (measured: 1 LSB, the integer transform's own rounding)"""
    n, F_ = 160, 50
    x = rows(F_, n, 21)[kind]
    cfg = nm.cfg_of(floor_q15=32768)
    out, rec, _ = check_against_model(driver, cfg, [(np.zeros((), nm.STATE), x, nm.RUN, 1)])
    err = np.abs(flat(out).astype(int)[DELAY:] - flat(x).astype(int)[:-DELAY]).max()
    print("unity path, largest error against the delayed input:", err)
    assert err <= 2
    assert (rec["min_gain_q15"] == nm.UNITY).all() and not (rec["flags"] & nm.SUPPRESSING).any() and (flat(out)[:DELAY] == 0).all()


def test_condition_2_silence(driver):
    """silence in gives exact zero out from the first hop from a fresh state, and from any state within 4 frames"""
    n, F_ = 160, 6
    zero = np.zeros((F_, n), np.int16)
    loud = rows(12, n, 3)[0]
    _, _, settled = check_against_model(driver, nm.cfg_of(), [(np.zeros((), nm.STATE), loud, nm.RUN, 1)])
    sts = [np.zeros((), nm.STATE), settled[0]] + states(31)[1:]
    out, rec, _ = check_against_model(driver, nm.cfg_of(), [(st, zero, ctl, 16) for st in sts for ctl in (nm.RUN, nm.FREEZE, nm.BYPASS)])
    assert not out[:, :3].any()                                            # fresh: from the first sample
    assert not out[4:].any() and not rec["out_energy"][4:].any()


@pytest.mark.parametrize("sigma", (8, 300, 3000))
def test_condition_3_and_7_noise(sigma):
    """Gaussian noise, defaults, after 2 s: the output over the next 2 s lies between floor and floor - 1 dB below the input (14.0 ..
    15.0 dB; measured 14.76 / 14.93 / 14.93), and within FLOAT_BOUND_DB of the float64 rule's"""
    x = nm.frames_of(nm.noise(sigma, 4 * R, 5))
    o, f = flat(nm.run(x)[0]).astype(float), flat(nm.run_float(x))
    i = flat(x)[2 * R - DELAY:4 * R - DELAY]
    down, dev = nm.level_db(i) - nm.level_db(o[2 * R:]), abs(nm.level_db(o[2 * R:]) - nm.level_db(f[2 * R:]))
    print("sigma", sigma, "suppression", down, "integer against float", dev)
    assert 14.0 <= down <= 15.0
    assert dev <= FLOAT_BOUND_DB


def test_condition_4_and_7_speech_like():
    """harmonic bursts (RMS 4000, 0.4 s on / 0.3 s off, the first second noise only) in noise at sigma = 1000, after 2 s: the output over
    the bursts within 1 dB of the clean bursts (measured 0.76 dB lower), the pauses at least 9 dB down (measured 11.7)"""
    count = 6 * R
    sig, mask = nm.bursts(count, 3)
    x = np.clip(np.rint(sig + nm.noise(1000, count, 4)), -32768, 32767).astype(np.int16)
    out, of = flat(nm.run(nm.frames_of(x))[0]).astype(float), flat(nm.run_float(nm.frames_of(x)))
    late = np.arange(count - DELAY) >= 2 * R
    on, off = mask[:-DELAY] & late, ~mask[:-DELAY] & late
    burst = nm.level_db(out[DELAY:][on]) - nm.level_db(sig[:-DELAY][on])
    pause = nm.level_db(x[:-DELAY].astype(float)[off]) - nm.level_db(out[DELAY:][off])
    dev = max(abs(nm.level_db(out[DELAY:][m]) - nm.level_db(of[DELAY:][m])) for m in (on, off))
    print("bursts against clean", burst, "pauses down", pause, "integer against float", dev)
    assert abs(burst) <= 1.0 and pause >= 9.0 and dev <= FLOAT_BOUND_DB


def test_condition_5_noise_step():
    """sigma 100 -> 400 after 2 s: suppression back above 13 dB within 8 s of the step (measured 12.97 dB in the sixth second, 14.83 in
    the seventh), and it is the third branch of the noise estimate that carries N there: right after the step S >= 4 N in most bands and
    N moves by N >> rise_shift + 1 exactly; with that branch alone N gains under 1 dB in 3 s, which the trace shows while S stays above"""
    x = np.concatenate([nm.noise(100, 2 * R, 6), nm.noise(400, 8 * R, 7)])
    tr = {}
    o = flat(nm.run(nm.frames_of(x), trace=tr)[0]).astype(float)
    sup = [nm.level_db(x[s * R - DELAY:(s + 1) * R - DELAY]) - nm.level_db(o[s * R:(s + 1) * R]) for s in range(2, 10)]
    print("suppression per second after the step", sup)
    assert sup[0] < 6.0 and max(sup) > 13.0 and min(s for s, v in enumerate(sup) if v > 13.0) < 8
    N, S = np.array([t[0] for t in tr["N"]]), np.array([t[0] for t in tr["S"]])           # [hops][32]
    step = 2 * R // nm.HOP
    third = (S[step + 1:] >= 4 * N[step:-1]) & (N[step + 1:] == N[step:-1] + (N[step:-1] >> 9) + 1)
    second = (S[step + 1:] < 4 * N[step:-1]) & (N[step + 1:] == N[step:-1] + ((S[step + 1:] - N[step:-1]) >> 4))
    assert (third | second).all()                                          # every move of N is one of the two branches, exactly
    assert third[:100].mean() > 0.5 and third[:100].any(axis=0).all()      # the first second after the step: the third branch, in every band
    assert not third[-100:].any()                                          # settled: the second branch alone
    before = N[step - 1].sum()
    assert 10 * np.log10(N[-1].sum() / before) > 11.0                     # the estimate followed the 12 dB step
    lone = N[step].astype(float) * (1 + 2.0 ** -9) ** 300                  # the third branch alone for 3 s
    assert 10 * np.log10(lone.sum() / N[step].sum()) < 3.0                # which is why speech, above 4 N only in its bursts, hardly moves it


def test_condition_6_tones():
    """the documented limit and the reason for FREEZE: a -20 dBFS 1 kHz sine present from hop 0 is learnt as noise and lands at the
    floor; the same sine starting after 1 s of sigma = 30 noise is still within 1 dB of its level 3 s later; and under FREEZE from its
    start a sine keeps its level too while N does not move"""
    sine = np.rint(3276.7 * np.sin(2 * np.pi * 1000 * np.arange(5 * R) / R))
    o = flat(nm.run(nm.frames_of(sine.astype(np.int16)))[0]).astype(float)
    down = nm.level_db(sine[3 * R:]) - nm.level_db(o[3 * R:])
    x = nm.noise(30, 5 * R, 8).astype(float)
    x[R:] += sine[:4 * R]
    xi = np.rint(x).astype(np.int16)
    o2 = flat(nm.run(nm.frames_of(xi))[0]).astype(float)
    kept = nm.level_db(x[4 * R - DELAY:5 * R - DELAY]) - nm.level_db(o2[4 * R:])
    print("sine from hop 0 down by", down, "sine after 1 s down by", kept)
    assert 14.0 <= down <= 15.5 and abs(kept) <= 1.0
    _, _, _, st = nm.run(nm.frames_of(xi[:R]))
    o3, rec, _, st2 = nm.run(nm.frames_of(xi[R:]), ctl=[nm.FREEZE], state=st)
    assert np.array_equal(st2["N"], st["N"]) and np.array_equal(st2["S"], st["S"]) and st2["hops"] == st["hops"] and (rec["flags"] & nm.FROZEN).all()
    assert abs(nm.level_db(x[4 * R - DELAY:5 * R - DELAY]) - nm.level_db(flat(o3).astype(float)[3 * R:])) <= 1.0


# ---- 4. the host mirror
def test_host_mirror_leg_denoiser(lib):
    """LegDenoiser (libigdsp_host.so) is one leg through igdsp_ns_frame: the same bytes; a cfg out of range leaves the old one in place"""
    import ctypes

    H = ctypes.CDLL(igbuild.HOST_LIB)
    H.igdsp_host_ns_new.restype = ctypes.c_void_p
    for name in ("free", "config", "control", "process", "rec", "reset"):
        getattr(H, "igdsp_host_ns_" + name).argtypes = [ctypes.c_void_p] + {"config": [ctypes.c_void_p], "control": [ctypes.c_uint32],
                                                                            "process": [ctypes.c_void_p, ctypes.c_void_p], "rec": [ctypes.c_void_p]}.get(name, [])
    assert H.igdsp_host_ns_new(12) is None and H.igdsp_host_ns_new(400) is None
    n, F_ = 160, 5
    h = H.igdsp_host_ns_new(n)
    x = rows(F_, n, 4)[0] // 4
    out, rec = np.zeros(n, np.int16), np.zeros((), capi.NS_REC)

    def play(cfg, state, ctl):
        for f in range(F_):
            assert H.igdsp_host_ns_process(h, x[f].ctypes.data, out.ctypes.data) == 0 and H.igdsp_host_ns_rec(h, rec.ctypes.data) == 0
            o, r = capi.ns_frame(cfg, state, x[f], ctl)
            assert np.array_equal(out, o) and rec.tobytes() == r.tobytes(), f

    st = np.zeros((), capi.NS_STATE)
    play(capi.ns_cfg_default(), st, nm.RUN)
    assert H.igdsp_host_ns_control(h, nm.FREEZE) == 0
    play(capi.ns_cfg_default(), st, nm.FREEZE)
    assert H.igdsp_host_ns_control(h, nm.BYPASS) == 0
    play(capi.ns_cfg_default(), st, nm.BYPASS)
    assert H.igdsp_host_ns_control(h, nm.RESET) == EINVAL and H.igdsp_host_ns_control(h, nm.RUN) == 0
    bad, good = capi.ns_cfg_default(), capi.ns_cfg_default()
    bad["over_q4"], good["floor_q15"] = 65, 16384
    assert H.igdsp_host_ns_config(h, bad.ctypes.data) == EINVAL and H.igdsp_host_ns_config(h, None) == EINVAL
    play(capi.ns_cfg_default(), st, nm.RUN)                                 # the old cfg stands, the state too
    assert H.igdsp_host_ns_config(h, good.ctypes.data) == 0
    play(good, st, nm.RUN)
    H.igdsp_host_ns_reset(h)
    play(good, np.zeros((), capi.NS_STATE), nm.RUN)
    assert H.igdsp_host_ns_process(h, None, out.ctypes.data) == EINVAL
    H.igdsp_host_ns_free(h)
    assert H.igdsp_host_ns_process(None, x[0].ctypes.data, out.ctypes.data) == EINVAL and H.igdsp_host_ns_rec(None, rec.ctypes.data) == EINVAL


# ---- 5. the same program under the sanitizers
def test_asan_ubsan_build_agrees(tmp_path):
    """the rule built with -fsanitize=address,undefined as a program of its own: full-scale rows, garbage states and cfgs at their range
    ends run without a report (no sum overflows, nothing is indexed by a field) and give the model's bytes, with one lane and sixteen"""
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if shutil.which("g++") is None or subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, timeout=300).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")            # decided on a trivial program: an error in the driver fails below
    exe = str(tmp_path / "ns_rule_driver_san")
    subprocess.run(["g++", *FLAGS, *san, "-o", exe], check=True, capture_output=True, timeout=300)
    ask = asker(exe, clean=True)
    F_ = 6
    for i, n in enumerate(NS):
        x = rows(F_, n, 77 + n)
        cfg = [nm.cfg_of(), nm.cfg_of(**{k: r[0] for k, r in nm.RANGES.items()}), nm.cfg_of(**{k: r[1] for k, r in nm.RANGES.items()}), nm.cfg_of(floor_q15=32768)][i]
        chans = [(st, x[(k + j) % 4], (nm.RUN, nm.RESET, nm.BYPASS, nm.FREEZE, 9)[(k + j) % 5], 16 if (k + j) % 2 else 1) for k in range(4) for j, st in enumerate(states(50 + k))]
        check_against_model(ask, cfg, chans)
    assert ask("T\n")[0].split()[0] == str(int(nm.WIN[0]))
