"""-m "not gpu": the filter's rule on the host (include/igdsp.h, "Filter") against tests/filt_model.py, bit for bit.  The rule runs twice:
as a program of its own, tests/route/filt_rule_driver.cpp, which compiles csrc/igdsp_filt.h with g++ alone and calls filt_frame_run
(what igdsp_filt_frame calls and k_filt compiles), and through the library's host-only entries igdsp_filt_frame, _plan_check, _design
and _plan_preset.  Every preset at 8 000, 16 000 and 48 000 Hz over random, full-scale and silent rows from fresh, garbage-under-tag and
wrong-tag states at every frame length, any split of the frames, the identity, BYPASS and a channel without a plan, bad plans, an
extremal section that clips without wrapping, the frequency response against the float64 response of the quantised coefficients, the
zero-input decay to exact zero, the designs against float64 numpy and the presets' pinned integers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import filt_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL = -22
RATES = (8000, 16000, 48000)
NS = (8, 24, 160, 256)
FREQS = (100, 150, 250, 300, 500, 1000, 2000, 3000, 3400)
# The largest deviation of the second half's RMS from the float64 response of the quantised coefficients, over every preset at 8 000
# and 48 000 Hz and the points of FREQS whose float64 response lies above -30 dB, measured with tests/filt_model.py: 0.0142 dB (DC_BLOCK
# at 48 000 Hz, 100 Hz; 0.0023 dB at 8 000 Hz).  The bound is twice that
RESPONSE_DEV_DB = 0.01422
RESPONSE_BOUND_DB = 2 * RESPONSE_DEV_DB
PINNED_8000 = {
    fm.VOICE_BAND: [(6934, -13868, 6934, -13674, 5871), (5863, 11727, 5863, 11051, 4211)],
    fm.CTCSS_HP: [(6646, -13291, 6646, -13105, 5285), (7416, -14833, 7416, -14625, 6848)],
    fm.DEEMPH: [(6124, -424, 0, -6472, 0)],
    fm.PREEMPH: [(10958, -8657, 0, -567, 0)],
    fm.DC_BLOCK: [(8128, -8128, 0, -8064, 0)],
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("filt_rule") / "filt_rule_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "filt_rule_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)

    def ask(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-300:] + r.stderr
        return r.stdout.splitlines()

    return ask


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


def hex6(rec):
    return " ".join(f"{int(w):x}" for w in np.frombuffer(np.asarray(rec).tobytes(), "<u8"))


def host(driver, cases):
    """cases: (plan PLAN record or None, state STATE record, x [F][n], ctl) -> per case (out [F][n] int16, rec [F] REC, state record)"""
    lines = []
    for plan, st, x, ctl in cases:
        x = np.asarray(x)
        p = np.zeros((), fm.PLAN) if plan is None else plan
        lines.append(f"{x.shape[1]} {x.shape[0]} {ctl} {0 if plan is None else 1} {hex6(p)} {hex6(st)} " + " ".join(map(str, x.reshape(-1).tolist())))
    outs = driver("\n".join(lines) + "\n")
    assert len(outs) == len(cases)
    res = []
    for (plan, st, x, ctl), line in zip(cases, outs):
        F_, n = np.asarray(x).shape
        tok = line.split()
        out, rec = np.zeros((F_, n), np.int16), np.zeros(F_, fm.REC)
        for f in range(F_):
            t = tok[f * (n + 2):(f + 1) * (n + 2)]
            rec[f] = np.frombuffer(np.array([int(t[0], 16), int(t[1], 16)], "<u8").tobytes(), fm.REC)[0]
            out[f] = np.array(t[2:], np.int64)
        sw = np.array([int(v, 16) for v in tok[F_ * (n + 2):]], "<u8")
        assert len(sw) == 6
        res.append((out, rec, np.frombuffer(sw.tobytes(), fm.STATE)[0]))
    return res


def rows(F_, n, seed):
    """[3][F][n]: random, full scale (square waves and runs of both extremes), silent"""
    rng = np.random.default_rng(seed)
    x = np.zeros((3, F_, n), np.int16)
    x[0] = rng.integers(-32768, 32768, (F_, n))
    x[1] = np.where(rng.integers(0, 2, (F_, n)) == 1, 32767, -32768)
    x[1, 0, : n // 2] = -32768
    return x


def states(seed):
    """fresh, garbage under the tag, garbage under a wrong tag"""
    return [np.zeros((), fm.STATE), fm.garbage_state(1, seed)[0], fm.garbage_state(1, seed + 1, tagged=False)[0]]


def check_against_model(driver, plans, chans, max_sections=0):
    """chans: (plan index or None, state, x [F][n], ctl): the driver's bytes equal the model's, channel by channel"""
    cases = [(None if pi is None else plans[pi], st, x, ctl) for pi, st, x, ctl in chans]
    got = host(driver, cases)
    x = np.stack([c[2] for c in chans], axis=1)
    out, rec, _, st = fm.run(plans, x, plan_of=[len(plans) if c[0] is None else c[0] for c in chans], ctl=[c[3] for c in chans],
                             state=np.array([c[1] for c in chans], fm.STATE), max_sections=max_sections)
    rec = rec.copy()
    rec["plan"] = 0                                                        # the host entry knows no index
    for i, (o, r, s) in enumerate(got):
        assert np.array_equal(o, out[:, i]), (i, np.argwhere(o != out[:, i])[:4])
        assert r.tobytes() == rec[:, i].tobytes(), (i, r, rec[:, i])
        assert s.tobytes() == st[i].tobytes(), (i, s, st[i])
    return out, rec, st


# ---- 1. every preset at every rate and frame length, every kind of row over every kind of state
@pytest.mark.parametrize("n", NS)
def test_host_equals_model(driver, n):
    plans = np.array([fm.plan_of_sections(fm.preset_sections(p, r), r) for p in fm.PRESETS for r in RATES], fm.PLAN)
    F_ = 3
    chans = []
    for pi in range(len(plans)):
        x = rows(F_, n, 100 * n + pi)
        for k, st in enumerate(states(7 * n + pi)):
            chans.append((pi, st, x[(k + pi) % 3], fm.RESET if (pi + k) % 7 == 0 else fm.RUN))
        chans.append((pi, states(pi)[1], x[0], 200))                        # a value above 2 counts as RUN
    _, rec, st = check_against_model(driver, plans, chans)
    assert (rec["flags"] & fm.CLIPPED).any() and (rec["flags"][0] & fm.WAS_RESET).any() and not (rec["flags"][1:] & fm.WAS_RESET).any()
    assert (st["tag"] == fm.TAG).all() and not st["reserved"].any() and (st["h"][:, :, 4] <= fm.EMASK).all()


def test_library_entry_is_the_rule(driver, lib):
    """igdsp_filt_frame through the library returns what the driver's filt_frame_run returns"""
    n, F_ = 160, 4
    for p in fm.PRESETS:
        plan = fm.plan_of_sections(fm.preset_sections(p, 16000), 16000)
        x = rows(F_, n, p)[0]
        st0 = states(p)[1]
        (out, rec, st), = host(driver, [(plan, st0, x, fm.RUN)])
        s = np.frombuffer(bytearray(st0.tobytes()), capi.FILT_STATE)
        for f in range(F_):
            o, r = capi.filt_frame(np.frombuffer(plan.tobytes(), capi.FILT_PLAN)[0], s, x[f])
            assert np.array_equal(o, out[f]) and r.tobytes() == rec[f].tobytes()
        assert s.tobytes() == st.tobytes()
    s = np.zeros((), capi.FILT_STATE)
    for bad_n in (0, 4, 12, 264):
        with pytest.raises(capi.IgdspError):
            capi.filt_frame(None, s, np.zeros(bad_n, np.int16))
    o, r = capi.filt_frame(None, s, np.arange(8, dtype=np.int16))
    assert np.array_equal(o, np.arange(8)) and r["flags"] == fm.NO_PLAN and not s.tobytes().strip(b"\0")


# ---- 2. any split of the frames writes the same bytes
def test_any_split(driver):
    n, F_ = 24, 6
    plan = fm.plan_of_sections(fm.preset_sections(fm.CTCSS_HP, 8000))
    x = rows(F_, n, 3)[0]
    for st0 in states(11):
        (out, rec, st), = host(driver, [(plan, st0, x, fm.RESET)])
        for cuts in ((1, 3, 6), (1, 2, 3, 4, 5, 6), (5, 6)):
            a, s, outs, recs = 0, st0, [], []
            for b in cuts:
                (o, r, s), = host(driver, [(plan, s, x[a:b], fm.RESET if a == 0 else fm.RUN)])
                outs.append(o)
                recs.append(r)
                a = b
            assert np.array_equal(np.concatenate(outs), out) and np.concatenate(recs).tobytes() == rec.tobytes() and s.tobytes() == st.tobytes(), cuts


# ---- 3. the identity; BYPASS and a channel without a plan leave the state's bytes alone
def test_identity_bypass_and_no_plan(driver):
    n, F_ = 160, 2
    x = rows(F_, n, 5)
    ident = fm.plan_of_sections([fm.IDENTITY], n_sections=4)
    voice = fm.plan_of_sections(fm.preset_sections(fm.VOICE_BAND, 8000))
    for st0 in states(21):
        for k in range(3):
            (out, rec, st), = host(driver, [(ident, st0, x[k], fm.RUN)])
            assert np.array_equal(out, x[k]) and not rec["n_clipped"].any() and (rec["in_peak"] == rec["out_peak"]).all()
            zero = st0["tag"] != fm.TAG
            assert np.array_equal(st["h"][:, 4], np.zeros(4) if zero else st0["h"][:, 4] & fm.EMASK)          # e stays (0 from fresh)
            for plan, ctl, flag in ((voice, fm.BYPASS, fm.BYPASSED), (None, fm.RUN, fm.NO_PLAN), (None, fm.RESET, fm.NO_PLAN),
                                    (fm.plan_of_sections([], n_sections=0), fm.RUN, fm.NO_PLAN)):
                (out, rec, st), = host(driver, [(plan, st0, x[k], ctl)])
                assert np.array_equal(out, x[k]) and (rec["flags"] == flag).all() and st.tobytes() == st0.tobytes()
                assert (rec["in_peak"] == np.abs(x[k].astype(np.int64)).max(axis=1)).all() and (rec["out_peak"] == rec["in_peak"]).all()
    chans = [(0, states(2)[1], x[0], fm.BYPASS), (None, states(2)[1], x[0], fm.RUN), (1, states(2)[2], x[1], fm.BYPASS)]
    check_against_model(driver, np.array([voice, fm.plan_of_sections([], n_sections=0)], fm.PLAN), chans)


# ---- 4. plans of any bytes
def test_bad_plans(driver, lib):
    n, F_ = 24, 3
    x = rows(F_, n, 9)
    good = fm.preset_sections(fm.CTCSS_HP, 8000)
    bad = (32767, -32768, 1, 0, 0)                                         # the magnitudes sum to 65 536
    assert not fm.valid(bad) and fm.valid((32767, -32767, 1, 0, 0))
    rng = np.random.default_rng(1)
    plans = np.array([fm.plan_of_sections([good[0], bad, good[1]]),         # 0: the middle section is not run, its history stays
                      fm.plan_of_sections(good + [bad, bad], n_sections=2),  # 1: invalid sections past n_sections do not matter
                      fm.plan_of_sections(good, n_sections=0),              # 2: no plan
                      fm.plan_of_sections(good + good, n_sections=5),       # 3: read as 4
                      fm.plan_of_sections(good + good, n_sections=255),     # 4: read as 4
                      fm.plan_of_sections([bad, bad, bad, bad]),            # 5: nothing runs, the state is still written
                      np.frombuffer(rng.integers(0, 256, 48, dtype=np.uint8).tobytes(), fm.PLAN)[0]], fm.PLAN)   # 6: any bytes
    chans = [(pi, st, x[k], fm.RUN) for pi in range(len(plans)) for k, st in enumerate(states(30 + min(pi, 3)))]   # plans 3 and 4: the same states
    out, rec, st = check_against_model(driver, plans, chans)
    fl, nsec = rec["flags"][:, ::3], rec["n_sections"][0, ::3]
    assert nsec.tolist()[:6] == [3, 2, 0, 4, 4, 4]
    assert (fl[:, 0] & fm.BAD_PLAN).all() and not (fl[:, 1] & fm.BAD_PLAN).any() and (fl[:, 2] == fm.NO_PLAN).all()
    assert not (fl[:, 3] & (fm.BAD_PLAN | fm.NO_PLAN)).any() and np.array_equal(out[:, 9:12], out[:, 12:15])
    assert (fl[:, 5] & fm.BAD_PLAN).all() and np.array_equal(out[:, 15:18], np.stack([c[2] for c in chans[15:18]], axis=1))
    # plan 0 equals its two valid sections run as a two-section plan, and section 1's history is what was read
    two = check_against_model(driver, np.array([fm.plan_of_sections([good[0], fm.IDENTITY, good[1]])], fm.PLAN), [(0, c[1], c[2], c[3]) for c in chans[:3]])
    assert np.array_equal(two[0], out[:, :3])
    assert np.array_equal(st["h"][1, 1], chans[1][1]["h"][1] & np.array([0xFFFF] * 4 + [fm.EMASK], np.uint16))
    # the launch's word: a plan with more sections than max_sections is not run at all
    o2, r2, _, s2 = fm.run(plans[:2], np.stack([x[0], x[0]], axis=1), plan_of=[0, 1], state=np.array([chans[1][1], chans[1][1]], fm.STATE), max_sections=2)
    assert (r2["flags"][:, 0] == (fm.NO_PLAN | fm.BAD_PLAN)).all() and np.array_equal(o2[:, 0], x[0]) and s2[0].tobytes() == chans[1][1].tobytes()
    assert not (r2["flags"][:, 1] & fm.NO_PLAN).any()
    # igdsp_filt_plan_check flags what the kernel flags
    want = [EINVAL, 0, EINVAL, EINVAL, EINVAL, EINVAL]
    assert [capi.filt_plan_check(np.frombuffer(p.tobytes(), capi.FILT_PLAN)[0]) for p in plans[:6]] == want
    assert [int(v) for v in driver("".join(f"K {hex6(p)}\n" for p in plans[:6]))] == want
    assert lib.igdsp_filt_plan_check(None) == EINVAL


# ---- 5. an extremal valid section clips without wrapping
@pytest.mark.parametrize("sec", ((32767, 32767, 1, 0, 0), (16384, 16383, 0, -32768, 0), (-32768, 0, 0, 0, 32767), (1, 1, 1, -32766, -32766)))
def test_extremal_section_clips(driver, sec):
    assert sum(abs(v) for v in sec) == fm.SUM_MAX
    n, F_ = 160, 2
    x = np.zeros((4, F_, n), np.int16)
    x[0], x[1] = -32768, 32767
    x[2, :, ::2], x[2, :, 1::2] = -32768, 32767
    x[3, 0], x[3, 1] = -32768, 32767
    plans = np.array([fm.plan_of_sections([sec])], fm.PLAN)
    _, rec, _ = check_against_model(driver, plans, [(0, states(1)[k % 3], x[k], fm.RUN) for k in range(4)])     # the model asserts int32
    assert rec["n_clipped"].max() > 0 and ((rec["flags"] & fm.CLIPPED) != 0).tolist() == (rec["n_clipped"] > 0).tolist()
    assert rec["n_clipped"].max() <= n


# ---- 6. the frequency response of every preset
@pytest.mark.parametrize("rate", (8000, 48000))
def test_frequency_response(lib, rate):
    count = 6400 * rate // 8000                                            # every frequency: whole periods in the second half
    worst = 0.0
    for p in fm.PRESETS:
        secs = fm.preset_sections(p, rate)
        plan = capi.filt_plan_preset(p, rate)
        for f in FREQS:
            x = fm.sine(8000, f, rate, count)
            s = np.zeros((), capi.FILT_STATE)
            out = np.concatenate([capi.filt_frame(plan, s, x[k:k + 256])[0] for k in range(0, count, 256)])
            got = fm.rms_db(out[count // 2:]) - fm.rms_db(x[count // 2:])
            want = 20 * np.log10(fm.plan_response(secs, f, rate))
            print(f"rate {rate} preset {p} {f} Hz: float64 {want:.4f} dB, measured {got:.4f} dB, deviation {got - want:+.5f} dB")
            if want > -30.0:
                worst = max(worst, abs(got - want))
            if want > -33.0:
                # (above -30 dB: the bound.  Between -33 and -30 dB "3 dB under -30 dB" cannot hold even for the float64 response
                # itself - VOICE_BAND at 48 000 Hz has -30.41 dB at 100 Hz - so such a point is held to the bound as well, which asks more)
                assert abs(got - want) <= RESPONSE_BOUND_DB, (p, f, got, want)
            else:
                assert got <= -30.0 + RESPONSE_BOUND_DB - 3.0, (p, f, got, want)     # a deep point: only that it is deep
    print(f"rate {rate}: largest deviation above -30 dB {worst:.5f} dB (bound {RESPONSE_BOUND_DB:.5f})")


# ---- 7. zero input: the output reaches exact zero and stays there
@pytest.mark.parametrize("rate", (8000, 48000))
def test_zero_input_decay(lib, rate):
    x = np.concatenate([fm.sine(20000, 440, rate, 800), np.zeros(4000, np.int16)])
    for p in fm.PRESETS:
        plan = capi.filt_plan_preset(p, rate)
        s = np.zeros((), capi.FILT_STATE)
        out = np.concatenate([capi.filt_frame(plan, s, x[k:k + 160])[0] for k in range(0, len(x), 160)])
        assert out[:800].any() and not out[-1000:].any(), (p, int(np.flatnonzero(out)[-1]))


# ---- 8. the designs
KINDS = (fm.LOWPASS, fm.HIGHPASS, fm.BANDPASS, fm.NOTCH, fm.PEAK, fm.LOWSHELF, fm.HIGHSHELF, fm.LP1, fm.HP1)


def test_design_matches_float64(driver):
    grid = [(k, r, f0, q, g) for k in KINDS for r in (8000, 16000, 48000) for f0 in (60.0, 300.0, 1000.0, 2500.0, 3400.0)
            for q in (0.5, 0.7071067811865476, 2.0, 8.0) for g in (-6.0, 4.0)]
    outs = driver("".join(f"D {k} {r} {f0!r} {q!r} {g!r}\n" for k, r, f0, q, g in grid))
    ok = 0
    for (k, r, f0, q, g), line in zip(grid, outs):
        tok = [int(v) for v in line.split()]
        real = fm.design_real(k, r, f0, q, g)
        want = fm.quantise(real)
        if tok[0] != 0:
            assert tok == [EINVAL, 0], (k, r, f0, q, g, tok)               # and it wrote nothing
            assert want is None, (k, r, f0, q, g)                          # the model rejects what the library rejects
            continue
        ok += 1
        assert all(abs(a - int(np.rint(b * fm.UNITY))) <= 1 for a, b in zip(tok[1:], real)), (k, r, f0, q, g, tok, real)
        assert fm.valid(tok[1:]) and abs(tok[5]) < fm.UNITY and abs(tok[4]) < fm.UNITY + tok[5]
    assert ok > len(grid) * 3 // 4
    for k, r, f0, q, g in grid[::37]:
        want = fm.quantise(fm.design_real(k, r, f0, q, g))
        if want is not None:
            assert max(abs(a - b) for a, b in zip(capi.filt_design(k, r, f0, q, g).tolist(), want)) <= 1, (k, r, f0, q, g)     # the library's entry


def test_design_rejects_and_writes_nothing(driver, lib):
    bad = [(fm.LOWPASS, 8000, 4000.0, 0.7, 0.0), (fm.LOWPASS, 8000, 0.0, 0.7, 0.0), (fm.HIGHPASS, 8000, 300.0, 0.0, 0.0), (fm.NOTCH, 8000, 300.0, -1.0, 0.0),
           (99, 8000, 300.0, 0.7, 0.0), (fm.LOWPASS, 0, 300.0, 0.7, 0.0), (fm.PEAK, 8000, 1000.0, 1.0, 40.0),   # a coefficient leaves int16
           (fm.LOWPASS, 48000, 5.0, 10.0, 0.0),                            # the quantised poles reach the unit circle
           (fm.HP1, 8000, 5000.0, 1.0, 0.0), (fm.HIGHSHELF, 8000, 1000.0, 0.7, 30.0)]
    outs = driver("".join(f"D {k} {r} {f0!r} {q!r} {g!r}\n" for k, r, f0, q, g in bad))
    assert [line.split() for line in outs] == [[str(EINVAL), "0"]] * len(bad), outs
    out = np.full(5, 77, np.int16)
    for k, r, f0, q, g in bad:
        assert lib.igdsp_filt_design(k, r, f0, q, g, out.ctypes.data) == EINVAL and (out == 77).all()
    assert lib.igdsp_filt_design(fm.LOWPASS, 8000, 300.0, 0.7, 0.0, None) == EINVAL
    assert fm.quantise(fm.design_real(fm.LOWPASS, 48000, 5.0, 10.0)) is None


def test_presets(driver, lib):
    for p, want in PINNED_8000.items():
        assert fm.preset_sections(p, 8000) == want, p                      # the committed integers are the model's
        plan = capi.filt_plan_preset(p, 8000)
        assert int(plan["n_sections"]) == len(want) and int(plan["clock_rate"]) == 8000 and int(plan["reserved"]) == 0
        got = [tuple(int(v) for v in s) for s in plan["s"].tolist()]
        assert got == want + [fm.IDENTITY] * (4 - len(want)), (p, got)
        assert capi.filt_plan_check(plan) == 0
    lines = driver("".join(f"P {p} {r}\n" for p in fm.PRESETS for r in RATES + (7999, 48001, 6800, 6801)) + "P 5 8000\n")
    i = 0
    for p in fm.PRESETS:
        for r in RATES + (7999, 48001, 6800, 6801):
            want = fm.preset_sections(p, r)
            tok = lines[i].split()
            i += 1
            if want is None:
                assert tok == [str(EINVAL)], (p, r)
                continue
            plan = np.frombuffer(np.array([int(v, 16) for v in tok[1:]], "<u8").tobytes(), fm.PLAN)[0]
            assert tok[0] == "0" and plan.tobytes() == fm.plan_of_sections(want, r).tobytes(), (p, r)
            assert plan.tobytes() == capi.filt_plan_preset(p, r).tobytes()
    assert lines[i].split() == [str(EINVAL)]
    assert fm.preset_sections(fm.VOICE_BAND, 6800) is None and fm.preset_sections(fm.CTCSS_HP, 8000) is not None     # a corner at Nyquist
    plan = np.zeros((), capi.FILT_PLAN)
    assert lib.igdsp_filt_plan_preset(0, 6800, plan.ctypes.data) == EINVAL and not plan.tobytes().strip(b"\0")
    assert lib.igdsp_filt_plan_preset(0, 8000, None) == EINVAL


def test_yardstick_binding_is_the_entrys():
    """igdsp_internal_filt_move takes igdsp_filt_run's arguments: capi.INTERNAL_MORE is that list and capi.internal finds it"""
    res, args = capi.INTERNAL_MORE["igdsp_internal_filt_move"]
    pub = {name: (r, a) for name, r, a in capi.PROTOTYPES}["igdsp_filt_run"]
    assert (res, list(args)) == (pub[0], list(pub[1])) and capi.INTERNAL_MORE_TWIN["igdsp_internal_filt_move"] == "igdsp_filt_run"
    assert "igdsp_internal_filt_move" not in capi.INTERNAL
    assert capi.FILT_PLAN.itemsize == fm.PLAN.itemsize == 48 and capi.FILT_STATE.itemsize == fm.STATE.itemsize == 48 and capi.FILT_REC.itemsize == 16
    hdr = open(os.path.join(ROOT, "include", "igdsp.h")).read()
    for name, val in (("TAG", capi.FILT_TAG), ("RUN", capi.FILT_RUN), ("BYPASS", capi.FILT_BYPASS), ("RESET", capi.FILT_RESET), ("CLIPPED", capi.FILT_CLIPPED),
                      ("NO_PLAN", capi.FILT_NO_PLAN), ("BAD_PLAN", capi.FILT_BAD_PLAN), ("BYPASSED", capi.FILT_BYPASSED), ("WAS_RESET", capi.FILT_WAS_RESET),
                      ("HP1", capi.FILT_HP1), ("DC_BLOCK", capi.FILT_DC_BLOCK)):
        import re

        m = re.search(rf"#define\s+IGDSP_FILT_{name}\s+(0x[0-9A-Fa-f]+|\d+)", hdr)
        assert m and int(m.group(1), 0) == val == getattr(fm, name, val), name


def test_host_mirror_leg_filter(lib):
    """LegFilter (libigdsp_host.so) is one leg through igdsp_filt_frame: the same bytes, a new plan forgets the histories, a plan the
    check rejects leaves the old one in place, without a plan the row passes through"""
    import ctypes

    H = ctypes.CDLL(igbuild.HOST_LIB)
    H.igdsp_host_filt_new.restype = ctypes.c_void_p
    for name in ("free", "plan", "preset", "process", "rec", "reset"):
        getattr(H, "igdsp_host_filt_" + name).argtypes = [ctypes.c_void_p] + {"plan": [ctypes.c_void_p], "preset": [ctypes.c_uint32, ctypes.c_uint32],
                                                                              "process": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32],
                                                                              "rec": [ctypes.c_void_p]}.get(name, [])
    assert H.igdsp_host_filt_new(12) is None and H.igdsp_host_filt_new(264) is None
    n, F_ = 160, 3
    h = H.igdsp_host_filt_new(n)
    x = rows(F_, n, 4)[0]
    out, rec = np.zeros(n, np.int16), np.zeros((), capi.FILT_REC)

    def play(plan, state):
        for f in range(F_):
            assert H.igdsp_host_filt_process(h, x[f].ctypes.data, out.ctypes.data, fm.RUN) == 0 and H.igdsp_host_filt_rec(h, rec.ctypes.data) == 0
            o, r = capi.filt_frame(plan, state, x[f])
            assert np.array_equal(out, o) and rec.tobytes() == r.tobytes(), f

    play(None, np.zeros((), capi.FILT_STATE))                               # no plan yet: NO_PLAN, the row as it came
    assert np.array_equal(out, x[-1]) and rec["flags"] == fm.NO_PLAN
    assert H.igdsp_host_filt_preset(h, fm.CTCSS_HP, 8000) == 0
    play(capi.filt_plan_preset(fm.CTCSS_HP, 8000), np.zeros((), capi.FILT_STATE))
    bad = capi.filt_plan_preset(fm.DC_BLOCK, 8000)
    bad["n_sections"] = 0
    assert H.igdsp_host_filt_plan(h, bad.ctypes.data) == EINVAL and H.igdsp_host_filt_preset(h, fm.VOICE_BAND, 6000) == EINVAL
    assert H.igdsp_host_filt_plan(h, None) == EINVAL and H.igdsp_host_filt_process(h, None, out.ctypes.data, 0) == EINVAL
    voice = capi.filt_plan_preset(fm.VOICE_BAND, 8000)
    assert H.igdsp_host_filt_plan(h, voice.ctypes.data) == 0               # a new plan: the histories are forgotten
    play(voice, np.zeros((), capi.FILT_STATE))
    H.igdsp_host_filt_reset(h)
    play(voice, np.zeros((), capi.FILT_STATE))
    H.igdsp_host_filt_free(h)
    assert H.igdsp_host_filt_process(None, x[0].ctypes.data, out.ctypes.data, 0) == EINVAL and H.igdsp_host_filt_rec(None, rec.ctypes.data) == EINVAL


def test_asan_ubsan_build_agrees(tmp_path):
    """the rule built with -fsanitize=address,undefined as a program of its own: extremal sections at full scale, garbage states and
    plans of any bytes run without a report (no product overflows, nothing is indexed by a field) and give the model's bytes"""
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if shutil.which("g++") is None or subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, timeout=300).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")            # decided on a trivial program: an error in the driver fails below
    exe = str(tmp_path / "filt_rule_driver_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "filt_rule_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)

    def ask(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        return r.stdout.splitlines()

    n, F_ = 24, 3
    x = rows(F_, n, 77)
    rng = np.random.default_rng(5)
    secs = [(32767, 32767, 1, 0, 0), (16384, 16383, 0, -32768, 0), (-32768, 0, 0, 0, 32767), (1, 1, 1, -32766, -32766), (32767, -32768, 1, 0, 0)]
    plans = np.array([fm.plan_of_sections([s, secs[(i + 1) % 5]]) for i, s in enumerate(secs)] +
                     [np.frombuffer(rng.integers(0, 256, 48, dtype=np.uint8).tobytes(), fm.PLAN)[0] for _ in range(6)] +
                     [fm.plan_of_sections(fm.preset_sections(p, 48000), 48000) for p in fm.PRESETS], fm.PLAN)
    chans = [(pi, st, x[(pi + k) % 3], (fm.RUN, fm.RESET, fm.BYPASS, 9)[(pi + k) % 4]) for pi in range(len(plans)) for k, st in enumerate(states(50 + pi))]
    check_against_model(ask, plans, chans)
    assert ask("D 3 8000 1000.0 8.0 0.0\nD 0 48000 5.0 10.0 0.0\nP 1 8000\nP 0 6800\n")[1::2] == ["-22 0", "-22"]
