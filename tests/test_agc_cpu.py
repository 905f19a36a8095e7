"""-m "not gpu": the level control's rule (csrc/igdsp_agc.h) against tests/agc_model.py, bit for bit: output, record, state.  The rule
runs as a program of its own (tests/route/agc_rule_driver.cpp, g++ alone, once more under -fsanitize=address,undefined) and through the
C ABI (igdsp_agc_frame); then what the rule is worth: the ceiling on every sample, the gain's slope, exact convergence within a frame
count the test derives from the slew shifts alone, one test per comparison of the rule, and the distance to the same rule in float64.
The rule is the library's own, UNVERIFIED against ITU-T G.169: what these tests show is what is promised."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import agc_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
NS = (8, 16, 24, 160, 256)
SEEDS = (0, 1, 2)
CFG_KEYS = ("target", "ceil", "gate", "gmin", "gmax", "att", "rel", "up", "down", "lrel")
# the largest gain deviation of the integer rule from the float64 rule on settled active frames, measured with the model over the
# scenes of fidelity_scenes() and SEEDS: 0.0297 dB (the tone at 8 000: the integer slew's rounding term has finished on 4 194 while the
# float64 one still creeps toward 4 194.3; noise 0.0215, the steps 0.0158); the bound is twice that, since other seeds will differ
FIDELITY_MEASURED_DB = 0.0297
FIDELITY_BOUND_DB = 2 * FIDELITY_MEASURED_DB


def state_of(tag=am.TAG, env=0, gain=am.UNITY, cap=am.CAP, flags=0):
    st = np.zeros((), am.STATE)
    st["tag"], st["env"], st["gain"], st["cap"], st["flags"] = tag, env, gain, cap, flags
    return st


class Driver:
    def __init__(self, d):
        self.dir = d
        self.exe = str(d / "agc_rule_driver")
        self.build(self.exe)
        self.inputs = []

    def build(self, exe, extra=()):
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        os.path.join(ROOT, "tests", "route", "agc_rule_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)

    @staticmethod
    def text(cases):
        lines = []
        for cfg, x, ctl, st in cases:
            x = np.asarray(x)
            st = np.zeros((), am.STATE) if st is None else st
            head = [x.shape[1], x.shape[0], ctl, int(st["tag"]), int(st["env"]), int(st["gain"]), int(st["cap"]), int(st["flags"]), int(st["reserved"])]
            lines.append(" ".join(map(str, head + [int(cfg[k]) for k in CFG_KEYS] + x.reshape(-1).tolist())))
        return "\n".join(lines) + "\n"

    @staticmethod
    def parse(cases, stdout):
        res = []
        lines = stdout.splitlines()
        assert len(lines) == len(cases)
        for (cfg, x, ctl, st), line in zip(cases, lines):
            F_, n = np.asarray(x).shape
            w = line.split()
            assert len(w) == F_ * (n + 2) + 2
            out, rec = np.zeros((F_, n), np.int16), np.zeros(F_, am.REC)
            for f in range(F_):
                o = f * (n + 2)
                rec[f:f + 1] = np.array([int(w[o], 16), int(w[o + 1], 16)], "<u8").view(am.REC)
                out[f] = [int(v) for v in w[o + 2:o + 2 + n]]
            res.append((out, rec, np.array([int(w[-2], 16), int(w[-1], 16)], "<u8").view(am.STATE)[0]))
        return res

    def run(self, cases, exe=None, keep=True):
        """cases: (cfg, x [F][n], ctl, state record or None) -> per case (out [F][n], rec [F], state)"""
        text = self.text(cases)
        if keep:
            self.inputs.append((cases, text))
        r = subprocess.run([exe or self.exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, (r.returncode, r.stderr[-2000:])
        return self.parse(cases, r.stdout)


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    return Driver(tmp_path_factory.mktemp("agc_rule"))


def model_one(cfg, x, ctl, st, **kw):
    x = np.asarray(x)
    return am.run(cfg, x[:, None, :], ctl=[ctl], state=None if st is None else np.array([st], am.STATE), **kw)


def same(got, model, what=""):
    (o, r, s), (mo, mr, _, ms) = got, model[:4]
    assert np.array_equal(o, mo[:, 0]), (what, np.argwhere(o != mo[:, 0])[:4].tolist())
    assert r.tobytes() == mr[:, 0].tobytes(), (what, [(k, r[k][r[k] != mr[k][:, 0]][:3], mr[k][:, 0][r[k] != mr[k][:, 0]][:3]) for k in mr.dtype.names
                                                      if not np.array_equal(r[k], mr[k][:, 0])])
    assert s.tobytes() == ms[0].tobytes(), (what, s, ms[0])


def check(drv, cases, what=""):
    """the driver's bytes are the model's; returns the models"""
    got = drv.run(cases)
    models = [model_one(*c, want_gains=True) for c in cases]
    for i, (g, m) in enumerate(zip(got, models)):
        same(g, m, (what, i))
    return models


# ---- the scenes of the issue, as (name, x [F][n], the state at the start); the step scenes start with the gain at its maximum, where the
# quiet tone holds it, and step in frame ONSET
ONSET = 4


def scenes():
    s = [(f"tone{a}", am.tone(a, 100, 160)[:, 0], None) for a in (300, 1000, 8000, 30000)]
    at_max = state_of(env=300, gain=32768)
    s += [("step_mid", am.step_scene(ONSET + 6, 160, ONSET * 160 + 77)[:, 0], at_max), ("step_first", am.step_scene(ONSET + 6, 160, ONSET * 160 + 3)[:, 0], at_max)]
    s += [(f"noise{seed}", am.noise(40, 1, 160, seed)[:, 0], None) for seed in SEEDS]
    s += [("zeros", np.zeros((4, 160), np.int64), None), ("min", np.full((4, 160), -32768, np.int64), None)]
    return s


def test_layouts_and_defaults():
    igbuild.build()
    for a, b in ((capi.AGC_CFG, am.CFG), (capi.AGC_STATE, am.STATE), (capi.AGC_REC, am.REC)):
        assert a.itemsize == b.itemsize == 16 and a.names == b.names and [a.fields[k] for k in a.names] == [b.fields[k] for k in b.names]
    assert capi.agc_cfg_default().tobytes() == am.cfg_default().tobytes()
    d = am.cfg_default()
    assert [int(d[k]) for k in CFG_KEYS] == [8192, 23170, 256, 1024, 32768, 1, 5, 5, 2, 6]
    assert (capi.AGC_RUN, capi.AGC_FREEZE, capi.AGC_BYPASS, capi.AGC_RESET) == (am.RUN, am.FREEZE, am.BYPASS, am.RESET) == (0, 1, 2, 3)
    assert (capi.AGC_ACTIVE, capi.AGC_LIMITED, capi.AGC_AT_MAX, capi.AGC_AT_MIN, capi.AGC_ATTACKED, capi.AGC_FROZEN, capi.AGC_BYPASSED) == (
        am.ACTIVE, am.LIMITED, am.AT_MAX, am.AT_MIN, am.ATTACKED, am.FROZEN, am.BYPASSED) == (1, 2, 4, 8, 16, 32, 64)
    assert (capi.AGC_TAG, capi.AGC_CAP, capi.AGC_UNITY, capi.AGC_BLOCK) == (am.TAG, am.CAP, am.UNITY, am.BLOCK)
    hdr = open(os.path.join(ROOT, "include", "igdsp.h")).read()
    assert f"#define IGDSP_AGC_TAG     0x{am.TAG:08X}u" in hdr and "UNVERIFIED against ITU-T G.169" in hdr
    assert "#define IGDSP_ABI_VERSION 3" in hdr


def test_yardstick_is_bound_like_the_entry():
    res, args = capi.INTERNAL_MORE["igdsp_internal_agc_move"]
    pub = {name: (r, a) for name, r, a in capi.PROTOTYPES}["igdsp_agc_run"]
    assert (res, list(args)) == (pub[0], list(pub[1])) and capi.INTERNAL_MORE_TWIN["igdsp_internal_agc_move"] == "igdsp_agc_run"
    assert "igdsp_internal_agc_move" not in capi.INTERNAL
    text = open(os.path.join(ROOT, "tools", "agc_bench.py")).read()
    assert 'capi.internal("igdsp_internal_agc_move")' in text and ".argtypes" not in text


def test_frame_rejects_through_the_abi():
    igbuild.build()
    L = capi.load()
    st, x = np.zeros((), capi.AGC_STATE), np.zeros(256, np.int16)
    p = lambda a: a.ctypes.data
    for n in (0, 4, 7, 12, 161, 264):
        assert L.igdsp_agc_frame(None, p(st), p(x), n, 0, None, None) == -22
    for bad in (dict(gate=0), dict(target=0), dict(target=23171), dict(ceil=32768, target=8192), dict(gmin=0), dict(gmin=4097), dict(gmax=4095),
                dict(att=16), dict(rel=16), dict(up=16), dict(down=16), dict(lrel=0), dict(lrel=16)):
        c = am.cfg_default(**bad)
        assert not am.cfg_valid(c) and L.igdsp_agc_frame(p(c), p(st), p(x), 160, 0, None, None) == -22, bad
    for good in (dict(gate=1, target=1, ceil=1), dict(target=32767, ceil=32767), dict(gmin=4096, gmax=4096), dict(gmin=1, gmax=65535),
                 dict(att=15, rel=15, up=15, down=15, lrel=15), dict(att=0, rel=0, up=0, down=0, lrel=1)):
        c = am.cfg_default(**good)
        assert am.cfg_valid(c) and L.igdsp_agc_frame(p(c), p(st), p(x), 160, 0, None, None) == 0, good
    assert L.igdsp_agc_frame(None, None, p(x), 160, 0, None, None) == -22 and L.igdsp_agc_frame(None, p(st), None, 160, 0, None, None) == -22
    st = np.zeros((), capi.AGC_STATE)
    assert L.igdsp_agc_frame(None, p(st), p(x), 160, 0, None, None) == 0   # out and rec optional, cfg NULL: the defaults
    assert st.tobytes() == state_of().tobytes()


def test_scenes_match_the_model_and_stay_under_the_ceiling(drv):
    """every scene of the issue under the defaults: the model's bytes; ATTACKED at the onset exactly when the step
    falls into a frame's first block; the model asserts |x t| <= ceil << 12 on every sample, the test |out| <= ceil"""
    cfg = am.cfg_default()
    sc = scenes()
    models = check(drv, [(cfg, x, am.RUN, st) for _, x, st in sc], "scenes")
    by = {name: m for (name, _, _), m in zip(sc, models)}
    for name, m in by.items():
        assert np.abs(m[0].astype(np.int64)).max() <= int(cfg["ceil"]), name
    mid, first = by["step_mid"][1]["flags"][:, 0], by["step_first"][1]["flags"][:, 0]
    assert by["step_mid"][1]["gain"][ONSET - 1, 0] == by["step_first"][1]["gain"][ONSET - 1, 0] == 32768          # the gain at its maximum
    assert not (mid[:ONSET + 1] & am.ATTACKED).any() and (mid[ONSET] & am.LIMITED)
    assert not (first[:ONSET] & am.ATTACKED).any() and (first[ONSET] & am.ATTACKED) and (first[ONSET] & am.LIMITED)
    for name in ("step_mid", "step_first") + tuple(f"noise{s}" for s in SEEDS):
        pk = int(by[name][1]["out_peak"].max())
        print(f"{name}: output peak {pk} under the ceiling {int(cfg['ceil'])}")
        assert 23000 <= pk <= 23170, (name, pk)
    assert np.all(by["zeros"][0] == 0) and by["zeros"][3]["gain"][0] == am.UNITY and not by["zeros"][1]["flags"].any()
    assert np.all(by["min"][1]["in_peak"] == 32768) and by["min"][3]["env"][0] == 32768
    # r = (23170 << 12) / 32768 = 2896 in every block; the gain falls 4096 -> 3328 -> 2752 -> 2320: limited while it is above 2896, and
    # the first frame's first block is an onset
    assert by["min"][1]["gain"][:3, 0].tolist() == [3328, 2752, 2320] and by["min"][1]["flags"][:, 0].tolist() == [19, 3, 1, 1]


@pytest.mark.parametrize("n", NS)
def test_every_frame_length_ctl_and_state(drv, n):
    """mixed rows at every frame length, launches whose ctl changes from one to the next on a carried state, from a fresh state, garbage
    under the tag and a wrong tag"""
    F_ = 6
    cfg = am.cfg_default()
    x = am.mixed_scene(5 * F_, 6, n, seed=n)
    cases, seen = [], 0
    for c in range(6):
        starts = (None, am.garbage_state(1, 10 * n + c)[0], am.garbage_state(1, 20 * n + c, tagged=False)[0])
        for st in starts:
            for k, ctl in enumerate((am.RUN, am.FREEZE, am.BYPASS, am.RESET, 200)):
                xs = x[k * F_:(k + 1) * F_, c]
                cases.append((cfg, xs, ctl, st))
                m = model_one(cfg, xs, ctl, st)
                st = m[3][0]
                seen |= int(np.bitwise_or.reduce(m[1]["flags"].reshape(-1)))
    check(drv, cases, n)
    assert seen == 127 or n == 8, seen                                     # every flag of the record came up


def test_ctl_semantics(drv):
    cfg = am.cfg_default()
    x = am.tone(3000, 4, 160)[:, 0]
    st = state_of(env=5000, gain=9000, cap=7000, flags=3)
    st["reserved"] = 0xDEADBEEF                                            # a bypass must leave it
    run, frz, byp, rst, big = (g for g in drv.run([(cfg, x, k, st) for k in (am.RUN, am.FREEZE, am.BYPASS, am.RESET, 77)]))
    for g, k in ((run, am.RUN), (frz, am.FREEZE), (byp, am.BYPASS), (rst, am.RESET), (big, 77)):
        same(g, model_one(cfg, x, k, st), k)
    assert np.array_equal(byp[0], x) and byp[2].tobytes() == st.tobytes() and np.all(byp[1]["flags"] == am.BYPASSED)
    assert np.all(byp[1]["gain"] == 9000) and np.all(byp[1]["tmin"] == 4096) and np.array_equal(byp[1]["in_peak"], byp[1]["out_peak"])
    assert np.all(frz[1]["gain"] == 9000) and np.all(frz[1]["env"] == 5000) and np.all(frz[1]["flags"] & am.FROZEN) and frz[2]["cap"] != 7000
    assert big[2].tobytes() == run[2].tobytes() and np.array_equal(big[0], run[0])
    fresh = drv.run([(cfg, x, am.RUN, None)])[0]
    assert np.array_equal(rst[0], fresh[0]) and rst[1].tobytes() == fresh[1].tobytes() and rst[2].tobytes() == fresh[2].tobytes()
    # gain is read clamped; env and cap stand as they are
    lo, hi = drv.run([(cfg, x[:1], am.FREEZE, state_of(gain=5)), (cfg, x[:1], am.FREEZE, state_of(gain=65535))])
    assert lo[1]["gain"][0] == 1024 and hi[1]["gain"][0] == 32768


def test_random_frames_stay_under_the_ceiling_through_the_abi():
    """2 000 random frames, each from a random valid state with gain = gmax, through igdsp_agc_frame: the model's bytes, |out| <= ceil"""
    igbuild.build()
    N, n = 2000, 160
    rng = np.random.default_rng(11)
    for cfg in (am.cfg_default(), am.cfg_default(ceil=32767, target=32767, gmax=65535, lrel=1)):
        x = am.mixed_scene(1, N, n, seed=5)
        x[0, ::3] = rng.integers(-32768, 32768, x[0, ::3].shape)
        st = am.garbage_state(N, 12)
        st["gain"] = cfg["gmax"]
        out, rec, _, ms = am.run(cfg, x, state=st)
        got_o, got_r, got_s = np.zeros((N, n), np.int16), np.zeros(N, capi.AGC_REC), st.view(capi.AGC_STATE).copy()
        for c in range(N):
            got_o[c], got_r[c] = capi.agc_frame(cfg.view(capi.AGC_CFG), got_s[c:c + 1].reshape(()), x[0, c])
        assert np.array_equal(got_o, out[0]) and got_r.tobytes() == rec[0].tobytes() and got_s.tobytes() == ms.tobytes()
        assert np.abs(got_o.astype(np.int64)).max() <= int(cfg["ceil"])
        assert (rec["flags"] & am.LIMITED).any() and (rec["flags"] & am.ATTACKED).any()


def test_gain_slope():
    """within a block the gain moves by no more than an eighth of the knots' difference, and one for the rounding, per sample"""
    cfg = am.cfg_default()
    for x in (am.mixed_scene(12, 12, 160, seed=3), am.step_scene(ONSET + 2, 160, ONSET * 160 + 77), am.noise(10, 2, 256, 1)):
        *_, t, T = am.run(cfg, x, want_gains=True)
        F_, C_, n = t.shape
        tb = t.reshape(F_, C_, n // 8, 8)
        bound = np.abs(np.diff(T, axis=2)) // 8 + 1
        assert np.all(np.abs(np.diff(tb, axis=3)) <= bound[..., None])
        assert np.all(tb[..., 0] == T[..., :-1])                           # a block starts at its left knot
        lo, hi = np.minimum(T[..., :-1], T[..., 1:]), np.maximum(T[..., :-1], T[..., 1:])
        assert np.all((tb >= lo[..., None]) & (tb <= hi[..., None]))         # and never leaves the two knots


def slew_frames(G, Gt, up, down):
    """frames the slew needs from G to Gt: the recurrence on integers, nothing of the library"""
    k = 0
    while G != Gt:
        G += ((Gt - G + (1 << up) - 1) >> up) if Gt >= G else -((G - Gt + (1 << down) - 1) >> down)
        k += 1
    return k


@pytest.mark.parametrize("amp", (300, 1000, 8000, 30000))
def test_convergence(drv, amp):
    """a steady tone from the RESET state: after the frames the slew recurrence takes, the gain is clamp((target << 12) / pk) exactly and
    stays; frames under the gate then leave gain and env as they are"""
    for kw in (dict(), dict(up=3, down=4), dict(up=0, down=0)):
        cfg = am.cfg_default(**kw)
        Gt = min(max((int(cfg["target"]) << 12) // amp, int(cfg["gmin"])), int(cfg["gmax"]))
        K = slew_frames(am.UNITY, Gt, int(cfg["up"]), int(cfg["down"]))
        loud, quiet = am.tone(amp, K + 3, 160)[:, 0], am.tone(200, 5, 160)[:, 0]
        assert np.all(np.abs(loud).max(axis=1) == amp)
        (out, rec, st), = drv.run([(cfg, loud, am.RUN, None)])
        same((out, rec, st), model_one(cfg, loud, am.RUN, None))
        assert np.all(rec["gain"][max(K - 1, 0):] == Gt) and (K < 2 or rec["gain"][K - 2] != Gt), (amp, kw, K, rec["gain"][-5:])
        assert np.all(rec["env"] == amp) and st["gain"] == Gt
        (_, rq, sq), = drv.run([(cfg, quiet, am.RUN, st)])
        assert np.all(rq["gain"] == Gt) and np.all(rq["env"] == amp) and not (rq["flags"] & am.ACTIVE).any() and sq["gain"] == Gt and sq["env"] == amp
    print(f"amplitude {amp}: gain {Gt} after {slew_frames(am.UNITY, Gt, 5, 2)} frames at the defaults")


# ---- one test per comparison of the rule: the expected numbers are worked out here by hand
def one(drv, cfg, x, st, ctl=am.RUN):
    case = (cfg, np.asarray(x, np.int64).reshape(1, -1), ctl, st)
    (out, rec, s), = drv.run([case])
    same((out, rec, s), model_one(*case))
    return out[0], rec[0], s


def test_edge_gate(drv):
    cfg = am.cfg_default()
    _, r, s = one(drv, cfg, [256] + [0] * 7, None)
    assert r["flags"] & am.ACTIVE and s["env"] == 256 and r["gain"] == 4096 + ((32768 - 4096 + 31) >> 5)        # pk == gate is active
    _, r, s = one(drv, cfg, [255] + [0] * 7, None)
    assert not r["flags"] & am.ACTIVE and s["env"] == 0 and r["gain"] == 4096


def test_edge_envelope(drv):
    cfg = am.cfg_default(att=2, rel=3)
    x = [1000] + [0] * 7
    assert one(drv, cfg, x, state_of(env=1000))[2]["env"] == 1000                   # pk == env: stays
    assert one(drv, cfg, x, state_of(env=999))[2]["env"] == 1000                    # rises by (1 + 3) >> 2: the rounding term
    assert one(drv, cfg, x, state_of(env=995))[2]["env"] == 997                     # (5 + 3) >> 2
    assert one(drv, cfg, x, state_of(env=1007))[2]["env"] == 1007                   # falls by 7 >> 3 = 0
    assert one(drv, cfg, x, state_of(env=1008))[2]["env"] == 1007                   # 8 >> 3
    assert one(drv, cfg, x, state_of(env=0))[2]["env"] == 1000                      # env 0 takes pk
    assert one(drv, cfg, x, state_of(env=65535))[2]["env"] == 65535 - (64535 >> 3)


def test_edge_slew(drv):
    cfg = am.cfg_default(up=3, down=2)
    x = [8192] + [0] * 7                                                            # env = pk = target: Gt = 4096
    for G, want in ((4096, 4096), (4095, 4096), (4088, 4089), (4087, 4089), (4097, 4096), (4100, 4099), (4101, 4099)):
        _, r, s = one(drv, cfg, x, state_of(env=8192, gain=G))
        assert r["gain"] == s["gain"] == want, (G, want, r["gain"])
    # Gt clamped: the flags say so, equality is not a clamp
    for tgt_env, flag in ((1023, am.AT_MAX), (1024, 0), (32767, 0)):
        _, r, _ = one(drv, am.cfg_default(target=8192, gmax=32768), [tgt_env] + [0] * 7, state_of(env=tgt_env))
        assert (r["flags"] & (am.AT_MAX | am.AT_MIN)) == flag, (tgt_env, r["flags"])
    _, r, _ = one(drv, am.cfg_default(gmin=4096), [8193] + [0] * 7, state_of(env=8193))   # 4095 < gmin
    assert r["flags"] & am.AT_MIN
    _, r, _ = one(drv, am.cfg_default(gmin=4096), [8192] + [0] * 7, state_of(env=8192))   # 4096 == gmin
    assert not r["flags"] & am.AT_MIN


def test_edge_ratio_and_zero_block(drv):
    cfg = am.cfg_default()
    # block 0 silent (r = CAP), block 1 at 30 000 (r = (23170 << 12) / 30000 = 3163): frozen at unity, the ramp runs through block 0
    x = [0] * 8 + [30000] * 8
    out, r, s = one(drv, cfg, x, state_of(), am.FREEZE)
    assert (23170 << 12) // 30000 == 3163 and s["cap"] == 3163 and r["tmin"] == 3163 and r["n_limited"] == 2 and r["flags"] == am.ACTIVE | am.FROZEN | am.LIMITED
    assert np.all(out[:8] == 0) and np.all(out[8:] == (30000 * 3163 + 2048) >> 12)
    # the same ramp seen through a constant: t_i = 4096 + (-933 i) / 8 toward zero
    out, _, _ = one(drv, cfg, [4096] * 8 + [30000] * 8, state_of(), am.FREEZE)
    assert out[:8].tolist() == [4096 - (933 * i) // 8 for i in range(8)] and out[1] == 4096 - 116
    # p == ceil << 12 / CAP: the quotient at and above the cap
    for p, want in ((1448, 65535), (1449, 65496), (1, 65535)):
        _, _, s = one(drv, cfg, [p] * 8, state_of(), am.FREEZE)
        assert s["cap"] == want == min(65535, (23170 << 12) // p), (p, s["cap"])


def test_edge_attacked(drv):
    cfg = am.cfg_default()
    x = [30000] * 8                                                                 # m_0 = 3163
    _, r, s = one(drv, cfg, x, state_of(cap=3163), am.FREEZE)
    assert not r["flags"] & am.ATTACKED and s["cap"] == 3163                        # m_0 == cap
    _, r, s = one(drv, cfg, x, state_of(cap=3164), am.FREEZE)
    assert r["flags"] & am.ATTACKED and r["tmin"] == 3163
    _, r, s = one(drv, cfg, x, state_of(cap=3162), am.FREEZE)
    assert not r["flags"] & am.ATTACKED and r["tmin"] == 3162 and s["cap"] == 3163  # the cap below m_0 holds at knot 0 and releases by 49 to m_1


def test_edge_release(drv):
    cfg = am.cfg_default()
    x = [4096] * 24                                                                 # r = 23170 in every block
    out, r, s = one(drv, cfg, x, state_of(cap=3), am.FREEZE)
    assert s["cap"] == 6 and r["tmin"] == 3 and r["n_limited"] == 4                 # 3 >> 6 = 0: the step is 1
    assert out[::8].tolist() == [3, 4, 5]
    _, _, s = one(drv, cfg, x, state_of(cap=127), am.FREEZE)
    assert s["cap"] == 132                                                          # 127 + 1, 128 + 2, 130 + 2: the shift takes over at 64
    _, _, s = one(drv, cfg, [0] * 16, state_of(cap=64000), am.FREEZE)
    assert s["cap"] == 65535 and 64000 + 1000 + (65000 >> 6) > 65535                # c reaches CAP and stays
    _, _, s = one(drv, cfg, [0] * 16, state_of(cap=63000), am.FREEZE)
    assert s["cap"] == 63000 + 984 + ((63000 + 984) >> 6) == 64983
    _, r, s = one(drv, cfg, [0] * 8, state_of(cap=0), am.FREEZE)
    assert s["cap"] == 1 and r["tmin"] == 0


def test_edge_knots_and_rounding(drv):
    """A_k = G + ((Gn - G) k) / B toward zero with a falling gain; out rounds to nearest with an arithmetic shift"""
    cfg = am.cfg_default(down=0, up=0)
    # env = pk = 16384: Gt = 2048; G 4099 falls to 2048 in one frame: A_k = 4099 + (-2051 k) / 3
    x = [16384] * 24
    out, r, _ = one(drv, cfg, x, state_of(env=16384, gain=4099))
    A = [4099 - (2051 * k) // 3 for k in range(4)]
    assert A == [4099, 3416, 2732, 2048] and r["gain"] == 2048 and r["tmin"] == 2048 and r["n_limited"] == 0
    assert out[::8].tolist() == [(16384 * a + 2048) >> 12 for a in A[:3]]
    # rounding: x t = -2048 gives 0, -2049 gives -1, 2047 gives 0, 2048 gives 1
    cfg = am.cfg_default(gate=32767)
    out, _, _ = one(drv, cfg, [-2048, -2049, 2047, 2048, 1, -1, 0, 6143], state_of(gain=4096), am.RUN)
    assert out.tolist() == [-2048, -2049, 2047, 2048, 1, -1, 0, 6143]
    out, _, _ = one(drv, cfg, [-2048, -2049, 2047, 2048, 3, -3, 0, 6143], state_of(gain=1), am.RUN)
    assert am.cfg_valid(am.cfg_default(gmin=1)) and one(drv, am.cfg_default(gmin=1, gate=32767), [-2048, -2049, 2047, 2048, 3, -3, 0, 6144],
                                                        state_of(gain=1))[0].tolist() == [0, -1, 0, 1, 0, 0, 0, 2]


def test_sanitizers(drv):
    """the stand-alone driver (its own main, nothing of it loaded into Python) built with -fsanitize=address,undefined: every input the
    tests above gave the plain driver, the same output, no report"""
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = drv.dir / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(drv.dir / "probe")], capture_output=True, timeout=300).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")            # decided on a trivial program: an error in the driver fails below
    exe = str(drv.dir / "agc_rule_driver_san")
    drv.build(exe, san)
    assert len(drv.inputs) >= 10
    for cases, text in drv.inputs:
        plain = subprocess.run([drv.exe], input=text, capture_output=True, text=True, timeout=600)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, r.stderr[-2000:]
        assert r.stdout == plain.stdout


# ---- fidelity: the integer rule against the same rule in float64
def fidelity_scenes():
    """(name, x [F][1][n], the first settled frame)"""
    s = []
    for a in (300, 1000, 8000, 30000):
        Gt = min(max((8192 << 12) // a, 1024), 32768)
        K = slew_frames(am.UNITY, Gt, 5, 2)
        s.append((f"tone{a}", am.tone(a, K + 20, 160), K))
    on = 240                                                                # the quiet tone has the gain at gmax after 233 frames
    s += [("step_mid", am.step_scene(on + 40, 160, on * 160 + 77), on + 27), ("step_first", am.step_scene(on + 40, 160, on * 160 + 3), on + 27)]
    s += [(f"noise{seed}", am.noise(40, 1, 160, seed), 25) for seed in SEEDS]
    return s


def test_fidelity_against_float64():
    cfg = am.cfg_default()
    worst = 0.0
    for name, x, settled in fidelity_scenes():
        _, rec, _, _ = am.run(cfg, x)
        _, gf, act = am.run_f64(cfg, x)
        gi = rec["gain"][settled:, 0].astype(np.float64) / 4096.0
        sel = act[settled:, 0] & ((rec["flags"][settled:, 0] & am.ACTIVE) != 0)
        assert sel.any(), name
        dev = float(np.abs(20.0 * np.log10(gi[sel] / gf[settled:, 0][sel])).max())
        print(f"{name}: largest settled gain deviation {dev:.4f} dB")
        worst = max(worst, dev)
    print(f"fidelity: {worst:.4f} dB measured, bound {FIDELITY_BOUND_DB:.4f} dB")
    assert worst <= FIDELITY_BOUND_DB


def test_host_mirror_level_control():
    """LevelControl (host/igdsp_host.h) through its C shims: the frames of a scene give igdsp_agc_frame's bytes, the record and the gain
    of the last frame are readable, reset forgets the state, bad frame lengths give no handle"""
    import ctypes

    igbuild.build()
    H = ctypes.CDLL(igbuild.HOST_LIB)
    vp, u, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    for name, res, args in (("igdsp_host_agc_new", vp, [u]), ("igdsp_host_agc_free", None, [vp]), ("igdsp_host_agc_process", i, [vp, vp, vp, u]),
                            ("igdsp_host_agc_rec", i, [vp, vp]), ("igdsp_host_agc_gain_db", ctypes.c_float, [vp]), ("igdsp_host_agc_reset", None, [vp])):
        fn = getattr(H, name)
        fn.restype, fn.argtypes = res, args
    n = 160
    x = am.step_scene(30, n, 20 * n + 5, lo=1000)
    want = am.run(am.cfg_default(), x)
    e = H.igdsp_host_agc_new(n)
    assert e
    try:
        out, rec = np.zeros(n, np.int16), np.zeros((), capi.AGC_REC)
        for f in range(len(x)):
            a = np.ascontiguousarray(x[f, 0], np.int16)
            assert H.igdsp_host_agc_process(e, a.ctypes.data, out.ctypes.data, am.RUN) == 0
            assert np.array_equal(out, want[0][f, 0]) and H.igdsp_host_agc_rec(e, rec.ctypes.data) == 0 and rec.tobytes() == want[1][f, 0].tobytes()
        assert abs(H.igdsp_host_agc_gain_db(e) - 20.0 * np.log10(float(rec["gain"]) / 4096.0)) < 1e-3 and rec["gain"] != 4096
        H.igdsp_host_agc_reset(e)
        assert H.igdsp_host_agc_process(e, a.ctypes.data, out.ctypes.data, am.BYPASS) == 0 and np.array_equal(out, a)
        assert H.igdsp_host_agc_rec(e, rec.ctypes.data) == 0 and rec["gain"] == 4096 and rec["flags"] == am.BYPASSED
        assert H.igdsp_host_agc_process(e, None, out.ctypes.data, 0) == -22 and H.igdsp_host_agc_process(None, a.ctypes.data, out.ctypes.data, 0) == -22
    finally:
        H.igdsp_host_agc_free(e)
    for bad in (0, 4, 12, 161, 264):
        assert not H.igdsp_host_agc_new(bad)
