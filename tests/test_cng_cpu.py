"""-m "not gpu": the comfort-noise generator's rule (csrc/igdsp_cng.h) against tests/cng_model.py, bit for bit: row, length, record,
state.  The rule runs as a program of its own (tests/route/cng_rule_driver.cpp, g++ alone, once more under -fsanitize=address,undefined)
and through the C ABI (igdsp_cng_frame); then what the rule is worth, on the model: the table and its hash, the gain of a payload,
seeds, the white-noise level, the loop through the voice detector's model (level and spectral shape), the gain's slew.
The rule is the library's own, UNVERIFIED against RFC 3389 and G.711 Appendix II: what these tests show is what is promised."""
import hashlib
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import cng_model as cm
from tests import vad_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
NS = tuple(range(16, 257, 8))
G_SHA256 = "71670a5818e2454cc9206a6065832b91b7c83deeedd06dc403b6eebeb1993752"
PAYLOADS = [[n] * 10 for n in (0, 1, 127, 254, 255)] + [[90, 150, 120], [40], [], [0, 254, 0, 254, 0, 254, 0, 254, 0, 254], [126, 128] * 5]


class Case:
    """one channel's frames: kind [F], sid [F][16], sid_len [F], voice [F][n] or None, ctl, seed, state record or None"""

    def __init__(self, n, kind, sid, sid_len, voice=None, ctl=cm.RUN, seed=0, state=None):
        self.n, self.kind, self.sid, self.sid_len = n, np.asarray(kind), np.asarray(sid, np.uint8), np.asarray(sid_len)
        self.voice, self.ctl, self.seed, self.state = voice, ctl, seed, np.zeros((), cm.STATE) if state is None else state

    def text(self):
        w = [self.n, len(self.kind), self.ctl, self.seed] + [format(int(v), "x") for v in np.frombuffer(self.state.tobytes(), "<u8")]
        for f in range(len(self.kind)):
            w += [int(self.kind[f]), int(self.sid_len[f]), 0 if self.voice is None else 1] + self.sid[f].tolist()
            if self.voice is not None:
                w += np.asarray(self.voice[f]).tolist()
        return " ".join(map(str, w))


def models(cases):
    """the model's (out [F][n], len [F], rec [F], state) per case; cases of one shape go through run() side by side"""
    res = [None] * len(cases)
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault((c.n, len(c.kind), c.voice is None), []).append(i)
    for (n, F_, novoice), ids in groups.items():
        cs = [cases[i] for i in ids]
        out, ln, rec, _, st = cm.run(np.stack([c.kind for c in cs], 1), np.stack([c.sid for c in cs], 1), n, np.stack([c.sid_len for c in cs], 1),
                                     None if novoice else np.stack([c.voice for c in cs], 1), [c.ctl for c in cs], [c.seed for c in cs],
                                     np.array([c.state for c in cs], cm.STATE))
        for j, i in enumerate(ids):
            res[i] = (out[:, j], ln[:, j], rec[:, j], st[j])
    return res


class Driver:
    def __init__(self, d):
        self.exe = str(d / "cng_rule_driver")
        self.build(self.exe)
        self.inputs = []

    def build(self, exe, extra=()):
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        os.path.join(ROOT, "tests", "route", "cng_rule_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)

    def lines(self, text, exe=None):
        r = subprocess.run([exe or self.exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, (r.returncode, r.stderr[-2000:])
        return r.stdout.splitlines()

    def run(self, cases, exe=None, keep=True):
        text = "\n".join(c.text() for c in cases) + "\n"
        if keep:
            self.inputs.append((cases, text))
        lines = self.lines(text, exe)
        assert len(lines) == len(cases)
        res = []
        for c, line in zip(cases, lines):
            w, F_, n = line.split(), len(c.kind), c.n
            assert len(w) == F_ * (3 + n) + 12
            fr = [w[f * (3 + n):(f + 1) * (3 + n)] for f in range(F_)]
            ln = np.array([int(q[0]) for q in fr], np.uint16)
            rec = np.array([[int(q[1], 16), int(q[2], 16)] for q in fr], "<u8").reshape(F_, 2).view(cm.REC).reshape(F_)
            out = np.array([[int(v) for v in q[3:]] for q in fr], np.int16).reshape(F_, n)
            res.append((out, ln, rec, np.array([int(v, 16) for v in w[F_ * (3 + n):]], "<u8").view(cm.STATE)[0]))
        return res


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    return Driver(tmp_path_factory.mktemp("cng_rule"))


def same(got, model, what=""):
    (o, ln, r, st), (mo, mln, mr, mst) = got, model
    assert np.array_equal(ln, mln), (what, ln, mln)
    assert r.tobytes() == mr.tobytes(), (what, [(k, r[k], mr[k]) for k in mr.dtype.names if not np.array_equal(r[k], mr[k])])
    assert np.array_equal(o, mo), (what, np.argwhere(o != mo)[:4])
    assert st.tobytes() == mst.tobytes(), (what, st, mst)


def check(drv, cases, what=""):
    got, ms = drv.run(cases), models(cases)
    for i, (g, m) in enumerate(zip(got, ms)):
        same(g, m, (what, i))
    return ms


def scene(F_, n, seed, voice=True):
    """kinds that drive every branch, payloads of every length, a voice row"""
    rng = np.random.default_rng(seed)
    kind = rng.choice([cm.NONE, cm.NONE, cm.SID, cm.VOICE, cm.VOICE, 7], F_)
    kind[0] = (cm.NONE, cm.SID, cm.VOICE)[seed % 3]
    sid = rng.integers(0, 256, (F_, 16)).astype(np.uint8)
    sid[:, 0] = rng.integers(0, 60, F_)
    sid[:, 1:] = np.clip(127 + rng.normal(0, 50, (F_, 15)), 0, 255).astype(np.uint8)
    sid_len = rng.integers(0, 17, F_)
    v = rng.integers(-32768, 32768, (F_, n)).astype(np.int16) if voice else None
    return kind, sid, sid_len, v


def three_states(seed):
    return [None, cm.garbage_state(1, seed)[0], cm.garbage_state(1, seed, tagged=False)[0]]


def all_cases():
    cases = []
    for n in NS:                                                           # every frame length, every ctl, the three states
        for i, ctl in enumerate((cm.RUN, cm.FREEZE, cm.BYPASS, cm.RESET, 200)):
            for j, st in enumerate(three_states(n + i)):
                if n in (16, 24, 160, 256) or (i + j + n // 8) % 5 == 0:
                    cases.append(Case(n, *scene(6, n, n + 7 * i + j, voice=(i + j) % 2 == 0), ctl=ctl, seed=0x1234 * n + i, state=st))
    rng = np.random.default_rng(3)                                         # every kind value, every payload length
    kind = rng.permutation(256)
    sid_len = np.arange(256) % 17
    _, sid, _, v = scene(256, 16, 5)
    for ctl in (cm.RUN, cm.FREEZE, cm.BYPASS):
        cases.append(Case(16, kind, sid, sid_len, v, ctl=ctl, seed=77))
    cases.append(Case(16, np.full(256, cm.SID), sid, sid_len, None, seed=78))
    return cases


def test_layouts_and_constants():
    igbuild.build()
    for a, b, size in ((capi.CNG_STATE, cm.STATE, 96), (capi.CNG_REC, cm.REC, 16)):
        assert a.itemsize == b.itemsize == size and a.names == b.names and [a.fields[k][1] for k in a.names] == [b.fields[k][1] for k in b.names]
    assert (capi.CNG_RUN, capi.CNG_FREEZE, capi.CNG_BYPASS, capi.CNG_RESET) == (cm.RUN, cm.FREEZE, cm.BYPASS, cm.RESET) == (0, 1, 2, 3)
    assert (capi.CNG_F_GENERATED, capi.CNG_F_SID, capi.CNG_F_NO_MODEL, capi.CNG_F_VOICE, capi.CNG_F_CLIPPED, capi.CNG_F_SID_EMPTY, capi.CNG_F_FROZEN,
            capi.CNG_F_BYPASSED) == (cm.F_GENERATED, cm.F_SID, cm.F_NO_MODEL, cm.F_VOICE, cm.F_CLIPPED, cm.F_SID_EMPTY, cm.F_FROZEN, cm.F_BYPASSED) == (
        1, 2, 4, 8, 16, 32, 64, 128)
    assert capi.CNG_TAG == cm.TAG and capi.CNG_GMAX == cm.GMAX == 3632640 and (cm.NONE, cm.VOICE, cm.SID) == (capi.VAD_NONE, capi.VAD_VOICE, capi.VAD_SID)
    hdr = open(os.path.join(ROOT, "include", "igdsp.h")).read()
    assert f"#define IGDSP_CNG_TAG     0x{cm.TAG:08X}u" in hdr and "#define IGDSP_ABI_VERSION 3" in hdr
    assert hdr.count("UNVERIFIED against RFC 3389 and G.711 Appendix II") >= 2
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "igdsp_cng_run" in text and text.count("UNVERIFIED against RFC 3389 and G.711 Appendix II") >= 2, doc


def test_yardstick_is_bound_as_its_entry():
    """igdsp_internal_cng_move takes igdsp_cng_run's arguments: capi.INTERNAL_MORE is that list and capi.internal finds it"""
    res, args = capi.INTERNAL_MORE["igdsp_internal_cng_move"]
    pub = {name: (r, a) for name, r, a in capi.PROTOTYPES}["igdsp_cng_run"]
    assert (res, list(args)) == (pub[0], list(pub[1])) and capi.INTERNAL_MORE_TWIN["igdsp_internal_cng_move"] == "igdsp_cng_run"
    assert "igdsp_internal_cng_move" not in capi.INTERNAL


def test_table_and_hash():
    """G[d] = isqrt(T8[d]), recomputed from the voice detector's table; its SHA-256 as little-endian uint32 is pinned"""
    igbuild.build()
    t8 = [int(v) for v in capi.vad_table()]
    g = [math.isqrt(t) for t in t8]
    assert g == cm.G == capi.cng_table().tolist()
    assert g[0] == 131072 and g[105] == 1 and all(v == 0 for v in g[106:]) and all(a >= b for a, b in zip(g, g[1:]))
    assert hashlib.sha256(np.array(g, "<u4").tobytes()).hexdigest() == G_SHA256
    tab = open(os.path.join(CSRC, "igdsp_cng_tab.h")).read()
    vals = [int(v.rstrip("u")) for v in tab.split("IGDSP_CNG_G_VALUES")[1].replace("\\", " ").replace(",", " ").split()]
    assert vals == g


def test_gain_of_a_payload(drv):
    """step 2 for all 128 levels x the payloads, through the rule's program and igdsp_cng_gain; g_tgt never passes 3 632 640"""
    igbuild.build()
    cases = [[lvl] + p for lvl in range(128) for p in PAYLOADS] + [[200] + PAYLOADS[2], [255], [0] + [127] * 15]
    got = drv.lines("".join(f"G {len(c)} {' '.join(map(str, c))}\n" for c in cases))
    for c, line in zip(cases, got):
        want = cm.gain(c, min(len(c), 11))[0]
        assert int(line) == want == capi.cng_gain(c) and want <= cm.GMAX, c
    assert cm.gain([0], 1)[0] == cm.GMAX and cm.gain([0] + [127] * 10, 11)[0] == cm.GMAX and cm.gain([106], 1)[0] == 0
    for bad in ([], [0] * 17):
        with pytest.raises(capi.IgdspError):
            capi.cng_gain(bad)


def test_sid_decode_and_step_2_agree():
    """every payload byte value: igdsp_sid_decode's k is the k step 2 halves and folds into the gain"""
    import ctypes

    igbuild.build()
    L = capi.load()
    st = np.zeros((), capi.CNG_STATE)
    for N in range(256):
        pay = np.array([30, N, 255 - N], np.uint8)
        lvl, k = ctypes.c_uint8(0), np.zeros(10, np.int16)
        assert L.igdsp_sid_decode(pay.ctypes.data, 3, ctypes.byref(lvl), k.ctypes.data) == 0
        assert (lvl.value, k.tolist()) == cm.sid_decode(pay, 3)
        g_tgt, kq, level, order = cm.gain(pay, 3)
        assert kq == [int(v / 2) for v in k.tolist()] and max(map(abs, kq)) <= cm.KQMAX
        st["tag"] = 0
        _, ln, rec = capi.cng_frame(st, cm.SID, 16, sid=pay, sid_len=3)
        assert ln == 16 and st["kq"].tolist() == kq and (int(st["g_tgt"]), int(st["level"]), int(st["order"])) == (g_tgt, level, order) == (
            int(rec["g_tgt"]), int(rec["level"]), int(rec["order"]))


def test_rule_matches_model(drv):
    """every frame length, ctl, kind value 0..255, payload length 0..16, from fresh, garbage-under-tag and wrong-tag states"""
    ms = check(drv, all_cases())
    seen = 0
    for m in ms:
        seen |= int(np.bitwise_or.reduce(m[2]["flags"]))
    assert seen == 0xFF, hex(seen)


def test_split_over_calls(drv):
    """F frames in one case equal the same frames in several, the state carried"""
    for n, ctl in ((24, cm.RUN), (160, cm.RESET), (160, cm.FREEZE)):
        k, s, sl, v = scene(9, n, n)
        st0 = cm.garbage_state(1, n)[0]
        whole = check(drv, [Case(n, k, s, sl, v, ctl=ctl, seed=9, state=st0)])[0]
        for cuts in ((4, 9), (1, 2, 9)):
            st, a, parts = st0, 0, []
            for b_ in cuts:
                c = ctl if a == 0 or ctl != cm.RESET else cm.RUN
                parts.append(check(drv, [Case(n, k[a:b_], s[a:b_], sl[a:b_], v[a:b_], ctl=c, seed=9, state=st)])[0])
                st, a = parts[-1][3], b_
            for i in range(3):
                assert np.concatenate([p[i] for p in parts]).tobytes() == whole[i].tobytes(), (n, cuts, i)
            assert st.tobytes() == whole[3].tobytes()


def test_abi_frame_matches_model():
    """igdsp_cng_frame, the same rule through the library"""
    igbuild.build()
    cases = [c for c in all_cases() if c.n in (16, 160) and len(c.kind) == 6]
    for c, m in zip(cases, models(cases)):
        st = np.array(c.state, capi.CNG_STATE)
        for f in range(len(c.kind)):
            ctl = c.ctl if f == 0 or c.ctl != cm.RESET else cm.RUN
            out, ln, rec = capi.cng_frame(st, c.kind[f], c.n, sid=c.sid[f], sid_len=c.sid_len[f], voice=None if c.voice is None else c.voice[f], ctl=ctl,
                                          seed=c.seed)
            assert ln == m[1][f] and np.array_equal(out, m[0][f]) and rec.tobytes() == m[2][f].tobytes(), (c.n, c.ctl, f)
        assert st.tobytes() == m[3].tobytes()
    st = np.zeros((), capi.CNG_STATE)
    for bad_n in (0, 8, 100, 264):
        with pytest.raises(capi.IgdspError):
            capi.cng_frame(st, cm.NONE, bad_n)
    with pytest.raises(capi.IgdspError):
        capi.cng_frame(st, cm.SID, 160, sid=None, sid_len=3)
    assert capi.cng_frame(st, cm.SID, 160, sid=None, sid_len=0)[1] == 0    # an empty SID reads no payload


def test_asan_ubsan_build_agrees(drv, tmp_path):
    """the same cases through the rule built with -fsanitize=address,undefined, as a program of its own"""
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, timeout=300).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")            # decided on a trivial program: an error in the driver fails below
    exe = str(tmp_path / "cng_rule_driver_san")
    drv.build(exe, san)
    cases = all_cases()
    for g, m in zip(drv.run(cases, exe=exe, keep=False), models(cases)):
        same(g, m, "san")
    assert drv.lines("G 11 0 255 255 255 255 255 255 255 255 255 255\nG 1 255\n", exe=exe) == [str(cm.gain([0] + [255] * 10, 11)[0]), "0"]


# ---- what the rule is worth, on the model
def generate(payloads, frames, n=160, seeds=None, ln=None):
    """a SID in frame 0, then NONE: out [frames][C][n], rec"""
    C_ = len(payloads)
    kind = np.zeros((frames, C_), np.int64)
    kind[0] = cm.SID
    sid = np.zeros((frames, C_, 16), np.uint8)
    sid[0] = payloads
    sl = None if ln is None else np.broadcast_to(np.asarray(ln), (frames, C_))
    out, _, rec, _, st = cm.run(kind, sid, n, sid_len=sl, seed=seeds)
    return out, rec, st


def db(ms):
    return 10 * math.log10(ms / 32768.0 ** 2) if ms > 0 else -math.inf


def test_seeds_decorrelate_and_repeat():
    """two seeds: normalised cross-correlation over 100 frames below 4 / sqrt(samples); the same seed: the same row"""
    out, _, _ = generate([cm.payload(30)] * 3, 100, seeds=[0x11111111, 0x22222222, 0x11111111], ln=1)
    a, b, c = (out[:, i].reshape(-1).astype(np.float64) for i in range(3))
    assert np.array_equal(out[:, 0], out[:, 2])
    r = abs(float(a @ b)) / math.sqrt(float(a @ a) * float(b @ b))
    print("cross-correlation", r, "bound", 4 / math.sqrt(len(a)))
    assert r < 4 / math.sqrt(len(a))


def test_white_noise_level():
    """a payload [L]: the mean-square level over 100 frames of 160 within 0.25 dB of -L dBov; L = 0 clips; L >= 106 is zeros, GENERATED"""
    levels = (6, 20, 40, 60, 70, 80)
    out, rec, _ = generate([cm.payload(L) for L in levels + (0, 106, 127)], 100, seeds=list(range(1, 10)), ln=1)
    for i, L in enumerate(levels):
        x = out[:, i].astype(np.float64)
        got = db(float((x * x).mean()))
        print("level", L, "got", got, "off", got + L)
        assert abs(got + L) <= 0.25, (L, got)
        assert L < 20 or not (rec["flags"][:, i] & cm.F_CLIPPED).any()      # e reaches 3.45 sd: -6 dBov clips a sample now and then
    assert (rec["flags"][:, 6] & cm.F_CLIPPED).any() and np.abs(out[:, 6].astype(np.int64)).max() >= 32767
    for i in (7, 8):
        assert not out[:, i].any() and (rec["flags"][:, i] & cm.F_GENERATED).all() and (rec["g"][:, i] == 0).all()


POLES = ((0.8,), (-0.6,), (0.95,), (0.9, 0.5))
# The bound on the autocorrelation against the input's is 0.03.  Where the model at this test's seeds exceeds it, the bound is 1.5 x the
# model's own figure (DESIGN 3.26 records both): the detector's noise model smooths about four frames, so what the payload carries is
# an estimate over some 640 samples and scatters around the input's autocorrelation by about 1 / sqrt(640) = 0.04.  What the generator
# itself adds is bounded separately below, against the autocorrelation the payload was made from.
ACF_BOUND = 0.03
MODEL_ACF_OFF = {(-0.6,): 0.0668, (0.95,): 0.0443}
# against the payload's own model: a coefficient is quantised to +-129 / 32768 = 0.004, three lags accumulate up to three of that, and
# the estimate over 32 000 samples scatters by about 0.006
ACF_OWN_BOUND = 0.02


def acf(x, lags=3):
    x = x.astype(np.float64)
    r0 = float(x @ x)
    return [float(x[k:] @ x[:-k]) / r0 for k in range(1, lags + 1)]


def test_loop_through_the_voice_detector():
    """AR noise of known poles at 300 rms through the voice detector's model (autocorr, 60 frames smoothed with asm_shift 2, sid_payload),
    200 frames generated from the payload: the level within 0.6 dB of -lvl, the normalised autocorrelation at lags 1..3 within 0.03 of
    the input's (the model's own figures, printed; DESIGN 3.26 records them)"""
    n, pays, lvls, want = 160, [], [], []
    for i, poles in enumerate(POLES):
        x = vm.ar_noise(60, n, 40 + i, 300, poles)
        A = None
        for f in range(60):
            r = [int(v) for v in vm.autocorr(x[f])]
            A = r if A is None else [a + ((q - a) >> 2) for a, q in zip(A, r)]
        lvl = vm.level(A[0], n)
        p = np.zeros(16, np.uint8)
        pay = vm.sid_payload(A, lvl, 10)
        p[:len(pay)] = pay
        pays.append(p)
        lvls.append(lvl)
        want.append((acf(np.asarray(x).reshape(-1)), [A[k] / A[0] for k in (1, 2, 3)]))
    out, _, _ = generate(pays, 201, n=n, seeds=[5, 6, 7, 8])
    for i, poles in enumerate(POLES):
        y = out[1:, i].reshape(-1)                                        # 200 frames behind the SID's own
        got = db(float((y.astype(np.float64) ** 2).mean()))
        ac = acf(y)
        off = max(abs(a - b) for a, b in zip(ac, want[i][0]))
        own = max(abs(a - b) for a, b in zip(ac, want[i][1]))
        print("poles", poles, "lvl", lvls[i], "level off", got + lvls[i], "acf", ac, "input", want[i][0], "off", off, "payload's", want[i][1], "off", own)
        assert abs(got + lvls[i]) <= 0.6, (poles, got, lvls[i])
        assert off <= (1.5 * MODEL_ACF_OFF[poles] if poles in MODEL_ACF_OFF else ACF_BOUND), (poles, ac, want[i][0])
        assert (poles in MODEL_ACF_OFF) == (off > ACF_BOUND), (poles, off)   # the table lists exactly the cases that exceed
        assert own <= ACF_OWN_BOUND, (poles, ac, want[i][1])


def test_gain_slew():
    """after a SID that moves the level by 20 dB g reaches g_tgt exactly, in at most 23 frames (g <= 3 632 640 < 2^22: the distance
    halves, rounded up, and is 0 after 22 halvings and one step)"""
    for a, b_ in ((20, 40), (40, 20), (0, 20), (60, 80), (105, 0)):
        F_ = 30
        kind = np.zeros((F_, 1), np.int64)
        kind[0] = kind[3] = cm.SID
        sid = np.zeros((F_, 1, 16), np.uint8)
        sid[0, 0, 0], sid[3, 0, 0] = a, b_
        _, _, rec, _, _ = cm.run(kind, sid, 16, sid_len=np.ones((F_, 1), np.int64))
        g, tgt = rec["g"][:, 0].astype(np.int64), rec["g_tgt"][:, 0].astype(np.int64)
        assert g[0] == tgt[0] == cm.gain([a], 1)[0] and tgt[3] == cm.gain([b_], 1)[0]
        arrived = np.nonzero(g[3:] == tgt[3])[0]
        assert len(arrived) and arrived[0] + 1 <= 23 and (g[3 + arrived[0]:] == tgt[3]).all(), (a, b_, g)
        d = np.abs(tgt[3] - g[3:])
        assert (d[1:] <= (d[:-1] + 1) // 2).all()


def test_host_mirror_comfort_noise():
    """ComfortNoise (host/igdsp_host.h) through its C shims: the frames of a scene give the model's rows, lengths and records"""
    import ctypes

    igbuild.build()
    H = ctypes.CDLL(igbuild.HOST_LIB)
    vp, u, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    for name, res, args in (("igdsp_host_cng_new", vp, [u, u]), ("igdsp_host_cng_free", None, [vp]), ("igdsp_host_cng_process", i, [vp, u, vp, u, vp, vp, u]),
                            ("igdsp_host_cng_rec", i, [vp, vp]), ("igdsp_host_cng_reset", None, [vp])):
        fn = getattr(H, name)
        fn.restype, fn.argtypes = res, args
    for bad in (0, 8, 100, 264):
        assert not H.igdsp_host_cng_new(bad, 1)
    for n in (24, 160):
        h = H.igdsp_host_cng_new(n, 0xABCD)
        assert h
        k, s, sl, v = scene(12, n, n + 1)
        for rep in range(2):
            H.igdsp_host_cng_reset(h)
            out, ln, rec, _, _ = cm.run(k[:, None], s[:, None], n, sl[:, None], v[:, None], seed=[0xABCD])
            for f in range(len(k)):
                row, got, got_rec = np.ascontiguousarray(v[f]), np.zeros(n, np.int16), np.zeros((), capi.CNG_REC)
                pay = np.ascontiguousarray(s[f])
                assert H.igdsp_host_cng_process(h, int(k[f]), pay.ctypes.data, int(sl[f]), row.ctypes.data, got.ctypes.data, 0) == ln[f, 0]
                assert np.array_equal(got, out[f, 0])
                assert H.igdsp_host_cng_rec(h, got_rec.ctypes.data) == 0 and got_rec.tobytes() == rec[f, 0].tobytes()
        assert H.igdsp_host_cng_process(h, 0, None, 0, None, None, 0) == -22 and H.igdsp_host_cng_process(None, 0, None, 0, None, None, 0) == -22
        H.igdsp_host_cng_free(h)
