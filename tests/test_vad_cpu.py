"""-m "not gpu": the voice detector's rule (csrc/igdsp_vad.h) against tests/vad_model.py, bit for bit: kind, record, payload, state.
The rule runs as a program of its own (tests/route/vad_rule_driver.cpp, g++ alone, once more under -fsanitize=address,undefined) and
through the C ABI (igdsp_vad_frame); then what the rule is worth, with integer expectations taken from the rule's text: noise alone,
onset and hangover, hysteresis, the floor's edges, the SID schedule, the level against exact decimal arithmetic, the table's hash, the
payload's quantiser and its inverse, the recursion on garbage, and the distance to a float64 Levinson recursion over the same sums.
The rule is the library's own, UNVERIFIED against RFC 3389 and G.711 Appendix II: what these tests show is what is promised."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import tdet_model
from tests import vad_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
NS = (16, 24, 160, 256)
T8_SHA256 = "8eb9711d2b90a1a62988beae8ee3d2b1da48311e75dfb30259fbffd476fa9947"


def state_of(**kw):
    st = np.zeros((), vm.STATE)
    st["tag"] = vm.TAG
    for k, v in kw.items():
        st[k] = v
    return st


class Driver:
    def __init__(self, d):
        self.exe = str(d / "vad_rule_driver")
        self.build(self.exe)
        self.inputs = []

    def build(self, exe, extra=()):
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        os.path.join(ROOT, "tests", "route", "vad_rule_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)

    @staticmethod
    def text(cases):
        lines = []
        for cfg, x, ctl, st in cases:
            x = np.asarray(x)
            st = np.zeros((), vm.STATE) if st is None else st
            head = [x.shape[1], x.shape[0], ctl] + [format(int(w), "x") for w in np.frombuffer(st.tobytes(), "<u8")]
            lines.append(" ".join(map(str, head + [int(cfg[k]) for k in vm.CFG_KEYS] + x.reshape(-1).tolist())))
        return "\n".join(lines) + "\n"

    @staticmethod
    def parse(cases, stdout):
        res = []
        lines = stdout.splitlines()
        assert len(lines) == len(cases)
        for (cfg, x, ctl, st), line in zip(cases, lines):
            F_ = np.asarray(x).shape[0]
            w = line.split()
            assert len(w) == 5 * F_ + 16
            kind = np.array([int(w[5 * f]) for f in range(F_)], np.uint8)
            rec = np.array([[int(w[5 * f + 1], 16), int(w[5 * f + 2], 16)] for f in range(F_)], "<u8").reshape(F_, 2).view(vm.REC).reshape(F_)
            sid = np.array([[int(w[5 * f + 3], 16), int(w[5 * f + 4], 16)] for f in range(F_)], "<u8").reshape(F_, 2).view(np.uint8).reshape(F_, 16)
            res.append((kind, rec, sid, np.array([int(v, 16) for v in w[5 * F_:]], "<u8").view(vm.STATE)[0]))
        return res

    def run(self, cases, exe=None, keep=True):
        """cases: (cfg, x [F][n], ctl, state record or None) -> per case (kind [F], rec [F], sid [F][16], state)"""
        text = self.text(cases)
        if keep:
            self.inputs.append((cases, text))
        r = subprocess.run([exe or self.exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, (r.returncode, r.stderr[-2000:])
        return self.parse(cases, r.stdout)

    def lines(self, text, exe=None):
        r = subprocess.run([exe or self.exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, (r.returncode, r.stderr[-2000:])
        return r.stdout.splitlines()


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    return Driver(tmp_path_factory.mktemp("vad_rule"))


def model_one(cfg, x, ctl, st):
    x = np.asarray(x)
    return vm.run(cfg, x[:, None, :], ctl=[ctl], state=None if st is None else np.array([st], vm.STATE))


def same(got, model, what=""):
    (k, r, s, st), (mk, mr, ms, _, mst) = got, model
    assert np.array_equal(k, mk[:, 0]), (what, k, mk[:, 0])
    assert r.tobytes() == mr[:, 0].tobytes(), (what, [(key, r[key], mr[key][:, 0]) for key in mr.dtype.names if not np.array_equal(r[key], mr[key][:, 0])])
    assert np.array_equal(s, ms[:, 0]), (what, s, ms[:, 0])
    assert st.tobytes() == mst[0].tobytes(), (what, st, mst[0])


def check(drv, cases, what=""):
    """the driver's bytes are the model's; returns the models"""
    got = drv.run(cases)
    models = [model_one(*c) for c in cases]
    for i, (g, m) in enumerate(zip(got, models)):
        same(g, m, (what, i))
    return models


def three_states(seed):
    return [None, vm.garbage_state(1, seed)[0], vm.garbage_state(1, seed, tagged=False)[0]]


def test_layouts_and_defaults():
    igbuild.build()
    for a, b, size in ((capi.VAD_CFG, vm.CFG, 32), (capi.VAD_STATE, vm.STATE, 128), (capi.VAD_REC, vm.REC, 16), (capi.VAD_EVENT, vm.EVENT, 16)):
        assert a.itemsize == b.itemsize == size and a.names == b.names and [a.fields[k][1] for k in a.names] == [b.fields[k][1] for k in b.names]
    assert capi.vad_cfg_default().tobytes() == vm.cfg_default().tobytes()
    d = vm.cfg_default()
    assert [int(d[k]) for k in vm.CFG_KEYS] == [212, 8, 1 << 20, 0, 80, 40, 2, 5, 7, 2, 5, 10, 2, 10, 1, 2, 2, 0x81, 0x80]
    assert (capi.VAD_RUN, capi.VAD_FREEZE, capi.VAD_BYPASS, capi.VAD_RESET) == (vm.RUN, vm.FREEZE, vm.BYPASS, vm.RESET) == (0, 1, 2, 3)
    assert (capi.VAD_NONE, capi.VAD_VOICE, capi.VAD_SID) == (vm.NONE, vm.VOICE, vm.SID) == (0, 1, 2)
    assert (capi.VAD_F_RAW, capi.VAD_F_VOICE, capi.VAD_F_ONSET, capi.VAD_F_OFFSET, capi.VAD_F_SID, capi.VAD_F_QUIET, capi.VAD_F_FROZEN, capi.VAD_F_BYPASSED) == (
        vm.F_RAW, vm.F_VOICE, vm.F_ONSET, vm.F_OFFSET, vm.F_SID, vm.F_QUIET, vm.F_FROZEN, vm.F_BYPASSED) == (1, 2, 4, 8, 16, 32, 64, 128)
    assert capi.VAD_EVENT_DEFAULT == vm.EVENT_DEFAULT == 12 and capi.VAD_TAG == vm.TAG and capi.VAD_KMAX == vm.KMAX == 126 * 258
    hdr = open(os.path.join(ROOT, "include", "igdsp.h")).read()
    assert f"#define IGDSP_VAD_TAG     0x{vm.TAG:08X}u" in hdr and "UNVERIFIED against RFC 3389 and G.711 Appendix II" in hdr
    assert "#define IGDSP_ABI_VERSION 3" in hdr
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        assert "UNVERIFIED against RFC 3389 and G.711 Appendix II" in open(os.path.join(ROOT, doc)).read(), doc


def test_yardstick_is_bound_as_its_entry():
    """igdsp_internal_vad_move takes igdsp_vad_run's arguments: capi.INTERNAL_MORE is that list and capi.internal finds it"""
    res, args = capi.INTERNAL_MORE["igdsp_internal_vad_move"]
    pub = {name: (r, a) for name, r, a in capi.PROTOTYPES}["igdsp_vad_run"]
    assert (res, list(args)) == (pub[0], list(pub[1])) and capi.INTERNAL_MORE_TWIN["igdsp_internal_vad_move"] == "igdsp_vad_run"
    assert "igdsp_internal_vad_move" not in capi.INTERNAL and len(pub[1]) == 20


def test_table_hash():
    """T8 recomputed with decimal arithmetic, the committed list, the ABI's copy: one digest"""
    igbuild.build()
    assert hashlib.sha256(np.array(vm.T8, "<u8").tobytes()).hexdigest() == T8_SHA256
    assert hashlib.sha256(capi.vad_table().tobytes()).hexdigest() == T8_SHA256
    text = open(os.path.join(CSRC, "igdsp_vad_tab.h")).read().split("IGDSP_VAD_T8_VALUES")[1]
    vals = [int(t.replace("ull", "")) for t in text.replace("\\", " ").replace(",", " ").split()]
    assert vals == vm.T8
    assert all(a >= b for a, b in zip(vm.T8, vm.T8[1:])) and vm.T8[0] == 1 << 34


def test_level_against_decimal_at_every_edge(drv):
    """level(e) at the least e that reaches T8[d], one below and one above, for every d and n; e = 0 and below read 127; a full-scale
    square wave reads 0"""
    q = []
    for n in NS:
        for d in range(127):
            edge = -(-(n * vm.T8[d]) // 256)                               # the least e with (e << 8) >= n T8[d]
            q += [(n, e) for e in (edge - 1, edge, edge + 1)]
        q += [(n, 0), (n, -1), (n, -(1 << 40)), (n, 1), (n, 1 << 40), (n, n * 8192 * 8192), (n, n * 8191 * 8191)]
    out = drv.lines("".join(f"L {n} {e}\n" for n, e in q))
    assert len(out) == len(q)
    for (n, e), line in zip(q, out):
        assert int(line) == vm.level(e, n), (n, e)
    for n in NS:
        assert vm.level(0, n) == 127 and vm.level(n * 8192 * 8192, n) == 0 and vm.level(n * 8191 * 8191, n) == 1
        for d in range(1, 60):                                             # lvl = ceil(-dBov): the edge of d lies within one of 2^34 10^(-d/10) n / 256
            edge = -(-(n * vm.T8[d]) // 256)
            assert vm.level(edge, n) == d and vm.level(edge - 1, n) == d + 1, (n, d)


def test_sid_decode_inverts_the_quantiser(drv):
    igbuild.build()
    out = drv.lines("".join(f"D 2 77 {N}\n" for N in range(256)))
    for N in range(255):
        rc, lvl, k = map(int, out[N].split())
        assert (rc, lvl, k) == (0, 77, 258 * (N - 127)) and vm.quant(k) == N and vm.sid_decode([77, N])[1][0] == k
        lv, kk = capi.sid_decode(np.array([77, N], np.uint8))
        assert lv == 77 and int(kk[0]) == k and not kk[1:].any()
    assert int(out[255].split()[2]) == 258 * 127
    # every k the recursion can give lands within half a step of its index's value
    for k in list(range(-vm.KMAX, vm.KMAX + 1, 7)) + [-vm.KMAX, vm.KMAX, 0, 129, 128, -129, -128]:
        N = vm.quant(k)
        assert 1 <= N <= 253 and abs(258 * (N - 127) - k) <= 129


@pytest.mark.parametrize("n", NS)
def test_bit_for_bit_every_ctl_and_state(drv, n):
    cases = []
    for ctl in (0, 1, 2, 3, 4, 255):
        for i, st in enumerate(three_states(10 * n + ctl)):
            x = vm.scene(16, 1, n, 100 * n + 10 * ctl + i, rms=(33, 100, 330)[i])[:, 0]
            cases.append((vm.cfg_default(sid_every=4 if ctl == 1 else 0, order=(10, 1, 0)[i]), x, ctl, st))
    models = check(drv, cases, n)
    kinds = np.concatenate([m[0].reshape(-1) for m in models])
    flags = np.concatenate([m[1]["flags"].reshape(-1) for m in models])
    assert all((kinds == k).any() for k in (0, 1, 2)) and all((flags & b).any() for b in (1, 2, 4, 8, 16, 64, 128))


def test_split_over_calls(drv):
    for n in NS:
        x = vm.scene(14, 1, n, n)[:, 0]
        for st in three_states(n):
            whole = drv.run([(vm.cfg_default(), x, vm.RUN, st)])[0]
            s, parts = st, []
            for lo, hi in ((0, 1), (1, 5), (5, 6), (6, 14)):
                got = drv.run([(vm.cfg_default(), x[lo:hi], vm.RUN, s)])[0]
                parts.append(got)
                s = got[3]
            assert np.array_equal(np.concatenate([p[0] for p in parts]), whole[0])
            assert np.concatenate([p[1] for p in parts]).tobytes() == whole[1].tobytes()
            assert np.array_equal(np.concatenate([p[2] for p in parts]), whole[2]) and s.tobytes() == whole[3].tobytes()


def test_abi_frame_is_the_rule():
    igbuild.build()
    for n in NS:
        for ctl in (0, 1, 2, 3, 9):
            for i, st in enumerate(three_states(n + ctl)):
                cfg = vm.cfg_default(order=(10, 3, 0)[i])
                x = vm.scene(13, 1, n, n + ctl + i)[:, 0]
                model = model_one(cfg, x, ctl, st)
                s = np.zeros((), capi.VAD_STATE) if st is None else np.array(st, capi.VAD_STATE)
                got = [capi.vad_frame(cfg, s, x[f].astype(np.int16), ctl if f == 0 or ctl != vm.RESET else vm.RUN) for f in range(len(x))]
                same((np.array([g[0] for g in got], np.uint8), np.frombuffer(b"".join(g[1].tobytes() for g in got), vm.REC), np.array([g[2] for g in got]), s), model, (n, ctl, i))
    s = np.zeros((), capi.VAD_STATE)
    for bad_n in (0, 8, 20, 264):
        with pytest.raises(capi.IgdspError):
            capi.vad_frame(None, s, np.zeros(bad_n, np.int16))
    with pytest.raises(capi.IgdspError):
        capi.vad_frame(vm.cfg_default(order=11), s, np.zeros(160, np.int16))
    assert capi.vad_frame(None, s, np.zeros(160, np.int16))[0] == vm.SID    # the first frame of a fresh leg with DTX: a SID


def test_asan_ubsan_build_agrees(drv, tmp_path):
    """the same cases through the rule built with -fsanitize=address,undefined, as a program of its own"""
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, timeout=300).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")            # decided on a trivial program: an error in the driver fails below
    exe = str(tmp_path / "vad_rule_driver_san")
    drv.build(exe, san)
    cases = [(vm.cfg_default(order=o), vm.scene(12, 1, n, n + o)[:, 0], ctl, st) for n in NS for o, ctl, st in
             zip((10, 5, 0, 10), (0, 1, 3, 2), three_states(n) + [None])] + garbage_cases()
    a, b = drv.run(cases, keep=False), drv.run(cases, exe=exe, keep=False)
    for g, h in zip(a, b):
        assert all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(g, h))


# ---- the scenes: integer expectations from the rule's text
def const_frames(levels, n=160):
    """frames of a square wave whose v is +-a: ms = a^2 exactly"""
    sign = np.where(np.arange(n) % 2 == 0, 1, -1)
    return np.array([4 * a * sign for a in levels], np.int64)


def test_noise_only_no_voice_after_frame_0(drv):
    for rms in (33, 100, 330):
        for seed in range(3):
            m = check(drv, [(vm.cfg_default(), vm.noise(200, 1, 160, seed, rms)[:, 0], vm.RUN, None)])[0]
            assert not (m[1]["flags"][1:, 0] & vm.F_VOICE).any() and not (m[0][1:, 0] == vm.VOICE).any(), (rms, seed)


def test_burst_onset_and_hangover(drv):
    c = vm.cfg_default()
    for n_burst, hang in ((7, 10), (5, 10), (2, 2), (4, 2), (1, 2)):
        levels = [20] * 30 + [200] * n_burst + [20] * 20
        x = const_frames(levels)
        m = check(drv, [(c, x, vm.RUN, None)])[0]
        fl, rec = m[1]["flags"][:, 0], m[1][:, 0]
        # ONSET on the first frame with ms * 16 > nf * ratio_on, nf the floor before that frame
        nf_before = np.concatenate([[0], rec["nf"][:-1]])
        first = next(f for f in range(1, len(levels)) if int(rec["ms"][f]) >= 212 and int(rec["ms"][f]) * 16 > int(nf_before[f]) * 80)
        assert first == 30 and np.flatnonzero(fl & vm.F_ONSET).tolist() == [first]
        last_raw = np.flatnonzero(fl & vm.F_RAW)[-1]
        assert last_raw == 30 + n_burst - 1
        # hang frames of VOICE behind the last raw frame, OFFSET on the one after them
        assert np.flatnonzero(fl & vm.F_OFFSET).tolist() == [last_raw + hang + 1]
        assert (fl[first:last_raw + hang + 1] & vm.F_VOICE).all() and not (fl[last_raw + hang + 1:] & vm.F_VOICE).any()
        assert m[0][last_raw + hang + 1, 0] == vm.SID and (m[0][first:last_raw + hang + 1, 0] == vm.VOICE).all()


def test_hysteresis(drv):
    """ms between nf * ratio_off / 16 and nf * ratio_on / 16 keeps VOICE and does not start it"""
    c = vm.cfg_default(up=15, up_v=15, dn=15)                              # the floor all but stands: nf = 400 +- a few
    mid = 35                                                               # ms = 1225: 400 * 40 / 16 = 1000 < 1225 < 2000 = 400 * 80 / 16
    x = const_frames([20] * 10 + [mid] * 10 + [60] * 6 + [mid] * 30 + [20] * 15)
    m = check(drv, [(c, x, vm.RUN, None)])[0]
    fl = m[1]["flags"][:, 0]
    assert not (fl[:20] & (vm.F_VOICE | vm.F_RAW)).any()                   # mid does not start it
    assert (fl[20:56] & vm.F_RAW).all() and (fl[20:56] & vm.F_VOICE).all() # 60^2 starts it, mid keeps it raw
    assert np.flatnonzero(fl & vm.F_OFFSET).tolist() == [56 + 10] and np.flatnonzero(fl & vm.F_ONSET).tolist() == [20]


def test_floor_edges(drv):
    c = vm.cfg_default()
    # QUIET frames (ms < nf_min: zeros, and A-law's silence x = 8, v = 2, ms = 4) leave nf
    x = np.concatenate([const_frames([20] * 5), np.zeros((10, 160), np.int64), np.full((10, 160), 8, np.int64), const_frames([20] * 3)])
    m = check(drv, [(c, x, vm.RUN, None)])[0]
    rec = m[1][:, 0]
    assert (rec["nf"] == 400).all() and (rec["flags"][5:25] & vm.F_QUIET).all() and not (rec["flags"][:5] & vm.F_QUIET).any()
    assert list(rec["ms"][5:25]) == [0] * 10 + [4] * 10
    # the max(1, .) term: nf = 9 with up = 5 gives 9 >> 5 = 0, the floor still climbs by 1 a frame toward ms = 100
    m = check(drv, [(c, const_frames([10] * 12), vm.RUN, state_of(nf=9))])[0]
    assert list(m[1]["nf"][:, 0]) == list(range(10, 22))
    # down: nf -= (nf - ms) >> dn
    m = check(drv, [(c, const_frames([10] * 3), vm.RUN, state_of(nf=1000))])[0]
    assert list(m[1]["nf"][:, 0]) == [775, 607, 481]
    # both clamps, on what is read and on what a frame leaves
    lo = vm.cfg_default(nf_min=50, nf_max=150)
    m = check(drv, [(lo, const_frames([7, 7, 100, 100]), vm.RUN, state_of(nf=51)), (lo, const_frames([100]), vm.RUN, state_of(nf=7)),
                    (lo, const_frames([3]), vm.RUN, state_of(nf=1 << 30)), (lo, const_frames([40] * 3), vm.RUN, None)])
    assert list(m[0][1]["nf"][:, 0]) == [51, 51, 52, 53] and (m[0][1]["flags"][:2, 0] & vm.F_QUIET).all()          # ms 49 < 50: QUIET, then + 1 a frame
    assert int(m[1][1]["nf"][0, 0]) == 51 and int(m[2][1]["nf"][0, 0]) == 150
    assert list(m[3][1]["nf"][:, 0]) == [150, 150, 150]                    # unset: clamp(1600) = 150, and ms above it cannot lift it
    # FREEZE: the decision runs, the floor and the model stand
    st = state_of(nf=400, avalid=1, A=[7] * 11, sid_sent=1, last_level=60)
    m = check(drv, [(c, const_frames([20, 100, 100, 20]), vm.FREEZE, st)])[0]
    assert (m[1]["nf"][:, 0] == 400).all() and (m[1]["flags"][:, 0] & vm.F_FROZEN).all() and list(m[1]["flags"][:, 0] & vm.F_RAW) == [0, 1, 1, 0]
    assert list(m[4]["A"][0]) == [7] * 11


def test_sid_schedule(drv):
    quiet = [20] * 40
    # a fresh leg: the first non-VOICE frame sends (no SID since RESET), then nothing while the level stands
    m = check(drv, [(vm.cfg_default(), const_frames(quiet), vm.RUN, None)])[0]
    assert m[0][:, 0].tolist() == [vm.SID] + [vm.NONE] * 39 and list(m[1]["sid_len"][:, 0]) == [11] + [0] * 39
    # sid_every
    m = check(drv, [(vm.cfg_default(sid_every=7), const_frames(quiet), vm.RUN, None)])[0]
    assert np.flatnonzero(m[0][:, 0] == vm.SID).tolist() == [0, 8, 16, 24, 32]   # since_sid counts the NONE frames: 7 of them, then the SID
    # sid_delta with sid_gap: the level steps by 20 dB at frame 10; A[0] follows at asm_shift = 2, a SID each time lvl has moved by >= 2
    # and two NONE frames lie behind the last one
    c = vm.cfg_default(sid_delta=2, sid_gap=2)
    x = const_frames([20] * 10 + [2] * 30)
    m = check(drv, [(c, x, vm.RUN, None)])[0]
    kinds = m[0][:, 0]
    assert not (m[1]["flags"][:, 0] & (vm.F_RAW | vm.F_VOICE)).any()       # every frame feeds the model and meets the schedule clause
    # the clause by hand: E = ms * n exactly on these rows, A[0] follows it at asm_shift = 2, lvl from the table
    want, A0, last, since = [], None, None, 0
    for f in range(len(x)):
        E = int(m[1]["ms"][f, 0]) * 160
        A0 = E if A0 is None else A0 + ((E - A0) >> 2)
        lvl = next((d for d in range(127) if (A0 << 8) >= 160 * vm.T8[d]), 127) if A0 > 0 else 127
        if last is None or (abs(lvl - last) >= 2 and since >= 2):
            want.append(f)
            last, since = lvl, 0
        else:
            since += 1
    sids = np.flatnonzero(kinds == vm.SID)
    assert sids.tolist() == want and (kinds[np.setdiff1d(np.arange(len(x)), sids)] == vm.NONE).all()
    assert len(sids) >= 4 and (np.diff(sids) >= 3).all() and sids[1] >= 10
    lv = [int(m[2][f, 0, 0]) for f in sids]
    assert all(abs(a - b) >= 2 for a, b in zip(lv, lv[1:])) and lv[-1] - lv[0] >= 18
    # dtx = 0: every frame VOICE, no payload, the flags still carry the decision
    m = check(drv, [(vm.cfg_default(dtx=0), const_frames([20] * 5 + [200] * 6 + [20] * 14), vm.RUN, None)])[0]
    assert (m[0] == vm.VOICE).all() and not m[2].any() and not m[1]["sid_len"].any()
    assert np.flatnonzero(m[1]["flags"][:, 0] & vm.F_ONSET).tolist() == [5] and np.flatnonzero(m[1]["flags"][:, 0] & vm.F_OFFSET).tolist() == [21]
    # the OFFSET frame sends whatever the gap
    m = check(drv, [(vm.cfg_default(sid_gap=255, sid_delta=255), const_frames([20] * 3 + [200] * 2 + [20] * 6), vm.RUN, None)])[0]
    assert np.flatnonzero(m[0][:, 0] == vm.SID).tolist() == [0, 7] and m[1]["flags"][7, 0] & vm.F_OFFSET


def test_noise_step_and_speech_like_bursts(drv):
    """What up_v = 7 costs and buys.  A 10 dB step of the noise itself reads as voice until the floor has climbed: raw holds while
    ms * 16 > nf * ratio_off_q4, that is nf < 0.4 ms; the floor starts near ms / 10 and gains 1 / 128 a raw frame, so ln 4 / ln (129 / 128)
    = 178 raw frames and hang_long more, 188.  A noise frame's ms scatters by sqrt(2 / 160) = 11 %, and three of that end the run up to
    ln (1 / 0.67) / ln (129 / 128) = 52 frames early; a floor a few per cent under the noise adds up to 12.  Under speech-like bursts (15
    frames on, 10 off, 20 dB above the noise, 10 s) every burst frame is VOICE and the floor moves less than 2 dB (10^0.2 = 1.585)."""
    c = vm.cfg_default()
    for seed in (1, 2):
        x = np.concatenate([vm.noise(60, 1, 160, seed, 100), vm.noise(500, 1, 160, seed + 9, 316)])[:, 0]
        m = check(drv, [(c, x, vm.RUN, None)])[0]
        v = (m[1]["flags"][:, 0] & vm.F_VOICE) != 0
        assert not v[1:60].any() and v[60] and 188 - 52 <= int(v[60:].sum()) <= 188 + 12, int(v[60:].sum())
        assert v[60:60 + int(v[60:].sum())].all()                          # one run of false VOICE, then none
    x = vm.noise(560, 1, 160, 5, 100)[:, 0].astype(np.float64)
    on = np.zeros(560, bool)
    for f0 in range(60, 560, 25):
        on[f0:f0 + 15] = True
    x[on] *= 10.0
    m = check(drv, [(c, np.rint(x).astype(np.int64), vm.RUN, None)])[0]
    fl, nf = m[1]["flags"][:, 0], m[1]["nf"][:, 0].astype(np.int64)
    assert ((fl[on] & vm.F_VOICE) != 0).all() and ((fl[on] & vm.F_RAW) != 0).all()
    assert int(nf[60:].max()) * 1000 < int(nf[59]) * 1585 and int(nf[60:].min()) * 1585 > int(nf[59]) * 1000


def garbage_cases():
    """states whose A is not an autocorrelation, frozen so that the first frame's SID is made of it"""
    big = 1 << 40
    As = [[0] * 11, [-5] + [9] * 10, [1] + [big] * 10, [1] + [-big] * 10, [big] * 11, [big] + [-big] * 10, [-big] * 11, [100] + [101, -101] * 5,
          [big] + [big, -big] * 5, [3, -3, 3, -3, 3, -3, 3, -3, 3, -3, 3], [1 << 62] * 11, [-(1 << 63)] * 11, [(1 << 63) - 1] + [-(1 << 63)] * 10, [2] + [1] * 10]
    rng = np.random.default_rng(5)
    As += [[int(v) for v in rng.integers(-big, big, 11)] for _ in range(40)] + [[int(abs(v)) >> 20] + [int(w) for w in rng.integers(-big, big, 10)]
                                                                               for v in rng.integers(1, big, 20)]
    return [(vm.cfg_default(order=10), const_frames([20]), vm.FREEZE, state_of(nf=400, A=A)) for A in As]


def test_recursion_is_safe_on_garbage(drv):
    cases = garbage_cases()
    for m in check(drv, cases):
        assert m[0][0, 0] == vm.SID and m[1]["sid_len"][0, 0] == 11
        p = m[2][0, 0]
        assert all(1 <= int(N) <= 253 for N in p[1:11]) and not p[11:].any() and int(p[0]) <= 127
    assert vm.sid_payload([0] * 11, 127, 10) == [127] + [127] * 10 and vm.sid_payload([-1] + [5] * 10, 127, 10)[1:] == [127] * 10
    assert all(abs(k) <= vm.KMAX for A in (c[3]["A"] for c in cases) for k in vm.reflection([max(-vm.AMAX, min(vm.AMAX, int(a))) for a in A], 10))


# ---- fidelity: the integer recursion against float64 over the same sums
def levinson_f64(A, order):
    R = np.array(A, np.float64)
    R[0] = R[0] * (1.0 + 1.0 / 1024.0) + 1.0                               # the rule's R0 = A0 + (A0 >> 10) + 1, in floating point
    a, err, k = np.zeros(order + 1), R[0], np.zeros(order)
    for i in range(1, order + 1):
        acc = R[i] + np.dot(a[1:i], R[i - 1:0:-1])
        ki = -acc / err
        a[1:i] = a[1:i] + ki * a[i - 1:0:-1]
        a[i] = ki
        k[i - 1] = ki
        err *= 1.0 - ki * ki
    return np.clip(k, -vm.KMAX / 32768.0, vm.KMAX / 32768.0)


def fidelity_cases():
    """(name, x [F][n] as PCM, the process's theoretical k_1, k_2): white, AR(1) and AR(2) noise of known poles, as PCM and through mu-law"""
    out = []
    procs = [("white", [], 0.0, 0.0), ("ar1+", [0.8], -0.8, 0.0), ("ar1-", [-0.6], 0.6, 0.0), ("ar1s", [0.95], -0.95, 0.0),
             ("ar2", [0.9 * np.exp(0.5j), 0.9 * np.exp(-0.5j)], None, 0.81), ("ar2r", [0.7, -0.4], None, -0.28)]
    for name, poles, k1, k2 in procs:
        if k1 is None:                                                     # A(z) = 1 + a1 z^-1 + a2 z^-2: k_2 = a2, k_1 = a1 / (1 + a2)
            a = np.real(np.poly(poles))
            k1 = a[1] / (1.0 + a[2])
        for rms in (30, 300, 1000):
            for seed in (1, 2):
                x = vm.ar_noise(25, 160, seed * 100 + rms, rms, poles)
                out.append((f"{name}/{rms}/{seed}/pcm", x, k1, k2))
                law = np.zeros(1, np.uint8)
                out.append((f"{name}/{rms}/{seed}/ulaw", tdet_model.decode(tdet_model.encode(x[:, None, :].astype(np.int16), law), law)[:, 0].astype(np.int64), k1, k2))
    return out


def test_fidelity_against_float64(drv):
    """The decoded k_i against a float64 Levinson over the same A: one index (258 in Q15), the quantiser's own step, no more.  The
    decoded k_1, k_2 against the process's theoretical values: the float64 recursion's own deviation over the same frames plus one index."""
    c = vm.cfg_default(thr_abs=1 << 30)                                    # nothing is ever raw: every frame feeds the model
    names, cases = [], []
    for name, x, k1, k2 in fidelity_cases():
        names.append((name, k1, k2))
        cases.append((c, np.concatenate([x, x[-1:]]), vm.RUN, None))
    exact = total = 0
    worst_f64 = worst_int = 0.0
    # the state before the last frame is the model that frame's payload is made of; a SID is forced on that frame, and the frame goes
    # through the driver: the indices counted below are the C++ recursion's
    forced = []
    for case, m in zip(cases, check(drv, cases)):
        st_before = model_one(c, case[1][:-1], vm.RUN, None)[4][0]
        st_before["sid_sent"] = 0
        forced.append((c, case[1][-1:], vm.RUN, st_before))
    got = drv.run(forced)
    for (name, k1, k2), case, g in zip(names, forced, got):
        model = model_one(*case)
        same(g, model, name)
        k, sid, st = g[0][:, None], g[2][:, None], [g[3]]
        assert k[0, 0] == vm.SID
        A = [int(v) for v in st[0]["A"]]
        kf = levinson_f64(A, 10)
        Nf = [vm.quant(int(round(v * 32768.0))) for v in kf]
        Ni = [int(v) for v in sid[0, 0, 1:11]]
        assert all(abs(a - b) <= 1 for a, b in zip(Ni, Nf)), (name, Ni, Nf)
        exact += sum(a == b for a, b in zip(Ni, Nf))
        total += 10
        kd = vm.sid_decode(sid[0, 0, :11])[1]
        dev_f64 = max(abs(kf[0] - k1), abs(kf[1] - k2)) * 32768.0
        dev_int = max(abs(kd[0] - k1 * 32768.0), abs(kd[1] - k2 * 32768.0))
        worst_f64, worst_int = max(worst_f64, dev_f64), max(worst_int, dev_int)
        assert dev_int <= dev_f64 + 258.0, (name, kd[:2], kf[:2] * 32768.0, (k1, k2))
    print(f"fidelity: {exact} of {total} indices exact ({exact / total:.4f}); float64 from theory at most {worst_f64:.0f} Q15, decoded at most {worst_int:.0f} Q15")
    assert total == 10 * len(cases)


def test_host_mirror_voice_detector():
    """VoiceDetector (host/igdsp_host.h) through its C shims: the frames of a scene give the model's kinds, records and payloads"""
    import ctypes

    igbuild.build()
    H = ctypes.CDLL(igbuild.HOST_LIB)
    vp, u, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    for name, res, args in (("igdsp_host_vad_new", vp, [u]), ("igdsp_host_vad_free", None, [vp]), ("igdsp_host_vad_process", i, [vp, vp, u]),
                            ("igdsp_host_vad_rec", i, [vp, vp]), ("igdsp_host_vad_sid", i, [vp, vp]), ("igdsp_host_vad_cfg", i, [vp, vp]),
                            ("igdsp_host_vad_reset", None, [vp])):
        fn = getattr(H, name)
        fn.restype, fn.argtypes = res, args
    for bad in (0, 8, 100, 264):
        assert not H.igdsp_host_vad_new(bad)
    for n in (24, 160):
        h = H.igdsp_host_vad_new(n)
        assert h
        x = vm.scene(14, 1, n, n + 1)
        for cfg in (vm.cfg_default(), vm.cfg_default(order=4, sid_every=3)):
            assert H.igdsp_host_vad_cfg(h, cfg.ctypes.data) == 0
            H.igdsp_host_vad_reset(h)
            k, rec, sid, _, _ = vm.run(cfg, x)
            for f in range(len(x)):
                row = np.ascontiguousarray(x[f, 0], np.int16)
                got_rec, got_sid = np.zeros((), capi.VAD_REC), np.zeros(16, np.uint8)
                assert H.igdsp_host_vad_process(h, row.ctypes.data, 0) == k[f, 0]
                assert H.igdsp_host_vad_rec(h, got_rec.ctypes.data) == 0 and got_rec.tobytes() == rec[f, 0].tobytes()
                assert H.igdsp_host_vad_sid(h, got_sid.ctypes.data) == rec[f, 0]["sid_len"] and np.array_equal(got_sid, sid[f, 0])
        assert H.igdsp_host_vad_process(h, None, 0) == -22 and H.igdsp_host_vad_process(None, None, 0) == -22
        H.igdsp_host_vad_free(h)
