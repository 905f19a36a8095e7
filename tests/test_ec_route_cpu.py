"""-m "not gpu": the geometry of igdsp_echo_cancel (ec_route in csrc/igdsp_route.h), compiled with g++ alone through
tests/route/ec_route_driver.cpp: a block of 4 waves owns 16 channels (16 lanes each), the grid covers every channel, the LDS holds per
channel the far history and frame between two pads of 8 values and the near row behind a pad, and every window a block of a frame
reads, anchored at the block's end for every lane, lies inside them.  Shapes that are not the kernel's launch nothing.
The rule itself (csrc/igdsp_ec.h) runs as a program of its own through tests/route/ec_rule_driver.cpp over full-scale rows, garbage
and saturated states, is compared with tests/ec_model.py, and is built once more with -fsanitize=address,undefined and run over the
same input."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
NS = list(range(2, 257, 2))
CASES = ([(1, 1, n, L) for n in NS for L in (128, 256)] + [(C, F, 160, L) for C in (1, 15, 16, 17, 63, 64, 65, 67, 4096, 65536) for F in (1, 5, 128)
                                                            for L in (128, 256)] + [(0xFFFFFFDF, 1, 160, 256), (1 << 28, 15, 2, 128)])
NOTHING = [(0, 5, 160, 256), (5, 0, 160, 256), (5, 5, 0, 256), (5, 5, 161, 256), (5, 5, 258, 256), (1 << 28, 16, 160, 256), (5, 5, 160, 64), (5, 5, 160, 192),
           (5, 5, 160, 512), (5, 5, 160, 0)]
FIELDS = "grid threads lds tail blocks x_lo x_hi n_lo n_hi move_hi xbuf nbuf pad chans resident".split()


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("ec_route") / "ec_route_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "ec_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    cases = CASES + NOTHING
    r = subprocess.run([exe], input="\n".join(" ".join(map(str, c)) for c in cases) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [dict(zip(FIELDS, map(int, line.split()))) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return dict(zip(cases, out))


def test_geometry(routes):
    for case in CASES:
        C, F, n, L = case
        r = routes[case]
        assert r["chans"] == 16 and r["threads"] == 16 * r["chans"] == 256 and r["pad"] == 8
        assert r["grid"] == -(-C // 16) and r["grid"] * 16 >= C
        assert r["tail"] == L and r["blocks"] == -(-n // 8)
        assert r["xbuf"] == 8 + 256 + 256 + 8 and r["nbuf"] == 8 + 256
        assert r["lds"] == 16 * (r["xbuf"] + r["nbuf"]) * 2 and r["lds"] * r["resident"] <= 160 * 1024 and r["resident"] == 3
        # every window of every lane and block lies inside the buffers, on a dword; the pads are what a short last block reaches into
        assert 0 <= r["x_lo"] and r["x_lo"] % 2 == 0 and r["x_hi"] <= r["xbuf"] and r["x_hi"] == 8 + L + n
        assert 0 <= r["n_lo"] and r["n_lo"] % 2 == 0 and r["n_hi"] == 8 + n <= r["nbuf"]
        assert r["x_lo"] == r["n_lo"] == min(8, n) and r["move_hi"] <= r["xbuf"]     # below the pad only when the frame is shorter than a block


def test_nothing_to_launch(routes):
    for case in NOTHING:
        assert routes[case]["grid"] == 0 and routes[case]["threads"] == 0, case


# ---- the rule as a program of its own, plain and under the sanitizers: n frames seed garbage tail mu_shift hang ctl
RULE_CASES = [(n, frames, 7 + n + g, g, L, mu, hang, ctl) for n, frames in ((160, 4), (164, 3), (24, 8), (2, 30), (256, 3)) for L in (128, 256)
              for g, mu, hang, ctl in ((0, 2, 80, 0), (1, 2, 2, 0), (2, 0, 0, 0), (2, 6, 0, 1), (1, 3, 0, 3), (1, 2, 0, 2))]


def _xorshift_case(n, frames, seed, garbage, L):
    """the driver's sequence: (the state or None, near [frames][n], far [frames][n])"""
    import numpy as np

    from tests import ec_model as em

    s = seed or 1

    def nxt():
        nonlocal s
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        return s

    st = None
    if garbage:
        st = np.frombuffer(bytes(nxt() & 0xFF for _ in range(em.STATE.itemsize)), em.STATE).copy()
        st["tag"] = em.TAG | L
        st["hang"] &= 3
        if garbage == 2:
            st["w"][0] = [(1 << 31) - 1 if nxt() & 1 else -(1 << 31) for _ in range(256)]
    rows = np.zeros((frames, 2, n), np.int16)
    for f in range(frames):
        for i in range(2 * n):
            r = nxt()
            rows[f, i // n, i % n] = -32768 if (r & 0x30000) == 0 else np.array(r & 0xFFFF, np.uint16).astype(np.int16)
    return st, rows[:, :1], rows[:, 1:]


def _fnv(b):
    h = 1469598103934665603
    for v in b:
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.fixture(scope="module")
def rule_driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("ec_rule")

    def build(exe, extra=()):
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        os.path.join(ROOT, "tests", "route", "ec_rule_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)

    exe = str(d / "ec_rule_driver")
    build(exe)
    text = "\n".join(" ".join(map(str, c)) for c in RULE_CASES) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(dir=d, build=build, input=text, out=r.stdout.splitlines())


def test_rule_program_matches_the_model(rule_driver):
    """ec_frame_run compiled by g++ alone over full-scale rows (-32768 among them), garbage and saturated states: the model's records,
    outputs and state"""
    from tests import ec_model as em

    assert len(rule_driver["out"]) == len(RULE_CASES)
    saturated = 0
    for case, line in zip(RULE_CASES, rule_driver["out"]):
        n, frames, seed, garbage, L, mu, hang, ctl = case
        st, near, far = _xorshift_case(n, frames, seed, garbage, L)
        cfg = em.cfg_default(L, mu_shift=mu, hang=hang, pmin=0)
        out, rec, _, st = em.cancel(cfg, near, far, ctl=[ctl], state=st)
        words = [int(w, 16) for w in line.split()]
        assert len(words) == 3 * frames + 1
        for f in range(frames):
            assert words[3 * f:3 * f + 2] == [int(v) for v in rec[f, 0].reshape(1).view("<u8")], (case, f)
            assert words[3 * f + 2] == _fnv(out[f, 0].tobytes()), (case, f)
        assert words[-1] == _fnv(st[0].tobytes()), case
        saturated += int((rec["flags"] & em.W_SATURATED).astype(bool).sum())
    assert saturated > 0


def test_rule_program_under_address_and_undefined_sanitizers(rule_driver):
    """the stand-alone driver (its own main, nothing of it loaded into Python) built with -fsanitize=address,undefined: the same input,
    the same output, no report"""
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = rule_driver["dir"] / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(rule_driver["dir"] / "probe")], capture_output=True, timeout=300).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")            # decided on a trivial program: an error in the driver fails below
    exe = str(rule_driver["dir"] / "ec_rule_driver_san")
    rule_driver["build"](exe, san)
    r = subprocess.run([exe], input=rule_driver["input"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.splitlines() == rule_driver["out"]
