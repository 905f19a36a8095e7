"""-m "not gpu": the geometry of igdsp_tone_detect (tdet_route in csrc/igdsp_route.h), compiled with g++ alone through
tests/route/tdet_route_driver.cpp: a block of 8 waves owns 32 channels (16 lanes each), the grid covers every channel, n % 8 and n % 4 pick the
kernel's instantiation, the LDS holds one plan's table (16 lanes x n / 4 entries of 16 bytes, sized for n = 256) and per channel
128 values of history with room for a frame of 256 behind them, d_work holds the counts of every (frame, 64 channels) behind the link
stage's 16-byte head and, when there is no d_rec, the records behind those.  Shapes that are not the kernel's launch nothing.
The rule itself (csrc/igdsp_tdet.h) runs as a program of its own through tests/route/tdet_rule_driver.cpp over full-scale rows and
garbage states, is compared with tests/tdet_model.py, and is built once more with -fsanitize=address,undefined and run over the same
input."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
NS = list(range(2, 257, 2))
CASES = ([(1, 1, n, 1, 1) for n in NS] + [(C, F, 160, li, wr) for C in (1, 31, 32, 33, 63, 64, 65, 67, 4096, 65536) for F in (1, 5, 128) for li in (0, 1) for wr in (0, 1)]
         + [(0xFFFFFFDF, 1, 160, 1, 0), (1 << 28, 15, 2, 1, 1)])
NOTHING = [(0, 5, 160, 1, 1), (5, 0, 160, 1, 1), (5, 5, 0, 1, 1), (5, 5, 161, 1, 1), (5, 5, 258, 1, 1), (1 << 28, 16, 160, 1, 1)]
FIELDS = "grid threads lds e0 waves list_grid counts_bytes work_bytes last_store last_move tab_entries counts_end rec_end buf chans".split()


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("tdet_route") / "tdet_route_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "tdet_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    cases = CASES + NOTHING
    r = subprocess.run([exe], input="\n".join(" ".join(map(str, c)) for c in cases) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [dict(zip(FIELDS, map(int, line.split()))) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return dict(zip(cases, out))


def test_geometry(routes):
    for case in CASES:
        C, F, n, li, wr = case
        r = routes[case]
        assert r["chans"] == 32 and r["threads"] == 16 * r["chans"] == 512
        assert r["grid"] == -(-C // 32) and r["grid"] * 32 >= C
        assert r["e0"] == (0 if n % 8 == 0 else 1 if n % 4 == 0 else 2)
        assert r["lds"] == 128 * 16 * 8 + 32 * r["buf"] * 2 + 32 * 4 and r["lds"] * 3 <= 160 * 1024          # three blocks per CU
        assert r["buf"] == 128 + 256 and r["last_store"] < r["buf"] and r["last_move"] < r["buf"] and r["tab_entries"] <= 64 * 16
        assert r["waves"] == -(-C // 64)
        if li:
            assert r["list_grid"] == -(-(F * r["waves"]) // 4)
            assert r["counts_bytes"] % 16 == 0 and r["counts_end"] <= r["counts_bytes"] < r["counts_end"] + 16
            assert r["work_bytes"] == r["rec_end"] == r["counts_bytes"] + (0 if wr else C * F * 8)
        else:
            assert r["list_grid"] == 0 and r["work_bytes"] == 0


def test_nothing_to_launch(routes):
    for case in NOTHING:
        assert routes[case]["grid"] == 0 and routes[case]["list_grid"] == 0, case


def test_work_bytes_is_the_routes(routes):
    from igate4xsoftphonedsp_amd import capi

    for case in CASES:
        C, F, n, li, wr = case
        if li:
            assert capi.tdet_work_bytes(C, F, bool(wr)) == routes[case]["work_bytes"], case


# ---- the rule as a program of its own, plain and under the sanitizers
RULE_CASES = [(n, frames, seed, garbage, plan) for n, frames in ((160, 6), (164, 5), (24, 12), (2, 40), (256, 4)) for plan in (0, 1, 2, 3)
              for seed, garbage in ((7 + n, 0), (11 + n, 1))]


def _xorshift_rows(n, frames, seed, garbage):
    """the driver's sequence: (the state's bytes or None, rows [frames][n])"""
    import numpy as np

    s = seed or 1

    def nxt():
        nonlocal s
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        return s

    state = bytes(nxt() & 0xFF for _ in range(264)) if garbage else None
    rows = np.zeros((frames, n), np.int16)
    for f in range(frames):
        for i in range(n):
            r = nxt()
            rows[f, i] = -32768 if (r & 0x30000) == 0 else np.array(r & 0xFFFF, np.uint16).astype(np.int16)
    return state, rows


@pytest.fixture(scope="module")
def rule_driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("tdet_rule")

    def build(exe, extra=()):
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        os.path.join(ROOT, "tests", "route", "tdet_rule_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)

    exe = str(d / "tdet_rule_driver")
    build(exe)
    text = "\n".join(" ".join(map(str, c)) for c in RULE_CASES) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(dir=d, build=build, input=text, out=r.stdout.splitlines())


def test_rule_program_matches_the_model(rule_driver):
    """tdet_frame_run compiled by g++ alone over full-scale rows (-32768 among them) and garbage states: the model's records and state"""
    import numpy as np

    from tests import tdet_model as tm

    plans = [tm.plan_dtmf(), tm.plan_8x8(), tm.plan_single(1000), tm.plan_single(3999)]
    assert len(rule_driver["out"]) == len(RULE_CASES)
    for case, line in zip(RULE_CASES, rule_driver["out"]):
        n, frames, seed, garbage, plan = case
        state, rows = _xorshift_rows(n, frames, seed, garbage)
        st = np.frombuffer(state, tm.STATE).copy() if state else None
        rec, st = tm.detect(plans[plan], rows[:, None, :], st)
        words = line.split()
        assert [int(w, 16) for w in words[:-1]] == [int(v) for v in rec[:, 0].view("<u8")], case
        h = 1469598103934665603
        for b in st[0].tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        assert int(words[-1], 16) == h, case


def test_rule_program_under_address_and_undefined_sanitizers(rule_driver):
    """the stand-alone driver (its own main, nothing of it loaded into Python) built with -fsanitize=address,undefined: the same input,
    the same output, no report"""
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = rule_driver["dir"] / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(rule_driver["dir"] / "probe")], capture_output=True, timeout=300).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")            # decided on a trivial program: an error in the driver fails below
    exe = str(rule_driver["dir"] / "tdet_rule_driver_san")
    rule_driver["build"](exe, san)
    r = subprocess.run([exe], input=rule_driver["input"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.splitlines() == rule_driver["out"]
