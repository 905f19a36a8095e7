"""-m "not gpu": the routes of igdsp_spectrum (spec_route in csrc/igdsp_route.h) and the rule that k_spec and igdsp_spec_frame share
(csrc/igdsp_spec.h), compiled with g++ through tests/route/spec_route_driver.cpp.  The route table pins the geometry (a wave per channel,
four to a block, the LDS of a block); the data flow's index functions are checked over all lanes and registers, with the bank spread of
both exchanges; the frame rule is run over cases from stdin and compared with tests/spec_model.py by its comparison rule; the same driver
is built once more with -fsanitize=address,undefined and run over the same input as its own program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import spec_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")

ROUTES = [
    # the bench's shapes
    ("C=65536 F=128 n=160", "grid=16384 threads=256 lds=26624"), ("C=65536 F=1 n=160", "grid=16384 threads=256 lds=26624"),
    # one wave, a partial block, a block plus one
    ("C=1 F=1", "grid=1 threads=256"), ("C=3 F=7", "grid=1"), ("C=4 F=7", "grid=1"), ("C=5 F=13", "grid=2"), ("C=64 F=13", "grid=16"),
    ("C=65537 F=2", "grid=16385"),
    # no parts: any number of frames is one launch
    ("C=3 F=100000", "grid=1"),
    # the frame sizes
    ("C=33 F=40 n=1", "grid=9"), ("C=33 F=40 n=24", "grid=9"), ("C=33 F=40 n=164", "grid=9"), ("C=33 F=40 n=256", "grid=9"),
    # the largest C does not wrap; what the argument rule rejects launches nothing here either
    ("C=0xFFFFFFDF F=1", "grid=1073741816"),
    ("C=0xFFFFFFE0 F=1", "grid=0"), ("C=0x10000000 F=16", "grid=0"), ("C=3 F=1 n=0", "grid=0"), ("C=3 F=1 n=257", "grid=0"),
    ("C=0 F=8", "grid=0 threads=0 lds=0"), ("C=8 F=0", "grid=0 threads=0 lds=0"),
]

# (n, frames, hop, alpha, input)
FRAMES = [(160, 9, 1, 0.25, "ulaw"), (164, 9, 2, 0.25, "alaw"), (24, 50, 7, 0.5, "ulaw"), (256, 6, 1, 1.0, "alaw"), (1, 40, 13, 0.25, "lsb"),
          (160, 8, 1, 0.25, "line65"), (160, 7, 1, 0.25, "zero"), (160, 9, 20, 0.25, "ulaw")]


def frames_input(i):
    n, F_, _, _, kind = FRAMES[i]
    if kind in ("ulaw", "alaw"):
        return sm.decode(sm.noise_codes(300 + i, F_, n)[:, None, :], [8 if kind == "alaw" else 0])[:, 0]
    if kind == "lsb":
        return sm.lsb_noise(300 + i, F_, n)
    return np.zeros((F_, n), np.int16) if kind == "zero" else sm.sine(65, F_, n, 12000.0, 0.3)


def build(exe, extra):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "spec_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("spec_route")
    exe = str(d / "spec_route_driver")
    build(exe, [])
    lines = ["static", "flow"] + ["route " + c for c, _ in ROUTES]
    for i, (n, _, hop, alpha, _) in enumerate(FRAMES):
        lines.append(f"frames n={n} hop={hop} alpha={alpha} x={','.join(map(str, frames_input(i).reshape(-1)))}")
    text = "\n".join(lines) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return {"dir": d, "input": text, "out": r.stdout.splitlines()}


@pytest.mark.parametrize("i", range(len(ROUTES)), ids=[c for c, _ in ROUTES])
def test_spec_route(driver, i):
    assert driver["out"][0] == "ok=1"
    got = dict(kv.split("=") for kv in driver["out"][2 + i].split())
    want = dict(kv.split("=") for kv in ROUTES[i][1].split())
    assert {k: got[k] for k in want} == want, f"{ROUTES[i][0]}: {got}"


def test_data_flow_and_bank_spread(driver):
    """every exchange is a permutation of the tile's 512 used slots, the mirror pairs bin k with 512 - k; the padded rows keep the first
    exchange and the second one's loads conflict-free (one lane of a 32-lane group per bank) and the second one's stores at two"""
    got = dict(kv.split("=") for kv in driver["out"][1].split())
    assert got["ok"] == "1"
    assert (int(got["x1_store"]), int(got["x1_load"]), int(got["x2_load"])) == (1, 1, 1) and int(got["x2_store"]) <= 2, got


def test_frame_rule_vs_model(driver):
    at = 2 + len(ROUTES)
    fl = lambda s: np.float32(float.fromhex(s))
    hopped = 0
    for i, (n, F_, hop, alpha, kind) in enumerate(FRAMES):
        rows = frames_input(i)
        ref = sm.reference(rows, hop, alpha)
        rec = dict(flags=np.zeros(F_, np.uint16), peak_bin=np.zeros(F_, np.uint16), peak_db=np.zeros(F_, np.float32))
        raws = {}
        for f in range(F_):
            t = driver["out"][at].split()
            at += 1
            rec["flags"][f], rec["peak_bin"][f], rec["peak_db"][f] = int(t[0]), int(t[1]), fl(t[2])
            assert len(t) == (3 + 512 if rec["flags"][f] else 3)
            if rec["flags"][f]:
                raws[len(raws)] = np.array([fl(v) for v in t[3:]], np.float32)
        t = driver["out"][at].split()
        at += 1
        assert [int(v) for v in t[:3]] == [F_ % hop, F_ // hop, 1], i
        np.testing.assert_array_equal(np.array(t[3:3 + 1024], np.int64), ref["r64"]["state"]["hist"])
        avg = np.array([fl(v) for v in t[3 + 1024:]], np.float32)
        assert len(avg) == 512
        sm.check(ref, raws, avg, rec, f"driver case {i} ({kind})")
        hopped += len(raws)
    assert at == len(driver["out"]) and hopped > 30


def test_driver_under_address_and_undefined_sanitizers(driver):
    """the stand-alone driver (its own main, nothing of it loaded into Python) built with -fsanitize=address,undefined: the same input,
    the same output, no report"""
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = driver["dir"] / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(driver["dir"] / "probe")], capture_output=True, timeout=300).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")            # decided on a trivial program: an error in the driver fails below
    exe = str(driver["dir"] / "spec_route_driver_san")
    build(exe, san)
    r = subprocess.run([exe], input=driver["input"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.splitlines() == driver["out"]
