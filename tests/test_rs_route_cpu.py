"""-m "not gpu": the routes of igdsp_resample (rs_route in csrc/igdsp_route.h) and the constexpr rules that k_rs and igdsp_rs_frame share,
compiled with g++ through tests/route/rs_route_driver.cpp.  The route table pins the geometry (the form, the units of a row, the channel
groups of 16 / 4, the frame chunks that give a wave about four items, the blocks a CU holds and the grid sized for them, the LDS of a
block, k_rs_state's grid); the packed tap pairs and the
frame rule are run over cases from stdin and compared with tests/rs_model.py; the same driver is built once more with
-fsanitize=address,undefined and run over the same input as its own program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import rs_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")

ROUTES = [
    # the bench's shape.  UP: 3 blocks of 4 waves per CU (the LDS), 4 096 groups cut into 3 chunks of frames = 4 items per wave;
    # DOWN by 6: 2 blocks per CU, 8 items per wave without a cut
    ("dir=0 R=6 C=65536 F=128 n=160", "vec=1 pieces=20 ch=16 groups=4096 chunk_frames=43 chunks=3 grid=768 threads=256 lds=43008 state_grid=2048 resident=3"),
    ("dir=1 R=6 C=65536 F=128 n=160", "vec=1 pieces=20 ch=4 groups=16384 chunk_frames=128 chunks=1 grid=512 lds=55296 resident=2"),
    ("dir=0 R=2 C=65536 F=128", "lds=38912 resident=3"), ("dir=0 R=3 C=65536 F=128", "lds=39936 resident=3"),
    ("dir=0 R=4 C=65536 F=128", "lds=40960 resident=3"), ("dir=1 R=2 C=65536 F=128", "lds=18432 grid=768 resident=3"),
    ("dir=1 R=3 C=65536 F=128", "lds=27648 resident=3"), ("dir=1 R=4 C=65536 F=128", "lds=36864 resident=3"),
    ("dir=0 R=2 C=65536 F=128 yardstick=1", "vec=1 chunks=3 grid=768 state_grid=0"),
    # the knob of the sweep: blocks per CU of the grid, and the cut that goes with it
    ("dir=0 R=6 C=65536 F=128 blocks=1", "chunk_frames=128 chunks=1 grid=256"), ("dir=0 R=6 C=65536 F=128 blocks=2", "chunk_frames=64 chunks=2 grid=512"),
    ("dir=0 R=6 C=65536 F=128 blocks=4", "chunk_frames=32 chunks=4 grid=1024"), ("dir=0 R=6 C=65536 F=128 blocks=0", "grid=768"),
    ("dir=0 R=6 C=65536 F=128 blocks=9", "grid=768"),
    # few channels: the frames are cut so that every wave has items
    ("dir=0 R=2 C=1 F=1", "groups=1 chunk_frames=1 chunks=1 grid=1 state_grid=1"),
    ("dir=0 R=2 C=17 F=7 n=25", "vec=0 pieces=4 groups=2 chunk_frames=1 chunks=7 grid=4 state_grid=17"),
    ("dir=1 R=3 C=17 F=7", "ch=4 groups=5 chunk_frames=1 chunks=7 grid=9"),
    ("dir=0 R=2 C=32805 F=3", "groups=2051 chunk_frames=1 chunks=3 grid=768"),
    ("dir=0 R=2 C=32805 F=9", "groups=2051 chunk_frames=2 chunks=5 grid=768"),
    ("dir=1 R=2 C=8229 F=7 n=8", "pieces=1 groups=2058 chunk_frames=2 chunks=4 grid=768"),
    ("dir=0 R=2 C=1024 F=100 cus=4", "groups=64 chunk_frames=34 chunks=3 grid=12 state_grid=32"),
    ("dir=0 R=2 C=1000 F=100 cus=4", "groups=63 chunk_frames=25 chunks=4 grid=12"),
    # the units of a row; the general form: n no multiple of 8, or a base off its alignment (16 bytes; a G.711 input: 8)
    ("dir=0 R=2 C=3 F=1 n=256", "vec=1 pieces=32"), ("dir=0 R=2 C=3 F=1 n=8", "vec=1 pieces=1"), ("dir=0 R=2 C=3 F=1 n=1", "vec=0 pieces=1"),
    ("dir=1 R=6 C=3 F=1 n=255", "vec=0 pieces=32"), ("dir=0 R=2 C=3 F=1 n=164", "vec=0 pieces=21"),
    ("dir=0 R=2 C=3 F=1 in=0x1002", "vec=0"), ("dir=0 R=2 C=3 F=1 in=0x1008", "vec=0"), ("dir=0 R=2 C=3 F=1 in=0x1008 g711=1", "vec=1"),
    ("dir=0 R=2 C=3 F=1 in=0x1004 g711=1", "vec=0"), ("dir=0 R=2 C=3 F=1 out=0x2008", "vec=0"), ("dir=0 R=2 C=3 F=1 out=0", "vec=1"),
    ("dir=0 R=2 C=3 F=1 in=0x1010 out=0x2010", "vec=1"),
    # the largest C does not wrap; what the argument rule rejects launches nothing here either
    ("dir=0 R=2 C=0xFFFFFFDF F=1", "groups=268435454 chunks=1 grid=768"),
    ("dir=0 R=2 C=0xFFFFFFE0 F=1", "grid=0"), ("dir=0 R=2 C=3 F=1 n=257", "grid=0"), ("dir=0 R=2 C=3 F=1 n=0", "grid=0"),
    ("dir=0 R=5 C=3 F=1", "grid=0"), ("dir=2 R=2 C=3 F=1", "grid=0"), ("dir=1 R=2 C=3 F=1 g711=1", "grid=0"),
    ("dir=0 R=2 C=0 F=8", "groups=0 grid=0 threads=0"), ("dir=0 R=2 C=8 F=0", "groups=0 grid=0 threads=0"),
]

# (direction, R, n_in, frames): the history spans several frames at the small sizes
FRAMES = [(d, R, n * (R if d == rm.DOWN else 1), f) for d in (rm.UP, rm.DOWN) for R in rm.FACTORS for n, f in ((1, 30), (7, 9), (8, 7), (25, 7), (160, 2))]
FRAMES += [(rm.UP, 6, 256, 2), (rm.DOWN, 6, 1536, 2), (rm.DOWN, 3, 765, 2)]


def frame_input(i, n):
    rng = np.random.default_rng(1000 + i)
    kind = i % 4
    x = rng.integers(-32768, 32768, n) if kind < 2 else (rng.choice([-32768, 32767], n) if kind == 2 else np.full(n, -32768))
    return x, rng.integers(-32768, 32768, 144)


def build(exe, extra):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "rs_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("rs_route")
    exe = str(d / "rs_route_driver")
    build(exe, [])
    lines = ["static"] + ["route " + c for c, _ in ROUTES] + [f"pairs dir={dr} R={R}" for dr in (rm.UP, rm.DOWN) for R in rm.FACTORS]
    for i, (dr, R, n_in, f) in enumerate(FRAMES):
        x, h = frame_input(i, n_in * f)
        lines.append(f"frames dir={dr} R={R} n_in={n_in} hist={','.join(map(str, h))} x={','.join(map(str, x))}")
    text = "\n".join(lines) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return {"dir": d, "input": text, "out": r.stdout.splitlines()}


@pytest.mark.parametrize("i", range(len(ROUTES)), ids=[c for c, _ in ROUTES])
def test_rs_route(driver, i):
    assert driver["out"][0] == "ok=1"
    got = dict(kv.split("=") for kv in driver["out"][1 + i].split())
    want = dict(kv.split("=") for kv in ROUTES[i][1].split())
    assert {k: got[k] for k in want} == want, f"{ROUTES[i][0]}: {got}"


def test_tap_pairs_vs_model(driver):
    """window sample t0 (oldest first) in the low half, t0 + 1 in the high half: the tap of window sample t is U[p][23 - t] / D[N - 1 - t]"""
    at = 1 + len(ROUTES)
    for dr in (rm.UP, rm.DOWN):
        for R in rm.FACTORS:
            got = np.array(driver["out"][at].split(), np.uint64)
            at += 1
            tabs = rm.up_table(R)[:, ::-1] if dr == rm.UP else rm.down_table(R)[None, ::-1]
            want = np.concatenate([(t[0::2] & 0xFFFF) | ((t[1::2] & 0xFFFF) << 16) for t in tabs])
            np.testing.assert_array_equal(got, want.astype(np.uint64))


def test_frame_rule_vs_model(driver):
    at = 1 + len(ROUTES) + 2 * len(rm.FACTORS)
    for i, (dr, R, n_in, f) in enumerate(FRAMES):
        x, h = frame_input(i, n_in * f)
        raw, new_hist = rm.convert(dr, R, x[None, :], h[None, :])
        n_out = n_in * R if dr == rm.UP else n_in // R
        raw = raw.reshape(f, n_out)
        for k in range(f):
            got = [int(v) for v in driver["out"][at].split()]
            at += 1
            assert got[0] == int((rm.clamp(raw[k]) != raw[k]).any()) and got[1] == k + 1, (i, k)
            assert got[2:] == rm.clamp(raw[k]).tolist(), (i, k)
        assert [int(v) for v in driver["out"][at].split()] == new_hist[0].tolist()
        at += 1
    assert at == len(driver["out"])


def test_driver_under_address_and_undefined_sanitizers(driver):
    """the stand-alone driver (its own main, nothing of it loaded into Python) built with -fsanitize=address,undefined: the same input,
    the same output, no report"""
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = driver["dir"] / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(driver["dir"] / "probe")], capture_output=True, timeout=300).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")            # decided on a trivial program: an error in the driver fails below
    exe = str(driver["dir"] / "rs_route_driver_san")
    build(exe, san)
    r = subprocess.run([exe], input=driver["input"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.splitlines() == driver["out"]
