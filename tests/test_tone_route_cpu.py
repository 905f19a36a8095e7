"""-m "not gpu": the routes of igdsp_tone_generate (tone_route in csrc/igdsp_route.h) and the constexpr tone rules that k_tone and
igdsp_tone_frame share, compiled with g++ through tests/route/tone_route_driver.cpp.  The route table pins the geometry (the form, the
pieces of a row, the port groups of 16, the frame chunks of a launch with few ports, who writes the state); the rules are run over
cases from stdin and compared with tests/tone_model.py; the same driver is built once more with -fsanitize=address,undefined and run
over the same input."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import tone_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")

ROUTES = [
    # the bench's shape: 65 536 ports = 4 096 groups = one per wave of 256 CUs x 16 waves: no chunks, the kernel writes the state
    ("P=65536 F=128 n=160", "mode=0 vec=1 pieces=20 groups=4096 chunk_frames=128 chunks=1 grid=256 threads=1024 state_grid=0 lds=4096"),
    ("P=65536 F=1 n=160", "groups=4096 chunk_frames=1 chunks=1 grid=256 state_grid=0"),
    ("P=131072 F=2 n=160", "groups=8192 chunks=1 grid=256"),
    # the single-output forms and the yardstick (no table, no state)
    ("P=65536 F=128 n=160 stats=0", "mode=1 vec=1"),
    ("P=65536 F=128 n=160 pcm=0 out=0", "mode=2 vec=1"),
    ("P=65536 F=128 n=160 yardstick=1", "mode=3 vec=1 state_grid=0 lds=0"),
    ("P=8 F=8 n=160 pcm=0 stats=0", "grid=0"),
    # few ports: the frames are cut so that every wave has an item, and k_tone_state writes the state
    ("P=1 F=1 n=160", "groups=1 chunk_frames=1 chunks=1 grid=1 state_grid=0"),
    ("P=1 F=128 n=160", "groups=1 chunk_frames=1 chunks=128 grid=8 state_grid=1"),
    ("P=16 F=7 n=160", "groups=1 chunk_frames=1 chunks=7 grid=1 state_grid=1"),
    ("P=17 F=5 n=160", "groups=2 chunk_frames=1 chunks=5 grid=1 state_grid=1"),
    ("P=257 F=7 n=160", "groups=17 chunks=7 grid=8 state_grid=2"),
    ("P=32768 F=128 n=160", "groups=2048 chunk_frames=64 chunks=2 grid=256 state_grid=128"),
    ("P=40000 F=128 n=160", "groups=2500 chunk_frames=64 chunks=2 grid=256"),
    ("P=1024 F=100 n=160 cus=4", "groups=64 chunk_frames=100 chunks=1 grid=4 state_grid=0"),
    ("P=1000 F=100 n=160 cus=4", "groups=63 chunk_frames=50 chunks=2 grid=4 state_grid=4"),
    # the pieces of a row; the general form: n no multiple of 8, or a base that is not 16-byte aligned
    ("P=3 F=1 n=256", "vec=1 pieces=32"),
    ("P=3 F=1 n=8", "vec=1 pieces=1"),
    ("P=3 F=1 n=1", "vec=0 pieces=1"),
    ("P=3 F=1 n=255", "vec=0 pieces=32"),
    ("P=3 F=1 n=164", "vec=0 pieces=21"),
    ("P=3 F=1 n=160 out=0x1002", "vec=0 pieces=20"),
    ("P=3 F=1 n=160 out=0x1008", "vec=0"),
    ("P=3 F=1 n=160 out=0x1010", "vec=1"),
    # the largest P does not wrap; what the argument rule rejects launches nothing here either
    ("P=0xFFFFFFDF F=1 n=160", "groups=268435454 chunks=1 grid=256"),
    ("P=0xFFFFFFE0 F=1 n=160", "grid=0"),
    ("P=3 F=1 n=257", "grid=0"),
    ("P=3 F=1 n=0", "grid=0"),
    ("P=0 F=8 n=160", "groups=0 grid=0 threads=0"),
    ("P=8 F=0 n=160", "groups=0 grid=0 threads=0"),
]

RING = [(440, 480, 2000, 1000)]
EDGES = [(440, 480, 30, 10)]
EIGHT = [(350, 440, 37, 5), (480, 620, 20, 0), (1000, 0, 13, 7), (1400, 0, 5, 1), (697, 1209, 50, 50, 32767), (3999, 1, 9, 3, 1),
         (2600, 0, 0, 11), (941, 1633, 2, 2, 20000)]
# (tones, clock, options, pos, flags, cmd, n, frames)
FRAMES = [
    (RING, 8000, 1, 15900, 1, 0, 160, 3), (RING, 8000, 1, 23900, 1, 0, 160, 2), (EDGES, 8000, 1, 7, 1, 0, 160, 9), (EDGES, 16000, 1, 0, 1, 0, 255, 9),
    (EIGHT, 8000, 1, 100, 1, 0, 256, 12), (EIGHT, 48000, 3, 5000, 1, 0, 1, 40), (EDGES, 8000, 0, 0, 1, 0, 160, 4), ([(440, 480, 35, 5)], 8000, 0, 0, 1, 0, 160, 4),
    ([(1, 0, 0, 1)], 8000, 1, 3, 1, 0, 256, 2),                          # a cycle of 8 samples wraps 32 times in a row
    (EDGES, 8000, 1, 100, 1, 2, 160, 2), (EDGES, 8000, 1, 100, 0, 1, 160, 2), (EDGES, 8000, 1, 100, 1, 3, 160, 2), (EDGES, 8000, 1, 100, 0, 5, 160, 2),
    (EDGES, 8000, 1, 100, 1, 4, 160, 2), (EDGES, 8000, 1, 0xFFFFFF00, 1, 0, 160, 2), (EDGES, 8000, 0, 0xFFFFFF00, 1, 0, 160, 2),
]


def frames_line(c):
    tones, clock, options, pos, flags, cmd, n, frames = c
    ts = ",".join(":".join(str(v) for v in (tuple(t) + (0,))[:5]) for t in tones)
    return f"frames clock={clock} options={options} tones={ts} pos={pos} flags={flags} cmd={cmd} n={n} frames={frames}"


def sample_cases():
    out = []
    for sg in tm.plan_build(EIGHT, 8000, 1)["seg"] + tm.plan_build(RING, 48000, 1)["seg"] + tm.plan_build(EDGES, 16000, 3)["seg"]:
        if sg["on"]:
            out.append(sg)
    return out


def build(exe, extra):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "tone_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("tone_route")
    exe = str(d / "tone_route_driver")
    build(exe, [])
    lines = ["static"] + ["route " + c for c, _ in ROUTES] + [frames_line(c) for c in FRAMES]
    lines += [f"sample step1={sg['step1']} step2={sg['step2']} vol={sg['vol']} on={sg['on']} fade_in={sg['fade_in']} fade_out={sg['fade_out']} k0=0 "
              f"count={sg['on']}" for sg in sample_cases()]
    text = "\n".join(lines) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return {"dir": d, "input": text, "out": r.stdout.splitlines()}


@pytest.mark.parametrize("i", range(len(ROUTES)), ids=[c for c, _ in ROUTES])
def test_tone_route(driver, i):
    assert driver["out"][0] == "ok=1"
    got = dict(kv.split("=") for kv in driver["out"][1 + i].split())
    want = dict(kv.split("=") for kv in ROUTES[i][1].split())
    assert {k: got[k] for k in want} == want, f"{ROUTES[i][0]}: {got}"


def test_frame_rules_vs_model(driver):
    at = 1 + len(ROUTES)
    for c in FRAMES:
        tones, clock, options, pos, flags, cmd, n, frames = c
        plan = tm.plan_build(tones, clock, options)
        p, fl = np.array([pos]), np.array([flags])
        for f in range(frames):
            pcm, ln, _, p, fl = tm.generate([plan], None, [cmd if f == 0 else 0], p, fl, 1, n)
            got = [int(v) for v in driver["out"][at].split()]
            at += 1
            assert got[:3] == [int(ln[0, 0]), int(p[0]), int(fl[0])], (c, f)
            assert got[3:] == pcm[0, 0].tolist(), (c, f)


def test_sample_rule_vs_model(driver):
    at = 1 + len(ROUTES) + sum(c[7] for c in FRAMES)
    for sg in sample_cases():
        got = np.array(driver["out"][at].split(), np.int64)
        at += 1
        np.testing.assert_array_equal(got, tm.seg_on(sg))
    assert at == len(driver["out"])


def test_driver_under_address_and_undefined_sanitizers(driver):
    """the stand-alone driver (its own main, nothing of it loaded into Python) built with -fsanitize=address,undefined: the same input,
    the same output, no report"""
    exe = str(driver["dir"] / "tone_route_driver_san")
    try:
        build(exe, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    except subprocess.CalledProcessError as e:
        if b"asan" in e.stderr or b"ubsan" in e.stderr or b"sanitize" in e.stderr:
            pytest.skip("the sanitizer runtimes are not installed")
        raise
    r = subprocess.run([exe], input=driver["input"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.splitlines() == driver["out"]
