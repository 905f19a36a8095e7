"""-m "not gpu": the routes of igdsp_ptt_arbitrate (ptt_route in csrc/igdsp_route.h), compiled with g++ through
tests/route/ptt_route_driver.cpp: form, groups per wave, grid, block size, the split into parts of kPttPart = 128 frames and the frames
a wave of average width takes per pass (kPttOps = 4 096 ops in LDS).  The GPU tests check outputs, not which geometry produced them;
this table pins the geometry."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")

CASES = [
    # 65 536 legs in 16 384 groups of 4 x 128 frames: 16 groups (64 slots) per wave, 4 waves per block, one part, two passes of 64 frames
    ("G=16384 F=128 members=65536", "form=0 gpw=16 vec_in=1 vec_out=1 grid=256 threads=256 part_frames=128 parts=1 pass_frames=64 slots_grid=256"),
    # the real-time shape
    ("G=16384 F=2 members=65536", "form=0 gpw=16 grid=256 threads=256 part_frames=2 parts=1 pass_frames=2 slots_grid=256"),
    # one group of 4
    ("G=1 F=2 members=4", "gpw=16 grid=1 threads=256 part_frames=2 parts=1 slots_grid=1"),
    # groups of 8 and of 2: 64 and 32 slots per wave; a window is at least one chunk of 64 slots, so 64 frames a pass either way
    ("G=8192 F=128 members=65536", "gpw=8 grid=256 pass_frames=64"),
    ("G=32768 F=128 members=65536", "gpw=16 grid=512 pass_frames=64"),
    # wide groups: a wave per group; 256 slots -> 16 frames a pass; more slots than the ops window -> a frame at a time
    ("G=16 F=128 members=4096", "gpw=1 grid=4 pass_frames=16"),
    ("G=2 F=128 members=20000", "gpw=1 grid=1 pass_frames=1"),
    # more frames than a part: parts of 128 frames, the last one takes the rest
    ("G=16384 F=300 members=65536", "part_frames=128 parts=3"),
    # PCM in, misaligned rows: scalar paths; odd n; no audio: no vector paths
    ("G=4 F=8 members=16 form=1 in=0x1004 out=0x1002", "form=1 vec_in=0 vec_out=0"),
    ("G=4 F=8 members=16 form=1 in=0x1008 out=0x1008", "form=1 vec_in=1 vec_out=1"),
    ("G=4 F=8 members=16 form=0 in=0x1004 out=0x1004", "form=0 vec_in=1 vec_out=0"),
    ("G=4 F=8 n=37 members=16", "vec_in=0 vec_out=0"),
    ("G=4 F=8 members=16 form=2", "form=2 vec_in=0 vec_out=0 grid=1"),
    # no member slots: no slot pass; nothing to do
    ("G=4 F=8 members=0", "gpw=16 slots_grid=0 grid=1 pass_frames=8"),
    ("G=0 F=8 members=0", "grid=0 parts=0 slots_grid=0"),
    ("G=8 F=0 members=32", "grid=0 parts=0"),
]


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("ptt_route") / "ptt_route_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "ptt_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], input="\n".join(c for c, _ in CASES) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(CASES)
    return {c: dict(kv.split("=") for kv in line.split()) for (c, _), line in zip(CASES, out)}


@pytest.mark.parametrize("case,expected", CASES, ids=[c for c, _ in CASES])
def test_ptt_route(routes, case, expected):
    got = routes[case]
    want = dict(kv.split("=") for kv in expected.split())
    assert {k: got[k] for k in want} == want, f"{case}: {got}"
