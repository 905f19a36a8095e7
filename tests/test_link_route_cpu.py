"""-m "not gpu": the routes of igdsp_link_watch (link_route and link_work_bytes in csrc/igdsp_route.h), compiled with g++ through
tests/route/link_route_driver.cpp: waves of 64 channels, grid, block size, the split into parts of kLinkPart = 128 ticks, one walk per
part without a list and two (count, scan, write) with one, and the bytes of d_work.  The GPU tests check outputs, not which geometry
produced them; this table pins the geometry."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")

CASES = [
    # 65 536 legs x 128 ticks: a lane per leg, 1 024 waves in 256 blocks of 4, one part; the counts are 128 x 1 024 words
    ("C=65536 T=128 list=1", "waves=1024 grid=256 threads=256 part_ticks=128 parts=1 passes=2 scan_threads=1024 work_bytes=524304 work=524304"),
    # no list: one walk, no scan, no work
    ("C=65536 T=128 list=0", "waves=1024 grid=256 threads=256 parts=1 passes=1 scan_threads=0 work_bytes=0 work=524304"),
    # the real-time shape
    ("C=65536 T=2 list=1", "waves=1024 grid=256 part_ticks=2 parts=1 passes=2 work_bytes=8208"),
    # one leg; a wave and one lane more; a block and one lane more
    ("C=1 T=1 list=1", "waves=1 grid=1 threads=256 part_ticks=1 parts=1 work_bytes=32"),
    ("C=65 T=1 list=1", "waves=2 grid=1 work_bytes=32"),
    ("C=257 T=3 list=1", "waves=5 grid=2 part_ticks=3 work_bytes=80"),
    ("C=4099 T=129 list=1", "waves=65 grid=17 part_ticks=128 parts=2 work_bytes=33296"),
    # more ticks than a part: parts of 128 ticks, the last one takes the rest; the work buffer is a part's
    ("C=65536 T=300 list=1", "part_ticks=128 parts=3 work_bytes=524304"),
    # the largest channel count does not wrap the wave count
    ("C=0xFFFFFFFF T=1 list=1", "waves=67108864 grid=16777216"),
    # nothing to do
    ("C=0 T=8 list=1", "grid=0 parts=0 passes=0 work_bytes=0 work=16"),
    ("C=8 T=0 list=1", "grid=0 parts=0 passes=0 work=16"),
]


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("link_route") / "link_route_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "link_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], input="\n".join(c for c, _ in CASES) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(CASES)
    return {c: dict(kv.split("=") for kv in line.split()) for (c, _), line in zip(CASES, out)}


@pytest.mark.parametrize("case,expected", CASES, ids=[c for c, _ in CASES])
def test_link_route(routes, case, expected):
    got = routes[case]
    want = dict(kv.split("=") for kv in expected.split())
    assert {k: got[k] for k in want} == want, f"{case}: {got}"
