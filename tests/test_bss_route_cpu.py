"""-m "not gpu": the routes of igdsp_bss_select (bss_route in csrc/igdsp_route.h), compiled with g++ through tests/route/route_driver.cpp
(entry "bss"): form, groups per wave, grid, block size and the split into parts of kBssPart = 128 frames, at the issue's shapes.  The
GPU tests check outputs, not which geometry produced them; this table pins the geometry."""
import shutil

import pytest

from tests import route_util

CASES = [
    # 65 536 channels in 16 384 groups of 4 x 128 frames: 16 groups (64 member slots) per wave, 4 waves per block, one part
    ("G=16384 F=128 members=65536", "form=0 gpw=16 vec_in=1 vec_out=1 grid=256 threads=256 part_frames=128 parts=1 words_grid=256"),
    # the real-time shape
    ("G=16384 F=2 members=65536", "form=0 gpw=16 grid=256 threads=256 part_frames=2 parts=1 words_grid=256"),
    # the reference's one group of 4
    ("G=1 F=2 members=4", "form=0 gpw=16 grid=1 threads=256 part_frames=2 parts=1 words_grid=1"),
    # skew: one group of 1 024 + 16 128 groups of 4 -> 5 slots per group on average: 8 groups per wave
    ("G=16129 F=128 members=65536", "gpw=8 grid=505 threads=256 parts=1"),
    # groups of 8 and of 2
    ("G=8192 F=128 members=65536", "gpw=8 grid=256"),
    ("G=32768 F=128 members=65536", "gpw=16 grid=512"),
    # one group of more than 64 members: a wave per group
    ("G=16 F=128 members=4096", "gpw=1 grid=4"),
    # more frames than a part: parts of 128 frames, the last one takes the rest
    ("G=16384 F=300 members=65536", "part_frames=128 parts=3"),
    # PCM in, misaligned rows: scalar paths; no audio: no vector paths
    ("G=4 F=8 members=16 form=1 in=0x1004 out=0x1002", "form=1 vec_in=0 vec_out=0"),
    ("G=4 F=8 n=37 members=16", "vec_in=0 vec_out=0"),
    ("G=4 F=8 members=16 form=2", "form=2 vec_in=0 vec_out=0 grid=1"),
    # no member slots: no words pass; nothing to do
    ("G=4 F=8 members=0", "gpw=16 words_grid=0 grid=1"),
    ("G=0 F=8 members=0", "grid=0 parts=0"),
]


@pytest.fixture(scope="module")
def routes():
    return dict(zip((case for case, _ in CASES), route_util.run(["bss " + case for case, _ in CASES])))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("case,expected", CASES, ids=[c for c, _ in CASES])
def test_bss_route(routes, case, expected):
    got = routes[case]
    want = dict(kv.split("=") for kv in expected.split())
    assert {k: got[k] for k in want} == want, f"{case}: {got}"
