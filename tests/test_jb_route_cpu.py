"""-m "not gpu": the routes of igdsp_jb_receive (jb_route in csrc/igdsp_route.h), compiled with g++ through tests/route/route_driver.cpp
(entry "jb"): 16 channels per wave and 4 waves per block, the split into parts of kJbPart = 128 ticks, the 16-byte store path and the
ring size, at the issue's shapes.  The GPU tests check outputs, not which geometry produced them; this table pins the geometry."""
import shutil

import pytest

from tests import route_util

CASES = [
    # J1 / J2: 65 536 channels x 128 ticks: 4 096 waves in 1 024 blocks, one part; ring 16 x (4 + 16 + 160) bytes per channel
    ("C=65536 T=128", "vec=1 pieces=10 grid=1024 threads=256 part_ticks=128 parts=1 ring=188743680"),
    # J3: the flush tick's shape
    ("C=65536 T=2", "grid=1024 part_ticks=2 parts=1"),
    # J4: the latency floor: one block, one wave with 4 channels
    ("C=4 T=1", "grid=1 threads=256 part_ticks=1 parts=1 ring=11520"),
    # odd channel counts: the last wave takes the rest
    ("C=37 T=200", "grid=1 part_ticks=128 parts=2"),
    ("C=65 T=129", "grid=2 parts=2"),
    # more ticks than a part: parts of 128 ticks, the last one takes the rest
    ("C=16 T=300", "part_ticks=128 parts=3"),
    # n not a multiple of 16, or a misaligned output: byte stores
    ("C=16 T=8 n=37", "vec=0 pieces=3 ring=17408"),
    ("C=16 T=8 out=0x1008", "vec=0 pieces=10"),
    ("C=16 T=8 n=256", "vec=1 pieces=16"),
    # nothing to do
    ("C=0 T=8", "grid=0 parts=0"),
    ("C=8 T=0", "grid=0 parts=0"),
]


@pytest.fixture(scope="module")
def routes():
    return dict(zip((case for case, _ in CASES), route_util.run(["jb " + case for case, _ in CASES])))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("case,expected", CASES, ids=[c for c, _ in CASES])
def test_jb_route(routes, case, expected):
    got = routes[case]
    want = dict(kv.split("=") for kv in expected.split())
    assert {k: got[k] for k in want} == want, f"{case}: {got}"
