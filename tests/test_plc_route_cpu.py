"""-m "not gpu": the routes of igdsp_plc_conceal (plc_route in csrc/igdsp_route.h), compiled with g++ through tests/route/route_driver.cpp
(entry "plc"): 16 channels per wave and 4 waves per block, parts of kPlcPart = 128 ticks, 8-sample pieces in batches of whole rows, and
the 16-byte path, at the issue's shapes.  The GPU tests check outputs, not which geometry produced them; this table pins the geometry."""
import shutil

import pytest

from tests import route_util

CASES = [
    # P1 / P2: 65 536 channels x 128 ticks: 4 096 waves in 1 024 blocks, one part; 20 pieces a row, 12 rows (240 pieces) a batch
    ("C=65536 T=128", "vec=1 pieces=20 batch_rows=12 grid=1024 threads=256 part_ticks=128 parts=1"),
    # P3: a live gateway's per-tick call
    ("C=65536 T=1", "grid=1024 part_ticks=1 parts=1"),
    # odd channel counts: the last wave takes the rest
    ("C=17 T=7", "grid=1 parts=1"),
    ("C=4099 T=2", "grid=65"),
    # more ticks than a part
    ("C=16 T=300", "part_ticks=128 parts=3"),
    # frame sizes: rows of 1 .. 32 pieces
    ("C=16 T=8 n=1", "vec=0 pieces=1 batch_rows=256"),
    ("C=16 T=8 n=24", "vec=1 pieces=3 batch_rows=85"),
    ("C=16 T=8 n=164", "vec=0 pieces=21 batch_rows=12"),
    ("C=16 T=8 n=256", "vec=1 pieces=32 batch_rows=8"),
    # alignment: G.711 rows need 8 bytes, PCM rows 16, the output 16
    ("C=16 T=8 in=0x1008", "vec=1"),
    ("C=16 T=8 in=0x1008 pcm=1", "vec=0"),
    ("C=16 T=8 out=0x1008", "vec=0"),
    ("C=16 T=8 in=0x1004", "vec=0"),
    # nothing to do
    ("C=0 T=8", "grid=0 parts=0"),
    ("C=8 T=0", "grid=0 parts=0"),
]


@pytest.fixture(scope="module")
def routes():
    return dict(zip((case for case, _ in CASES), route_util.run(["plc " + case for case, _ in CASES])))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("case,expected", CASES, ids=[c for c, _ in CASES])
def test_plc_route(routes, case, expected):
    got = routes[case]
    want = dict(kv.split("=") for kv in expected.split())
    assert {k: got[k] for k in want} == want, f"{case}: {got}"
