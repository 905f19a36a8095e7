"""-m "not gpu": the geometry of igdsp_cng_run (cng_route in csrc/igdsp_route.h), compiled with g++ alone through
tests/route/cng_route_driver.cpp: a lane owns a channel, a block is one wave and 64 channels; the grid covers every channel; a pass of
the wave over the tile visits every 16-byte piece of every row once, the multiplier that stands for the division by the pieces per row
is exact for every item, a piece stays inside its row and the row inside the LDS asked for, which with the byte per row behind the
tile is the kernel's; the resident blocks' LDS fits a CU; the instantiation k_cng<IN, COPY> follows the voice input and the entry.
Shapes that are not the kernel's launch nothing."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
NS = list(range(16, 257, 8))
KINDS = [(g, p, y) for g, p in ((0, 0), (1, 0), (0, 1)) for y in (0, 1)]
CASES = ([(1, 1, n, g, p, y) for n in NS for g, p, y in KINDS] +
         [(C, F, 160, g, p, y) for C in (1, 2, 63, 64, 65, 127, 128, 129, 4096, 65536) for F in (1, 128) for g, p, y in KINDS] +
         [(0xFFFFFFDF, 1, 160, 1, 0, 0), (1 << 28, 15, 16, 0, 0, 0)])
NOTHING = [(0, 5, 160, 1, 0, 0), (5, 0, 160, 1, 0, 0), (5, 5, 0, 1, 0, 0), (5, 5, 8, 1, 0, 0), (5, 5, 20, 0, 1, 0), (5, 5, 161, 0, 0, 0), (5, 5, 264, 1, 0, 0),
           (1 << 28, 16, 160, 1, 0, 0)]
FIELDS = "grid threads lds in copy pieces passes inv visited exact row_hi tile_hi who_hi top_chan chans resident vgprs".split()


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("cng_route") / "cng_route_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "cng_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    cases = CASES + NOTHING
    r = subprocess.run([exe], input="\n".join(" ".join(map(str, c)) for c in cases) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [dict(zip(FIELDS, map(int, line.split()))) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return dict(zip(cases, out))


def test_geometry(routes):
    for case in CASES:
        C, F, n, g, p, y = case
        r = routes[case]
        assert r["chans"] == 64 and r["threads"] == 64 and r["resident"] == 4 and r["vgprs"] == 128, case
        assert r["grid"] == -(-C // 64) and (r["grid"] - 1) * 64 < C <= r["grid"] * 64, case                   # every channel, no idle block
        assert C - 1 <= r["top_chan"] < C + 64, case                         # the last lane's channel: at or past the end, which the kernel masks
        assert r["pieces"] == n // 8 <= 32 and r["passes"] == r["pieces"] and r["visited"] == 64 * r["pieces"] and r["exact"] == 1, case
        stride = n // 2 + 1                                                  # dwords between rows: odd
        assert stride % 2 == 1 and r["row_hi"] == n // 2 < stride and r["tile_hi"] == 4 * (63 * stride + n // 2) <= 4 * 64 * stride, case
        assert r["lds"] == r["who_hi"] == 4 * 64 * stride + 64 and r["resident"] * r["lds"] <= 160 * 1024, case
        assert r["inv"] == (1 << 20) // r["pieces"] + 1 and (64 * r["pieces"] - 1) * r["inv"] < 1 << 32, case   # the product stays in 32 bits


def test_instantiation_follows_voice_input_and_entry(routes):
    for case in CASES:
        assert (routes[case]["in"], routes[case]["copy"]) == (1 if case[3] else (2 if case[4] else 0), case[5]), case


def test_nothing_to_launch(routes):
    for case in NOTHING:
        assert routes[case]["grid"] == 0 and routes[case]["threads"] == 0 and routes[case]["lds"] == 0, case
