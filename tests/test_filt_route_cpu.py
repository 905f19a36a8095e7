"""-m "not gpu": the geometry of igdsp_filt_run (filt_route in csrc/igdsp_route.h), compiled with g++ alone through
tests/route/filt_route_driver.cpp: a lane owns a channel, a block is one wave and 64 channels; the grid covers every channel; the early
and the late turns of the wave over the tile visit every 16-byte piece of every row once, the multiplier that stands for the division by
the pieces per row is exact for every item, a piece stays inside its row and the row inside the LDS asked for, which with the byte per
row behind the tile is the kernel's; a clamped fetch never leaves the block's rows; the resident blocks' LDS fits a CU; the
instantiation k_filt<IN, S, COPY> follows the input's form, max_sections and the entry.  Shapes that are not the kernel's launch nothing."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
NS = list(range(8, 257, 8))
KINDS = [(g, m, y) for g in (0, 1) for m in (0, 1, 2, 3, 4) for y in (0, 1)]
CASES = ([(1, 1, n, g, m, y) for n in NS for g, m, y in KINDS] +
         [(C, F, 160, g, m, y) for C in (1, 2, 63, 64, 65, 127, 128, 129, 4096, 65536) for F in (1, 128) for g, m, y in KINDS] +
         [(0xFFFFFFDF, 1, 160, 1, 0, 0), (1 << 28, 15, 8, 0, 2, 0)])
NOTHING = [(0, 5, 160, 1, 0, 0), (5, 0, 160, 1, 0, 0), (5, 5, 0, 1, 0, 0), (5, 5, 4, 1, 0, 0), (5, 5, 20, 0, 1, 0), (5, 5, 161, 0, 0, 0), (5, 5, 264, 1, 0, 0),
           (5, 5, 160, 1, 5, 0), (1 << 28, 16, 160, 1, 0, 0)]
FIELDS = ("grid threads lds in sections copy pieces inv max_sections visited exact row_hi tile_hi law_hi fetch_hi top_chan chans resident vgprs ahead "
          "max_pieces").split()


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("filt_route") / "filt_route_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "filt_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    cases = CASES + NOTHING
    r = subprocess.run([exe], input="\n".join(" ".join(map(str, c)) for c in cases) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [dict(zip(FIELDS, map(int, line.split()))) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return dict(zip(cases, out))


def test_geometry(routes):
    for case in CASES:
        C, F, n, g, m, y = case
        r = routes[case]
        assert r["chans"] == 64 and r["threads"] == 64 and r["resident"] == 4 and r["vgprs"] == 256 and r["ahead"] == 16 and r["max_pieces"] == 32, case
        assert r["grid"] == -(-C // 64) and (r["grid"] - 1) * 64 < C <= r["grid"] * 64, case                   # every channel, no idle block
        assert C - 1 <= r["top_chan"] < C + 64, case                         # the last lane's channel: at or past the end, which the kernel masks
        assert r["pieces"] == n // 8 <= r["max_pieces"] and r["visited"] == 64 * r["pieces"] and r["exact"] == 1, case
        assert r["fetch_hi"] == r["pieces"] - 1, case                        # a clamped turn reads the block's last piece at most
        stride = n // 2 + 1                                                  # dwords between rows: odd
        assert stride % 2 == 1 and r["row_hi"] == n // 2 < stride and r["tile_hi"] == 4 * (63 * stride + n // 2) <= 4 * 64 * stride, case
        assert r["lds"] == r["law_hi"] == 4 * 64 * stride + 64 and r["resident"] * r["lds"] <= 160 * 1024 and 2 * r["vgprs"] <= 512, case
        assert r["inv"] == (1 << 20) // r["pieces"] + 1 and (64 * r["max_pieces"] - 1) * r["inv"] < 1 << 32, case   # the product stays in 32 bits


def test_instantiation_follows_input_sections_and_entry(routes):
    for case in CASES:
        C, F, n, g, m, y = case
        r = routes[case]
        assert (r["in"], r["copy"]) == (1 if g else 2, y), case
        assert r["max_sections"] == (m or 4), case
        assert r["sections"] == (1 if y else {0: 4, 1: 1, 2: 2, 3: 4, 4: 4}[m]), case
        assert y or r["sections"] >= r["max_sections"], case                 # a plan that may run fits the kernel's sections


def test_nothing_to_launch(routes):
    for case in NOTHING:
        assert routes[case]["grid"] == 0 and routes[case]["threads"] == 0 and routes[case]["lds"] == 0, case
