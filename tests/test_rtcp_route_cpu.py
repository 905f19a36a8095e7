"""-m "not gpu": the geometry of igdsp_rtcp_build, igdsp_rtcp_parse and igdsp_srtcp_protect / igdsp_srtcp_unprotect (rtcp_build_route,
rtcp_parse_route, srtcp_route in csrc/igdsp_route.h), compiled with g++ alone through tests/route/rtcp_route_driver.cpp: a lane owns a
leg, a block is one wave and 64 legs; the grid covers every leg with no idle block.  Build: the nine turns visit every 16-byte item of
every row once, stay inside the rows, and with the owner's tail store exactly the largest packet's 136 bytes, which every legal stride
holds.  Parse: the four turns of a piece visit every quarter of every row once and stay inside the tile, a load never leaves its
packet's slot and the pieces cover it.  SRTCP is SRTP's route.  The resident blocks' LDS and registers fit a CU.  Shapes that are not
the kernels' launch nothing."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
BUILD = [(0, C, F, s, 0, 0, y) for C in (1, 64, 65, 65536) for F in (1, 16) for s in (136, 152, 192, 2048) for y in (0, 1)] + [(0, 0xFFFFFFDF, 1, 152, 0, 0, 0)]
PARSE = [(1, C, F, s, 0, 0, y) for C in (1, 64, 65, 65536) for F in (1, 16) for s in (8, 12, 64, 152, 192, 196, 2044, 2048) for y in (0, 1)] + [(1, 1 << 28, 15, 8, 0, 0, 0)]
SRTCP = [(2, C, 3, s, o, d, y) for C in (1, 65, 65536) for s, o in ((152, 152), (152, 192), (2048, 2048), (12, 28)) for d, y in ((0, 0), (1, 0), (0, 1))]
NOTHING = [(0, 0, 5, 152, 0, 0, 0), (0, 5, 0, 152, 0, 0, 0), (0, 5, 5, 132, 0, 0, 0), (0, 5, 5, 150, 0, 0, 0), (0, 5, 5, 2052, 0, 0, 0), (0, 1 << 28, 16, 152, 0, 0, 0),
           (1, 0, 5, 152, 0, 0, 0), (1, 5, 0, 152, 0, 0, 0), (1, 5, 5, 4, 0, 0, 0), (1, 5, 5, 150, 0, 0, 0), (1, 5, 5, 2052, 0, 0, 0), (1, 1 << 28, 16, 152, 0, 0, 0),
           (2, 5, 5, 8, 152, 0, 0), (2, 5, 5, 152, 150, 1, 0), (2, 5, 5, 152, 152, 2, 0), (2, 0, 5, 152, 152, 0, 0)]
FIELDS = ("grid threads lds dir move max_pieces visited once tile_hi tile_words slot_hi covered top chans row_words row_pitch row_items resident vgprs "
          "build_lds parse_lds srtp_lds sizeof_state sizeof_src sizeof_built sizeof_seen").split()


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("rtcp_route") / "rtcp_route_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "rtcp_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    cases = BUILD + PARSE + SRTCP + NOTHING
    r = subprocess.run([exe], input="\n".join(" ".join(map(str, c)) for c in cases) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [dict(zip(FIELDS, map(int, line.split()))) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return dict(zip(cases, out))


def common(r, C, case):
    assert (r["chans"], r["row_words"], r["row_pitch"], r["row_items"], r["threads"], r["resident"], r["vgprs"]) == (64, 34, 35, 9, 64, 8, 256), case
    assert (r["sizeof_state"], r["sizeof_src"], r["sizeof_built"], r["sizeof_seen"]) == (80, 16, 8, 32), case
    assert r["grid"] == -(-C // 64) and (r["grid"] - 1) * 64 < C <= r["grid"] * 64, case                         # every leg, no idle block
    assert C - 1 <= r["top"] < C + 64, case                                  # the last lanes' leg: at or past the end, which the kernel masks
    assert r["resident"] * r["lds"] <= 160 * 1024 and (r["resident"] // 4) * r["vgprs"] <= 512, case


def test_build_geometry(routes):
    for case in BUILD:
        _, C, F, stride = case[:4]
        r = routes[case]
        common(r, C, case)
        assert r["once"] == 1 and r["visited"] == 64 * 8 and r["tile_hi"] == 63 * 35 + 34 <= r["tile_words"] == 64 * 35, case
        assert r["slot_hi"] == 136 <= stride and r["covered"] == 64 * 136, case  # the largest packet, whole, and nothing behind it
        assert r["lds"] == r["build_lds"] == 64 * 35 * 4 + 256 and r["move"] == case[6], case


def test_parse_geometry(routes):
    for case in PARSE:
        _, C, F, stride = case[:4]
        r = routes[case]
        common(r, C, case)
        assert r["max_pieces"] == -(-stride // 64), case
        assert r["once"] == 1 and r["tile_hi"] == 63 * 17 + 16 <= r["tile_words"] == 64 * 17, case
        assert r["slot_hi"] == stride and r["covered"] == 64 * stride and r["visited"] == 64 * -(-stride // 16), case
        assert r["lds"] == r["parse_lds"] == 64 * 17 * 4 + 256 and r["move"] == case[6], case


def test_srtcp_route_is_srtps(routes):
    for case in SRTCP:
        _, C, F, stride, ostride, d, y = case
        r = routes[case]
        common(r, C, case)
        assert (r["dir"], r["move"]) == ((0 if y else d), y) and r["lds"] == r["srtp_lds"] and r["max_pieces"] == -(-stride // 64) + 1, case


def test_nothing_to_launch(routes):
    for case in NOTHING:
        assert routes[case]["grid"] == 0 and routes[case]["threads"] == 0 and routes[case]["lds"] == 0, case
