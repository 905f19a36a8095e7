"""-m "not gpu": the geometry of igdsp_agc_run (agc_route in csrc/igdsp_route.h), compiled with g++ alone through
tests/route/agc_route_driver.cpp: half a wave (32 lanes) owns a channel, a lane a block of 8 samples, a block of 4 waves 8 channels;
the grid covers every channel, a frame's blocks fit the 32 lanes and reach exactly the row's end, no LDS is asked for, and the
instantiation k_agc<IN_G711, COPY> follows the input kind and the entry (the output set picks none: the outputs are run-time
pointers).  Shapes that are not the kernel's launch nothing."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
NS = list(range(8, 257, 8))
KINDS = [(g, y) for g in (0, 1) for y in (0, 1)]
CASES = ([(1, 1, n, g, y) for n in NS for g, y in KINDS] + [(C, F, 160, g, y) for C in (1, 2, 3, 7, 8, 9, 15, 16, 17, 4096, 65536) for F in (1, 128) for g, y in KINDS]
         + [(0xFFFFFFDF, 1, 160, 1, 0), (1 << 28, 15, 8, 0, 0)])
NOTHING = [(0, 5, 160, 1, 0), (5, 0, 160, 1, 0), (5, 5, 0, 1, 0), (5, 5, 4, 1, 0), (5, 5, 12, 0, 0), (5, 5, 161, 0, 0), (5, 5, 264, 1, 0), (1 << 28, 16, 160, 1, 0)]
FIELDS = "grid threads lds g711 copy blocks top_chan row_hi busy lanes chans resident waves".split()


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("agc_route") / "agc_route_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "agc_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    cases = CASES + NOTHING
    r = subprocess.run([exe], input="\n".join(" ".join(map(str, c)) for c in cases) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [dict(zip(FIELDS, map(int, line.split()))) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return dict(zip(cases, out))


def test_geometry(routes):
    for case in CASES:
        C, F, n, g, y = case
        r = routes[case]
        assert r["lanes"] == 32 and r["waves"] == 4 and r["chans"] == 8 and r["threads"] == 32 * r["chans"] == 64 * r["waves"] == 256, case
        assert r["grid"] == -(-C // 8) and r["grid"] * 8 >= C and (r["grid"] - 1) * 8 < C, case              # every channel, no idle block
        assert C - 1 <= r["top_chan"] < C + 8, case                          # the last thread's channel: at or past the end, which the kernel masks
        assert r["blocks"] == n // 8 == r["busy"] <= 32 and r["row_hi"] == n, case                            # the busy lanes cover the row exactly
        assert r["lds"] == 0 and r["resident"] == 8, case


def test_instantiation_follows_input_kind_and_entry(routes):
    for case in CASES:
        _, _, _, g, y = case
        assert (routes[case]["g711"], routes[case]["copy"]) == (g, y), case


def test_nothing_to_launch(routes):
    for case in NOTHING:
        assert routes[case]["grid"] == 0 and routes[case]["threads"] == 0, case
