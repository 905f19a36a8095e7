"""-m "not gpu": the geometry of igdsp_vad_run (vad_route in csrc/igdsp_route.h), compiled with g++ alone through
tests/route/vad_route_driver.cpp: a row of 16 lanes owns a channel, a lane two pieces of 8 samples, a block of 4 waves 16 channels; the
grid covers every channel, the pieces taken cover the row exactly, every value a lag sum reads lies in the channel's own LDS row (the
zeros in front reach back to lag 15, the zeros behind a row of 256 are the row's own), the LDS asked for is the kernel's, and the
instantiation k_vad<IN_G711, COPY> follows the input kind and the entry.  The list's geometry and the work size follow the shape and
whether d_rec is given.  Shapes that are not the kernel's launch nothing."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
NS = list(range(16, 257, 8))
KINDS = [(g, y) for g in (0, 1) for y in (0, 1)]
LISTS = [(0, 1), (1, 1), (1, 0)]
CASES = ([(1, 1, n, g, y, 0, 1) for n in NS for g, y in KINDS] +
         [(C, F, 160, g, y, li, wr) for C in (1, 2, 3, 15, 16, 17, 63, 64, 65, 4096, 65536) for F in (1, 128) for g, y in KINDS for li, wr in LISTS] +
         [(0xFFFFFFDF, 1, 160, 1, 0, 1, 0), (1 << 28, 15, 16, 0, 0, 1, 1)])
NOTHING = [(0, 5, 160, 1, 0, 1, 1), (5, 0, 160, 1, 0, 1, 1), (5, 5, 0, 1, 0, 0, 1), (5, 5, 8, 1, 0, 0, 1), (5, 5, 20, 0, 0, 0, 1), (5, 5, 161, 0, 0, 0, 1),
           (5, 5, 264, 1, 0, 0, 1), (1 << 28, 16, 160, 1, 0, 0, 1)]
FIELDS = ("grid threads lds g711 copy pieces waves list_grid counts_bytes work_bytes top_chan row_hi taken read_lo read_hi lanes chans resident nwaves "
          "pad buf lds_bytes").split()


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("vad_route") / "vad_route_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "vad_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    cases = CASES + NOTHING
    r = subprocess.run([exe], input="\n".join(" ".join(map(str, c)) for c in cases) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [dict(zip(FIELDS, map(int, line.split()))) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return dict(zip(cases, out))


def test_geometry(routes):
    for case in CASES:
        C, F, n, g, y, li, wr = case
        r = routes[case]
        assert r["lanes"] == 16 and r["nwaves"] == 4 and r["chans"] == 16 and r["threads"] == 16 * r["chans"] == 64 * r["nwaves"] == 256, case
        assert r["grid"] == -(-C // 16) and r["grid"] * 16 >= C and (r["grid"] - 1) * 16 < C, case            # every channel, no idle block
        assert C - 1 <= r["top_chan"] < C + 16, case                         # the last thread's channel: at or past the end, which the kernel masks
        assert r["pieces"] == n // 8 == r["taken"] <= 32 and r["row_hi"] == n, case                           # two turns of 16 lanes cover the row exactly
        # the lag sums stay inside the channel's row: the zeros reach back far enough, the row's buffer holds the dword past 256 samples
        assert r["pad"] == 16 and r["read_lo"] == 16 - 14 and r["read_hi"] == r["pad"] + n + 2 <= r["buf"] == 280, case   # lag 15: 14 values back, one more in its pair
        assert r["lds"] == r["lds_bytes"] == 128 * 8 + 16 * (280 * 2 + 256 * 2 + 3 * 12 * 8 + 16) and r["resident"] * r["lds"] <= 160 * 1024, case


def test_instantiation_follows_input_kind_and_entry(routes):
    for case in CASES:
        assert (routes[case]["g711"], routes[case]["copy"]) == (case[3], case[4]), case


def test_list_and_work(routes):
    for case in CASES:
        C, F, n, g, y, li, wr = case
        r = routes[case]
        waves = -(-C // 64)
        assert r["waves"] == waves, case
        if not li:
            assert r["list_grid"] == 0 and r["counts_bytes"] == 0 and r["work_bytes"] == 0, case
            continue
        counts = 16 + (F * waves * 4 + 15) // 16 * 16
        assert r["list_grid"] == -(-(F * waves) // 4) and r["counts_bytes"] == counts, case
        assert r["work_bytes"] == counts + (0 if wr else C * F * 16) and r["counts_bytes"] % 16 == 0, case   # the records behind the counts are 16-byte aligned


def test_nothing_to_launch(routes):
    for case in NOTHING:
        assert routes[case]["grid"] == 0 and routes[case]["threads"] == 0 and routes[case]["list_grid"] == 0, case
