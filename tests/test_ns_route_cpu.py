"""-m "not gpu": the geometry of igdsp_ns_run (ns_route in csrc/igdsp_route.h) and the index arithmetic of its transform
(csrc/igdsp_ns.h), compiled with g++ alone through tests/route/ns_route_driver.cpp: 16 lanes own a channel, a block is one wave and four
channels; the grid covers every channel; the turns of a channel's lanes visit every 16-byte piece of its row once, a piece stays inside
the row and the last channel's row inside the LDS asked for; a clamped fetch never leaves the row; the resident blocks' LDS fits a CU;
the instantiation k_ns<IN, COPY> follows the input's form and the entry.  Shapes that are not the kernel's launch nothing.  The
transform: every pass's butterflies, as the 16 lanes take them, are a permutation of the 128 points (no item of a phase touches what
another does), the split pass's mirror pairs cover every position once, every twiddle index lies in the table."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
NS = (80, 160, 240, 320)
KINDS = [(g, y) for g in (0, 1) for y in (0, 1)]
CASES = ([(1, 1, n, g, y) for n in NS for g, y in KINDS] +
         [(C, F, n, g, y) for C in (1, 3, 4, 5, 63, 64, 65, 4096, 65536) for F in (1, 128) for n in (160, 320) for g, y in KINDS] +
         [(0xFFFFFFDF, 1, 160, 1, 0), (1 << 28, 15, 80, 0, 0)])
NOTHING = [(0, 5, 160, 1, 0), (5, 0, 160, 1, 0), (5, 5, 0, 1, 0), (5, 5, 8, 1, 0), (5, 5, 40, 0, 0), (5, 5, 161, 0, 0), (5, 5, 256, 1, 0), (5, 5, 400, 1, 0),
           (1 << 28, 16, 160, 1, 0)]
FIELDS = ("grid threads lds in copy pieces visited once row_hi row_bytes lds_hi fetch_hi top_chan lanes chans resident vgprs turns state_bytes work_bytes "
          "sizeof_state sizeof_work").split()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("ns_route") / "ns_route_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "ns_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)

    def ask(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.splitlines()
    return ask


@pytest.fixture(scope="module")
def routes(driver):
    cases = CASES + NOTHING
    out = [dict(zip(FIELDS, map(int, line.split()))) for line in driver("\n".join(" ".join(map(str, c)) for c in cases) + "\n")]
    assert len(out) == len(cases)
    return dict(zip(cases, out))


def test_geometry(routes):
    for case in CASES:
        C, F, n, g, y = case
        r = routes[case]
        assert (r["lanes"], r["chans"], r["threads"], r["resident"], r["vgprs"], r["turns"]) == (16, 4, 64, 8, 256, 3), case
        assert r["state_bytes"] == r["sizeof_state"] == 1072 and r["work_bytes"] == r["sizeof_work"] == 1680, case
        assert r["grid"] == -(-C // 4) and (r["grid"] - 1) * 4 < C <= r["grid"] * 4, case                       # every channel, no idle block
        assert C - 1 <= r["top_chan"] < C + 4, case                          # the last lanes' channel: at or past the end, which the kernel masks
        assert r["pieces"] == n // 8 <= r["turns"] * r["lanes"] and r["visited"] == r["pieces"] and r["once"] == 1, case
        assert r["fetch_hi"] == r["pieces"] - 1 and r["row_hi"] == r["row_bytes"] == 2 * n, case
        chan = 1072 + 1680 + 2 * n
        assert chan % 16 == 0 and r["lds"] == 4 * chan == r["lds_hi"], case   # the last channel's row ends where the block's LDS ends
        assert r["resident"] * r["lds"] <= 160 * 1024 and (r["resident"] // 4) * r["vgprs"] <= 512, case


def test_instantiation_follows_input_and_entry(routes):
    for case in CASES:
        C, F, n, g, y = case
        assert (routes[case]["in"], routes[case]["copy"]) == (1 if g else 2, y), case


def test_nothing_to_launch(routes):
    for case in NOTHING:
        assert routes[case]["grid"] == 0 and routes[case]["threads"] == 0 and routes[case]["lds"] == 0, case


def test_transform_indices(driver):
    v = list(map(int, driver("X\n")[0].split()))
    passes, rest = v[:14], v[14:]
    for sh in range(7):
        assert passes[2 * sh] == 1, sh                                       # the pass is a permutation of the 128 points
        assert passes[2 * sh + 1] == ((1 << sh) - 1) << (7 - sh) < 128, sh   # W^pos of the span, in the 256-point table
    invol, pairs, tmax, bands = rest
    assert invol == 1 and pairs == 1 and tmax == 127 and bands == 1
