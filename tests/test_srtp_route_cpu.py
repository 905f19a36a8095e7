"""-m "not gpu": the geometry of igdsp_srtp_protect / igdsp_srtp_unprotect (srtp_route in csrc/igdsp_route.h), compiled with g++ alone
through tests/route/srtp_route_driver.cpp: a lane owns a channel, a block is one wave and 64 channels; the grid covers every channel
with no idle block; the four turns of a piece visit every 16-byte quarter of every row once and stay inside the tile; a load never
leaves its packet's slot (a stride that is no multiple of 16 ends in dword loads) and the pieces cover the slot; the resident blocks'
LDS and registers fit a CU; the instantiation k_srtp<DIR, MOVE> follows the entry.  Shapes that are not the kernel's launch nothing."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
KINDS = [(0, 0), (1, 0), (0, 1)]
STRIDES = (12, 64, 180, 192, 196, 2044, 2048)
CASES = ([(C, F, 192, 192, d, y) for C in (1, 64, 65, 65536) for F in (1, 128) for d, y in KINDS] +
         [(65, 3, s, o, d, y) for s in STRIDES for o in (s, 2048) for d, y in KINDS] + [(0xFFFFFFDF, 1, 192, 192, 0, 0), (1 << 28, 15, 12, 24, 1, 0)])
NOTHING = [(0, 5, 192, 192, 0, 0), (5, 0, 192, 192, 1, 0), (5, 5, 8, 192, 0, 0), (5, 5, 190, 192, 0, 0), (5, 5, 2052, 192, 0, 0), (5, 5, 192, 8, 0, 0),
           (5, 5, 192, 194, 1, 0), (5, 5, 192, 2052, 0, 0), (5, 5, 192, 192, 2, 0), (1 << 28, 16, 192, 192, 0, 0)]
FIELDS = ("grid threads lds dir move max_pieces visited once tile_hi tile_words slot_hi covered top_chan chans pitch turns resident vgprs lds_bytes "
          "sizeof_state sizeof_rec").split()


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("srtp_route") / "srtp_route_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "srtp_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    cases = CASES + NOTHING
    r = subprocess.run([exe], input="\n".join(" ".join(map(str, c)) for c in cases) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [dict(zip(FIELDS, map(int, line.split()))) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return dict(zip(cases, out))


def test_geometry(routes):
    for case in CASES:
        C, F, stride, ostride, d, y = case
        r = routes[case]
        assert (r["chans"], r["pitch"], r["turns"], r["threads"], r["resident"], r["vgprs"]) == (64, 17, 4, 64, 8, 256), case
        assert r["sizeof_state"] == 288 and r["sizeof_rec"] == 8, case
        assert r["grid"] == -(-C // 64) and (r["grid"] - 1) * 64 < C <= r["grid"] * 64, case                     # every channel, no idle block
        assert C - 1 <= r["top_chan"] < C + 64, case                         # the last lanes' channel: at or past the end, which the kernel masks
        assert r["max_pieces"] == -(-stride // 64) + 1, case                 # the data's pieces and the block the hash's padding may add
        assert r["once"] == 1 and r["tile_hi"] == 63 * 17 + 16 <= r["tile_words"] == 64 * 17, case
        assert r["slot_hi"] == stride and r["covered"] == 64 * stride, case  # a load never leaves the slot; the pieces cover all of it
        assert r["visited"] == 64 * -(-stride // 16), case
        assert r["lds"] == r["lds_bytes"] == 1024 + 64 * 17 * 4 + 2 * 256 + 44 * 256, case
        assert r["resident"] * r["lds"] <= 160 * 1024 and (r["resident"] // 4) * r["vgprs"] <= 512, case


def test_instantiation_follows_the_entry(routes):
    for case in CASES:
        C, F, stride, ostride, d, y = case
        assert (routes[case]["dir"], routes[case]["move"]) == ((0 if y else d), y), case


def test_nothing_to_launch(routes):
    for case in NOTHING:
        assert routes[case]["grid"] == 0 and routes[case]["threads"] == 0 and routes[case]["lds"] == 0, case
