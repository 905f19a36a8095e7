"""-m "not gpu": the geometry of igdsp_srtp_gcm_protect / igdsp_srtp_gcm_unprotect (srtp_gcm_route in csrc/igdsp_route.h), compiled with
g++ alone through tests/route/srtp_gcm_route_driver.cpp: k_srtp's geometry (a lane owns a leg, a block is one wave and 64 legs; the grid
covers every leg with no idle block; the four turns of a piece visit every 16-byte quarter of every row once and stay inside the tile;
a load never leaves its packet's slot and the pieces cover the slot) with LDS and a residency of its own: the resident blocks' LDS and
registers fit a CU and one block more would not; GHASH's slots: for every header length and packet end a slot holds, the pieces a
pass walks stay within max_pieces, and their slots deal every AAD block and every ciphertext block out once, in order; the instantiation
k_srtp_gcm<DIR, MOVE> follows the entry.  Shapes that are not the kernel's launch nothing."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
KINDS = [(0, 0), (1, 0), (0, 1)]
STRIDES = (12, 64, 180, 192, 196, 208, 2044, 2048)
CASES = ([(C, F, 192, 192, d, y) for C in (1, 64, 65, 65536) for F in (1, 128) for d, y in KINDS] +
         [(65, 3, s, o, d, y) for s in STRIDES for o in (s, 2048) for d, y in KINDS[:1 if s > 1000 else 3]] + [(0xFFFFFFDF, 1, 192, 192, 0, 0), (1 << 28, 15, 12, 24, 1, 0)])
NOTHING = [(0, 5, 192, 192, 0, 0), (5, 0, 192, 192, 1, 0), (5, 5, 8, 192, 0, 0), (5, 5, 190, 192, 0, 0), (5, 5, 2052, 192, 0, 0), (5, 5, 192, 8, 0, 0),
           (5, 5, 192, 194, 1, 0), (5, 5, 192, 2052, 0, 0), (5, 5, 192, 192, 2, 0), (1 << 28, 16, 192, 192, 0, 0)]
FIELDS = ("grid threads lds dir move max_pieces visited once tile_hi tile_words slot_hi covered top_chan chans pitch turns resident vgprs lds_bytes "
          "sizeof_state sizeof_rec pieces_hi slots_ok").split()
LDS = 1024 + 64 * 17 * 4 + 2 * 256 + 60 * 256 + 64 * 256 + 64             # Te0, the tile, two words a row, the round keys [60][64], the multiples of H [16][4][64], the reduction


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("srtp_gcm_route") / "srtp_gcm_route_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "srtp_gcm_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
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
        assert (r["chans"], r["pitch"], r["turns"], r["threads"]) == (64, 17, 4, 64), case
        assert r["sizeof_state"] == 320 and r["sizeof_rec"] == 8, case
        assert r["grid"] == -(-C // 64) and (r["grid"] - 1) * 64 < C <= r["grid"] * 64, case                     # every leg, no idle block
        assert C - 1 <= r["top_chan"] < C + 64, case                         # the last lanes' leg: at or past the end, which the kernel masks
        assert r["max_pieces"] == -(-stride // 64) + 1, case                 # the data's pieces and the one the last ciphertext block's slot may add
        assert r["once"] == 1 and r["tile_hi"] == 63 * 17 + 16 <= r["tile_words"] == 64 * 17, case
        assert r["slot_hi"] == stride and r["covered"] == 64 * stride, case  # a load never leaves the slot; the pieces cover all of it
        assert r["visited"] == 64 * -(-stride // 16), case


def test_ghash_slots(routes):
    for case in CASES:
        r = routes[case]
        assert r["slots_ok"] == 1 and 1 <= r["pieces_hi"] <= r["max_pieces"], case


def test_residency_budget(routes):
    """kSrtpGcmResident = 4 blocks of one wave per CU: their LDS fits the CU's 160 KiB and a fifth block's would not; a SIMD then holds
    one wave, which may take all of its 512 registers (kSrtpGcmVgprs)"""
    for case in CASES:
        r = routes[case]
        assert (r["resident"], r["vgprs"]) == (4, 512) and r["lds"] == r["lds_bytes"] == LDS == 37696, case
        assert r["resident"] * r["lds"] <= 160 * 1024 < (r["resident"] + 1) * r["lds"] and -(-r["resident"] // 4) * r["vgprs"] <= 512, case


def test_instantiation_follows_the_entry(routes):
    for case in CASES:
        C, F, stride, ostride, d, y = case
        assert (routes[case]["dir"], routes[case]["move"]) == ((0 if y else d), y), case


def test_nothing_to_launch(routes):
    for case in NOTHING:
        assert routes[case]["grid"] == 0 and routes[case]["threads"] == 0 and routes[case]["lds"] == 0, case
