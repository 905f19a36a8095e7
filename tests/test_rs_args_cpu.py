"""-m "not gpu": the argument rule of igdsp_resample (resample in csrc/igdsp_args.h), compiled with g++ alone through
tests/route/rs_args_driver.cpp: every clause in its order, which code wins when two apply, the direction / factor / layout ahead of
nothing to do, the inputs of each direction, the row strides, the range on both sides.  tests/test_gpu_rs.py replays the clauses
through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL, ERANGE = -22, -34
BASE = dict(dir=0, R=2, layout=0, payload="0", codec="0", pcm="x", len="x", state="x", C=5, F=3, n=160, rn=0, rw=0, out="x", stats="x")

# (overrides, rc, run, the verdict names its rule)
CASES = [
    (dict(), 0, 1, 0),
    (dict(dir=1, R=6, layout=1), 0, 1, 0),
    (dict(R=3), 0, 1, 0), (dict(R=4), 0, 1, 0), (dict(R=6), 0, 1, 0),
    # 1. the direction, the factor and the layout, whether or not there is work
    (dict(dir=2), EINVAL, 0, 0), (dict(R=0), EINVAL, 0, 0), (dict(R=1), EINVAL, 0, 0), (dict(R=5), EINVAL, 0, 0), (dict(R=8), EINVAL, 0, 0),
    (dict(layout=2), EINVAL, 0, 0),
    (dict(C=0, R=5), EINVAL, 0, 0), (dict(F=0, dir=7), EINVAL, 0, 0), (dict(F=0, layout=9), EINVAL, 0, 0),
    # 2. nothing to do, whatever else is wrong
    (dict(C=0), 0, 0, 0), (dict(F=0), 0, 0, 0),
    (dict(C=0, pcm="0", state="0", out="0", stats="0", n=0, rn=3), 0, 0, 0),
    (dict(F=0, n=9999, out="state", stats="x4"), 0, 0, 0),
    # 3. the input of the direction
    (dict(pcm="0"), EINVAL, 0, 0),
    (dict(payload="x", codec="x"), EINVAL, 0, 0),                       # both
    (dict(payload="x", codec="x", pcm="0"), 0, 1, 0),
    (dict(payload="x", pcm="0"), EINVAL, 0, 0),                         # G.711 without its codec bytes
    (dict(dir=1, payload="x", codec="x", pcm="0"), EINVAL, 0, 0),       # DOWN takes PCM only
    (dict(dir=1, payload="x", codec="x"), EINVAL, 0, 0),
    (dict(dir=1, pcm="0"), EINVAL, 0, 0),
    # 4. the state, and at least one of the rows and the records
    (dict(state="0"), EINVAL, 0, 0),
    (dict(out="0", stats="0"), EINVAL, 0, 0),
    (dict(out="0"), 0, 1, 0), (dict(stats="0"), 0, 1, 0), (dict(len="0"), 0, 1, 0),
    # 5. the row strides: 0 = C, else >= C
    (dict(rn=4), EINVAL, 0, 0), (dict(rw=4), EINVAL, 0, 0), (dict(rn=5, rw=5), 0, 1, 0), (dict(rn=1000, rw=7), 0, 1, 0),
    # 6. the shape: n first, then rows x frames on both sides
    (dict(n=0), EINVAL, 0, 0), (dict(n=257), EINVAL, 0, 0), (dict(n=1), 0, 1, 0), (dict(n=256), 0, 1, 0),
    (dict(C=0x10000000, F=16), ERANGE, 0, 0),
    (dict(C=0xFFFFFFDF, F=1), 0, 1, 0),                                 # 2^32 - 33: the last that fits
    (dict(C=0xFFFFFFE0, F=1), ERANGE, 0, 0),
    (dict(rn=0x10000000, F=16), ERANGE, 0, 0), (dict(rw=0x10000000, F=16), ERANGE, 0, 0), (dict(rw=0x10000000, F=15), 0, 1, 0),
    (dict(C=0x08000000, F=16, layout=1), ERANGE, 0, 0),                 # the wide side has F R frames in the sub-frame layout
    (dict(C=0x08000000, F=16, layout=0), 0, 1, 0),
    (dict(C=0x08000000, F=5, R=6, layout=1), 0, 1, 0), (dict(C=0x08000000, F=6, R=6, layout=1), ERANGE, 0, 0),
    (dict(C=0x10000000, F=16, n=0), EINVAL, 0, 0),                      # a bad n wins over too many rows
    (dict(C=0x10000000, F=16, rn=1), EINVAL, 0, 0),                     # a bad stride wins over both
    # 7. alignment: 2 for rows and lengths, 4 for the state, 8 for the records
    (dict(pcm="x1"), EINVAL, 0, 0), (dict(len="x1"), EINVAL, 0, 0), (dict(out="x1"), EINVAL, 0, 0), (dict(state="x2"), EINVAL, 0, 0),
    (dict(stats="x4"), EINVAL, 0, 0),
    (dict(payload="x1", codec="x1", pcm="0"), 0, 1, 0),                 # bytes
    (dict(pcm="x2", len="x6", out="x2", state="x4", stats="x8"), 0, 1, 0),
    (dict(C=0x10000000, F=16, pcm="x1"), ERANGE, 0, 0),                 # too many rows wins over the alignment
    # 8. an output that is an input or the state: the one rule with a text; the alignment wins over it
    (dict(out="pcm"), EINVAL, 0, 1), (dict(out="state"), EINVAL, 0, 1), (dict(out="len"), EINVAL, 0, 1), (dict(stats="state"), EINVAL, 0, 1),
    (dict(stats="pcm"), EINVAL, 0, 1), (dict(payload="x", codec="x", pcm="0", out="payload"), EINVAL, 0, 1),
    (dict(payload="x", codec="x", pcm="0", stats="codec"), EINVAL, 0, 1),
    (dict(out="state", stats="x4"), EINVAL, 0, 0),
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("rs_args") / "rs_args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "rs_args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    lines = [" ".join(f"{k}={v}" for k, v in {**BASE, **over}.items()) for over, _, _, _ in CASES]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [dict(kv.split("=") for kv in line.split()) for line in out]


@pytest.mark.parametrize("i", range(len(CASES)), ids=[",".join(f"{k}={v}" for k, v in c[0].items()) or "base" for c in CASES])
def test_rule(verdicts, i):
    _, rc, run, why = CASES[i]
    v = verdicts[i]
    assert (int(v["rc"]), int(v["run"]), int(v["why"])) == (rc, run, why)
