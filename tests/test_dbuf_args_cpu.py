"""-m "not gpu": the argument rule of igdsp_dbuf_run (dbuf_run in csrc/igdsp_args.h), compiled with g++ alone through
tests/route/dbuf_args_driver.cpp: every clause in its order and which code wins when two apply: the frame and the maximum ahead of
nothing to do, the required buffers, the range, the alignment, the overlap of byte ranges.  tests/test_gpu_dbuf.py replays the clauses
through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL, ERANGE = -22, -34
BASE = dict(ops="x", state="x", out="x", flags="x", len="x", fill="x", stats="x", C=5, T=3, n=160, M=960)
BASE["in"] = "x"

# (overrides, rc, run, the verdict names its rule).  Sizes at the base shape: ops 15, in / out 4 800, state 10 560, flags 15,
# len / fill 30, stats 240 bytes
CASES = [
    (dict(), 0, 1, 0),
    (dict(flags="0", len="0", fill="0", stats="0"), 0, 1, 0),
    (dict(n=1, M=2), 0, 1, 0), (dict(n=256, M=512), 0, 1, 0), (dict(n=256, M=1024), 0, 1, 0), (dict(n=24, M=48), 0, 1, 0),
    # 1. the frame and the maximum, whether or not there is work
    (dict(n=0), EINVAL, 0, 0), (dict(n=257, M=1024), EINVAL, 0, 0), (dict(M=319), EINVAL, 0, 0), (dict(M=1025), EINVAL, 0, 0),
    (dict(M=0), EINVAL, 0, 0), (dict(n=1, M=1), EINVAL, 0, 0),
    (dict(C=0, n=0), EINVAL, 0, 0), (dict(T=0, M=2000), EINVAL, 0, 0),
    # 2. nothing to do, whatever else is wrong
    (dict(C=0), 0, 0, 0), (dict(T=0), 0, 0, 0),
    (dict(C=0, ops="0", state="0", out="0", stats="x4"), 0, 0, 0),
    (dict(T=0, out="in", fill="x1"), 0, 0, 0),
    # 3. the required buffers
    (dict(ops="0"), EINVAL, 0, 0), (dict(state="0"), EINVAL, 0, 0), (dict(out="0"), EINVAL, 0, 0),
    ({"in": "0"}, EINVAL, 0, 0),
    # 4. the range
    (dict(C=0x10000000, T=16), ERANGE, 0, 0),
    (dict(C=0xFFFFFFDF, T=1, flags="0", len="0", fill="0", stats="0"), 0, 1, 0),                     # 2^32 - 33: the last that fits
    (dict(C=0xFFFFFFE0, T=1), ERANGE, 0, 0),
    (dict(C=0x10000000, T=16, n=0), EINVAL, 0, 0),                       # a bad n wins over too many steps
    (dict(C=0x10000000, T=16, out="0"), EINVAL, 0, 0),                   # a missing buffer too
    # 5. alignment: 2 for rows, lengths and fills, 4 for the state, 8 for the records
    ({"in": "x1"}, EINVAL, 0, 0), (dict(out="x1"), EINVAL, 0, 0), (dict(len="x1"), EINVAL, 0, 0), (dict(fill="x1"), EINVAL, 0, 0),
    (dict(state="x2"), EINVAL, 0, 0), (dict(stats="x4"), EINVAL, 0, 0),
    (dict(ops="x1", flags="x3"), 0, 1, 0),                               # bytes
    ({"in": "x2", "out": "x6", "len": "x2", "fill": "x2", "state": "x4", "stats": "x8"}, 0, 1, 0),
    (dict(C=0x10000000, T=16, out="x1"), ERANGE, 0, 0),                  # too many steps wins over the alignment
    # 6. an output that overlaps an input, the state or another output: the rule with a text; the alignment wins over it
    (dict(out="in"), EINVAL, 0, 1), (dict(out="in+4798"), EINVAL, 0, 1), (dict(out="in+4800"), 0, 1, 0),
    (dict(out="state+10558"), EINVAL, 0, 1), (dict(out="state+10560"), 0, 1, 0), (dict(out="ops"), EINVAL, 0, 1),
    (dict(flags="ops+14"), EINVAL, 0, 1), (dict(flags="ops+15"), 0, 1, 0), (dict(flags="state"), EINVAL, 0, 1),
    (dict(stats="in+4792"), EINVAL, 0, 1), (dict(stats="state+2112"), EINVAL, 0, 1),
    (dict(len="fill"), EINVAL, 0, 1), (dict(len="fill+28"), EINVAL, 0, 1), (dict(len="fill+30"), 0, 1, 0),
    (dict(fill="out+4798"), EINVAL, 0, 1), (dict(flags="out+4800"), 0, 1, 0), (dict(stats="out+4800"), 0, 1, 0),
    (dict(flags="stats+239"), EINVAL, 0, 1), (dict(flags="stats+240"), 0, 1, 0),
    (dict(out="in+4799"), EINVAL, 0, 0),                                 # misaligned and overlapping: no text
    ({"in": "ops"}, 0, 1, 0),                                            # two inputs may share memory
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("dbuf_args") / "dbuf_args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "dbuf_args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
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
