"""-m "not gpu": the argument rule of igdsp_tone_generate (tone_generate in csrc/igdsp_args.h), compiled with g++ alone through
tests/route/tone_args_driver.cpp: every clause in its order, which code wins when two apply, nothing to do at P = 0 and F = 0, the row
stride, the optional buffers.  tests/test_gpu_tone.py replays the clauses through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL, ERANGE = -22, -34
BASE = dict(plans="x", n_plans=2, plan_of="x", cmd="x", state="x", P=5, F=3, n=160, rpf=0, pcm="x", len="x", stats="x")

# (overrides, rc, run, the verdict names its rule)
CASES = [
    (dict(), 0, 1, 0),
    # 1. nothing to do comes first, whatever else is wrong
    (dict(P=0), 0, 0, 0),
    (dict(F=0), 0, 0, 0),
    (dict(P=0, plans="0", state="0", pcm="0", stats="0", n=0, n_plans=0, rpf=3), 0, 0, 0),
    (dict(F=0, n=9999, pcm="state", stats="x4"), 0, 0, 0),
    # 2. the plans, the state, and at least one of the rows and the records
    (dict(plans="0"), EINVAL, 0, 0),
    (dict(state="0"), EINVAL, 0, 0),
    (dict(n_plans=0), EINVAL, 0, 0),
    (dict(pcm="0", stats="0"), EINVAL, 0, 0),
    (dict(pcm="0"), 0, 1, 0),                                           # records only
    (dict(stats="0"), 0, 1, 0),                                         # rows only
    (dict(plan_of="0", cmd="0", len="0"), 0, 1, 0),                     # the optional ones
    (dict(pcm="0", len="0"), 0, 1, 0),
    # 3. the row stride: 0 = P, else >= P
    (dict(rpf=4), EINVAL, 0, 0),
    (dict(rpf=5), 0, 1, 0),
    (dict(rpf=1000), 0, 1, 0),
    # 4. the shape: n first, then rows x frames with the stride
    (dict(n=0), EINVAL, 0, 0),
    (dict(n=257), EINVAL, 0, 0),
    (dict(n=1), 0, 1, 0),
    (dict(n=256), 0, 1, 0),
    (dict(P=0x10000000, F=16), ERANGE, 0, 0),
    (dict(P=0xFFFFFFDF, F=1), 0, 1, 0),                                 # 2^32 - 33: the last that fits
    (dict(P=0xFFFFFFE0, F=1), ERANGE, 0, 0),
    (dict(P=5, rpf=0x10000000, F=16), ERANGE, 0, 0),                    # the stride counts, not the ports
    (dict(P=5, rpf=0x10000000, F=15), 0, 1, 0),
    (dict(P=0x10000000, F=16, n=0), EINVAL, 0, 0),                      # a bad n wins over too many rows
    (dict(P=0x10000000, F=16, rpf=1), EINVAL, 0, 0),                    # a bad stride wins over both
    # 5. alignment: 2 for rows, lengths and plan indices, 4 for plans and state, 8 for the records
    (dict(pcm="x1"), EINVAL, 0, 0),
    (dict(len="x1"), EINVAL, 0, 0),
    (dict(plan_of="x1"), EINVAL, 0, 0),
    (dict(plans="x2"), EINVAL, 0, 0),
    (dict(state="x2"), EINVAL, 0, 0),
    (dict(stats="x4"), EINVAL, 0, 0),
    (dict(cmd="x1"), 0, 1, 0),                                          # bytes
    (dict(pcm="x2", len="x6", plan_of="x2", plans="x4", state="x4", stats="x8"), 0, 1, 0),
    (dict(P=0x10000000, F=16, pcm="x1"), ERANGE, 0, 0),                 # too many rows wins over the alignment
    # 6. an output that is an input or the state: the one rule with a text; the alignment wins over it
    (dict(pcm="state"), EINVAL, 0, 1),
    (dict(pcm="plans"), EINVAL, 0, 1),
    (dict(len="plan_of"), EINVAL, 0, 1),
    (dict(stats="cmd"), EINVAL, 0, 1),
    (dict(stats="state"), EINVAL, 0, 1),
    (dict(pcm="state", stats="x4"), EINVAL, 0, 0),
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("tone_args") / "tone_args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "tone_args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
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
