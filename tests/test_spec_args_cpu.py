"""-m "not gpu": the argument rule of igdsp_spectrum (spec_run in csrc/igdsp_args.h), compiled with g++ alone through
tests/route/spec_args_driver.cpp: every clause in its order and which code wins when two apply: the frame and the cfg ahead of nothing to
do, the input form and the state, the range, the alignment, the overlap of byte ranges.  tests/test_gpu_spec.py replays the clauses
through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL, ERANGE = -22, -34
BASE = dict(g711="x", codec="x", pcm="0", state="x", rec="x", avg="x", raw="x", C=5, F=3, n=160, hop=1, alpha=0.25)
PCM = dict(g711="0", codec="0", pcm="x")

# (overrides, rc, run, the verdict names its rule).  Sizes at the base shape: g711 2 400, codec 5, pcm 4 800, state 20 560, rec 120,
# avg / raw 10 240 bytes
CASES = [
    (dict(), 0, 1, 0), (PCM, 0, 1, 0),
    (dict(rec="0", avg="0", raw="0"), 0, 1, 0),
    (dict(hop="none"), 0, 1, 0), (dict(n=1), 0, 1, 0), (dict(n=256), 0, 1, 0), (dict(n=24, hop=7), 0, 1, 0), (dict(alpha=1.0), 0, 1, 0),
    (dict(hop=0xFFFFFFFF, alpha=1e-6), 0, 1, 0),
    # 1. the frame and the cfg, whether or not there is work
    (dict(n=0), EINVAL, 0, 0), (dict(n=257), EINVAL, 0, 0), (dict(hop=0), EINVAL, 0, 0), (dict(alpha=0.0), EINVAL, 0, 0),
    (dict(alpha=-0.25), EINVAL, 0, 0), (dict(alpha=1.0001), EINVAL, 0, 0), (dict(alpha="nan"), EINVAL, 0, 0), (dict(alpha="inf"), EINVAL, 0, 0),
    (dict(C=0, n=0), EINVAL, 0, 0), (dict(F=0, hop=0), EINVAL, 0, 0), (dict(C=0, alpha=2.0), EINVAL, 0, 0),
    # 2. nothing to do, whatever else is wrong
    (dict(C=0), 0, 0, 0), (dict(F=0), 0, 0, 0),
    (dict(C=0, g711="0", state="0", rec="x4"), 0, 0, 0), (dict(F=0, pcm="x", avg="raw"), 0, 0, 0),
    # 3. exactly one input form, the codes with their laws, the state
    (dict(g711="0"), EINVAL, 0, 0), (dict(pcm="x"), EINVAL, 0, 0), (dict(codec="0"), EINVAL, 0, 0), (dict(state="0"), EINVAL, 0, 0),
    ({**PCM, "state": "0"}, EINVAL, 0, 0), ({**PCM, "codec": "x"}, 0, 1, 0),
    # 4. the range
    (dict(C=0x10000000, F=16), ERANGE, 0, 0),
    (dict(C=0xFFFFFFDF, F=1, rec="0", avg="0", raw="0"), 0, 1, 0),                                    # 2^32 - 33: the last that fits
    (dict(C=0xFFFFFFE0, F=1), ERANGE, 0, 0),
    (dict(C=0x10000000, F=16, n=0), EINVAL, 0, 0),                        # a bad n wins over too many frames
    (dict(C=0x10000000, F=16, state="0"), EINVAL, 0, 0),                  # a missing state too
    # 5. alignment: 2 for PCM, 4 for the state and the float arrays, 8 for the records
    ({**PCM, "pcm": "x1"}, EINVAL, 0, 0), (dict(state="x2"), EINVAL, 0, 0), (dict(avg="x2"), EINVAL, 0, 0), (dict(raw="x1"), EINVAL, 0, 0),
    (dict(rec="x4"), EINVAL, 0, 0),
    (dict(g711="x1", codec="x3"), 0, 1, 0),                               # bytes
    ({**PCM, "pcm": "x2", "state": "x4", "avg": "x4", "raw": "x12", "rec": "x8"}, 0, 1, 0),
    (dict(C=0x10000000, F=16, rec="x4"), ERANGE, 0, 0),                   # too many frames wins over the alignment
    # 6. the state or an output that overlaps an input, or another of them: the rule with a text; the alignment wins over it
    (dict(state="g711"), EINVAL, 0, 1), (dict(state="g711+2396"), EINVAL, 0, 1), (dict(state="g711+2400"), 0, 1, 0),
    (dict(rec="g711+2392"), EINVAL, 0, 1), (dict(avg="codec+4"), EINVAL, 0, 1), (dict(avg="codec+8"), 0, 1, 0),
    ({**PCM, "raw": "pcm+4796"}, EINVAL, 0, 1), ({**PCM, "raw": "pcm+4800"}, 0, 1, 0), ({**PCM, "avg": "codec"}, 0, 1, 0),
    (dict(rec="state+20552"), EINVAL, 0, 1), (dict(rec="state+20560"), 0, 1, 0), (dict(avg="state+4112"), EINVAL, 0, 1),
    (dict(avg="raw"), EINVAL, 0, 1), (dict(avg="raw+10236"), EINVAL, 0, 1), (dict(avg="raw+10240"), 0, 1, 0),
    (dict(raw="rec+112"), EINVAL, 0, 1), (dict(raw="rec+120"), 0, 1, 0), (dict(state="avg+10240"), 0, 1, 0), (dict(state="avg+10236"), EINVAL, 0, 1),
    (dict(avg="raw+10238"), EINVAL, 0, 0),                                # misaligned and overlapping: no text
    (dict(codec="g711"), 0, 1, 0),                                        # two inputs may share memory
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("spec_args") / "spec_args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "spec_args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
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
