"""-m "not gpu": the argument rule of igdsp_tone_detect (tdet_run in csrc/igdsp_args.h), compiled with g++ alone through
tests/route/tdet_args_driver.cpp: every clause in its order and which code wins when two apply: the frame length and the list's own
pointers ahead of nothing to do (which still launches when a list is asked for: the counts are written as 0), the input form, the plans
and the state, the range, the alignment (the codes 2, PCM 4, the events 16 bytes: what the kernel's loads and stores take), the overlap of byte ranges.  tests/test_gpu_tdet.py replays the clauses through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL, ERANGE = -22, -34
BASE = dict(g711="x", codec="x", pcm="0", plans="x", n_plans=2, plan_of="x", state="x", rec="x", events="x", cap=4, count="x", work="x", C=5, F=3, n=160)
PCM = dict(g711="0", codec="0", pcm="x")
NOLIST = dict(events="0", cap=0, count="0", work="0")

# (overrides, rc, run, the verdict names its rule).  Sizes at the base shape: g711 2 400, codec 5, pcm 4 800, plans 168, plan_of 10,
# state 1 320, rec 120, events 64, count 8, work 16 + 16 (with rec) or + 120 more (without)
CASES = [
    (dict(), 0, 1, 0), (PCM, 0, 1, 0), (NOLIST, 0, 1, 0), (dict(rec="0"), 0, 1, 0), ({**NOLIST, "rec": "0"}, 0, 1, 0), (dict(plan_of="0"), 0, 1, 0),
    (dict(n=2), 0, 1, 0), (dict(n=256), 0, 1, 0), (dict(n=24), 0, 1, 0), (dict(events="0", cap=0), 0, 1, 0),
    # 1. the frame length, whether or not there is work
    (dict(n=0), EINVAL, 0, 0), (dict(n=1), EINVAL, 0, 0), (dict(n=161), EINVAL, 0, 0), (dict(n=258), EINVAL, 0, 0), (dict(C=0, n=3), EINVAL, 0, 0),
    (dict(F=0, n=0), EINVAL, 0, 0),
    # 2. the list's own pointers, whether or not there is work
    (dict(count="x2"), EINVAL, 0, 0), (dict(work="x8"), EINVAL, 0, 0), (dict(work="0"), EINVAL, 0, 0), (dict(events="0"), EINVAL, 0, 0),
    (dict(C=0, work="0"), EINVAL, 0, 0), (dict(F=0, events="0"), EINVAL, 0, 0),
    # 3. nothing to do: a launch of the counts alone with a list, nothing without one, whatever else is wrong
    (dict(C=0), 0, 1, 0), (dict(F=0), 0, 1, 0), ({**NOLIST, "C": 0}, 0, 0, 0), ({**NOLIST, "F": 0, "state": "0", "plans": "0"}, 0, 0, 0),
    (dict(C=0, g711="0", state="0", rec="x4"), 0, 1, 0),
    # 4. exactly one input form, the codes with their laws, the plans, the state
    (dict(g711="0"), EINVAL, 0, 0), (dict(pcm="x"), EINVAL, 0, 0), (dict(codec="0"), EINVAL, 0, 0), (dict(state="0"), EINVAL, 0, 0),
    (dict(plans="0"), EINVAL, 0, 0), (dict(n_plans=0), EINVAL, 0, 0), ({**PCM, "codec": "x"}, 0, 1, 0),
    # 5. the range
    (dict(C=0x10000000, F=16), ERANGE, 0, 0), (dict(C=0xFFFFFFE0, F=1), ERANGE, 0, 0),
    ({**NOLIST, "C": 0xFFFFFFDF, "F": 1, "rec": "0"}, 0, 1, 0),                                     # 2^32 - 33: the last that fits
    (dict(C=0x10000000, F=16, n=0), EINVAL, 0, 0), (dict(C=0x10000000, F=16, state="0"), EINVAL, 0, 0),
    # 6. alignment: 2 for the codes and plan_of, 4 for PCM, the plans, the state (and the counts), 8 for the records, 16 for the events:
    # the kernel reads a row two samples at a time and stores an event as 16 bytes
    ({**PCM, "pcm": "x1"}, EINVAL, 0, 0), ({**PCM, "pcm": "x2"}, EINVAL, 0, 0), (dict(g711="x1"), EINVAL, 0, 0), (dict(g711="x3"), EINVAL, 0, 0),
    (dict(plan_of="x1"), EINVAL, 0, 0), (dict(plans="x2"), EINVAL, 0, 0), (dict(state="x2"), EINVAL, 0, 0),
    (dict(rec="x4"), EINVAL, 0, 0), (dict(events="x4"), EINVAL, 0, 0), (dict(events="x8"), EINVAL, 0, 0),
    (dict(g711="x2", codec="x3", plan_of="x2", plans="x4", state="x4", rec="x8", events="x16", count="x4", work="x16"), 0, 1, 0),
    ({**PCM, "pcm": "x4"}, 0, 1, 0), ({**NOLIST, "events": "x8"}, EINVAL, 0, 0),                     # the alignment is looked at with or without a list
    (dict(C=0x10000000, F=16, rec="x4"), ERANGE, 0, 0),                   # too many frames wins over the alignment
    # 7. the state or an output that overlaps an input, or another of them: the rule with a text; the alignment wins over it
    (dict(state="g711"), EINVAL, 0, 1), (dict(state="g711+2396"), EINVAL, 0, 1), (dict(state="g711+2400"), 0, 1, 0),
    (dict(rec="g711+2392"), EINVAL, 0, 1), (dict(rec="plans+160"), EINVAL, 0, 1), (dict(rec="plans+168"), 0, 1, 0),
    (dict(state="plan_of+8"), EINVAL, 0, 1), (dict(state="plan_of+12"), 0, 1, 0), (dict(events="codec"), EINVAL, 0, 1),
    ({**PCM, "count": "pcm+4796"}, EINVAL, 0, 1), ({**PCM, "count": "pcm+4800"}, 0, 1, 0), ({**PCM, "rec": "codec"}, 0, 1, 0),
    (dict(rec="state+1312"), EINVAL, 0, 1), (dict(rec="state+1320"), 0, 1, 0), (dict(events="rec+112"), EINVAL, 0, 1), (dict(events="rec+128"), 0, 1, 0), (dict(events="rec+120"), EINVAL, 0, 0),
    (dict(count="events+60"), EINVAL, 0, 1), (dict(count="events+64"), 0, 1, 0), (dict(work="rec+112"), EINVAL, 0, 1),
    (dict(rec="work+16"), EINVAL, 0, 1), (dict(rec="work+32"), 0, 1, 0),                             # with records the work is 32 bytes
    (dict(rec="0", state="work+144"), EINVAL, 0, 1), (dict(rec="0", state="work+152"), 0, 1, 0),     # without, the records live in it
    ({**NOLIST, "rec": "state+8"}, EINVAL, 0, 1), ({**NOLIST, "events": "state", "work": "state"}, 0, 1, 0),   # no list: its buffers are not looked at
    (dict(events="rec+116"), EINVAL, 0, 0),                               # misaligned and overlapping: no text
    (dict(codec="g711", plan_of="plans"), 0, 1, 0),                       # inputs may share memory
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("tdet_args") / "tdet_args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "tdet_args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
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
