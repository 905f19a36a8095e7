"""-m "not gpu": the argument rule of igdsp_vad_run (vad_run in csrc/igdsp_args.h), compiled with g++ alone through
tests/route/vad_args_driver.cpp: every clause in its order and which code wins when two apply: the frame length and the cfg ahead of
everything, the list's own rules ahead of nothing to do (a list with no work still writes its counts), the input form, the state and
at least one output, the range, the alignment (the codes 8, PCM rows, the state, records, payloads, events and work 16 bytes, the counts
4: what the kernel's loads and stores take), the overlap of byte ranges.  tests/test_gpu_vad.py replays clauses through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL, ERANGE = -22, -34
DEF = dict(thr_abs=212, nf_min=8, nf_max=1 << 20, sid_every=0, ratio_on_q4=80, ratio_off_q4=40, dn=2, up=5, up_v=7, asm_shift=2, burst=5, hang_long=10,
           hang_short=2, order=10, dtx=1, sid_delta=2, sid_gap=2, vox_on=0x81, vox_off=0x80)


def cfg(**kw):
    return ":".join(str(v) for v in {**DEF, **kw}.values())


BASE = dict(g711="x", codec="x", pcm="0", ctl="x", cfg=cfg(), state="x", kind="x", rec="x", sid="x", txctl="x", events="x", count="x", work="x", cap=4,
            C=5, F=3, n=160)
PCM = dict(g711="0", codec="0", pcm="x")
NOLIST = dict(events="0", count="0", work="0", cap=0)
NOOUT = dict(kind="0", rec="0", sid="0", txctl="0")
BIG = dict(C=0x10000000, F=16)
BAD_CFGS = [dict(nf_min=0), dict(nf_min=9, nf_max=8), dict(nf_max=(1 << 24) + 1), dict(ratio_off_q4=15), dict(ratio_off_q4=81), dict(ratio_on_q4=15, ratio_off_q4=15),
            dict(dn=16), dict(up=16), dict(up_v=16), dict(asm_shift=16), dict(order=11), dict(hang_short=11)]
GOOD_CFGS = [dict(nf_min=1), dict(nf_min=1 << 24, nf_max=1 << 24), dict(ratio_off_q4=16, ratio_on_q4=16), dict(ratio_on_q4=255, ratio_off_q4=255),
             dict(dn=15, up=15, up_v=15, asm_shift=15), dict(dn=0, up=0, up_v=0, asm_shift=0), dict(order=0), dict(hang_short=10), dict(hang_long=0, hang_short=0),
             dict(thr_abs=0), dict(thr_abs=0xFFFFFFFF), dict(burst=0, dtx=0, sid_every=65535, sid_delta=0, sid_gap=255, vox_on=0, vox_off=255)]

# (overrides, rc, run, the verdict names its rule).  Sizes at the base shape: g711 2 400, codec 5, pcm 4 800, ctl 5, state 640, kind 15,
# rec 240, sid 240, txctl 15, events 64, count 8, work 32 (272 without d_rec)
CASES = [
    (dict(), 0, 1, 0), (PCM, 0, 1, 0), (dict(cfg="0"), 0, 1, 0), (NOLIST, 0, 1, 0), ({**NOLIST, "ctl": "0", "kind": "0", "rec": "0", "sid": "0"}, 0, 1, 0),
    ({**NOLIST, "rec": "0", "sid": "0", "txctl": "0"}, 0, 1, 0), (NOOUT, 0, 1, 0), (dict(n=16), 0, 1, 0), (dict(n=256), 0, 1, 0), (dict(n=24), 0, 1, 0),
    # 1. the frame length and the cfg, whether or not there is work
    (dict(n=0), EINVAL, 0, 0), (dict(n=8), EINVAL, 0, 0), (dict(n=20), EINVAL, 0, 0), (dict(n=162), EINVAL, 0, 0), (dict(n=264), EINVAL, 0, 0),
    (dict(C=0, n=8), EINVAL, 0, 0), (dict(F=0, n=257), EINVAL, 0, 0),
    *[(dict(cfg=cfg(**b)), EINVAL, 0, 0) for b in BAD_CFGS], *[(dict(cfg=cfg(**b), C=0), EINVAL, 0, 0) for b in BAD_CFGS[:3]],
    *[(dict(cfg=cfg(**g)), 0, 1, 0) for g in GOOD_CFGS],
    # 2. the list's own rules, ahead of nothing to do: the counts 4-byte, the work 16-byte aligned and there, events unless cap is 0
    (dict(count="x2"), EINVAL, 0, 0), (dict(count="x4"), 0, 1, 0), (dict(work="x8"), EINVAL, 0, 0), (dict(work="0"), EINVAL, 0, 0),
    (dict(events="0"), EINVAL, 0, 0), (dict(events="0", cap=0), 0, 1, 0), (dict(C=0, work="0"), EINVAL, 0, 0), (dict(C=0, count="x1"), EINVAL, 0, 0),
    (dict(count="0", work="0"), 0, 1, 0), (dict(count="0", events="0", work="x8"), EINVAL, 0, 0),
    # 3. nothing to do: with a list the counts are still written, whatever else is wrong
    (dict(C=0), 0, 1, 0), (dict(F=0), 0, 1, 0), ({**NOLIST, "C": 0}, 0, 0, 0), ({**NOLIST, "F": 0}, 0, 0, 0),
    ({**NOLIST, "C": 0, "g711": "0", "state": "0", "rec": "x2", "kind": "0"}, 0, 0, 0), (dict(C=0, g711="0", state="0"), 0, 1, 0),
    # 4. exactly one input form, the codes with their laws, the state, at least one output or the list
    (dict(g711="0"), EINVAL, 0, 0), (dict(pcm="x"), EINVAL, 0, 0), (dict(codec="0"), EINVAL, 0, 0), (dict(state="0"), EINVAL, 0, 0),
    ({**NOLIST, **NOOUT}, EINVAL, 0, 0), ({**PCM, "codec": "x"}, 0, 1, 0),
    # 5. the range: channels x frames
    (BIG, ERANGE, 0, 0), (dict(C=0xFFFFFFE0, F=1), ERANGE, 0, 0), ({**NOLIST, "C": 0xFFFFFFDF, "F": 1}, 0, 1, 0),
    ({**BIG, "n": 0}, EINVAL, 0, 0), ({**BIG, "state": "0"}, EINVAL, 0, 0), ({**BIG, **NOLIST, **NOOUT}, EINVAL, 0, 0),
    # 6. alignment: 8 for the codes, 16 for the PCM rows, the state, the records, the payloads and the events
    ({**PCM, "pcm": "x2"}, EINVAL, 0, 0), ({**PCM, "pcm": "x8"}, EINVAL, 0, 0), (dict(g711="x1"), EINVAL, 0, 0), (dict(g711="x4"), EINVAL, 0, 0),
    (dict(rec="x8"), EINVAL, 0, 0), (dict(sid="x8"), EINVAL, 0, 0), (dict(sid="x4"), EINVAL, 0, 0), (dict(events="x8"), EINVAL, 0, 0),
    (dict(state="x8"), EINVAL, 0, 0), (dict(state="x4"), EINVAL, 0, 0),
    (dict(g711="x8", codec="x3", ctl="x1", state="x16", kind="x1", rec="x16", sid="x16", txctl="x3", events="x16", count="x4", work="x16"), 0, 1, 0),
    ({**PCM, "pcm": "x16"}, 0, 1, 0),
    ({**BIG, "rec": "x4"}, ERANGE, 0, 0),                                 # too many frames wins over the alignment
    # 7. the state or an output that overlaps an input, or another of them: the rule with a text; the alignment wins over it
    (dict(state="g711"), EINVAL, 0, 1), (dict(state="g711+2384"), EINVAL, 0, 1), (dict(state="g711+2400"), 0, 1, 0),
    (dict(kind="ctl"), EINVAL, 0, 1), (dict(kind="ctl+4"), EINVAL, 0, 1), (dict(kind="ctl+5"), 0, 1, 0), (dict(txctl="codec+4"), EINVAL, 0, 1),
    ({**PCM, "sid": "pcm+4784"}, EINVAL, 0, 1), ({**PCM, "sid": "pcm+4800"}, 0, 1, 0), ({**PCM, "kind": "codec"}, 0, 1, 0),
    (dict(rec="state+624"), EINVAL, 0, 1), (dict(rec="state+640"), 0, 1, 0), (dict(sid="rec+224"), EINVAL, 0, 1), (dict(sid="rec+240"), 0, 1, 0),
    (dict(txctl="kind+14"), EINVAL, 0, 1), (dict(txctl="kind+15"), 0, 1, 0), (dict(kind="sid+239"), EINVAL, 0, 1), (dict(kind="sid+240"), 0, 1, 0),
    (dict(events="rec+224"), EINVAL, 0, 1), (dict(events="rec+240"), 0, 1, 0), (dict(rec="events+48"), EINVAL, 0, 1), (dict(rec="events+64"), 0, 1, 0),
    (dict(count="events+60"), EINVAL, 0, 1), (dict(count="events+64"), 0, 1, 0), (dict(work="count"), EINVAL, 0, 1), (dict(kind="work+31"), EINVAL, 0, 1),
    (dict(kind="work+32"), 0, 1, 0), (dict(rec="0", kind="work+271"), EINVAL, 0, 1), (dict(rec="0", kind="work+272"), 0, 1, 0),
    (dict(work="state+16"), EINVAL, 0, 1), (dict(txctl="count+7"), EINVAL, 0, 1),
    (dict(rec="sid+232"), EINVAL, 0, 0),                                  # misaligned and overlapping: no text
    (dict(codec="g711", ctl="g711"), 0, 1, 0),                            # inputs may share memory
    ({**NOLIST, "events": "rec", "work": "rec"}, 0, 1, 0),                # without a list neither d_events nor d_work is a buffer
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("vad_args") / "vad_args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "vad_args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    lines = [" ".join(f"{k}={v}" for k, v in {**BASE, **over}.items()) for over, _, _, _ in CASES]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [dict(kv.split("=") for kv in line.split()) for line in out]


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{j}:" + (",".join(f"{k}={v}" for k, v in c[0].items()) or "base")[:60] for j, c in enumerate(CASES)])
def test_rule(verdicts, i):
    _, rc, run, why = CASES[i]
    v = verdicts[i]
    assert (int(v["rc"]), int(v["run"]), int(v["why"])) == (rc, run, why)
