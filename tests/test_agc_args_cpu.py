"""-m "not gpu": the argument rule of igdsp_agc_run (agc_run in csrc/igdsp_args.h), compiled with g++ alone through
tests/route/agc_args_driver.cpp: every clause in its order and which code wins when two apply: the frame length and the cfg ahead of
nothing to do, the input form, the state and at least one output, the range, the alignment (the codes and the PCM records 8, PCM rows,
the state and the records 16 bytes: what the kernel's loads and stores take), the overlap of byte ranges.
tests/test_gpu_agc.py replays the clauses through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL, ERANGE = -22, -34
DEF = dict(target=8192, ceil=23170, gate=256, gmin=1024, gmax=32768, att=1, rel=5, up=5, down=2, lrel=6)


def cfg(**kw):
    return ":".join(str(v) for v in {**DEF, **kw}.values())


BASE = dict(g711="x", codec="x", pcm="0", ctl="x", cfg=cfg(), state="x", out="x", rec="x", stats="x", C=5, F=3, n=160)
PCM = dict(g711="0", codec="0", pcm="x")
BIG = dict(C=0x10000000, F=16)
BAD_CFGS = [dict(gate=0), dict(target=0), dict(target=23171), dict(ceil=32768), dict(ceil=8191), dict(gmin=0), dict(gmin=4097), dict(gmax=4095),
            dict(att=16), dict(rel=16), dict(up=16), dict(down=16), dict(lrel=0), dict(lrel=16)]
GOOD_CFGS = [dict(gate=1), dict(gate=65535), dict(target=1), dict(target=23170), dict(ceil=32767, target=32767), dict(ceil=8192), dict(gmin=1),
             dict(gmin=4096), dict(gmax=4096), dict(gmax=65535), dict(att=15, rel=15, up=15, down=15, lrel=15), dict(att=0, rel=0, up=0, down=0, lrel=1)]

# (overrides, rc, run, the verdict names its rule).  Sizes at the base shape: g711 2 400, codec 5, pcm 4 800, ctl 5, state 80, out 4 800,
# rec 240, stats 240
CASES = [
    (dict(), 0, 1, 0), (PCM, 0, 1, 0), (dict(cfg="0"), 0, 1, 0), (dict(ctl="0", out="0", rec="0"), 0, 1, 0), (dict(ctl="0", rec="0", stats="0"), 0, 1, 0),
    (dict(out="0", stats="0"), 0, 1, 0), (dict(n=8), 0, 1, 0), (dict(n=256), 0, 1, 0), (dict(n=24), 0, 1, 0),
    # 1. the frame length and the cfg, whether or not there is work
    (dict(n=0), EINVAL, 0, 0), (dict(n=4), EINVAL, 0, 0), (dict(n=12), EINVAL, 0, 0), (dict(n=162), EINVAL, 0, 0), (dict(n=264), EINVAL, 0, 0),
    (dict(C=0, n=7), EINVAL, 0, 0), (dict(F=0, n=257), EINVAL, 0, 0),
    *[(dict(cfg=cfg(**b)), EINVAL, 0, 0) for b in BAD_CFGS], *[(dict(cfg=cfg(**b), C=0), EINVAL, 0, 0) for b in BAD_CFGS[:3]],
    *[(dict(cfg=cfg(**g)), 0, 1, 0) for g in GOOD_CFGS],
    # 2. nothing to do, whatever else is wrong
    (dict(C=0), 0, 0, 0), (dict(F=0), 0, 0, 0), (dict(C=0, g711="0", state="0", out="x2", rec="0", stats="0"), 0, 0, 0),
    # 3. exactly one input form, the codes with their laws, the state, at least one output
    (dict(g711="0"), EINVAL, 0, 0), (dict(pcm="x"), EINVAL, 0, 0), (dict(codec="0"), EINVAL, 0, 0), (dict(state="0"), EINVAL, 0, 0),
    (dict(out="0", rec="0", stats="0"), EINVAL, 0, 0), ({**PCM, "codec": "x"}, 0, 1, 0),
    # 4. the range: channels x frames
    (BIG, ERANGE, 0, 0), (dict(C=0xFFFFFFE0, F=1), ERANGE, 0, 0), (dict(C=0xFFFFFFDF, F=1), 0, 1, 0),
    ({**BIG, "n": 0}, EINVAL, 0, 0), ({**BIG, "state": "0"}, EINVAL, 0, 0), ({**BIG, "out": "0", "rec": "0", "stats": "0"}, EINVAL, 0, 0),
    # 5. alignment: 8 for the codes and the PCM records, 16 for the PCM rows, the output, the state and the records
    ({**PCM, "pcm": "x2"}, EINVAL, 0, 0), ({**PCM, "pcm": "x8"}, EINVAL, 0, 0), (dict(g711="x1"), EINVAL, 0, 0), (dict(g711="x4"), EINVAL, 0, 0),
    (dict(out="x2"), EINVAL, 0, 0), (dict(out="x8"), EINVAL, 0, 0), (dict(stats="x4"), EINVAL, 0, 0), (dict(rec="x8"), EINVAL, 0, 0),
    (dict(state="x8"), EINVAL, 0, 0), (dict(state="x4"), EINVAL, 0, 0),
    (dict(g711="x8", codec="x3", ctl="x1", state="x16", out="x16", rec="x16", stats="x8"), 0, 1, 0), ({**PCM, "pcm": "x16"}, 0, 1, 0),
    ({**BIG, "rec": "x4"}, ERANGE, 0, 0),                                 # too many frames wins over the alignment
    # 6. the state or an output that overlaps an input, or another of them: the rule with a text; the alignment wins over it
    (dict(state="g711"), EINVAL, 0, 1), (dict(state="g711+2384"), EINVAL, 0, 1), (dict(state="g711+2400"), 0, 1, 0),
    (dict(stats="ctl"), EINVAL, 0, 1), (dict(stats="ctl+8"), 0, 1, 0), (dict(out="codec"), EINVAL, 0, 1), (dict(out="codec+16"), 0, 1, 0),
    ({**PCM, "out": "pcm+4784"}, EINVAL, 0, 1), ({**PCM, "out": "pcm+4800"}, 0, 1, 0), ({**PCM, "out": "codec"}, 0, 1, 0),
    (dict(out="state+64"), EINVAL, 0, 1), (dict(out="state+80"), 0, 1, 0), (dict(rec="out+4784"), EINVAL, 0, 1), (dict(rec="out+4800"), 0, 1, 0),
    (dict(stats="rec+232"), EINVAL, 0, 1), (dict(stats="rec+240"), 0, 1, 0), (dict(stats="state+72"), EINVAL, 0, 1), (dict(rec="state"), EINVAL, 0, 1),
    (dict(rec="out+4792"), EINVAL, 0, 0),                                 # misaligned and overlapping: no text
    (dict(codec="g711", ctl="g711"), 0, 1, 0),                            # inputs may share memory
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("agc_args") / "agc_args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "agc_args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
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
