"""-m "not gpu": the argument rule of igdsp_echo_cancel (ec_run in csrc/igdsp_args.h), compiled with g++ alone through
tests/route/ec_args_driver.cpp: every clause in its order and which code wins when two apply: the frame length and the cfg ahead of
nothing to do, the input form, the far end and the state, the range, the alignment (the codes 2, PCM rows and d_far_of 4, the PCM
records 8, the state and the records 16 bytes: what the kernel's loads and stores take), the overlap of byte ranges.
tests/test_gpu_ec.py replays the clauses through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL, ERANGE = -22, -34
BASE = dict(g711="x", codec="x", pcm="0", far="x", P=4, far_of="x", ctl="x", cfg="256:2", state="x", out="x", rec="x", stats="x", C=5, F=3, n=160)
PCM = dict(g711="0", codec="0", pcm="x")
BIG = dict(C=0x10000000, F=16)

# (overrides, rc, run, the verdict names its rule).  Sizes at the base shape: g711 2 400, codec 5, pcm 4 800, far 3 840, far_of 20,
# ctl 5, state 7 760, out 4 800, rec 240, stats 240
CASES = [
    (dict(), 0, 1, 0), (PCM, 0, 1, 0), (dict(cfg="0"), 0, 1, 0), (dict(cfg="128:0"), 0, 1, 0), (dict(cfg="256:6"), 0, 1, 0),
    (dict(far_of="0", ctl="0", out="0", rec="0", stats="0"), 0, 1, 0), (dict(n=2), 0, 1, 0), (dict(n=256), 0, 1, 0), (dict(n=164), 0, 1, 0),
    # 1. the frame length and the cfg, whether or not there is work
    (dict(n=0), EINVAL, 0, 0), (dict(n=1), EINVAL, 0, 0), (dict(n=161), EINVAL, 0, 0), (dict(n=258), EINVAL, 0, 0), (dict(C=0, n=3), EINVAL, 0, 0),
    (dict(cfg="64:2"), EINVAL, 0, 0), (dict(cfg="192:2"), EINVAL, 0, 0), (dict(cfg="512:2"), EINVAL, 0, 0), (dict(cfg="0:0"), EINVAL, 0, 0),
    (dict(cfg="256:7"), EINVAL, 0, 0), (dict(F=0, cfg="128:7"), EINVAL, 0, 0),
    # 2. nothing to do, whatever else is wrong
    (dict(C=0), 0, 0, 0), (dict(F=0), 0, 0, 0), (dict(C=0, g711="0", state="0", out="x2"), 0, 0, 0),
    # 3. exactly one input form, the codes with their laws, the far end unless it has no rows, the state
    (dict(g711="0"), EINVAL, 0, 0), (dict(pcm="x"), EINVAL, 0, 0), (dict(codec="0"), EINVAL, 0, 0), (dict(state="0"), EINVAL, 0, 0),
    (dict(far="0"), EINVAL, 0, 0), (dict(far="0", P=0), 0, 1, 0), (dict(P=0), 0, 1, 0), ({**PCM, "codec": "x"}, 0, 1, 0),
    # 4. the range: channels x frames and far rows x frames
    (BIG, ERANGE, 0, 0), (dict(C=0xFFFFFFE0, F=1), ERANGE, 0, 0), (dict(P=0x80000000, F=2), ERANGE, 0, 0),
    (dict(C=0xFFFFFFDF, F=1, P=0, far="0", out="0", rec="0", stats="0", g711="0", pcm="0", codec="0", n=0), EINVAL, 0, 0),
    ({**BIG, "n": 0}, EINVAL, 0, 0), ({**BIG, "state": "0"}, EINVAL, 0, 0),
    # 5. alignment: 2 for the codes, 4 for the PCM rows, the far rows, d_far_of and the output, 8 for the PCM records, 16 for the state
    # and the records: rows go two samples, weights and records 16 bytes at a time
    ({**PCM, "pcm": "x1"}, EINVAL, 0, 0), ({**PCM, "pcm": "x2"}, EINVAL, 0, 0), (dict(g711="x1"), EINVAL, 0, 0), (dict(g711="x3"), EINVAL, 0, 0),
    (dict(far="x2"), EINVAL, 0, 0), (dict(far_of="x2"), EINVAL, 0, 0), (dict(out="x2"), EINVAL, 0, 0), (dict(stats="x4"), EINVAL, 0, 0),
    (dict(rec="x8"), EINVAL, 0, 0), (dict(state="x8"), EINVAL, 0, 0), (dict(state="x4"), EINVAL, 0, 0),
    (dict(g711="x2", codec="x3", far="x4", far_of="x4", ctl="x1", state="x16", out="x4", rec="x16", stats="x8"), 0, 1, 0),
    ({**PCM, "pcm": "x4"}, 0, 1, 0),
    ({**BIG, "rec": "x4"}, ERANGE, 0, 0),                                 # too many frames wins over the alignment
    # 6. the state or an output that overlaps an input, or another of them: the rule with a text; the alignment wins over it
    (dict(state="g711"), EINVAL, 0, 1), (dict(state="g711+2384"), EINVAL, 0, 1), (dict(state="g711+2400"), 0, 1, 0),
    (dict(out="far+3836"), EINVAL, 0, 1), (dict(out="far+3840"), 0, 1, 0), (dict(rec="far_of+16"), EINVAL, 0, 1), (dict(rec="far_of+32"), 0, 1, 0),
    (dict(stats="ctl"), EINVAL, 0, 1), (dict(stats="ctl+8"), 0, 1, 0), (dict(out="codec+4"), EINVAL, 0, 1), (dict(out="codec+8"), 0, 1, 0),
    ({**PCM, "out": "pcm+4796"}, EINVAL, 0, 1), ({**PCM, "out": "pcm+4800"}, 0, 1, 0), ({**PCM, "out": "codec"}, 0, 1, 0),
    (dict(out="state+7756"), EINVAL, 0, 1), (dict(out="state+7760"), 0, 1, 0), (dict(rec="out+4784"), EINVAL, 0, 1), (dict(rec="out+4800"), 0, 1, 0),
    (dict(stats="rec+232"), EINVAL, 0, 1), (dict(stats="rec+240"), 0, 1, 0), (dict(stats="state+7752"), EINVAL, 0, 1),
    (dict(rec="out+4788"), EINVAL, 0, 0),                                 # misaligned and overlapping: no text
    (dict(P=0, out="far"), 0, 1, 0),                                      # no far rows: nothing of d_far_pcm is read
    (dict(codec="g711", ctl="far", far_of="far"), 0, 1, 0),               # inputs may share memory
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("ec_args") / "ec_args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "ec_args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
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
