"""-m "not gpu": the argument rules of igdsp_snd_combine / igdsp_snd_split (snd_combine / snd_split in csrc/igdsp_args.h), compiled with
g++ alone through tests/route/snd_args_driver.cpp: every clause in its order, which code wins when two apply, nothing to do at D = 0 and
F = 0, the row count taken in 64 bits, both single-output forms.  tests/test_gpu_snd.py replays the clauses through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL, ERANGE = -22, -34
BASE = dict(D=3, K=6, F=2, n=160, bulk="a", stats="a")
BASE["in"] = "a"

# (overrides, rc, run, the verdict names its rule)
CASES = [
    (dict(), 0, 1, 0),
    # 1. nothing to do comes first, whatever else is wrong
    (dict(D=0), 0, 0, 0),
    (dict(F=0), 0, 0, 0),
    ({"D": 0, "in": "0", "bulk": "0", "stats": "0", "K": 0, "n": 0}, 0, 0, 0),
    (dict(F=0, K=99, n=9999, bulk="in", stats="a4"), 0, 0, 0),
    # 2. the input, and at least one output
    ({"in": "0"}, EINVAL, 0, 0),
    (dict(bulk="0", stats="0"), EINVAL, 0, 0),
    (dict(bulk="0"), 0, 1, 0),                                          # records only
    (dict(stats="0"), 0, 1, 0),                                         # bulk only
    # 3. the channel count
    (dict(K=0), EINVAL, 0, 0),
    (dict(K=9), EINVAL, 0, 0),
    (dict(K=1), 0, 1, 0),
    (dict(K=8), 0, 1, 0),
    # 4. the shape: n first, then the rows
    (dict(n=0), EINVAL, 0, 0),
    (dict(n=257), EINVAL, 0, 0),
    (dict(n=1), 0, 1, 0),
    (dict(n=256), 0, 1, 0),
    (dict(D=0x10000000, F=3), ERANGE, 0, 0),                            # 18 * 2^28 rows x frames
    (dict(D=0x1FFFFFFB, K=8, F=1), 0, 1, 0),                            # 2^32 - 40: the last that fits
    (dict(D=0x1FFFFFFC, K=8, F=1), ERANGE, 0, 0),                       # 2^32 - 32
    (dict(D=0x20000000, K=8, F=1), ERANGE, 0, 0),                       # D * K = 2^32: would wrap to 0 in 32 bits
    (dict(D=0x80000000, K=8, F=0xFFFFFFFF), ERANGE, 0, 0),              # D * K * F past 64 bits
    (dict(D=0x10000000, F=3, n=0), EINVAL, 0, 0),                       # a bad n wins over too many rows
    (dict(D=0x10000000, F=3, K=9), EINVAL, 0, 0),                       # a bad K wins over both
    (dict(K=9, n=0, bulk="0", stats="0"), EINVAL, 0, 0),
    # 5. alignment: 2 for the bulk buffers, 8 for the records
    ({"in": "a1"}, EINVAL, 0, 0),
    (dict(bulk="a1"), EINVAL, 0, 0),
    (dict(stats="a4"), EINVAL, 0, 0),
    ({"in": "a2", "bulk": "a6", "stats": "a8"}, 0, 1, 0),
    (dict(D=0x10000000, F=3, bulk="a1"), ERANGE, 0, 0),                 # too many rows wins over the alignment
    # 6. the output is the input: the one rule with a text; the alignment wins over it
    (dict(bulk="in"), EINVAL, 0, 1),
    (dict(bulk="in", stats="a4"), EINVAL, 0, 0),
    ({"in": "a1", "bulk": "in"}, EINVAL, 0, 0),
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("snd_args") / "snd_args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "snd_args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    lines = [f"{rule} " + " ".join(f"{k}={v}" for k, v in {**BASE, **over}.items()) for rule in ("snd_combine", "snd_split") for over, _, _, _ in CASES]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [dict(kv.split("=") for kv in line.split()) for line in out]


@pytest.mark.parametrize("rule", [0, 1], ids=["snd_combine", "snd_split"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[",".join(f"{k}={v}" for k, v in c[0].items()) or "base" for c in CASES])
def test_rule(verdicts, rule, i):
    _, rc, run, why = CASES[i]
    v = verdicts[rule * len(CASES) + i]
    assert (int(v["rc"]), int(v["run"]), int(v["why"])) == (rc, run, why)
