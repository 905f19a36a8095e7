"""-m "not gpu": the argument rule of igdsp_srtp_gcm_protect / igdsp_srtp_gcm_unprotect (srtp_gcm_run in csrc/igdsp_args.h), compiled with g++ alone
through tests/route/srtp_gcm_args_driver.cpp: every clause in its order and which code wins when two apply: the strides ahead of
everything, nothing to do, d_sizes (required here, with a text), the required buffers, the range, the alignment (sizes 2, packets 4,
records 8, the state 16 bytes: what the kernel's loads and stores take), the overlap of byte ranges with in place as the one
exception.  tests/test_gpu_srtp_gcm.py replays clauses through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL, ERANGE = -22, -34
BASE = dict(ctl="x", packets="x", sizes="x", state="x", out="x", sizes_out="x", rec="x", C=5, F=3, stride=192, ostride=192)
BIG = dict(C=0x10000000, F=16)

# (overrides, rc, run, the verdict names its rule).  Sizes at the base shape: ctl 15, packets 2 880, sizes 30, state 1 600 (five igdsp_srtp_gcm_state), out 2 880,
# sizes_out 30, rec 120
CASES = [
    (dict(), 0, 1, 0), (dict(ctl="0"), 0, 1, 0), (dict(rec="0"), 0, 1, 0), (dict(stride=12, ostride=24), 0, 1, 0), (dict(stride=2048, ostride=2048), 0, 1, 0),
    (dict(stride=180, ostride=192), 0, 1, 0),
    # 1. the strides, whether or not there is work
    (dict(stride=0), EINVAL, 0, 0), (dict(stride=8), EINVAL, 0, 0), (dict(stride=190), EINVAL, 0, 0), (dict(stride=2052), EINVAL, 0, 0),
    (dict(ostride=0), EINVAL, 0, 0), (dict(ostride=8), EINVAL, 0, 0), (dict(ostride=193), EINVAL, 0, 0), (dict(ostride=4096), EINVAL, 0, 0),
    (dict(C=0, stride=190), EINVAL, 0, 0), (dict(F=0, ostride=2052), EINVAL, 0, 0),
    # 2. nothing to do, whatever else is wrong
    (dict(C=0), 0, 0, 0), (dict(F=0), 0, 0, 0), (dict(C=0, state="0", sizes="0", out="x2"), 0, 0, 0),
    # 3. d_sizes is required (with a text), then the other buffers
    (dict(sizes="0"), EINVAL, 0, 1), (dict(sizes="0", packets="0"), EINVAL, 0, 1), (dict(packets="0"), EINVAL, 0, 0), (dict(state="0"), EINVAL, 0, 0),
    (dict(out="0"), EINVAL, 0, 0), (dict(sizes_out="0"), EINVAL, 0, 0),
    # 4. the range: channels x frames
    (BIG, ERANGE, 0, 0), (dict(C=0xFFFFFFE0, F=1), ERANGE, 0, 0), (dict(C=0xFFFFFFDF, F=1), 0, 1, 0),
    ({**BIG, "stride": 190}, EINVAL, 0, 0), ({**BIG, "state": "0"}, EINVAL, 0, 0), ({**BIG, "sizes": "0"}, EINVAL, 0, 1),
    # 5. alignment
    (dict(sizes="x1"), EINVAL, 0, 0), (dict(sizes_out="x1"), EINVAL, 0, 0), (dict(packets="x2"), EINVAL, 0, 0), (dict(out="x2"), EINVAL, 0, 0),
    (dict(out="x1"), EINVAL, 0, 0), (dict(rec="x4"), EINVAL, 0, 0), (dict(state="x8"), EINVAL, 0, 0), (dict(state="x4"), EINVAL, 0, 0),
    (dict(ctl="x1", packets="x4", sizes="x2", state="x16", out="x4", sizes_out="x2", rec="x8"), 0, 1, 0),
    ({**BIG, "rec": "x4"}, ERANGE, 0, 0),                                 # too many frames wins over the alignment
    # 6. in place: the packets with equal strides, the sizes; each alone as well
    (dict(out="packets"), 0, 1, 0), (dict(sizes_out="sizes"), 0, 1, 0), (dict(out="packets", sizes_out="sizes"), 0, 1, 0),
    (dict(out="packets", ostride=196), EINVAL, 0, 1), (dict(out="packets", stride=188), EINVAL, 0, 1),
    (dict(out="packets+192"), EINVAL, 0, 1), (dict(out="packets+2876"), EINVAL, 0, 1), (dict(out="packets+2880"), 0, 1, 0),
    (dict(sizes_out="sizes+2"), EINVAL, 0, 1), (dict(sizes_out="sizes+28"), EINVAL, 0, 1), (dict(sizes_out="sizes+30"), 0, 1, 0),
    # 7. any other overlap: the rule with a text; the alignment wins over it
    (dict(state="packets"), EINVAL, 0, 1), (dict(state="packets+2864"), EINVAL, 0, 1), (dict(state="packets+2880"), 0, 1, 0),
    (dict(rec="ctl"), EINVAL, 0, 1), (dict(rec="ctl+8"), EINVAL, 0, 1), (dict(rec="ctl+16"), 0, 1, 0), (dict(rec="sizes+24"), EINVAL, 0, 1),
    (dict(out="sizes"), EINVAL, 0, 1), (dict(sizes_out="packets"), EINVAL, 0, 1), (dict(sizes_out="ctl+14"), EINVAL, 0, 1), (dict(sizes_out="ctl+16"), 0, 1, 0),
    (dict(out="state+1596"), EINVAL, 0, 1), (dict(out="state+1600"), 0, 1, 0), (dict(sizes_out="out+2878"), EINVAL, 0, 1), (dict(sizes_out="out+2880"), 0, 1, 0),
    (dict(rec="sizes_out+24"), EINVAL, 0, 1), (dict(rec="sizes_out+32"), 0, 1, 0), (dict(rec="out+2872"), EINVAL, 0, 1), (dict(rec="state+1592"), EINVAL, 0, 1),
    (dict(rec="state+1596"), EINVAL, 0, 0),                               # misaligned and overlapping: no text
    (dict(out="state+1440"), EINVAL, 0, 1), (dict(rec="state+1440"), EINVAL, 0, 1),   # five igdsp_srtp_state would end here; five GCM states do not
    (dict(ctl="packets"), 0, 1, 0), (dict(ctl="sizes"), 0, 1, 0),       # inputs may share memory
    (dict(ctl="packets", out="packets"), EINVAL, 0, 1),                   # but then the output written in place overlaps the other input
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("srtp_gcm_args") / "srtp_gcm_args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "srtp_gcm_args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
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
