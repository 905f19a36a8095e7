"""-m "not gpu": the argument rules of igdsp_rtcp_build, igdsp_rtcp_parse and igdsp_srtcp_protect / igdsp_srtcp_unprotect (rtcp_build,
rtcp_parse, srtcp_run in csrc/igdsp_args.h), compiled with g++ alone through tests/route/rtcp_args_driver.cpp: every clause in its
order and which code wins when two apply: the stride ahead of everything, nothing to do, the required buffers, d_cname with
d_cname_len (with a text), the range, the alignment the kernels' loads and stores take, the overlap of byte ranges (with a text).
SRTCP's rule is SRTP's, in place included.  tests/test_gpu_rtcp.py replays clauses through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL, ERANGE = -22, -34
NAMES = "ctl jb src now cname cname_len state packets sizes rec out sizes_out arrival local".split()
BASE = dict({k: "x" for k in NAMES}, C=5, F=3, stride=152, ostride=152)
BIG = dict(C=0x10000000, F=16)

# (rule, overrides, rc, run, the verdict names its rule).  Sizes at the base shape: ctl 15, jb 400, src 240, now 24, cname 320,
# cname_len 5, state 400 (srtcp: 1 440), packets 2 280, sizes 30, rec 120 (parse: 480), arrival 60, local 20
CASES = [
    ("build", dict(), 0, 1, 0), ("build", dict(jb="0", rec="0", cname="0", cname_len="0"), 0, 1, 0), ("build", dict(stride=136), 0, 1, 0), ("build", dict(stride=2048), 0, 1, 0),
    ("build", dict(stride=132), EINVAL, 0, 0), ("build", dict(stride=150), EINVAL, 0, 0), ("build", dict(stride=2052), EINVAL, 0, 0), ("build", dict(C=0, stride=12), EINVAL, 0, 0),
    ("build", dict(C=0), 0, 0, 0), ("build", dict(F=0, state="0", src="x3"), 0, 0, 0),
    ("build", dict(ctl="0"), EINVAL, 0, 0), ("build", dict(src="0"), EINVAL, 0, 0), ("build", dict(now="0"), EINVAL, 0, 0), ("build", dict(state="0"), EINVAL, 0, 0),
    ("build", dict(packets="0"), EINVAL, 0, 0), ("build", dict(sizes="0"), EINVAL, 0, 0),
    ("build", dict(cname="0"), EINVAL, 0, 1), ("build", dict(cname_len="0"), EINVAL, 0, 1), ("build", dict(cname="0", ctl="0"), EINVAL, 0, 0),
    ("build", BIG, ERANGE, 0, 0), ("build", dict(C=0xFFFFFFDF, F=1), 0, 1, 0), ("build", {**BIG, "src": "0"}, EINVAL, 0, 0), ("build", {**BIG, "rec": "x4"}, ERANGE, 0, 0),
    ("build", dict(sizes="x1"), EINVAL, 0, 0), ("build", dict(packets="x2"), EINVAL, 0, 0), ("build", dict(now="x4"), EINVAL, 0, 0), ("build", dict(rec="x4"), EINVAL, 0, 0),
    ("build", dict(jb="x8"), EINVAL, 0, 0), ("build", dict(src="x8"), EINVAL, 0, 0), ("build", dict(cname="x4"), EINVAL, 0, 0), ("build", dict(state="x8"), EINVAL, 0, 0),
    ("build", dict(ctl="x1", cname_len="x3", sizes="x2", packets="x4", now="x8", rec="x8", jb="x16", src="x16", cname="x16", state="x16"), 0, 1, 0),
    ("build", dict(packets="src"), EINVAL, 0, 1), ("build", dict(packets="src+240"), 0, 1, 0), ("build", dict(state="jb"), EINVAL, 0, 1), ("build", dict(state="jb+384"), EINVAL, 0, 1),
    ("build", dict(state="jb+400"), 0, 1, 0), ("build", dict(rec="state+392"), EINVAL, 0, 1), ("build", dict(rec="state+400"), 0, 1, 0), ("build", dict(sizes="packets+2278"), EINVAL, 0, 1),
    ("build", dict(sizes="cname_len+4"), EINVAL, 0, 1), ("build", dict(sizes="cname_len+6"), 0, 1, 0), ("build", dict(rec="now+16"), EINVAL, 0, 1), ("build", dict(rec="now+24"), 0, 1, 0),
    ("build", dict(ctl="src", jb="cname"), 0, 1, 0),                        # inputs may share memory
    ("parse", dict(), 0, 1, 0), ("parse", dict(rec="0"), 0, 1, 0), ("parse", dict(stride=8), 0, 1, 0), ("parse", dict(stride=2048), 0, 1, 0),
    ("parse", dict(stride=4), EINVAL, 0, 0), ("parse", dict(stride=150), EINVAL, 0, 0), ("parse", dict(stride=2052), EINVAL, 0, 0), ("parse", dict(F=0, stride=4), EINVAL, 0, 0),
    ("parse", dict(C=0, state="0"), 0, 0, 0), ("parse", dict(F=0), 0, 0, 0),
    ("parse", dict(packets="0"), EINVAL, 0, 0), ("parse", dict(sizes="0"), EINVAL, 0, 0), ("parse", dict(arrival="0"), EINVAL, 0, 0), ("parse", dict(local="0"), EINVAL, 0, 0),
    ("parse", dict(state="0"), EINVAL, 0, 0), ("parse", BIG, ERANGE, 0, 0), ("parse", {**BIG, "state": "0"}, EINVAL, 0, 0),
    ("parse", dict(sizes="x1"), EINVAL, 0, 0), ("parse", dict(packets="x2"), EINVAL, 0, 0), ("parse", dict(arrival="x2"), EINVAL, 0, 0), ("parse", dict(local="x2"), EINVAL, 0, 0),
    ("parse", dict(state="x8"), EINVAL, 0, 0), ("parse", dict(rec="x8"), EINVAL, 0, 0), ("parse", dict(sizes="x2", packets="x4", arrival="x4", local="x4", state="x16", rec="x16"), 0, 1, 0),
    ("parse", dict(rec="packets"), EINVAL, 0, 1), ("parse", dict(rec="packets+2272"), EINVAL, 0, 1), ("parse", dict(rec="packets+2288"), 0, 1, 0), ("parse", dict(state="local+16"), EINVAL, 0, 1),
    ("parse", dict(state="local+32"), 0, 1, 0), ("parse", dict(rec="state+384"), EINVAL, 0, 1), ("parse", dict(rec="state+400"), 0, 1, 0), ("parse", dict(state="arrival+48"), EINVAL, 0, 1),
    ("srtcp", dict(), 0, 1, 0), ("srtcp", dict(ctl="0", rec="0"), 0, 1, 0), ("srtcp", dict(stride=12, ostride=28), 0, 1, 0), ("srtcp", dict(stride=8), EINVAL, 0, 0),
    ("srtcp", dict(ostride=2052), EINVAL, 0, 0), ("srtcp", dict(C=0), 0, 0, 0), ("srtcp", dict(sizes="0"), EINVAL, 0, 1), ("srtcp", dict(state="0"), EINVAL, 0, 0),
    ("srtcp", BIG, ERANGE, 0, 0), ("srtcp", dict(state="x8"), EINVAL, 0, 0), ("srtcp", dict(out="packets", sizes_out="sizes"), 0, 1, 0), ("srtcp", dict(out="packets", ostride=156), EINVAL, 0, 1),
    ("srtcp", dict(rec="state+1432"), EINVAL, 0, 1), ("srtcp", dict(rec="state+1440"), 0, 1, 0),
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("rtcp_args") / "rtcp_args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "rtcp_args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    lines = [" ".join(f"{k}={v}" for k, v in {**BASE, **over, "rule": rule}.items()) for rule, over, _, _, _ in CASES]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [dict(kv.split("=") for kv in line.split()) for line in out]


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{j}:{c[0]}:" + (",".join(f"{k}={v}" for k, v in c[1].items()) or "base")[:60] for j, c in enumerate(CASES)])
def test_rule(verdicts, i):
    _, _, rc, run, why = CASES[i]
    v = verdicts[i]
    assert (int(v["rc"]), int(v["run"]), int(v["why"])) == (rc, run, why)
