"""-m "not gpu": the argument rules of the batched C entries (csrc/igdsp_args.h), compiled with g++ through
tests/route/args_driver.cpp and run over the table in tests/args_cases.py: for every row the code the entry returns and whether it
would launch.  The header is host-only, so every rule runs here; tests/test_gpu_args.py replays the rows that launch nothing through
the library."""
import os
import shutil
import subprocess

import pytest

from tests import args_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("args") / "args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], input="\n".join(ac.line(e, kv) for e, kv, _, _ in ac.CASES) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(ac.CASES)
    return [dict(kv.split("=") for kv in line.split()) for line in out]


def test_table_is_well_formed():
    assert set(ac.SIG) == set(ac.BASE) == {e for e, _, _, _ in ac.CASES}
    for entry, sig in ac.SIG.items():
        keys = [k for k, _ in sig]
        extra = [f"win.{f}" for f in ac.WIN_FIELDS] if "win" in keys else [f"cfg.{f}" for f in ac.CFG_FIELDS] if "cfg" in keys else []
        assert set(ac.BASE[entry]) == set(keys + extra), entry
    ids = [ac.case_id(c) for c in ac.CASES]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    for entry, kv, rc, run in ac.CASES:
        ac.full(entry, kv)
        assert rc in (0, ac.EINVAL, ac.ERANGE) and run in (0, 1) and not (run and rc), ac.case_id((entry, kv, rc, run))
    for entry in ac.SIG:                                      # every entry launches, has nothing to do and rejects somewhere in the table
        seen = {(rc, run) for e, _, rc, run in ac.CASES if e == entry}
        assert {(0, 1), (0, 0), (ac.EINVAL, 0)} <= seen, entry


@pytest.mark.parametrize("i", range(len(ac.CASES)), ids=[ac.case_id(c) for c in ac.CASES])
def test_rule(verdicts, i):
    _, _, rc, run = ac.CASES[i]
    assert (int(verdicts[i]["rc"]), int(verdicts[i]["run"])) == (rc, run)
