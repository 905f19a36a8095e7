"""-m "not gpu": ThreadSanitizer over the drop-in receive path's staging (csrc/igdsp_rxstage.h) and the snapshot pool
(csrc/igdsp_snappool.h), neither with a HIP include, driven by tests/san/rx_stage_tsan.cpp: four producer threads (two of them on
the same channels), a thread setting the ED-137 words, an owner snapshotting repeatedly in 4 parts over a pool of 3 helpers.  No data
race, every frame taken once or counted as dropped, per-producer order kept per channel, every word one the setter wrote."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")


def _has_tsan():
    try:
        out = subprocess.run(["g++", "-fsanitize=thread", "-x", "c++", "-", "-o", os.devnull], input=b"int main(){return 0;}",
                             capture_output=True, timeout=60)
        return out.returncode == 0
    except Exception:
        return False


@pytest.mark.skipif(shutil.which("g++") is None or not _has_tsan(), reason="g++ with libtsan not available")
def test_rx_staging_under_tsan(tmp_path):
    exe = tmp_path / "rx_stage_tsan"
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=thread", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           os.path.join(ROOT, "tests", "san", "rx_stage_tsan.cpp"), "-lpthread", "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:exitcode=66")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "rx stage ok" in r.stdout and "ThreadSanitizer" not in r.stderr
