"""-m "not gpu": the AES-GCM SRTP rule's two per-packet functions under AddressSanitizer and UndefinedBehaviorSanitizer.
tests/san/srtp_gcm_san_driver.cpp is a stand-alone program with its own main, compiled here with -fsanitize=address,undefined against
csrc/igdsp_srtp_gcm.h alone (no library, no HIP, nothing loaded into Python): the malformed packets, a few thousand seeded random byte
strings as packets, a tampered stream across the sequence wrap under both key sizes, and states of random bytes and of the other
suites, every buffer a heap block of exactly the size passed.  It runs as a child process and has to end clean."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")


def test_per_packet_rules_under_asan_ubsan(tmp_path):
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if shutil.which("g++") is None or subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, timeout=300).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")            # decided on a trivial program: an error in the driver fails below
    exe = str(tmp_path / "srtp_gcm_san_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "san", "srtp_gcm_san_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-300:] + r.stderr[-2000:]
    line = r.stdout.strip().splitlines()[-1]
    assert line.startswith("ok "), line
    counts = {k: int(v) for k, v in (kv.split("=") for kv in line.split()[1:])}
    # every outcome of the rule was reached, the refusals in numbers
    assert all(counts[k] > 0 for k in ("no_key", "ok", "auth_fail", "replay", "old", "malformed", "empty", "rolled", "bypassed")), counts
    assert counts["malformed"] > 1000 and counts["ok"] > 3000, counts
