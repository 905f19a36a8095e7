"""The route driver of the CPU route tests: tests/route/route_driver.cpp, compiled with g++ once per process against csrc/igdsp_route.h.

run(lines) feeds it case lines ("<entry> key=value ...", the entries route_driver.cpp lists) with IGDSP_* removed from the
environment, so that only a case's own IGDSP_* keys set a knob, and returns one dict of the printed fields per line."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _driver():
    tmp = tempfile.mkdtemp(prefix="igdsp_route_")
    atexit.register(shutil.rmtree, tmp, True)
    exe = os.path.join(tmp, "route_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    return exe


def run(lines):
    env = {k: v for k, v in os.environ.items() if not k.startswith("IGDSP_")}
    r = subprocess.run([_driver()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [dict(kv.split("=") for kv in line.split()) for line in out]
