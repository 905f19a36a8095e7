"""-m "not gpu": the routes of igdsp_dbuf_run (dbuf_route in csrc/igdsp_route.h) and the constexpr rule that k_dbuf and igdsp_dbuf_step
share (csrc/igdsp_dbuf.h), compiled with g++ through tests/route/dbuf_route_driver.cpp.  The route table pins the geometry (a wave per
channel, four to a block, parts of 128 steps, the LDS of a block, the vector form by alignment); the step rule is run over cases from
stdin and compared with tests/dbuf_model.py; the same driver is built once more with -fsanitize=address,undefined and run over the
same input as its own program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dbuf_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")

ROUTES = [
    # the bench's shapes: D1 / D2 (128 steps: one part) and D3 (the live gateway's one step)
    ("C=65536 T=128 n=160", "vec=1 grid=16384 threads=256 lds=4480 part_steps=128 parts=1"),
    ("C=65536 T=1 n=160", "vec=1 grid=16384 threads=256 lds=4480 part_steps=1 parts=1"),
    # odd channel counts: the last block has idle waves
    ("C=1 T=1", "grid=1 threads=256"), ("C=4 T=9", "grid=1"), ("C=5 T=9", "grid=2"), ("C=67 T=9", "grid=17 part_steps=9 parts=1"),
    ("C=65537 T=2", "grid=16385"),
    # more steps than a part
    ("C=67 T=129", "part_steps=128 parts=2"), ("C=67 T=130", "part_steps=128 parts=2"), ("C=67 T=256", "parts=2"), ("C=67 T=257", "parts=3"),
    ("C=3 T=100000", "part_steps=128 parts=782"),
    # the frame sizes
    ("C=33 T=40 n=1 M=2", "vec=0 grid=9"), ("C=33 T=40 n=24 M=48", "vec=1"), ("C=33 T=40 n=164 M=1024", "vec=1"),
    ("C=33 T=40 n=256 M=512", "vec=1"), ("C=33 T=40 n=255 M=1024", "vec=0"),
    # the vector form: n even and both row buffers dword aligned
    ("C=3 T=1 in=0x1002", "vec=0"), ("C=3 T=1 out=0x2002", "vec=0"), ("C=3 T=1 in=0x1004 out=0x2004", "vec=1"),
    ("C=3 T=1 in=0x1002 out=0x2002", "vec=0"), ("C=3 T=1 n=7 M=14", "vec=0"),
    # the largest C does not wrap; what the argument rule rejects launches nothing here either
    ("C=0xFFFFFFDF T=1", "grid=1073741816 parts=1"),
    ("C=0xFFFFFFE0 T=1", "grid=0"), ("C=0x10000000 T=16", "grid=0"), ("C=3 T=1 n=0", "grid=0"), ("C=3 T=1 n=257 M=1024", "grid=0"),
    ("C=3 T=1 n=160 M=319", "grid=0"), ("C=3 T=1 n=160 M=1025", "grid=0"),
    ("C=0 T=8", "grid=0 threads=0 parts=0"), ("C=8 T=0", "grid=0 threads=0 parts=0"),
]

# (n, M, steps, P(PUT), P(GET), the state's scalars to start from)
STEPS = [(160, 960, 120, 0.95, 0.80, {}), (160, 320, 60, 0.95, 0.80, {}), (24, 48, 80, 0.95, 0.80, {}), (1, 2, 50, 0.9, 0.9, {}),
         (164, 984, 100, 1.0, 0.7, {}), (256, 1024, 40, 0.95, 0.8, {}), (80, 1024, 150, 1.0, 0.85, {}), (160, 960, 60, 0.8, 0.95, {}),
         (160, 960, 40, 0.9, 0.9, dict(head=5000, len=2000, eff=0, level=65535, max_level=40000, since=60000, last_op=9)),
         (160, 480, 40, 0.9, 0.9, dict(head=1023, len=470, eff=3, level=65534, max_level=65535, since=199, last_op=1))]


def steps_input(i):
    n, M, T, pp, pg, _ = STEPS[i]
    rng = np.random.default_rng(2000 + i)
    ops = ((rng.random(T) < pp) * 1 + (rng.random(T) < pg) * 2).astype(np.uint8)
    kind = i % 3
    x = dm.speech(rng, T, n, 90.0 + 11 * i) if kind == 0 else (dm.square(T, n) if kind == 1 else np.zeros((T, n), np.int16))
    return ops, x


def build(exe, extra):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "dbuf_route_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("dbuf_route")
    exe = str(d / "dbuf_route_driver")
    build(exe, [])
    lines = ["static"] + ["route " + c for c, _ in ROUTES]
    for i, (n, M, T, _, _, start) in enumerate(STEPS):
        ops, x = steps_input(i)
        rows = x[(ops & 1) != 0].reshape(-1)
        lines.append(f"steps n={n} M={M} ops={','.join(map(str, ops))} x={','.join(map(str, rows))} " + " ".join(f"{k}={v}" for k, v in start.items()))
    text = "\n".join(lines) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return {"dir": d, "input": text, "out": r.stdout.splitlines()}


@pytest.mark.parametrize("i", range(len(ROUTES)), ids=[c for c, _ in ROUTES])
def test_dbuf_route(driver, i):
    assert driver["out"][0] == "ok=1"
    got = dict(kv.split("=") for kv in driver["out"][1 + i].split())
    want = dict(kv.split("=") for kv in ROUTES[i][1].split())
    assert {k: got[k] for k in want} == want, f"{ROUTES[i][0]}: {got}"


def test_step_rule_vs_model(driver):
    at = 1 + len(ROUTES)
    events = dict(shrinks=0, dropped=0, underruns=0)
    for i, (n, M, T, _, _, start) in enumerate(STEPS):
        ops, x = steps_input(i)
        st = dm.new_state()
        st.update(start)
        for t in range(T):
            row, flag = dm.step(st, int(ops[t]), x[t], n, M)
            got = [int(v) for v in driver["out"][at].split()]
            at += 1
            assert got[:2] == [flag, st["len"]], (i, t)
            assert got[2:] == ([] if row is None else row.tolist()), (i, t)
        got = [int(v) for v in driver["out"][at].split()]
        at += 1
        assert tuple(got[:13]) == dm.scalars(st), i
        assert got[13:] == dm.live(st).tolist(), i
        for k in events:
            events[k] += st[k]
    assert at == len(driver["out"]) and all(events.values()), events


def test_driver_under_address_and_undefined_sanitizers(driver):
    """the stand-alone driver (its own main, nothing of it loaded into Python) built with -fsanitize=address,undefined: the same input,
    the same output, no report"""
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = driver["dir"] / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(driver["dir"] / "probe")], capture_output=True, timeout=300).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")            # decided on a trivial program: an error in the driver fails below
    exe = str(driver["dir"] / "dbuf_route_driver_san")
    build(exe, san)
    r = subprocess.run([exe], input=driver["input"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.splitlines() == driver["out"]
