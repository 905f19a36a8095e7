"""-m "not gpu": igdsp_io_alloc's placement search (csrc/igdsp_io.hip, unchanged) on the CPU.  tests/ioalloc/fake_hip.cpp stands in
for the HIP calls and the probe launch: a device whose memory comes in classes laid out by a class map ("A120 B200 A*": the first
120 chunks created are class A, ...), where a probe that writes the class it reads runs 15 % slower (0.252 against 0.219 ms, the
levels measured on MI355X).  tests/ioalloc/io_alloc_driver.cpp runs a scenario against a bare igdsp_ctx and prints the report, the
class of every chunk behind each buffer and the spare counts; the fake exits non-zero if an address is ever mapped onto a second
handle or over a live mapping.

The assertions are about classes, not probe counts: they hold for any search that finds what the box offers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
ENOMEM = -12

# the workload's shape: 65 536 x 128 x 160 payload bytes (10 chunks of 128 MiB) and its records (1 chunk)
SMALL = "in:1280 rec:128"
# 10 GiB of inputs and 1.25 GiB of records; with two bulk outputs of 10 chunks each
BIG = "in:10240 rec:1280"
BULK = BIG + " bulk:1280 bulk:1280"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    if not os.path.exists(os.path.join(HIP_INC, "hip", "hip_runtime.h")):
        pytest.skip("HIP headers not available")
    exe = tmp_path_factory.mktemp("ioalloc") / "io_alloc_driver"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I", HIP_INC,
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-x", "c++", os.path.join(CSRC, "igdsp_io.hip"), "-x", "none",
                        os.path.join(ROOT, "tests", "ioalloc", "fake_hip.cpp"), os.path.join(ROOT, "tests", "ioalloc", "io_alloc_driver.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return str(exe)


def run(driver, lines, settle=False, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith(("IGDSP_", "IOFAKE_"))}
    if not settle:
        e["IGDSP_IO_SETTLE"] = "0"
    e.update(env)
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, env=e)
    assert r.returncode == 0, r.stdout + r.stderr
    return parse(r.stdout.splitlines())


def parse(lines):
    """-> {"alloc": {name: report}, "bufs": {name: [(role, [class letter per chunk])]}, "spares": [[4 counts] after each step],
    "live": [{handles, mappings, mallocs}]}"""
    out = {"alloc": {}, "bufs": {}, "spares": [], "live": []}
    for ln in lines:
        key, _, rest = ln.partition(" ")
        if key == "alloc":
            name, *kv = rest.split()
            out["alloc"][name] = {k: float(v) if "." in v else int(v) for k, v in (x.split("=") for x in kv)}
        elif key == "buf":
            name, _, role, *runs = rest.split()
            chunks = None if runs == ["null"] else [r[0] for r in runs for _ in range(int(r[1:]))]
            out["bufs"].setdefault(name, []).append((role, chunks))
        elif key == "spares":
            out["spares"].append([int(x) for x in rest.split()])
        elif key == "live":
            out["live"].append({k: int(v) for k, v in (x.split("=") for x in rest.split())})
    return out


def scenario(device, *allocs):
    """device line, then for each (name, limit MiB, spec) an alloc, then everything freed and the spares dropped"""
    lines = [f"device {device}"] + [f"alloc {name} {limit} {spec}" for name, limit, spec in allocs]
    return lines + [f"free {name}" for name, _, _ in allocs] + ["drop", "live"]


def one_class(chunks):
    assert chunks and len(set(chunks)) == 1, chunks
    return chunks[0]


def assert_nothing_left(out):
    assert out["live"][-1] == {"handles": 0, "mappings": 0, "mallocs": 0}


def assert_two_class_placement(out, name="s1"):
    """every input chunk in one class, every output chunk in one other class"""
    (_, inp), *outs = out["bufs"][name]
    a = one_class(inp)
    b = one_class([c for _, chunks in outs for c in chunks])
    assert a != b
    return a, b


def assert_bulk_spread(out, name="s1"):
    """records and every bulk buffer's first half in class B, the second halves in class C, neither the inputs' class"""
    bufs = out["bufs"][name]
    a = one_class(bufs[0][1])
    b = one_class([c for role, chunks in bufs if role == "rec" for c in chunks] +
                  [c for role, chunks in bufs if role == "bulk" for c in chunks[:len(chunks) - len(chunks) // 2]])
    c = one_class([c for role, chunks in bufs if role == "bulk" for c in chunks[len(chunks) - len(chunks) // 2:]])
    assert len({a, b, c}) == 3, (a, b, c)


def test_two_classes(driver):
    out = run(driver, scenario("280 1 A120 B200 A*", ("s1", 0, BIG)))
    rep = out["alloc"]["s1"]
    assert (rep["rc"], rep["placed"], rep["classes_found"], rep["bulk_spread"]) == (0, 1, 2, 0)
    assert rep["probes"] > 0 and rep["probe_ms_other"] < rep["probe_ms_same"]
    assert assert_two_class_placement(out) == ("A", "B")
    assert_nothing_left(out)


def test_source_a_straddles_a_run_boundary(driver):
    out = run(driver, scenario("280 1 A6 B200 A*", ("s1", 0, BIG)))       # source A: 6 chunks of A, 4 of B
    rep = out["alloc"]["s1"]
    assert (rep["rc"], rep["placed"], rep["classes_found"]) == (0, 1, 2) and rep["reseeds"] >= 1
    assert_two_class_placement(out)
    assert_nothing_left(out)


def test_three_classes_spread_the_bulk_outputs(driver):
    out = run(driver, scenario("280 1 A120 B1160 C*", ("s1", 0, BULK)))    # the third class from chunk 1 280 (160 GiB), inside 85 %
    rep = out["alloc"]["s1"]
    assert (rep["rc"], rep["placed"], rep["classes_found"], rep["bulk_spread"]) == (0, 1, 3, 1)
    assert_bulk_spread(out)
    assert_nothing_left(out)


def test_third_class_beyond_the_explore_limit(driver):
    out = run(driver, scenario("280 1 A120 B1160 C*", ("s1", 100 << 10, BULK)))   # the limit ends at chunk 800
    rep = out["alloc"]["s1"]
    assert (rep["rc"], rep["placed"], rep["classes_found"], rep["bulk_spread"]) == (0, 1, 2, 0)
    assert rep["chunks_explored"] <= 800
    assert assert_two_class_placement(out) == ("A", "B")                   # B serves both halves
    assert_nothing_left(out)


@pytest.mark.parametrize("classes,reseeds", [
    ("A120 BC*", 0),        # ten consecutive pool chunks hold B and C evenly: every 2nd of them is one class
    ("A120 BBC*", 1),       # ten consecutive pool chunks hold 7 B, 3 C: a mixed source B, re-seeded from its larger group
], ids=["evenly_mixed", "mixed"])
def test_interleaved_second_and_third_class(driver, classes, reseeds):
    out = run(driver, scenario(f"280 1 {classes}", ("s1", 0, BULK)))
    rep = out["alloc"]["s1"]
    assert (rep["rc"], rep["placed"], rep["classes_found"], rep["bulk_spread"]) == (0, 1, 3, 1)
    assert rep["reseeds"] == reseeds
    assert_bulk_spread(out)
    assert_nothing_left(out)


def test_one_class(driver):
    out = run(driver, scenario("280 1 A*", ("s1", 0, BIG)))
    rep = out["alloc"]["s1"]
    assert (rep["rc"], rep["placed"], rep["bulk_spread"]) == (0, 0, 0) and rep["probes"] > 0
    assert all(chunks and set(chunks) == {"A"} for _, chunks in out["bufs"]["s1"])      # returned, and mapped
    assert_nothing_left(out)


@pytest.mark.parametrize("device,spec,env,mapped", [
    ("280 1 A120 B*", "in:256 rec:16", {}, True),                  # inputs below 512 MiB: nothing to place
    ("280 0 A120 B*", BIG, {}, False),                              # no virtual-memory API: plain allocations
    ("280 1 A120 B*", BIG, {"IGDSP_IO_PLAIN": "1"}, False),
], ids=["small_inputs", "no_vmm", "plain_knob"])
def test_unplaced_paths(driver, device, spec, env, mapped):
    out = run(driver, [f"device {device}", f"alloc s1 0 {spec}", "live", "free s1", "drop", "live"], **env)
    rep = out["alloc"]["s1"]
    assert (rep["rc"], rep["placed"], rep["probes"], rep["classes_found"], rep["chunks_explored"]) == (0, 0, 0, 0, 0)
    for _, chunks in out["bufs"]["s1"]:
        assert chunks and set(chunks) == ({"A"} if mapped else {"-"})
    assert out["live"][0]["mallocs"] == (0 if mapped else len(spec.split()))
    assert_nothing_left(out)


def test_later_calls_are_served_from_spares(driver):
    lines = ["device 280 1 A120 B200 A*", f"alloc s1 0 {SMALL}", f"alloc s2 0 {SMALL}", "free s1", "free s2", f"alloc s3 0 {SMALL}",
             "free s3", "live", "drop", "live"]
    out = run(driver, lines)
    rep1, rep2, rep3 = (out["alloc"][n] for n in ("s1", "s2", "s3"))
    assert (rep1["placed"], rep1["classes_found"]) == (1, 2) and rep1["probes"] > 0
    first = assert_two_class_placement(out, "s1")
    for rep, name in ((rep2, "s2"), (rep3, "s3")):
        assert (rep["rc"], rep["placed"], rep["probes"], rep["chunks_explored"], rep["settle"]) == (0, 1, 0, 0, 0)
        assert assert_two_class_placement(out, name) == first
    assert out["live"][0]["handles"] > 0 and out["live"][0]["mappings"] == 0     # only spares are left
    assert_nothing_left(out)


def test_mapping_failure_on_the_spare_path(driver):
    """the k-th hipMemMap failing while spares are mapped: IGDSP_ENOMEM (the call used to wait forever on its own lock)"""
    lines = ["device 280 1 A120 B200 A*", f"alloc s1 0 {SMALL}", "fail map 5", f"alloc s2 0 {SMALL}", "free s1", "drop", "live"]
    out = run(driver, lines)
    rep = out["alloc"]["s2"]
    assert (rep["rc"], rep["probes"]) == (ENOMEM, 0)
    assert out["bufs"]["s2"] == [("in", None), ("rec", None)]
    assert_nothing_left(out)


def test_settle_wait(driver):
    """the call waits until the finished set streams as fast as before the release; a small search keeps that wait short"""
    out = run(driver, scenario("280 1 A20 B*", ("s1", 6 << 10, SMALL)), settle=True)
    rep = out["alloc"]["s1"]
    assert (rep["rc"], rep["placed"], rep["classes_found"], rep["settle"]) == (0, 1, 2, 1)
    assert rep["chunks_explored"] <= 48
    assert_nothing_left(out)
