"""-m "not gpu": the link supervision kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): every instantiation
the launcher can pick is there, none spills VGPRs or uses scratch, and the LDS / VGPR budget link_route relies on holds."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_link_kernels_no_spill_and_budget(resources):
    """k_link_watch: blocks of kLinkWaves = 4 waves without LDS, kLinkU = 16 records (and sizes) of a lane in flight: 32 + 16 VGPRs of loads
    and the state, well inside 128.  k_link_scan: one block of 1 024 threads, so at most 128 VGPRs, and one word of LDS per wave."""
    link = [r for r in resources if "k_link_" in r["demangled"]]
    names = {r["demangled"] for r in link}
    # the product and the compute-free yardstick, the three passes, with and without d_sizes; and the scan
    want = {f"void igdsp::k_link_watch<{c}, {p}, {z}>" for c in ("false", "true") for p in (0, 1, 2) for z in ("false", "true")}
    assert want <= names, want - names
    assert any("k_link_scan" in x for x in names), names
    for r in link:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 128, r
        if "k_link_scan" in r["demangled"]:
            assert 0 < r["lds"] <= 1024, r
        else:
            assert r["lds"] == 0, r
