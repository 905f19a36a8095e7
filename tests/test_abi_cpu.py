"""CPU-side checks of the drop-in boundary: libigdsp.so loads without a GPU, exports every
symbol include/igdsp.h declares, the struct layouts agree between header, binding and oracle,
and the product fails loudly (no CPU fallback) when no gfx950 device is present."""
import ctypes
import os
import re

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


def test_header_symbols_all_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "igdsp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(igdsp_[a-z0-9_]+)\s*\(", hdr))
    bound = {name for name, _, _ in capi.PROTOTYPES}
    assert declared == bound, (declared ^ bound)
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    assert lib.igdsp_abi_version() == capi.ABI_VERSION == 3


def _param_types(text, name):
    """the parameter-type list of the one declaration / definition `int name(...)` in C text: comments dropped, names dropped"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = re.findall(rf"^\s*int\s+{name}\s*\(([^)]*)\)", text, flags=re.M)
    assert len(found) == 1, (name, len(found))
    types = []
    for p in found[0].split(","):
        m = re.fullmatch(r"\s*(.*?)\s*\b[A-Za-z_]\w*\s*", p, flags=re.S)           # everything ahead of the parameter's name
        assert m and m.group(1), (name, p)
        types.append(re.sub(r"\s*\*\s*", " *", " ".join(m.group(1).split())))
    return types


def _ctype_of(t):
    if t.endswith("*"):
        return ctypes.c_void_p
    return {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32, "int": ctypes.c_int}[t]


def _csrc():
    d = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
    return "\n".join(open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.startswith("igdsp_capi") and f.endswith(".hip"))


@pytest.mark.parametrize("name", sorted(capi.INTERNAL_TWIN))
def test_yardstick_signature_is_its_twins(name):
    """a yardstick entry takes "arguments as" its public twin: the parameter types of its extern "C" definition equal those the header
    declares for the twin, and the binding's row (derived from the twin's) is that list"""
    twin = capi.INTERNAL_TWIN[name]
    got = _param_types(_csrc(), name)
    exp = _param_types(open(os.path.join(ROOT, "include", "igdsp.h")).read(), twin)
    assert got == exp, (name, twin)
    res, args = capi.INTERNAL[name]
    assert res is ctypes.c_int and list(args) == [_ctype_of(t) for t in got]


def test_yardstick_table_is_complete():
    """every igdsp_internal_*_copy / _fill the library defines is in the table, and tx_copy's own row matches its definition"""
    src = re.sub(r"//[^\n]*", "", _csrc())
    defined = set(re.findall(r"^int\s+(igdsp_internal_\w+_(?:copy|fill))\s*\(", src, flags=re.M))
    assert defined == set(capi.INTERNAL) and len(defined) == 10, defined ^ set(capi.INTERNAL)
    res, args = capi.INTERNAL["igdsp_internal_tx_copy"]
    assert res is ctypes.c_int and list(args) == [_ctype_of(t) for t in _param_types(_csrc(), "igdsp_internal_tx_copy")]
    with pytest.raises(KeyError):
        capi.internal("igdsp_internal_stream_rw")


def test_tools_bind_their_yardstick_through_the_table():
    """tools/<stage>_bench.py takes its yardstick from capi.internal and writes no argtypes of its own"""
    for name in capi.INTERNAL:
        stage = name[len("igdsp_internal_"):].split("_")[0]
        text = open(os.path.join(ROOT, "tools", f"{stage}_bench.py")).read()
        assert f'capi.internal("{name}")' in text and ".argtypes" not in text, stage


def test_struct_layouts_agree(orc):
    assert capi.FRAME_STATS.itemsize == orc.FRAME_STATS.itemsize == 16
    assert capi.CHAN_HOLD.itemsize == orc.CHAN_HOLD.itemsize == 32
    assert capi.AGGREGATE.itemsize == orc.AGGREGATE.itemsize == 8 * capi.AGG_WORDS == 896
    assert ctypes.sizeof(capi.Level) == 20
    # ABI 3: the gated window
    assert capi.CHAN_PROBE.itemsize == orc.CHAN_PROBE.itemsize == ctypes.sizeof(capi.ChanProbe) == 8
    assert ctypes.sizeof(capi.Window) == 8 + 4 * ctypes.sizeof(ctypes.c_void_p) == 40
    assert (capi.GATE_ALWAYS, capi.GATE_SQU, capi.GATE_PTT, capi.GATE_SQU_OR_PTT) == (orc.GATE_ALWAYS, orc.GATE_SQU, orc.GATE_PTT, orc.GATE_SQU_OR_PTT) == (0, 1, 2, 3)
    for a, b in ((capi.FRAME_STATS, orc.FRAME_STATS), (capi.CHAN_HOLD, orc.CHAN_HOLD), (capi.AGGREGATE, orc.AGGREGATE)):
        assert a.names == b.names
        assert [a.fields[n][1] for n in a.names] == [b.fields[n][1] for n in b.names]
    # header constants mirrored in the binding
    hdr = open(os.path.join(ROOT, "include", "igdsp.h")).read()
    for name, val in (("IGDSP_PT_PCMU", capi.PT_PCMU), ("IGDSP_PT_PCMA", capi.PT_PCMA), ("IGDSP_PT_R2S", capi.PT_R2S),
                      ("IGDSP_SAMPLES_PER_FRAME", capi.SAMPLES_PER_FRAME), ("IGDSP_MAX_PAYLOAD", capi.MAX_PAYLOAD),
                      ("IGDSP_AGG_MAX_RANKS", capi.AGG_MAX_RANKS), ("IGDSP_PROBE_ALARM", capi.PROBE_ALARM), ("IGDSP_PKT_MIXED", capi.PKT_MIXED),
                      ("IGDSP_GATE_SQU_OR_PTT", capi.GATE_SQU_OR_PTT), ("IGDSP_ABI_VERSION", capi.ABI_VERSION)):
        m = re.search(rf"#define\s+{name}\s+(\d+)", hdr)
        assert m and int(m.group(1)) == val, name


def test_no_cpu_fallback_without_gpu(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = ctypes.c_void_p()
    assert lib.igdsp_create(ctypes.byref(h), 0, 16) == -19        # IGDSP_ENODEV
    assert not h.value
    with pytest.raises(capi.IgdspError):
        capi.Context(device=0, max_channels=16)
    # NULL-context calls are rejected, never computed on the host
    assert lib.igdsp_decode_meter(None, None, None, None, 1, 1, 160, None, None, None, 0, None) == -22
    assert lib.igdsp_flush(None, None) == -22
    assert lib.igdsp_destroy(None) == 0


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under the package may reference it."""
    pkg = os.path.join(ROOT, "igate4xsoftphonedsp_amd")
    for dirpath, _, files in os.walk(pkg):
        if "_asm" in dirpath or "__pycache__" in dirpath:
            continue
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                txt = open(os.path.join(dirpath, fn), errors="ignore").read()
                assert "igdsp_oracle" not in txt and "from oracle" not in txt and "import oracle" not in txt, fn
    so = open(capi.LIB_PATH, "rb").read()
    assert b"orc_" not in so
