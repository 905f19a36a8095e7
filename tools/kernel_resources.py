#!/usr/bin/env python3
"""Per-kernel register / scratch / LDS use from the saved ISA (python -m igate4xsoftphonedsp_amd.build --asm)."""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM_DIR = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "_asm")


def asm_files():
    import glob
    return sorted(glob.glob(os.path.join(ASM_DIR, "igdsp_k_*-hip-amdgcn-amd-amdhsa-gfx950.s")))


def resources(paths=None):
    out = []
    for path in (paths or asm_files()):
        out += _resources_of(path)
    return out


def fresh_resources():
    """resources() of a current _asm/: build(save_asm=True) first when an igdsp_k_* translation unit has no .s there, or when a device
    source, a header (include/igdsp.h among them) or build.py is newer than the oldest of those .s files."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from igate4xsoftphonedsp_amd import build as b

    asm = [os.path.join(ASM_DIR, os.path.splitext(s)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s") for s in b.DEVICE_SOURCES if s.startswith("igdsp_k_")]
    deps = [os.path.join(b.CSRC, s) for s in b.DEVICE_SOURCES + b.HEADERS] + [os.path.abspath(b.__file__)]
    if not all(map(os.path.exists, asm)) or max(map(os.path.getmtime, deps)) > min(map(os.path.getmtime, asm)):
        b.build(save_asm=True)
    return resources()


def _resources_of(path):
    s = open(path).read()
    meta = s[s.index("amdhsa.kernels:"):]
    out = []
    for blk in meta.split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)
        out.append({"name": g("name"), "vgpr": int(g("vgpr_count")), "sgpr": int(g("sgpr_count")), "spill": int(g("vgpr_spill_count")),
                    "sgpr_spill": int(g("sgpr_spill_count")), "scratch": int(g("private_segment_fixed_size")), "lds": int(g("group_segment_fixed_size"))})
    names = subprocess.run(["c++filt"] + [r["name"] for r in out], capture_output=True, text=True).stdout.split("\n")
    for r, d in zip(out, names):
        r["demangled"] = d.split("(")[0]
        r["file"] = os.path.basename(path).split("-")[0]
    return out

def loop_valu_count(path, mangled, marker):
    """Vector ALU instructions (lines that begin with v_) in the basic-block run of kernel `mangled` in the .s file `path` that holds the
    instruction `marker`: from the last label in front of the marker to the first branch behind it, the body of a loop that was not split"""
    text = open(path).read().split("\n")
    start = next(i for i, line in enumerate(text) if line.startswith(mangled + ":"))
    end = next(i for i in range(start, len(text)) if "s_endpgm" in text[i])
    at = next(i for i in range(start, end) if text[i].strip().startswith(marker))
    top = max(i for i in range(start, at) if re.match(r"\.LBB\d+_\d+:", text[i]))
    bottom = next(i for i in range(at, end) if text[i].strip().startswith("s_cbranch"))
    return sum(1 for line in text[top + 1:bottom] if line.strip().startswith("v_"))


def loop_count(path, mangled, marker):
    """How often the instruction `marker` itself stands in that same basic-block run: that the run is the whole loop (k_filt: five
    v_mad_i32_i24 a section and sample, two samples a turn)"""
    text = open(path).read().split("\n")
    start = next(i for i, line in enumerate(text) if line.startswith(mangled + ":"))
    end = next(i for i in range(start, len(text)) if "s_endpgm" in text[i])
    at = next(i for i in range(start, end) if text[i].strip().startswith(marker))
    top = max(i for i in range(start, at) if re.match(r"\.LBB\d+_\d+:", text[i]))
    bottom = next(i for i in range(at, end) if text[i].strip().startswith("s_cbranch"))
    return sum(1 for line in text[top + 1:bottom] if line.strip().startswith(marker))


def block_counts(path, mangled):
    """Every basic block of kernel `mangled` in the .s file `path`, in order: its label, whether the compiler marks it as (part of) a
    loop, its vector ALU instructions (lines that begin with v_), its LDS instructions (ds_) and how often each v_ mnemonic stands in
    it (k_ns: the block of one forward and of one inverse butterfly is the one with four v_mad_i64_i32, two LDS reads and two writes)"""
    text = open(path).read().split("\n")
    start = next(i for i, line in enumerate(text) if line.startswith(mangled + ":"))
    end = next(i for i in range(start, len(text)) if "s_endpgm" in text[i])
    blocks = [{"label": "entry", "loop": False, "valu": 0, "lds": 0, "names": {}}]
    for line in text[start + 1:end]:
        m = re.match(r"(\.LBB\d+_\d+):(.*)", line)
        if m:
            blocks.append({"label": m.group(1), "loop": "Loop" in m.group(2), "valu": 0, "lds": 0, "names": {}})
            continue
        word = line.strip().split(" ")[0]
        if word.startswith("v_"):
            blocks[-1]["valu"] += 1
            blocks[-1]["names"][word] = blocks[-1]["names"].get(word, 0) + 1
        elif word.startswith("ds_"):
            blocks[-1]["lds"] += 1
    return blocks


def blocks_with(path, mangled, name, at_least, lds_at_least=0):
    """The basic blocks of kernel `mangled` (block_counts) in which the v_ mnemonic `name` stands at least `at_least` times and that hold
    at least `lds_at_least` LDS instructions (k_srtp: one AES-128 block is the block with at least 100 v_alignbit_b32, the table words'
    rotations, and at least 160 LDS reads; one SHA-1 compression the block with at least 200 v_alignbit_b32 and no LDS instruction)"""
    return [b for b in block_counts(path, mangled) if b["names"].get(name, 0) >= at_least and b["lds"] >= lds_at_least]


if __name__ == "__main__":
    for r in resources():
        if len(sys.argv) < 2 or sys.argv[1] in r["demangled"]:
            print(f"{r['demangled']:<60} vgpr {r['vgpr']:>3} sgpr {r['sgpr']:>3} spill {r['spill']} scratch {r['scratch']:>3} lds {r['lds']}")
