"""Builds ``libigdsp.so`` (HIP kernels + C ABI) for gfx950 with hipcc, in-tree.

    python -m igate4xsoftphonedsp_amd.build [--force] [--asm]

hipcc cross-compiles without a GPU, so this also runs in the build container;
the resulting .so travels to the GPU box with the repo snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")
LIB = os.path.join(PKG, "libigdsp.so")
HOST_LIB = os.path.join(PKG, "libigdsp_host.so")

DEVICE_SOURCES = ["igdsp_k_meter.hip", "igdsp_k_packets.hip", "igdsp_k_codec.hip", "igdsp_k_misc.hip", "igdsp_k_tx.hip", "igdsp_k_txstage.hip", "igdsp_k_conf.hip", "igdsp_k_bss.hip", "igdsp_k_ptt.hip", "igdsp_k_link.hip", "igdsp_k_jb.hip", "igdsp_k_plc.hip", "igdsp_k_snd.hip", "igdsp_k_tone.hip", "igdsp_k_rs.hip", "igdsp_k_dbuf.hip", "igdsp_k_spec.hip", "igdsp_k_tdet.hip", "igdsp_k_ec.hip", "igdsp_k_agc.hip", "igdsp_k_vad.hip", "igdsp_k_cng.hip", "igdsp_k_filt.hip", "igdsp_k_ns.hip", "igdsp_k_srtp.hip", "igdsp_k_rtcp.hip", "igdsp_k_srtp_gcm.hip", "igdsp_capi.hip", "igdsp_capi_ctx.hip", "igdsp_capi_tx.hip", "igdsp_capi_bench.hip", "igdsp_capi_snd.hip", "igdsp_capi_tone.hip", "igdsp_capi_rs.hip", "igdsp_capi_dbuf.hip", "igdsp_capi_spec.hip", "igdsp_capi_tdet.hip", "igdsp_capi_ec.hip", "igdsp_capi_agc.hip", "igdsp_capi_vad.hip", "igdsp_capi_cng.hip", "igdsp_capi_filt.hip", "igdsp_capi_ns.hip", "igdsp_capi_srtp.hip", "igdsp_capi_rtcp.hip", "igdsp_capi_srtp_gcm.hip", "igdsp_io.hip"]
HOST_SOURCES = ["igdsp_host.cpp"]          # C++ mirror of the reference's adapter/hook interface
HEADERS = sorted(h for h in os.listdir(CSRC) if h.endswith(".h")) + [os.path.join(INCLUDE, "igdsp.h")]   # every header: none can be forgotten


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the gfx950 code objects cannot be built")


def _stale(target: str, sources: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources if os.path.exists(s))


def _compile_all(objdir: str, extra: list[str], verbose: bool, cwd: str) -> list[str]:
    """hipcc -c every device source into objdir, four at a time (the translation units are independent), and return the objects."""
    from concurrent.futures import ThreadPoolExecutor

    os.makedirs(objdir, exist_ok=True)
    base = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", INCLUDE, "-I", CSRC, "-Wall", "-Wno-unused-result"]
    base[1:1] = os.environ.get("IGDSP_CXXFLAGS", "").split()      # A/B experiments: -DIGDSP_...=N
    jobs = []
    for src in DEVICE_SOURCES:
        obj = os.path.join(objdir, os.path.splitext(src)[0] + ".o")
        jobs.append((base + extra + ["-c", os.path.join(CSRC, src), "-o", obj], obj))

    def run(job):
        cmd, obj = job
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True, cwd=cwd, stderr=None if verbose or not extra else subprocess.DEVNULL)
        return obj

    with ThreadPoolExecutor(max_workers=min(4, os.cpu_count() or 1)) as ex:
        return list(ex.map(run, jobs))


# what the last build() call did: translation units compiled vs libraries found up to date (the driver's "does it build" check reads
# this through __graft_entry__.build(): a reused library and a fresh compile must not look the same)
LAST = {"device_compiled": 0, "device_reused": 0, "host_compiled": 0, "host_reused": 0}


def build(force: bool = False, save_asm: bool = False, verbose: bool = False) -> str:
    srcs = [os.path.join(CSRC, s) for s in DEVICE_SOURCES]
    deps = srcs + [h if os.path.isabs(h) else os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    LAST.update(device_compiled=0, device_reused=0, host_compiled=0, host_reused=0)
    if force or _stale(LIB, deps):
        objs = _compile_all(os.path.join(PKG, "_obj"), [], verbose, PKG)
        link = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs]
        if verbose:
            print(" ".join(link))
        subprocess.run(link, check=True, cwd=PKG)
        LAST["device_compiled"] = len(objs)
    else:
        LAST["device_reused"] = len(DEVICE_SOURCES)
    if save_asm:   # a pass of its own: keeps every translation unit's .s (and the resource remarks) under _asm/
        asm_dir = os.path.join(PKG, "_asm")
        _compile_all(asm_dir, ["-save-temps=obj", "-Rpass-analysis=kernel-resource-usage"], verbose, asm_dir)
    host_srcs = [os.path.join(PKG, "host", s) for s in HOST_SOURCES]
    if all(os.path.exists(s) for s in host_srcs):
        hdeps = host_srcs + [os.path.join(PKG, "host", "igdsp_host.h"), os.path.join(INCLUDE, "igdsp.h")]
        if force or _stale(HOST_LIB, hdeps + [LIB]):
            cmd = [
                "g++", "-O2", "-std=c++11", "-fPIC", "-shared", "-Wall", "-I", INCLUDE, "-I", os.path.join(PKG, "host"),
                "-o", HOST_LIB, *host_srcs, "-L", PKG, "-ligdsp", "-Wl,-rpath,$ORIGIN", "-lpthread",
            ]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True, cwd=PKG)
            LAST["host_compiled"] = len(host_srcs)
        else:
            LAST["host_reused"] = len(host_srcs)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, save_asm="--asm" in sys.argv, verbose=True)
    print("built", LIB, LAST)
