"""igdsp_spectrum timing: microseconds per launch (device events on the launch stream; median, min and max), nanoseconds per spectrum,
the arithmetic rate the transforms represent and the algorithmic bytes, beside the same launch with d_state only, the compute-free
yardstick, and torch.fft.rfft (rocFFT) over a batch of 1 024-point float32 rows scaled to the time per transform, all in one process.

    python tools/spec_bench.py [--reps 20] [--warmup 3] [--out profiles/spec_bench.json] [--only S1,S4,S0] [--rfft-rows 1048576]

Shapes (n = 160, G.711 input with mixed laws, alpha 0.25):
    S1  C = 65 536, 128 frames, hop 1: 8.4 M spectra
    S4  C = 65 536, 128 frames, hop 4: 2.1 M spectra
    S0  C = 65 536, 1 frame, hop 1 (a live gateway's per-tick call)
Every timed launch continues the same state.  Arithmetic per spectrum: 5 N log2 N = 51 200 FLOP for N = 1 024 (the customary count of a
complex transform of that size; the real transform here does about half of it, so the rate is a label for comparison, not a share of
peak).  Algorithmic bytes: n per frame in, 8 per record, per channel and launch the state read and written (2 x 4 112) and the two arrays
(2 x 2 048).  The yardstick (igdsp_internal_spec_move) makes the same traversal, ring and tile traffic and stores with no transform.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libigdsp.so: one HIP runtime per process)

from igate4xsoftphonedsp_amd import capi  # noqa: E402

N, FLOP_PER_SPECTRUM = 160, 5 * 1024 * 10


def shape(name):
    """C, F, hop"""
    return {"S1": (65536, 128, 1), "S4": (65536, 128, 4), "S0": (65536, 1, 1)}[name]


def timed(fn, s, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        t.append(a.elapsed_time(b) * 1000.0)
    return {"median": round(float(np.median(t)), 2), "min": round(float(min(t)), 2), "max": round(float(max(t)), 2)}


def run_case(ctx, name, reps, warmup):
    C_, F_, hop = shape(name)
    torch.manual_seed(C_ + F_ + hop)
    codes = torch.randint(0, 256, (F_, C_, N), dtype=torch.uint8, device="cuda")
    codec = torch.where(torch.arange(C_, device="cuda") % 2 == 0, 0, 8).to(torch.uint8)
    state = torch.zeros(C_ * capi.SPEC_STATE.itemsize, dtype=torch.uint8, device="cuda")
    rec = torch.empty(F_ * C_ * 8, dtype=torch.uint8, device="cuda")
    avg = torch.empty(C_ * 512, dtype=torch.float32, device="cuda")
    raw = torch.empty(C_ * 512, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream()
    cfg = capi.SpecCfg(hop, 0.25)
    mv = capi.internal("igdsp_internal_spec_move")
    import ctypes as C

    cfg_p = C.cast(C.pointer(cfg), C.c_void_p)

    def full():
        ctx.spectrum(state, C_, F_, N, g711=codes, codec=codec, cfg=cfg, rec=rec, avg=avg, raw=raw, stream=s.cuda_stream)

    def bare():
        ctx.spectrum(state, C_, F_, N, g711=codes, codec=codec, cfg=cfg, stream=s.cuda_stream)

    def move():
        rc = mv(ctx.h, codes.data_ptr(), codec.data_ptr(), None, C_, F_, N, cfg_p, state.data_ptr(), rec.data_ptr(), avg.data_ptr(), raw.data_ptr(),
                s.cuda_stream)
        assert rc == 0, rc

    for _ in range(8):                                   # the histories full before anything is timed
        bare()
    t_full, t_bare, t_move = timed(full, s, reps, warmup), timed(bare, s, reps, warmup), timed(move, s, reps, warmup)
    spectra = C_ * (F_ // hop) if F_ >= hop else 0
    alg = C_ * F_ * (N + 8) + C_ * (2 * capi.SPEC_STATE.itemsize + 2 * 2048)
    us = t_full["median"]
    return {"case": name, "C": C_, "F": F_, "n": N, "hop": hop, "spectra": spectra, "us": t_full, "state_only_us": t_bare, "move_us": t_move,
            "ns_per_spectrum": round(us * 1e3 / spectra, 3) if spectra else None,
            "state_only_ns_per_spectrum": round(t_bare["median"] * 1e3 / spectra, 3) if spectra else None,
            "tflops_5nlogn": round(spectra * FLOP_PER_SPECTRUM / (us * 1e-6) / 1e12, 3) if spectra else None, "alg_bytes": alg,
            "frac_8TBps": round(alg / (us * 1e-6) / 8.0e12, 4), "move_over_run": round(t_move["median"] / us, 3), "reps": reps}


def run_rfft(rows, reps, warmup):
    """torch.fft.rfft (rocFFT's batched real transform) over rows x 1 024 float32: the library reads 4 KiB and writes 4 KiB per transform"""
    x = torch.randn((rows, 1024), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream()
    t = timed(lambda: torch.fft.rfft(x, dim=1), s, reps, warmup)
    return {"case": "rfft", "rows": rows, "us": t, "ns_per_transform": round(t["median"] * 1e3 / rows, 3),
            "tflops_5nlogn": round(rows * FLOP_PER_SPECTRUM / (t["median"] * 1e-6) / 1e12, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="S1,S4,S0")
    ap.add_argument("--rfft-rows", type=int, default=1 << 20)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    with capi.Context(device=0, max_channels=64) as ctx:
        for name in a.only.split(","):
            r = run_case(ctx, name, a.reps, a.warmup)
            print(json.dumps(r), flush=True)
            rows.append(r)
            torch.cuda.empty_cache()
    if a.rfft_rows:
        r = run_rfft(a.rfft_rows, a.reps, a.warmup)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
