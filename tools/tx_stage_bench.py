"""igdsp_tx_flush timing: the staged ED-137 send path's owner-thread cost per bridge tick, split into snapshot (host clock), upload,
kernel and download (HIP events on the TX stream), and the whole call (host clock); beside it, in the same process, one
igdsp_tx_packetize launch over the same (legs x frames) shape (device events).

    python tools/tx_stage_bench.py [--reps 20] [--warmup 5] [--out profiles/r05_tx_stage_bench.json]

Cases: 4 096 and 65 536 legs x 1, 2 and 8 frames per flush, n = 160, every leg on PTT (20 + n bytes out per frame).  Staging runs in
one native loop (igdsp_internal_tx_stage_many) and is not timed.  Upload bytes = 16 per run + per frame 16 + 172 (12 + n rounded to
4); download bytes = 8 + 256 per frame + 64 per run.  Prints one JSON line per case and writes them all to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libigdsp.so: one HIP runtime per process)

from igate4xsoftphonedsp_amd import capi  # noqa: E402

N, CALL0 = 160, 1


def med(xs):
    return round(statistics.median(xs), 4)


def staged_case(ctx, L, F, reps, warmup):
    lib = ctx.L
    stage = lib.igdsp_internal_tx_stage_many
    stage.restype = ctypes.c_int
    stage.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                      ctypes.c_uint64, ctypes.c_uint32]
    timing = lib.igdsp_internal_tx_timing
    timing.restype = ctypes.c_int
    timing.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    rng = np.random.default_rng(L + F)
    pk = rng.integers(0, 256, (64, 12 + N), dtype=np.uint8)
    pk[:, 0], pk[:, 1] = 0x80, 8
    ph = [[] for _ in range(5)]
    wall = []
    t = 1_000_000
    assert timing(ctx.h, 1, None) == 0
    for r in range(warmup + reps):
        assert stage(ctx.h, CALL0, L, F, pk.ctypes.data, 64, 12 + N, t, 20) == 0
        t0 = time.perf_counter()
        n = ctx.tx_flush()
        t1 = time.perf_counter()
        assert n == L * F
        out = (ctypes.c_float * 5)()
        assert timing(ctx.h, 1, out) == 0
        if r >= warmup:
            wall.append((t1 - t0) * 1e3)
            for i in range(5):
                ph[i].append(out[i])
        t += 20 * F
    up = L * 16 + L * F * (16 + 172)
    down = L * F * (8 + 256) + L * 64
    return {"flush_wall_ms": med(wall), "flush_wall_ms_max": round(max(wall), 4), "snapshot_ms": med(ph[0]), "h2d_ms": med(ph[1]),
            "kernel_ms": med(ph[2]), "d2h_ms": med(ph[3]), "flush_call_ms": med(ph[4]), "upload_bytes": up, "download_bytes": down}


def batched_case(ctx, L, F, reps, warmup):
    g = torch.Generator(device="cuda").manual_seed(L * 7 + F)
    src = torch.randint(0, 256, (F * L * N,), dtype=torch.uint8, device="cuda", generator=g)
    st = np.zeros((L,), capi.TX_CHAN)
    st["pt"], st["keepalive_ms"], st["calltype"], st["ptt"], st["packet_cnt"] = 8, 200, capi.TX_CT_TX, 1, 30
    d_st = torch.from_numpy(st.view(np.uint8).reshape(-1)).cuda()
    last = torch.zeros((L * N,), dtype=torch.uint8, device="cuda")
    pkts = torch.empty((F * L * 256,), dtype=torch.uint8, device="cuda")
    sizes = torch.empty((F * L * 2,), dtype=torch.uint8, device="cuda")
    info = torch.empty((F * L * 8,), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()
    ms = []
    for r in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        ctx.tx_packetize(d_st, last, pkts, 256, sizes, info, L, F, N, 1_000_000 + r * 20 * F, 20, g711=src, stream=s.cuda_stream)
        b.record(s)
        b.synchronize()
        if r >= warmup:
            ms.append(a.elapsed_time(b))
    return {"packetize_kernel_ms": med(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tx_stage_bench needs a GPU"
    torch.cuda.set_device(0)
    rows = []
    for L in (4096, 65536):
        with capi.Context(device=0, max_channels=L) as ctx:
            for c in range(L):
                ctx.map_call(CALL0 + c, c)
                ctx.tx_open(CALL0 + c, "Tx", False, 200, 1_000_000)
                ctx.tx_set_ptt(CALL0 + c, True, 0, 0)
            for F in (1, 2, 8):
                row = {"legs": L, "frames_per_leg": F, "n": N, "reps": a.reps}
                row.update(staged_case(ctx, L, F, a.reps, a.warmup))
                row.update(batched_case(ctx, L, F, a.reps, a.warmup))
                print(json.dumps(row), flush=True)
                rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "cases": rows}, f, indent=1)


if __name__ == "__main__":
    main()
