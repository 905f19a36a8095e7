"""igdsp_plc_conceal timing: microseconds per call (device events on the launch stream), algorithmic bytes and the fraction of the
8 TB/s nominal HBM rate they represent, beside igdsp_decode_meter (d_pcm + d_stats) over the same rows and the compute-free yardstick,
all in one process.

    python tools/plc_bench.py [--reps 20] [--warmup 5] [--out profiles/r09_plc_bench.json] [--only P1,P3]

Shapes (mu-law, n = 160; out + len_out + stats written):
    P1  C = 65 536, 128 ticks, every tick PLAYED
    P2  as P1 with 3 % of ticks LOST in bursts (mean 2, up to 8 ticks) and 1 % IDLE
    P3  C = 65 536, 1 tick, every tick PLAYED (a live gateway's per-tick call)
Every timed call continues the same state (runs cross calls in P2).  Algorithmic bytes per channel-tick: the flag and the 160 payload
bytes read, 320 bytes of PCM, the 2-byte len and the 16-byte record written; per channel and call, the 16 scalar bytes of the state
read and written and the 560-byte ring written (P2 also reads back the ring of the channels that start a run in their first ticks, not
counted).  Decode is igdsp_decode_meter with d_pcm and d_stats on the same payload rows.  The yardstick (igdsp_internal_plc_copy)
walks the same rows with every tick PLAIN and no decode, search, synthesis or stats.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libigdsp.so: one HIP runtime per process)

from igate4xsoftphonedsp_amd import capi  # noqa: E402

N, PEAK = 160, 8.0e12
BARS = {"P1": 1.2, "P2": 1.5, "P3": 2.0}


def shape(name):
    """C, T, lossy"""
    return {"P1": (65536, 128, False), "P2": (65536, 128, True), "P3": (65536, 1, False)}[name]


def flags_for(C_, T, lossy, g):
    fl = torch.full((T, C_), capi.JB_PLAYED, dtype=torch.uint8, device="cuda")
    if not lossy:
        return fl
    # bursts: a burst starts with p = 0.03 / mean length; lengths 1 .. 8, mean 2 (geometric, capped)
    start = torch.rand((T, C_), device="cuda", generator=g) < 0.015
    ln = torch.clamp(torch.distributions.Geometric(probs=torch.tensor(0.5, device="cuda")).sample((T, C_)).to(torch.int64) + 1, max=8)
    lost = torch.zeros((T, C_), dtype=torch.bool, device="cuda")
    for k in range(8):
        sh = torch.roll(start & (ln > k), shifts=k, dims=0)
        sh[:k] = False
        lost |= sh
    idle = (torch.rand((T, C_), device="cuda", generator=g) < 0.01) & ~lost
    fl[lost] = capi.JB_LOST
    fl[idle] = capi.JB_IDLE
    return fl


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
    return float(np.median(t)), float(min(t))


def run_case(ctx, name, reps, warmup):
    C_, T, lossy = shape(name)
    g = torch.Generator(device="cuda").manual_seed(C_ + T)
    pl = torch.randint(0, 256, (T * C_ * N,), dtype=torch.uint8, device="cuda", generator=g)
    codec = torch.zeros(C_, dtype=torch.uint8, device="cuda")
    fl = flags_for(C_, T, lossy, g)
    state = torch.zeros(C_ * capi.PLC_STATE.itemsize, dtype=torch.uint8, device="cuda")
    out = torch.empty(T * C_ * N, dtype=torch.int16, device="cuda")
    lo = torch.empty(T * C_, dtype=torch.int16, device="cuda")
    st = torch.empty(T * C_ * 16, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()
    cp = capi.internal("igdsp_internal_plc_copy")

    def plc():
        ctx.plc_conceal(fl, state, out, C_, T, N, payload=pl, codec=codec, len_out=lo, stats=st, stream=s.cuda_stream)

    def copy():
        rc = cp(ctx.h, fl.data_ptr(), pl.data_ptr(), codec.data_ptr(), None, None, C_, T, N, state.data_ptr(), out.data_ptr(), lo.data_ptr(),
                st.data_ptr(), s.cuda_stream)
        assert rc == 0, rc

    def dec():
        ctx.decode_meter(pl, codec, C_, T, N, st, pcm=out, stream=s.cuda_stream)

    us, us_min = timed(plc, s, reps, warmup)
    frac_lost = float((fl == capi.JB_LOST).float().mean().item())
    frac_idle = float((fl == capi.JB_IDLE).float().mean().item())
    dus, _ = timed(dec, s, reps, warmup)
    cus, _ = timed(copy, s, reps, warmup)
    alg = int(C_ * T * (1 + N + 2 * N + 2 + 16) + C_ * (2 * 16 + 560))
    bar = BARS[name]
    return {"case": name, "C": C_, "T": T, "lost_frac": round(frac_lost, 4), "idle_frac": round(frac_idle, 4), "us_per_call": round(us, 2),
            "us_min": round(us_min, 2), "alg_bytes": alg, "frac_8TBps": round(alg / (us * 1e-6) / PEAK, 4), "decode_us": round(dus, 2),
            "copy_us": round(cus, 2), "copy_frac_8TBps": round(alg / (cus * 1e-6) / PEAK, 4), "plc_over_decode": round(us / dus, 3),
            "plc_over_copy": round(us / cus, 3), "copy_over_decode": round(cus / dus, 3), "bar": bar, "bar_met": bool(us <= bar * dus),
            "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="P1,P2,P3")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    with capi.Context(device=0, max_channels=64) as ctx:
        for name in a.only.split(","):
            r = run_case(ctx, name, a.reps, a.warmup)
            print(json.dumps(r), flush=True)
            rows.append(r)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
