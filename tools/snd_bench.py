"""igdsp_snd_combine / igdsp_snd_split timing: microseconds per launch (device events on the launch stream, the median of --reps launches
after a warm-up), algorithmic bytes and the fraction of the 8 TB/s nominal HBM rate they represent, beside the compute-free yardstick
(igdsp_internal_snd_copy: the same items, the same bytes in memory order, no transpose, no records) in the same process on the same
buffers.  Input, bulk output (IGDSP_IO_BULK) and records come from igdsp_io_alloc.

    python tools/snd_bench.py [--reps 20] [--warmup 5] [--out profiles/snd_bench.json] [--only S1,S4]

Shapes (n = 160 samples, random int16 input):
    S1 conf_bench's B1 ports  D = 8 192 cards of K = 8 channels, F = 128: 2.7 GB each way, far beyond the Infinity Cache
    S2 the reference's card   D = 10 922 cards of K = 6, F = 128
    S3 single-output forms    S1 records only and S1 bulk only
    S4 real time              S1 at F = 2
    S5 one card               D = 1, K = 6, F = 2: the fixed cost of a launch
    S6 S2's single outputs    S2 records only and S2 bulk only: where the reference's card spends its time
Algorithmic bytes = the input + the bulk output + 16 per record, each only where it is read or written (the yardstick: input + bulk).
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

N, PEAK = 160, 8.0e12
SHAPES = {"S1": (8192, 8, 128, ("both",)), "S2": (10922, 6, 128, ("both",)), "S3": (8192, 8, 128, ("stats", "bulk")), "S4": (8192, 8, 2, ("both",)),
          "S5": (1, 6, 2, ("both",)), "S6": (10922, 6, 128, ("stats", "bulk"))}


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
    D_, K_, F_, modes = SHAPES[name]
    nb, rb = F_ * D_ * K_ * N * 2, F_ * D_ * K_ * 16
    ioset, (p_in, p_out, p_st), rep = ctx.io_alloc([(nb, capi.IO_INPUT), (nb, capi.IO_BULK), (rb, capi.IO_RECORD)])
    s = torch.cuda.current_stream()
    ctx.gen_uniform(p_in, nb, seed=D_ + K_ + F_, stream=s.cuda_stream)
    cp = capi.internal("igdsp_internal_snd_copy")

    def copy():
        rc = cp(ctx.h, p_in, D_, K_, F_, N, p_out, None, s.cuda_stream)
        assert rc == 0, rc

    cus, cus_min = timed(copy, s, reps, warmup)
    rows = []
    for mode in modes:
        bulk, st = (p_out if mode != "stats" else None), (p_st if mode != "bulk" else None)
        alg = nb + (nb if bulk else 0) + (rb if st else 0)
        for direction in ("combine", "split"):
            if direction == "combine":
                fn = lambda: ctx.snd_combine(p_in, D_, K_, F_, N, frames=bulk, stats=st, stream=s.cuda_stream)   # noqa: E731
            else:
                fn = lambda: ctx.snd_split(p_in, D_, K_, F_, N, pcm=bulk, stats=st, stream=s.cuda_stream)        # noqa: E731
            us, us_min = timed(fn, s, reps, warmup)
            rows.append({"case": name, "direction": direction, "outputs": mode, "D": D_, "K": K_, "F": F_, "n": N, "us_per_launch": round(us, 2),
                         "us_min": round(us_min, 2), "alg_bytes": alg, "frac_8TBps": round(alg / (us * 1e-6) / PEAK, 4), "copy_us": round(cus, 2),
                         "copy_us_min": round(cus_min, 2), "copy_frac_8TBps": round(2 * nb / (cus * 1e-6) / PEAK, 4),
                         "copy_over_snd": round(cus / us, 3), "bulk_spread": rep.get("bulk_spread"), "reps": reps})
    cus2, _ = timed(copy, s, reps, 1)                                   # once more after the entries: drift within the visit
    for r in rows:
        r["copy_us_again"] = round(cus2, 2)
    ioset.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="S1,S2,S3,S4,S5,S6")
    a = ap.parse_args()
    assert a.reps >= 1
    torch.cuda.set_device(0)
    rows = []
    with capi.Context(device=0, max_channels=64) as ctx:
        for name in a.only.split(","):
            for r in run_case(ctx, name, a.reps, a.warmup):
                print(json.dumps(r), flush=True)
                rows.append(r)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
