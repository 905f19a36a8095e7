"""igdsp_tone_generate timing: microseconds per launch (device events on the launch stream; median, min and max of --reps launches after
a warm-up), bytes written and the fraction of the 8 TB/s nominal HBM rate they represent, beside the compute-free yardstick
(igdsp_internal_tone_fill: the same items in the same order, the same rows, lengths and records stored, no plan, no state, no
oscillator) in the same process on the same buffers.  Rows (IGDSP_IO_BULK) and records come from igdsp_io_alloc.

    python tools/tone_bench.py [--reps 20] [--warmup 5] [--out profiles/tone_bench.json] [--only T1,T3]

Shapes (65 536 ports, n = 160 samples, one plan for all ports, positions uniform over the cycle):
    T1 every row ON      440 + 480 Hz, 60 s on, no pause, no fades, F = 128: 2.7 GB of rows, far beyond the Infinity Cache;
                         also rows only and records only
    T2 the ring          the reference's plan, 2 s on / 1 s off, F = 128: a third of the rows are silent
    T3 real time         T1 at F = 1
The figure judged is fill_over_tone, the yardstick's time over the entry's in the same run (target 0.95 at T1).
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

P, N, PEAK = 65536, 160, 8.0e12
ALL_ON = [(440, 480, 60000, 0)]
RING = [(440, 480, 2000, 1000)]
SHAPES = {"T1": (ALL_ON, capi.TONE_LOOP | capi.TONE_NO_FADE, 128, ("both", "pcm", "stats")), "T2": (RING, capi.TONE_LOOP, 128, ("both",)),
          "T3": (ALL_ON, capi.TONE_LOOP | capi.TONE_NO_FADE, 1, ("both",))}


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
    return float(np.median(t)), float(min(t)), float(max(t))


def run_case(ctx, name, reps, warmup):
    tones, options, F_, modes = SHAPES[name]
    nb, rb, lb = F_ * P * N * 2, F_ * P * 16, F_ * P * 2
    ioset, (p_pcm, p_st), rep = ctx.io_alloc([(nb, capi.IO_BULK), (rb, capi.IO_RECORD)])
    s = torch.cuda.current_stream()
    plan = capi.tone_plan_build(tones, 8000, options)
    d_plan = torch.from_numpy(np.frombuffer(plan.tobytes(), np.uint8).copy()).cuda()
    st = np.zeros(P, capi.TONE_STATE)
    st["pos"] = np.random.default_rng(1).integers(0, int(plan["cycle"]), P)
    st["flags"] = capi.TONE_PLAYING
    d_state = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    d_len = torch.zeros(lb, dtype=torch.uint8, device="cuda")
    fill = capi.internal("igdsp_internal_tone_fill")
    rows = []
    for mode in modes:
        pcm, stats = (p_pcm if mode != "stats" else None), (p_st if mode != "pcm" else None)
        length = d_len.data_ptr() if pcm else None

        def gen():
            ctx.tone_generate(d_plan, 1, d_state, P, F_, N, pcm=pcm, length=length, stats=stats, stream=s.cuda_stream)

        def yard():                                                        # the yardstick writes rows: records only has none of its own
            rc = fill(ctx.h, d_plan.data_ptr(), 1, None, None, d_state.data_ptr(), P, F_, N, 0, p_pcm, length, stats, s.cuda_stream)
            assert rc == 0, rc

        fus, fus_min, fus_max = timed(yard, s, reps, warmup) if pcm else (None, None, None)
        us, us_min, us_max = timed(gen, s, reps, warmup)
        live = int((d_len.view(torch.int16) != 0).sum()) if pcm else None
        alg = (nb + lb if pcm else 0) + (rb if stats else 0)
        row = {"case": name, "outputs": mode, "P": P, "F": F_, "n": N, "us_per_launch": round(us, 2), "us_min": round(us_min, 2),
               "us_max": round(us_max, 2), "bytes_written": alg, "frac_8TBps": round(alg / (us * 1e-6) / PEAK, 4), "live_rows": live,
               "bulk_spread": rep.get("bulk_spread"), "reps": reps}
        if pcm:
            fus2, _, _ = timed(yard, s, reps, 1)                           # once more after the entry: drift within the visit
            row.update({"fill_us": round(fus, 2), "fill_us_min": round(fus_min, 2), "fill_us_max": round(fus_max, 2), "fill_us_again": round(fus2, 2),
                        "fill_frac_8TBps": round(alg / (fus * 1e-6) / PEAK, 4), "fill_over_tone": round(fus / us, 3)})
        rows.append(row)
    ioset.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="T1,T2,T3")
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
