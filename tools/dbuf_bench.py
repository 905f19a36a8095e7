"""igdsp_dbuf_run timing: microseconds per launch (device events on the launch stream), algorithmic bytes and the fraction of the 8 TB/s
nominal HBM rate they represent, beside the same launch without records, the compute-free yardstick, and for scale igdsp_plc_conceal
(lossless, PCM input) and igdsp_snd_split (8 channels per card) at the same row count, all in one process on the same buffers.

    python tools/dbuf_bench.py [--reps 20] [--warmup 3] [--out profiles/dbuf_bench.json] [--only D1,D3]

Shapes (n = 160, M = 960, speech-like input: a harmonic series with a per-channel fundamental; every optional output written):
    D1  C = 65 536, 128 steps, every step PUT|GET, steady
    D2  as D1 with every channel's producer 1 % fast: one step in a hundred of a channel is a second PUT (no GET), the phases spread
        over the channels; six launches ahead of the timed ones fill the buffers to where about one channel in a hundred shrinks per step
    D3  C = 65 536, 1 step, PUT|GET (a live gateway's per-tick call)
Every timed launch continues the same state; a PUT-only step ahead of everything gives every channel a frame of delay.  Algorithmic
bytes per step: the op byte, 2 n in per PUT, 2 n out per GET, the flag, the 2-byte len, the 2-byte fill and the 16-byte record; per
channel and launch the 40 scalar bytes of the state read and written and the live samples (the mean fill) read and written once: the
state bytes a launch must touch.  The rows' way through the ring inside a launch is not counted.  The yardstick
(igdsp_internal_dbuf_move) takes every step as PUT|GET at a fixed fill of n with no update, search, blend or record arithmetic.  Kernel
times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libigdsp.so: one HIP runtime per process)

from igate4xsoftphonedsp_amd import capi  # noqa: E402

N, M, PEAK = 160, 960, 8.0e12


def shape(name):
    """C, T, drift"""
    return {"D1": (65536, 128, False), "D2": (65536, 128, True), "D3": (65536, 1, False)}[name]


def speech(C_, T):
    """[T][C][N] int16: four harmonics of a fundamental between 70 and 190 Hz per channel, continuous over the launch"""
    k = torch.arange(T * N, device="cuda", dtype=torch.float32).view(T, 1, N)
    f0 = (70.0 + 120.0 * torch.rand(C_, device="cuda")).view(1, C_, 1)
    x = torch.zeros((T, C_, N), device="cuda", dtype=torch.float32)
    for h, a in ((1, 6000.0), (2, 3000.0), (3, 1500.0), (4, 700.0)):
        x += a * torch.sin(2.0 * np.pi * h * f0 * k / 8000.0 + 0.7 * h)
    return x.round().clamp(-32768, 32767).to(torch.int16).contiguous()


def ops_for(C_, T, drift, launch):
    ops = torch.full((T, C_), capi.DBUF_PUT | capi.DBUF_GET, dtype=torch.uint8, device="cuda")
    if drift:
        t = (torch.arange(T, device="cuda", dtype=torch.float64) + launch * T).view(T, 1)
        ph = (torch.arange(C_, device="cuda", dtype=torch.float64) / C_).view(1, C_)
        extra = torch.floor((t + 1) * 0.01 + ph) > torch.floor(t * 0.01 + ph)
        ops[extra] = capi.DBUF_PUT
    return ops


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
    C_, T, drift = shape(name)
    torch.manual_seed(C_ + T)
    x = speech(C_, T)
    ops = ops_for(C_, T, drift, 0)
    state = torch.zeros(C_ * capi.DBUF_STATE.itemsize, dtype=torch.uint8, device="cuda")
    out = torch.zeros(T * C_ * N, dtype=torch.int16, device="cuda")
    fl = torch.empty(T * C_, dtype=torch.uint8, device="cuda")
    lo = torch.empty(T * C_, dtype=torch.int16, device="cuda")
    fi = torch.empty(T * C_, dtype=torch.int16, device="cuda")
    st = torch.empty(T * C_ * 16, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()
    mv = capi.internal("igdsp_internal_dbuf_move")

    def run():
        ctx.dbuf_run(ops, x, state, C_, T, N, M, out, flags=fl, length=lo, fill=fi, stats=st, stream=s.cuda_stream)

    def bare():
        ctx.dbuf_run(ops, x, state, C_, T, N, M, out, flags=fl, length=lo, fill=fi, stream=s.cuda_stream)

    def move():
        rc = mv(ctx.h, ops.data_ptr(), x.data_ptr(), C_, T, N, M, state.data_ptr(), out.data_ptr(), fl.data_ptr(), lo.data_ptr(), fi.data_ptr(),
                st.data_ptr(), s.cuda_stream)
        assert rc == 0, rc

    # one PUT of delay, as a port that has started
    ctx.dbuf_run(torch.full((1, C_), capi.DBUF_PUT, dtype=torch.uint8, device="cuda"), x, state, C_, 1, N, M, out, stream=s.cuda_stream)
    if drift:
        for _ in range(6):
            run()
    us, us_min = timed(run, s, reps, warmup)
    torch.cuda.synchronize()
    host = np.frombuffer(state.cpu().numpy().tobytes(), capi.DBUF_STATE)
    shrinks_per_step = None
    if drift:
        before = host["shrinks"].astype(np.int64).sum()
        run()
        torch.cuda.synchronize()
        after = np.frombuffer(state.cpu().numpy().tobytes(), capi.DBUF_STATE)["shrinks"].astype(np.int64).sum()
        shrinks_per_step = float(after - before) / (C_ * T)
    bus, _ = timed(bare, s, reps, warmup)
    mus, _ = timed(move, s, reps, warmup)
    # for scale: the concealment (lossless, PCM in) and the splitter over the same rows
    plc_state = torch.zeros(C_ * capi.PLC_STATE.itemsize, dtype=torch.uint8, device="cuda")
    played = torch.full((T, C_), capi.JB_PLAYED, dtype=torch.uint8, device="cuda")
    pus, _ = timed(lambda: ctx.plc_conceal(played, plc_state, out, C_, T, N, pcm=x, len_out=lo, stats=st, stream=s.cuda_stream), s, reps, warmup)
    sus, _ = timed(lambda: ctx.snd_split(x, C_ // 8, 8, T, N, pcm=out, stats=st, stream=s.cuda_stream), s, reps, warmup)
    gets = float((ops & capi.DBUF_GET).ne(0).float().mean().item())
    puts = float((ops & capi.DBUF_PUT).ne(0).float().mean().item())
    alg = int(C_ * T * (1 + 1 + 2 + 2 + 16 + puts * 2 * N + gets * 2 * N) + C_ * 2 * (40 + 2 * float(host["len"].mean())))
    return {"case": name, "C": C_, "T": T, "n": N, "max_samples": M, "put_frac": round(puts, 4), "get_frac": round(gets, 4),
            "shrinks_per_channel_step": None if shrinks_per_step is None else round(shrinks_per_step, 5),
            "mean_fill": round(float(host["len"].mean()), 1), "us_per_call": round(us, 2), "us_min": round(us_min, 2), "alg_bytes": alg,
            "frac_8TBps": round(alg / (us * 1e-6) / PEAK, 4), "no_records_us": round(bus, 2), "move_us": round(mus, 2),
            "move_frac_8TBps": round(alg / (mus * 1e-6) / PEAK, 4), "move_over_run": round(mus / us, 3), "plc_lossless_us": round(pus, 2),
            "snd_split_us": round(sus, 2), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="D1,D2,D3")
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
