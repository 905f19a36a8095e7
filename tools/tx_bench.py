"""igdsp_tx_packetize timing: microseconds per launch (device events on the launch stream), algorithmic bytes and the fraction of the
8 TB/s nominal HBM rate they represent.

    python tools/tx_bench.py [--reps 20] [--warmup 5] [--out profiles/r04_tx_bench.json]

Algorithmic bytes = input (2n or n per channel-frame) + ctl (1) + sizes (2) + info (8) per channel-frame, + the sum of the packet
sizes written, + state (64 read + 64 written) and send buffer (n read + n written) per channel.  Inputs are generated on the device.
Cases: 65 536 x 128 all-audio (PCM and G.711 input), 65 536 x 128 with a realistic mix (90 % of the legs idle: keep-alive
cadence), 65 536 x {1, 2, 8} and 4 096 x {1, 128}.  Prints one JSON line per case.
--ab: for every all-audio case also the compute-free packet writer (igdsp_internal_tx_copy: the same traversal and packet bytes,
no decisions, no encoder, no records) on the same buffers, in the same process.  --only N: just the first N cases."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libigdsp.so: one HIP runtime per process)

from igate4xsoftphonedsp_amd import capi  # noqa: E402

N, STRIDE, PEAK = 160, 180, 8.0e12
AB = False


def states(C_, mix, t0):
    st = np.zeros((C_,), capi.TX_CHAN)
    st["pt"] = np.where(np.arange(C_) & 1, 8, 0)
    st["ssrc"] = np.arange(C_) * 2654435761 & 0xFFFFFFFF
    st["keepalive_ms"] = 200
    st["calltype"] = capi.TX_CT_TX
    st["tx_slave"] = st["tx_slave_changed"] = 1
    st["slave_count"] = 5
    st["packet_cnt"] = 30
    st["r2s_send_ms"] = t0 - (np.arange(C_) % 10) * 20          # idle legs: one keep-alive per 10 frames, staggered
    active = np.ones(C_, bool) if not mix else (np.arange(C_) % 10) == 0
    st["ptt"] = active
    return st


def run_case(ctx, C_, F_, form, mix, reps, warmup):
    t0 = 1_000_000
    g = torch.Generator(device="cuda").manual_seed(C_ * 131 + F_)
    if form == "pcm":
        src = torch.randint(-32768, 32768, (F_ * C_ * N,), dtype=torch.int16, device="cuda", generator=g)
    else:
        src = torch.randint(0, 256, (F_ * C_ * N,), dtype=torch.uint8, device="cuda", generator=g)
    ctl = torch.zeros((F_ * C_,), dtype=torch.uint8, device="cuda")
    st0 = torch.from_numpy(states(C_, mix, t0).view(np.uint8).reshape(-1)).cuda()
    st = st0.clone()
    last = torch.zeros((C_ * N,), dtype=torch.uint8, device="cuda")
    pk = torch.empty((F_ * C_ * STRIDE,), dtype=torch.uint8, device="cuda")
    sizes = torch.empty((F_ * C_ * 2,), dtype=torch.uint8, device="cuda")
    info = torch.empty((F_ * C_ * 8,), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()

    def launch():
        ctx.tx_packetize(st, last, pk, STRIDE, sizes, info, C_, F_, N, t0, 20, pcm=src if form == "pcm" else None,
                         g711=src if form == "g711" else None, ctl=ctl, stream=s.cuda_stream)

    for _ in range(warmup):
        st.copy_(st0)
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        st.copy_(st0)                                     # the same decisions every repetition
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        launch()
        b.record(s)
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    sz = sizes.view(torch.int16).to(torch.int64) & 0xFFFF
    sent_bytes = int(sz.sum().item())
    in_b = (2 if form == "pcm" else 1) * N
    alg = C_ * F_ * (in_b + 1 + 2 + 8) + sent_bytes + C_ * (128 + 2 * N)
    us = float(np.median(times))
    ab = None
    if AB and not mix:
        fn = capi.internal("igdsp_internal_tx_copy")
        tcopy = []
        for r in range(warmup + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            rc = fn(ctx.h, src.data_ptr() if form == "pcm" else None, src.data_ptr() if form == "g711" else None, C_, F_, N, pk.data_ptr(),
                    STRIDE, s.cuda_stream)
            b.record(s)
            b.synchronize()
            assert rc == 0, rc
            if r >= warmup:
                tcopy.append(a.elapsed_time(b) * 1000.0)
        ab = round(float(np.median(tcopy)), 2)
    return {"case": f"{C_}x{F_}", "input": form, "mix": "idle-90%" if mix else "all-audio", "us_per_launch": round(us, 2),
            "us_min": round(min(times), 2), "alg_bytes": alg, "sent_bytes": sent_bytes,
            "frac_8TBps": round(alg / (us * 1e-6) / PEAK, 4), "reps": reps,
            **({"copy_us": ab, "copy_frac_8TBps": round(alg / (ab * 1e-6) / PEAK, 4)} if ab else {})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--only", type=int, default=0)
    a = ap.parse_args()
    global AB
    AB = a.ab
    torch.cuda.set_device(0)
    cases = [(65536, 128, "pcm", False), (65536, 128, "g711", False), (65536, 128, "pcm", True), (65536, 1, "pcm", False),
             (65536, 2, "pcm", False), (65536, 8, "pcm", False), (4096, 1, "pcm", False), (4096, 128, "pcm", False)]
    if a.only:
        cases = cases[:a.only]
    rows = []
    with capi.Context(device=0, max_channels=64) as ctx:
        for C_, F_, form, mix in cases:
            r = run_case(ctx, C_, F_, form, mix, a.reps, a.warmup)
            print(json.dumps(r), flush=True)
            rows.append(r)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
