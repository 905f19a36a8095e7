"""igdsp_ptt_arbitrate timing: microseconds per call (device events on the launch stream), algorithmic bytes and the fraction of the
8 TB/s nominal HBM rate they represent, beside its two yardsticks timed in the same process on the same buffers: igdsp_bss_select
(the receiver vote: the same bytes in and out) and the compute-free form of the same traversal (igdsp_internal_ptt_copy).

    python tools/ptt_bench.py [--reps 20] [--warmup 5] [--out profiles/r10_ptt_bench.json] [--only T1,T2]

Shapes (65 536 legs in 16 384 groups of 4 consecutive channels, 160-sample G.711 frames generated on the device, PCM output, records,
sel, tick and ctl; the payload, the PCM output and the records come from igdsp_io_alloc):
    T1  F = 128
    T2  F = 2: the real-time shape
Each channel's ED-137 word is constant over the frames: keyed (PTT type 1 .. 3) with probability 0.9 and squelch open with probability
0.9, so that most groups hold a transmitter (and a latched vote); a warm-up call brings the state there first.  Algorithmic bytes per
group-frame: 8 m of info + 160 payload bytes when held + 320 out + 16 record + 4 sel + 8 tick + 1 ctl.  Kernel times: run this under
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

N, PEAK, C_, M = 160, 8.0e12, 65536, 4
FRAMES = {"T1": 128, "T2": 2}


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
    F_ = FRAMES[name]
    G_ = C_ // M
    ptr = np.arange(0, C_ + 1, M, dtype=np.uint32)
    rng = np.random.default_rng(len(name) + C_ + F_)
    w = (np.where(rng.random(C_) < 0.9, rng.integers(1, 4, C_), 0) << 29) | np.where(rng.random(C_) < 0.9, 1 << 28, 0) | (rng.integers(0, 64, C_) << 22) \
        | (rng.integers(0, 32, C_) << 3)
    info = np.zeros((F_, C_), capi.RTP_INFO)
    info["ed137"], info["payload_len"], info["pt"] = w.astype(np.uint32)[None, :], N, 8
    ioset, (p_pl, p_out, p_st), rep = ctx.io_alloc([(F_ * C_ * N, capi.IO_INPUT), (F_ * G_ * N * 2, capi.IO_BULK), (F_ * G_ * 16, capi.IO_RECORD)])
    s = torch.cuda.current_stream()
    ctx.gen_uniform(p_pl, F_ * C_ * N, seed=C_ + F_, stream=s.cuda_stream)
    codec = torch.full((C_,), 8, dtype=torch.uint8, device="cuda")
    d_info = torch.from_numpy(info.view(np.uint8).reshape(-1)).cuda()
    d_ptr = torch.from_numpy(ptr.view(np.int32)).cuda()
    d_mem = torch.arange(C_, dtype=torch.int32, device="cuda")
    pstate = torch.zeros(G_ * 4, dtype=torch.int32, device="cuda")
    pslots = torch.zeros(C_ * 2, dtype=torch.int32, device="cuda")
    bstate = torch.zeros(G_ * 4, dtype=torch.int32, device="cuda")
    bwords = torch.zeros(C_, dtype=torch.int32, device="cuda")
    sel = torch.empty(F_ * G_, dtype=torch.int32, device="cuda")
    tick = torch.empty(F_ * G_ * 2, dtype=torch.int32, device="cuda")
    ctl = torch.empty(F_ * G_, dtype=torch.uint8, device="cuda")
    cp = capi.internal("igdsp_internal_ptt_copy")

    def ptt():
        ctx.ptt_arbitrate(d_info, d_ptr, d_mem, C_, pstate, pslots, C_, G_, F_, N, payload=p_pl, codec=codec, sel=sel, tick=tick, ctl_out=ctl,
                          out=p_out, stats=p_st, stream=s.cuda_stream)

    def copy():
        rc = cp(ctx.h, d_info.data_ptr(), p_pl, codec.data_ptr(), None, None, None, d_ptr.data_ptr(), d_mem.data_ptr(), C_, None, C_, G_, F_, N, 0,
                pstate.data_ptr(), pslots.data_ptr(), sel.data_ptr(), tick.data_ptr(), ctl.data_ptr(), p_out, p_st, s.cuda_stream)
        assert rc == 0, rc

    def bss():
        ctx.bss_select(d_info, d_ptr, d_mem, C_, bstate, bwords, C_, G_, F_, N, payload=p_pl, codec=codec, sel=sel, out=p_out, stats=p_st,
                       stream=s.cuda_stream)

    # warm state: the groups hold their transmitters and their latched votes (T2 then runs on it)
    for _ in range(max(1, 12 // F_)):
        ptt()
        bss()
    torch.cuda.synchronize()
    voted = float((sel.view(F_, G_) >= 0).float().mean().item())
    ptt()
    torch.cuda.synchronize()
    held = float((sel.view(F_, G_) >= 0).float().mean().item())
    us, us_min = timed(ptt, s, reps, warmup)
    bus, bus_min = timed(bss, s, reps, warmup)
    cus, _ = timed(copy, s, reps, warmup)
    us2, _ = timed(ptt, s, reps, 1)                                   # once more after the yardsticks: drift within the visit
    alg = int(F_ * (8 * C_ + held * G_ * N + G_ * (2 * N + 16 + 4 + 8 + 1)))
    ioset.close()
    return {"case": name, "C": C_, "G": G_, "F": F_, "held_frac": round(held, 4), "bss_voted_frac": round(voted, 4), "us_per_call": round(us, 2),
            "us_min": round(us_min, 2), "us_again": round(us2, 2), "alg_bytes": alg, "frac_8TBps": round(alg / (us * 1e-6) / PEAK, 4),
            "bss_us": round(bus, 2), "bss_us_min": round(bus_min, 2), "copy_us": round(cus, 2), "ptt_over_bss": round(us / bus, 3),
            "ptt_over_copy": round(us / cus, 3), "target": "parity with igdsp_bss_select", "target_met": bool(us <= 1.02 * bus),
            "bulk_spread": rep.get("bulk_spread"), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="T1,T2")
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
