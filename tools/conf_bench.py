"""igdsp_conf_mix timing: microseconds per launch (device events on the launch stream), algorithmic bytes and the fraction of the
8 TB/s nominal HBM rate they represent, beside the compute-free yardstick in the same process.

    python tools/conf_bench.py [--reps 20] [--warmup 5] [--out profiles/r06_conf_bench.json] [--only B1,B4]

Shapes (160 samples, G.711 input generated on the device, PCM output and records):
    B1 consoles, contiguous   C = 65 536, P = 8 192 ports of 8 consecutive channels, F = 128
    B2 consoles, random       B1 with the members a random permutation of the channels
    B3 fan-out                every channel in 2 of P = 16 384 ports of 8 members
    B4 skew                   P = 16 ports of 4 096 members (the block-split form)
    B5 the reference's shape  4 calls connected to 5 ports, F = 2: the fixed cost of a launch
Algorithmic bytes = the distinct channels' frames (F x n each) + their codec byte and gain, + port_ptr and members, + the output PCM
(F x P x n x 2) and records (F x P x 16).  Every gain is 256: the reference's start level 2.0, the full scale-and-clamp path.
The yardstick (igdsp_internal_conf_copy) walks the same items and member lists and reads and writes the same bytes, with no decode,
scale, clamp or record arithmetic.  Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
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


def shape(name):
    rng = np.random.default_rng(ord(name[1]))
    if name == "B1":
        return 65536, 8192, 128, np.arange(65536), np.arange(65536) // 8
    if name == "B2":
        return 65536, 8192, 128, rng.permutation(65536), np.arange(65536) // 8
    if name == "B3":
        C_, P_ = 65536, 16384
        return C_, P_, 128, np.concatenate([np.arange(C_), np.arange(C_)]), np.concatenate([np.arange(C_) // 8, (np.arange(C_) // 8 + P_ // 2) % P_])
    if name == "B4":
        return 65536, 16, 128, np.arange(65536), np.arange(65536) // 4096
    return 4, 5, 2, np.repeat(np.arange(4), 5), np.tile(np.arange(5), 4)


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
    C_, P_, F_, ch, pt = shape(name)
    ptr, mem = capi.conf_build(ch, pt, C_, P_)
    g = torch.Generator(device="cuda").manual_seed(C_ + P_)
    src = torch.randint(0, 256, (F_ * C_ * N,), dtype=torch.uint8, device="cuda", generator=g)
    codec = torch.from_numpy(np.where(np.arange(C_) & 1, 8, 0).astype(np.uint8)).cuda()
    gain = torch.full((C_,), 256, dtype=torch.int16, device="cuda")
    d_ptr, d_mem = torch.from_numpy(ptr.view(np.int32)).cuda(), torch.from_numpy(mem.view(np.int32)).cuda()
    out = torch.empty((F_ * P_ * N,), dtype=torch.int16, device="cuda")
    st = torch.empty((F_ * P_ * 16,), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()
    cp = capi.internal("igdsp_internal_conf_copy")

    def mix():
        ctx.conf_mix(gain, d_ptr, d_mem, len(mem), C_, P_, F_, N, out=out, stats=st, payload=src, codec=codec, stream=s.cuda_stream)

    def copy():
        rc = cp(ctx.h, src.data_ptr(), codec.data_ptr(), None, None, gain.data_ptr(), d_ptr.data_ptr(), d_mem.data_ptr(), len(mem), C_, P_, F_, N,
                out.data_ptr(), st.data_ptr(), s.cuda_stream)
        assert rc == 0, rc

    us, us_min = timed(mix, s, reps, warmup)
    cus, _ = timed(copy, s, reps, warmup)
    distinct = len(np.unique(mem))
    alg = distinct * (F_ * N + 1 + 2) + (P_ + 1) * 4 + len(mem) * 4 + F_ * P_ * (2 * N + 16)
    return {"case": name, "C": C_, "P": P_, "F": F_, "n_members": int(len(mem)), "us_per_launch": round(us, 2), "us_min": round(us_min, 2),
            "alg_bytes": alg, "frac_8TBps": round(alg / (us * 1e-6) / PEAK, 4), "copy_us": round(cus, 2),
            "copy_frac_8TBps": round(alg / (cus * 1e-6) / PEAK, 4), "mix_over_copy": round(us / cus, 3),
            "ns_per_MB": round(us * 1e3 / (alg / 1e6), 3), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="B1,B2,B3,B4,B5")
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
