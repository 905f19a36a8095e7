"""igdsp_bss_select timing: microseconds per call (device events on the launch stream), algorithmic bytes and the fraction of the
8 TB/s nominal HBM rate they represent, beside the compute-free yardstick and igdsp_decode_meter(..., d_pcm) over a [F][G][160]
payload (the emit's bytes: one frame in, one PCM frame and record out per group-frame), all in one process.

    python tools/bss_bench.py [--reps 20] [--warmup 5] [--out profiles/r07_bss_bench.json] [--only S1,S5]

Shapes (160-sample G.711 frames generated on the device, PCM output, records and sel; each channel's ED-137 word is constant over
the frames, open with probability 0.9, so that most groups hold a latched vote; a warm-up call brings the state there first):
    S1  C = 65 536, 16 384 groups of 4 consecutive channels, F = 128
    S2  S1 at F = 2: the real-time shape
    S3a groups of 2 (32 768 groups), S3b groups of 8 (8 192 groups), F = 128
    S4  skew: one group of 1 024 members, the rest groups of 4, F = 128
    S5  the reference's shape: one group of 4 at F = 2: the fixed cost of a call
Algorithmic bytes per group-frame: 8 m of info + 160 payload bytes when voted + 320 out + 16 record + 4 sel.  The yardstick
(igdsp_internal_bss_copy) walks the same groups, reads every info record and gathers the first member's frame of every group,
with no decode, scale, clamp, records or state machine.  Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run
of its own."""
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
    """C, F, group sizes"""
    if name == "S1":
        return 65536, 128, np.full(16384, 4)
    if name == "S2":
        return 65536, 2, np.full(16384, 4)
    if name == "S3a":
        return 65536, 128, np.full(32768, 2)
    if name == "S3b":
        return 65536, 128, np.full(8192, 8)
    if name == "S4":
        return 65536, 128, np.concatenate([[1024], np.full((65536 - 1024) // 4, 4)])
    return 4, 2, np.array([4])


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
    C_, F_, sizes = shape(name)
    G_ = len(sizes)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    rng = np.random.default_rng(len(name) + C_ + F_)
    w = np.where(rng.random(C_) < 0.9, 1 << 28, 0) | (rng.integers(0, 32, C_) << 3)
    info = np.zeros((F_, C_), capi.RTP_INFO)
    info["ed137"], info["payload_len"], info["pt"] = w.astype(np.uint32)[None, :], N, 8
    g = torch.Generator(device="cuda").manual_seed(C_ + F_)
    src = torch.randint(0, 256, (F_ * C_ * N,), dtype=torch.uint8, device="cuda", generator=g)
    codec = torch.full((C_,), 8, dtype=torch.uint8, device="cuda")
    d_info = torch.from_numpy(info.view(np.uint8).reshape(-1)).cuda()
    d_ptr = torch.from_numpy(ptr.view(np.int32)).cuda()
    d_mem = torch.arange(C_, dtype=torch.int32, device="cuda")
    state = torch.zeros(G_ * 4, dtype=torch.int32, device="cuda")
    words = torch.zeros(C_, dtype=torch.int32, device="cuda")
    sel = torch.empty(F_ * G_, dtype=torch.int32, device="cuda")
    out = torch.empty((F_ * G_ * N,), dtype=torch.int16, device="cuda")
    st = torch.empty((F_ * G_ * 16,), dtype=torch.uint8, device="cuda")
    # the decode + PCM reference over [F][G][160]
    rsrc = torch.randint(0, 256, (F_ * G_ * N,), dtype=torch.uint8, device="cuda", generator=g)
    rcodec = torch.full((G_,), 8, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()
    cp = capi.internal("igdsp_internal_bss_copy")

    def select():
        ctx.bss_select(d_info, d_ptr, d_mem, C_, state, words, C_, G_, F_, N, payload=src, codec=codec, sel=sel, out=out, stats=st,
                       stream=s.cuda_stream)

    def copy():
        rc = cp(ctx.h, d_info.data_ptr(), src.data_ptr(), codec.data_ptr(), None, None, None, d_ptr.data_ptr(), d_mem.data_ptr(), C_, None, C_,
                G_, F_, N, 0, state.data_ptr(), words.data_ptr(), sel.data_ptr(), out.data_ptr(), st.data_ptr(), s.cuda_stream)
        assert rc == 0, rc

    def decode():
        ctx.decode_meter(rsrc, rcodec, G_, F_, N, st, pcm=out, stream=s.cuda_stream)

    # warm state: a full-length call brings the groups to their latched votes (S2 / S5 then run on it)
    for _ in range(max(1, 12 // F_)):
        select()
    torch.cuda.synchronize()
    voted = float((sel.view(F_, G_) >= 0).float().mean().item())
    us, us_min = timed(select, s, reps, warmup)
    cus, _ = timed(copy, s, reps, warmup)
    dus, _ = timed(decode, s, reps, warmup)
    alg = int(F_ * (8 * C_ + voted * G_ * N + G_ * (2 * N + 16 + 4)))
    return {"case": name, "C": C_, "G": G_, "F": F_, "max_group": int(sizes.max()), "voted_frac": round(voted, 4),
            "us_per_call": round(us, 2), "us_min": round(us_min, 2), "alg_bytes": alg, "frac_8TBps": round(alg / (us * 1e-6) / PEAK, 4),
            "copy_us": round(cus, 2), "copy_frac_8TBps": round(alg / (cus * 1e-6) / PEAK, 4), "decode_pcm_us": round(dus, 2),
            "select_over_copy": round(us / cus, 3), "select_over_decode_pcm": round(us / dus, 3), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="S1,S2,S3a,S3b,S4,S5")
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
