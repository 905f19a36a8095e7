"""igdsp_agc_run timing: microseconds per launch (device events on the launch stream; median, min and max) beside, in the same
process, igdsp_decode_meter with its PCM store on the same codes and the compute-free yardstick igdsp_internal_agc_move.

    python tools/agc_bench.py [--reps 10] [--warmup 2] [--out profiles/agc_bench.json] [--only G,P,R,L,G1,P1]

Shapes (n = 160, C = 65 536 channels; every output unless said):
    G   128 frames of G.711 (mixed laws): noise under a 3 Hz envelope, the channels' levels spread over 40 dB
    P   the same rows as PCM
    R   128 frames of G.711, records only (d_out NULL)
    L   128 frames of G.711 with a full-scale sample at a random place of every frame and gmin = 4096, so that the slow gain cannot
        duck under the spikes: a limiter event in every frame
    G1  1 frame of G.711 (a live gateway's per-tick call)
    P1  1 frame of PCM
The yardstick makes the same row loads and decode, state load and store, row, record and PCM-record stores with no block peak,
division, recurrence or gain.  The aim is 1.5 x the larger of the yardstick and decode + PCM store (igdsp_decode_meter writes the same
bytes of PCM and one 16-byte record per frame from the same codes; for the PCM shapes it runs on the codes the rows came from)."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libigdsp.so: one HIP runtime per process)

from igate4xsoftphonedsp_amd import capi  # noqa: E402

N, C_ALL = 160, 65536
SHAPES = {"G": (128, "g711", True, False), "P": (128, "pcm", True, False), "R": (128, "g711", False, False), "L": (128, "g711", True, True),
          "G1": (1, "g711", True, False), "P1": (1, "pcm", True, False)}


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


def scene(F_, C_, spikes):
    """int16 [F][C][n] on the device: noise under a 3 Hz envelope, channel c at 100 * 10^((c % 5) / 2.5): 100 .. 4 000; with spikes one
    sample of every frame is 32767"""
    g = torch.Generator(device="cuda").manual_seed(1)
    out = torch.empty((F_, C_, N), dtype=torch.int16, device="cuda")
    level = (100.0 * 10.0 ** ((torch.arange(C_, device="cuda") % 5) / 2.5)).view(1, C_, 1)
    for f0 in range(0, F_, 8):                                             # by pieces: the whole scene in float would be 5 GB
        f1 = min(F_, f0 + 8)
        t = (torch.arange(f0 * N, f1 * N, device="cuda") / 8000.0).view(f1 - f0, 1, N)
        env = 0.2 + torch.sin(2 * math.pi * 3.0 * t) ** 2
        x = torch.randn((f1 - f0, C_, N), device="cuda", generator=g) * level * env
        if spikes:
            at = torch.randint(0, N, (f1 - f0, C_, 1), device="cuda", generator=g)
            x.scatter_(2, at, 32767.0)
        out[f0:f1] = x.round().clamp(-32768, 32767).to(torch.int16)
    return out


def run_case(ctx, name, reps, warmup, C_):
    F_, form, with_out, spikes = SHAPES[name]
    s = torch.cuda.current_stream()
    codec = torch.where(torch.arange(C_, device="cuda") % 2 == 0, 0, 8).to(torch.uint8)
    pcm = scene(F_, C_, spikes)
    codes = torch.empty((F_, C_, N), dtype=torch.uint8, device="cuda")
    ctx.encode(pcm, codec, C_, F_, N, codes, stream=s.cuda_stream)
    torch.cuda.synchronize()
    g711 = form == "g711"
    state = torch.zeros(C_ * capi.AGC_STATE.itemsize, dtype=torch.uint8, device="cuda")
    out = torch.empty(F_ * C_ * N * 2, dtype=torch.uint8, device="cuda") if with_out else None
    rec = torch.empty(F_ * C_ * 16, dtype=torch.uint8, device="cuda")
    stats = torch.empty(F_ * C_ * 16, dtype=torch.uint8, device="cuda")
    dm_pcm = torch.empty(F_ * C_ * N * 2, dtype=torch.uint8, device="cuda")
    cfg = capi.agc_cfg_default()
    if spikes:
        cfg["gmin"] = 4096
    mv = capi.internal("igdsp_internal_agc_move")
    ptr = lambda t: None if t is None else t.data_ptr()

    def full():
        ctx.agc_run(state, C_, F_, N, g711=codes if g711 else None, codec=codec if g711 else None, pcm=None if g711 else pcm, cfg=cfg, out=out,
                    rec=rec, stats=stats, stream=s.cuda_stream)

    def move():
        rc = mv(ctx.h, ptr(codes) if g711 else None, ptr(codec) if g711 else None, None if g711 else ptr(pcm), None, cfg.ctypes.data, C_, F_, N, ptr(state),
                ptr(out), ptr(rec), ptr(stats), s.cuda_stream)
        assert rc == 0, rc

    def meter():
        ctx.decode_meter(codes, codec, C_, F_, N, stats, pcm=dm_pcm, stream=s.cuda_stream)

    t_full = timed(full, s, reps, warmup)
    r = np.frombuffer(rec.cpu().numpy().tobytes(), capi.AGC_REC).reshape(F_, C_)
    limited = float((r["flags"] & capi.AGC_LIMITED).astype(bool).mean())
    active = float((r["flags"] & capi.AGC_ACTIVE).astype(bool).mean())
    t_move = timed(move, s, reps, warmup)
    t_meter = timed(meter, s, reps, warmup)
    aim = 1.5 * max(t_move["median"], t_meter["median"])
    bytes_moved = F_ * C_ * (N * (1 if g711 else 2) + (N * 2 if with_out else 0) + 32) + C_ * 32
    return {"case": name, "C": C_, "F": F_, "n": N, "form": form, "out": with_out, "spikes": spikes, "us": t_full, "move_us": t_move,
            "decode_meter_pcm_us": t_meter, "aim_us": round(aim, 2), "over_aim": round(t_full["median"] / aim, 3),
            "ns_per_channel_frame": round(t_full["median"] * 1e3 / (C_ * F_), 3), "algorithmic_bytes": bytes_moved,
            "share_of_8_TBps": round(bytes_moved / (t_full["median"] * 1e-6) / 8e12, 4), "limited_frames_share": round(limited, 3),
            "active_frames_share": round(active, 3), "max_out_peak": int(r["out_peak"].max()), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="G,P,R,L,G1,P1")
    ap.add_argument("--channels", type=int, default=C_ALL)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    with capi.Context(device=0, max_channels=64) as ctx:
        for name in a.only.split(","):
            r = run_case(ctx, name, a.reps, a.warmup, a.channels)
            print(json.dumps(r), flush=True)
            rows.append(r)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
