"""igdsp_echo_cancel timing: microseconds per launch (device events on the launch stream; median, min and max) beside, in the same
process, igdsp_decode_meter on the same codes, the compute-free yardstick igdsp_internal_ec_move, and a floor computed from the
kernel's own count of dot-product instructions at the clock the run reports.

    python tools/ec_bench.py [--reps 10] [--warmup 2] [--out profiles/ec_bench.json] [--only A2,A1,P2,R2,Z2,O2,O1]

Shapes (n = 160, C = 65 536 channels; four receivers share a transmitter's far row through d_far_of; every output unless said):
    A2  128 frames, L = 256, the near end G.711 (mixed laws): an echo of the far row at -6 dB, 40 samples late, and a little noise
    A1  the same at L = 128
    P2  128 frames, L = 256, the near end PCM
    R2  128 frames, L = 256, G.711, records only (d_out NULL)
    Z2  128 frames, L = 256, G.711, every channel IGDSP_EC_FREEZE: the filter and the detector, no gradient, no update
    O2  1 frame, L = 256, G.711 (a live gateway's per-tick call)
    O1  1 frame, L = 128, G.711
The floor: per block of 8 samples a lane of k_ec issues, with T = L / 16 taps, 4 T v_dot2_i32_i16 for the eight outputs, 4 T for the
gradient (none when frozen) and T / 2 for P; a wave is four channels, its instruction occupies its SIMD for four cycles, a CU has four
SIMDs: floor = C F / 4 * blocks * dots * 4 / (4 CUs) / clock.  The yardstick makes the same row loads, LDS stores, history moves,
records, row and state stores with no window read, dot product, reduction or update.  The aim is 1.5 x the larger of the two."""
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
SHAPES = {"A2": (128, 256, "g711", True, False), "A1": (128, 128, "g711", True, False), "P2": (128, 256, "pcm", True, False),
          "R2": (128, 256, "g711", False, False), "Z2": (128, 256, "g711", True, True), "O2": (1, 256, "g711", True, False),
          "O1": (1, 128, "g711", True, False)}


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


def device_clock_mhz(fallback, busy):
    """(MHz, where it came from): the shader clock while `busy` (a function that enqueues launches) keeps the device loaded, as the run
    can read it: the largest of a few torch.cuda.clock_rate samples, else the device properties' clock, else --clock-mhz"""
    best = 0.0
    try:
        for _ in range(6):
            busy()
            best = max(best, float(torch.cuda.clock_rate()))
        torch.cuda.synchronize()
    except Exception:
        torch.cuda.synchronize()
    if best >= 500.0:
        return best, "torch.cuda.clock_rate under load"
    props = torch.cuda.get_device_properties(0)
    if getattr(props, "clock_rate", 0):
        return props.clock_rate / 1e3, "device properties"
    return fallback, "--clock-mhz"


def scene(F_, C_, P_):
    """(near int16 [F][C][n], far int16 [F][P][n]) on the device: far rows of noise under a 4 Hz envelope, channel c hears row c // 4 at
    half the level, 40 samples late, with noise of sigma 20"""
    g = torch.Generator(device="cuda").manual_seed(1)
    S = F_ * N
    env = torch.sin(2 * math.pi * 4.0 * torch.arange(S, device="cuda") / 8000.0) ** 2
    far = (torch.randn((P_, S), device="cuda", generator=g) * 2000.0 * (0.2 + env)).round().clamp(-32768, 32767)
    echo = 0.5 * torch.roll(far, 40, dims=1)
    near = torch.empty((C_, S), device="cuda")
    for p0 in range(0, P_, 2048):                                         # by pieces: the whole near end in float would be 5 GB
        rows = echo[p0:p0 + 2048].repeat_interleave(4, dim=0)
        near[4 * p0:4 * p0 + rows.shape[0]] = rows + torch.randn(rows.shape, device="cuda", generator=g) * 20.0
    cut = lambda a, R: a.round().clamp(-32768, 32767).to(torch.int16).view(R, F_, N).permute(1, 0, 2).contiguous()
    return cut(near, C_), cut(far, P_)


def run_case(ctx, name, reps, warmup, C_, clock_fallback):
    F_, L, form, with_out, frozen = SHAPES[name]
    P_ = C_ // 4
    s = torch.cuda.current_stream()
    codec = torch.where(torch.arange(C_, device="cuda") % 2 == 0, 0, 8).to(torch.uint8)
    pcm, far = scene(F_, C_, P_)
    codes = None
    if form == "g711":
        codes = torch.empty((F_, C_, N), dtype=torch.uint8, device="cuda")
        ctx.encode(pcm, codec, C_, F_, N, codes, stream=s.cuda_stream)
        torch.cuda.synchronize()
        pcm = None
    far_of = (torch.arange(C_, device="cuda") // 4).to(torch.int32)
    ctl = torch.full((C_,), capi.EC_FREEZE if frozen else capi.EC_RUN, dtype=torch.uint8, device="cuda")
    cfg = capi.ec_cfg_default(L)
    state = torch.zeros(C_ * capi.EC_STATE.itemsize, dtype=torch.uint8, device="cuda")
    out = torch.empty(F_ * C_ * N * 2, dtype=torch.uint8, device="cuda") if with_out else None
    rec = torch.empty(F_ * C_ * 16, dtype=torch.uint8, device="cuda")
    stats = torch.empty(F_ * C_ * 16, dtype=torch.uint8, device="cuda")
    mv = capi.internal("igdsp_internal_ec_move")
    ptr = lambda t: None if t is None else t.data_ptr()

    def full():
        ctx.echo_cancel(far, P_, state, C_, F_, N, g711=codes, codec=codec if codes is not None else None, pcm=pcm, far_of=far_of, ctl=ctl, cfg=cfg,
                        out=out, rec=rec, stats=stats, stream=s.cuda_stream)

    def move():
        rc = mv(ctx.h, ptr(codes), ptr(codec) if codes is not None else None, ptr(pcm), ptr(far), P_, ptr(far_of), ptr(ctl), cfg.ctypes.data, C_, F_, N,
                ptr(state), ptr(out), ptr(rec), ptr(stats), s.cuda_stream)
        assert rc == 0, rc

    def meter():
        ctx.decode_meter(codes, codec, C_, F_, N, stats, stream=s.cuda_stream)

    t_full = timed(full, s, reps, warmup)
    clock = device_clock_mhz(clock_fallback, full)
    r = np.frombuffer(rec.cpu().numpy().tobytes(), capi.EC_REC).reshape(F_, C_)
    adapt_share = float(r["n_adapt"].sum()) / (F_ * C_ * math.ceil(N / 8))
    ne, oe = float(r["near_e"][-1].astype(np.float64).sum()), float(r["out_e"][-1].astype(np.float64).sum())
    t_move = timed(move, s, reps, warmup)
    t_meter = timed(meter, s, reps, warmup) if codes is not None else None
    cus, clock_hz = torch.cuda.get_device_properties(0).multi_processor_count, clock[0] * 1e6
    T = L // 16
    dots = (C_ * F_ / 4.0) * math.ceil(N / 8) * (4 * T + (0 if frozen else 4 * T) + T // 2)
    floor_us = dots * 4.0 / (4.0 * cus) / clock_hz * 1e6
    aim = 1.5 * max(floor_us, t_move["median"])
    return {"case": name, "C": C_, "F": F_, "n": N, "tail": L, "form": form, "out": with_out, "frozen": frozen, "us": t_full, "move_us": t_move,
            "decode_meter_us": t_meter, "dot_floor_us": round(floor_us, 2), "clock_mhz": round(clock[0]), "clock_from": clock[1], "compute_units": cus,
            "aim_us": round(aim, 2), "over_aim": round(t_full["median"] / aim, 3), "ns_per_channel_frame": round(t_full["median"] * 1e3 / (C_ * F_), 3),
            "adapting_blocks_share": round(adapt_share, 3), "erle_db_last_frame": round(10.0 * math.log10(max(ne, 1.0) / max(oe, 1.0)), 2), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="A2,A1,P2,R2,Z2,O2,O1")
    ap.add_argument("--channels", type=int, default=C_ALL)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="used only when the run cannot read the device's clock")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    with capi.Context(device=0, max_channels=64) as ctx:
        for name in a.only.split(","):
            r = run_case(ctx, name, a.reps, a.warmup, a.channels, a.clock_mhz)
            print(json.dumps(r), flush=True)
            rows.append(r)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
