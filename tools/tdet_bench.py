"""igdsp_tone_detect timing: microseconds per launch (device events on the launch stream; median, min and max) beside, in the same
process, igdsp_decode_meter on the same codes, the compute-free yardstick igdsp_internal_tdet_move, and a floor computed from the
kernel's own count of dot-product instructions at the clock the run reports.

    python tools/tdet_bench.py [--reps 10] [--warmup 2] [--out profiles/tdet_bench.json] [--only DG,DS,DP,EG,DR,D1,DC,DI]

Shapes (n = 160, C = 65 536; the DTMF plan unless said; records and the event list unless said):
    DG  128 frames, G.711 (mixed laws), every row a digit (channel c plays digit c mod 16 without pause)
    DS  128 frames, G.711, silence: the time should not depend on the data
    DP  128 frames, PCM, every row a digit
    EG  128 frames, G.711, the 8 + 8 plan
    DR  128 frames, G.711, records only (no list)
    D1  1 frame, G.711 (a live gateway's per-tick call)
    DC  128 frames, G.711, every channel a digit of 4 frames on / 4 frames off: every launch raises about 32 events per channel, so the
        list's write pass has events to store (in DG, DS, DP, EG and D1 the state carries the digit from launch to launch and the timed
        launches raise none: there the list costs its count pass, the scan and an empty write pass)
    DI  128 frames, G.711, every row a digit, four copies of the DTMF plan interleaved through d_plan_of (channel c has plan c mod 4):
        the four channels a wave works on together have four plans, the worst case of d_plan_of
The floor: k_tdet issues per frame and wave (four channels) 8 v_dot2_i32_i16 per table entry (two sample pairs, two evaluations, I and
Q), n / 4 entries per lane, half of that for a plan of at most 4 + 4 bins (two lanes share a bin's window), and 2 ceil(n / 32) for E; a
wave's instruction occupies its SIMD for four cycles, a CU has four SIMDs: floor = C F / 4 * dots * 4 / (4 CUs) / clock.  The yardstick makes the same row loads, LDS stores, history moves,
record and state stores and list passes with no table, pair read or dot product.  The aim is 1.5 x the larger of the two."""
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
LO, HI = (697, 770, 852, 941), (1209, 1336, 1477, 1633)
SHAPES = {"DG": (128, "g711", "digits", "dtmf", True), "DS": (128, "g711", "silence", "dtmf", True), "DP": (128, "pcm", "digits", "dtmf", True),
          "EG": (128, "g711", "digits", "8x8", True), "DR": (128, "g711", "digits", "dtmf", False), "D1": (1, "g711", "digits", "dtmf", True),
          "DC": (128, "g711", "cadence", "dtmf", True), "DI": (128, "g711", "digits", "dtmf4", True)}


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
    can read it: the largest of a few torch.cuda.clock_rate samples (the management library's current clock; an idle device reports
    its idle clock, hence the load), else the device properties' clock, else --clock-mhz"""
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


def digit_rows(F_, C_, cadence=False):
    """int16 [F][C][n] on the device: channel c plays digit c mod 16, 4 000 per tone"""
    t = torch.arange(F_ * N, device="cuda", dtype=torch.float64) / 8000.0
    pat = torch.stack([4000 * torch.sin(2 * math.pi * LO[d // 4] * t) + 4000 * torch.sin(2 * math.pi * HI[d % 4] * t) for d in range(16)])
    pat = pat.round().to(torch.int16).view(16, F_, N).permute(1, 0, 2)
    if cadence:                                                           # 4 frames on, 4 frames off
        pat = pat * ((torch.arange(F_, device="cuda") // 4) % 2 == 0).to(torch.int16).view(F_, 1, 1)
    return pat.repeat(1, C_ // 16, 1).contiguous()


def run_case(ctx, name, reps, warmup, C_, clock_fallback):
    F_, form, data, plan_name, with_list = SHAPES[name]
    s = torch.cuda.current_stream()
    codec = torch.where(torch.arange(C_, device="cuda") % 2 == 0, 0, 8).to(torch.uint8)
    pcm = digit_rows(F_, C_, data == "cadence") if data != "silence" else torch.zeros((F_, C_, N), dtype=torch.int16, device="cuda")
    codes = None
    if form == "g711":
        codes = torch.empty((F_, C_, N), dtype=torch.uint8, device="cuda")
        ctx.encode(pcm, codec, C_, F_, N, codes, stream=s.cuda_stream)
        torch.cuda.synchronize()
        pcm = None
    plan = capi.tdet_plan_build((350, 440, 480, 620) + LO, HI + (1800, 2000, 2200, 2400)) if plan_name == "8x8" else capi.tdet_plan_dtmf()
    n_plans = 4 if plan_name == "dtmf4" else 1
    d_plan = torch.from_numpy(np.frombuffer(plan.tobytes() * n_plans, np.uint8).copy()).cuda()
    plan_of = (torch.arange(C_, device="cuda") % 4).to(torch.int16) if n_plans > 1 else None
    state = torch.zeros(C_ * capi.TDET_STATE.itemsize, dtype=torch.uint8, device="cuda")
    rec = torch.empty(F_ * C_ * 8, dtype=torch.uint8, device="cuda")
    cap = 1 << 22
    events = torch.empty(cap * 16, dtype=torch.uint8, device="cuda")
    count = torch.zeros(2, dtype=torch.int32, device="cuda")
    work = torch.empty(capi.tdet_work_bytes(C_, F_, True) + 16, dtype=torch.uint8, device="cuda")
    stats = torch.empty(F_ * C_ * 16, dtype=torch.uint8, device="cuda")
    mv = capi.internal("igdsp_internal_tdet_move")
    lst = dict(events=events, event_cap=cap, event_count=count, work=work) if with_list else {}

    def full():
        ctx.tone_detect(d_plan, state, C_, F_, N, g711=codes, codec=codec if codes is not None else None, pcm=pcm, n_plans=n_plans, plan_of=plan_of, rec=rec,
                        stream=s.cuda_stream, **lst)

    def move():
        rc = mv(ctx.h, codes.data_ptr() if codes is not None else None, codec.data_ptr() if codes is not None else None,
                pcm.data_ptr() if pcm is not None else None, d_plan.data_ptr(), n_plans, plan_of.data_ptr() if plan_of is not None else None, C_, F_, N, 0, state.data_ptr(), rec.data_ptr(),
                events.data_ptr() if with_list else None, cap if with_list else 0, count.data_ptr() if with_list else None,
                work.data_ptr() if with_list else None, s.cuda_stream)
        assert rc == 0, rc

    def meter():
        ctx.decode_meter(codes, codec, C_, F_, N, stats, stream=s.cuda_stream)

    t_full = timed(full, s, reps, warmup)
    clock = device_clock_mhz(clock_fallback, full)
    n_events = int(count.cpu()[0]) if with_list else None
    t_move = timed(move, s, reps, warmup)
    t_meter = timed(meter, s, reps, warmup) if codes is not None else None
    cus, clock_hz = torch.cuda.get_device_properties(0).multi_processor_count, clock[0] * 1e6
    entries = math.ceil(N / 4)
    per_lane = entries if plan_name == "8x8" else math.ceil(entries / 2)
    dots = (C_ * F_ / 4.0) * (8 * per_lane + 2 * math.ceil(N / 32)) * (4 if n_plans > 1 else 1)     # interleaved plans: a wave runs four passes
    floor_us = dots * 4.0 / (4.0 * cus) / clock_hz * 1e6
    aim = 1.5 * max(floor_us, t_move["median"])
    return {"case": name, "C": C_, "F": F_, "n": N, "form": form, "data": data, "plan": plan_name, "list": with_list, "us": t_full, "move_us": t_move,
            "decode_meter_us": t_meter, "dot_floor_us": round(floor_us, 2), "clock_mhz": round(clock[0]), "clock_from": clock[1], "compute_units": cus,
            "aim_us": round(aim, 2), "over_aim": round(t_full["median"] / aim, 3), "ns_per_channel_frame": round(t_full["median"] * 1e3 / (C_ * F_), 3),
            "events_last_launch": n_events, "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="DG,DS,DP,EG,DR,D1,DC,DI")
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
