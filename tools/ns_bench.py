"""igdsp_ns_run timing: microseconds per launch (device events on the launch stream; median, min and max of at least 20 launches after
warm-up) beside, in the same process, the compute-free yardstick igdsp_internal_ns_move, igdsp_decode_meter on the same codes, the
headline meter (igdsp_decode_meter, records only, on uniform random codes in the same buffers: nothing else moved; here the scene's
codes are those uniform codes already, so decode_meter_us and headline_meter_us are the same call timed twice) and a floor computed from
the kernel's own count of vector instructions per butterfly at the clock the run reports.

    python tools/ns_bench.py [--reps 20] [--warmup 3] [--out profiles/ns_bench.json] [--only G,P,...]

Shapes (n = 160, C = 65 536 channels, 128 frames unless said; rows, records and PCM records unless said; the codes, the PCM rows, the
state and the outputs come from one igdsp_io_alloc call; the state starts without a tag, so every channel starts fresh):
    G   from G.711 (mixed laws)
    P   the same from PCM (the decoded codes)
    R   G without d_out: records and PCM records only
    Z   G with every channel at IGDSP_NS_FREEZE
    T   1 frame of G (a live gateway's per-tick call)
The floor: per hop and channel the transform is 14 passes of 64 butterflies, four a lane and pass; a butterfly is VALU_PER_BUTTERFLY
vector instructions (counted in the saved ISA of k_ns<IN, false>; tests/test_ns_resources_cpu.py recounts them from the .s file with
tools/kernel_resources.py's block_counts and fails when a constant is stale), a wave is four channels, and a SIMD issues one vector
instruction of one wave every 4 cycles however many waves it holds: floor = waves per SIMD x hops x 7 x 4 x (forward + inverse) x 4 /
clock.  It counts the passes alone (no split pass, bands, window, decode) and every instruction at full rate (v_mad_i64_i32 is not).
The aim is 1.5 x the larger of the yardstick and that floor.  Only the 16-lanes-per-channel shape with the points in LDS exists and
was timed."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libigdsp.so: one HIP runtime per process)

from igate4xsoftphonedsp_amd import capi  # noqa: E402

N, C_ALL, HOP = 160, 65536, 80
VALU_PER_BUTTERFLY = {"forward": 32, "inverse": 39}   # tests/test_ns_resources_cpu.py counts the saved ISA's butterfly blocks against these
ISSUE_CYCLES = 4.0
SHAPES = {"G": (128, "g711", True, capi.NS_RUN), "P": (128, "pcm", True, capi.NS_RUN), "R": (128, "g711", False, capi.NS_RUN),
          "Z": (128, "g711", True, capi.NS_FREEZE), "T": (1, "g711", True, capi.NS_RUN)}


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


def run_case(ctx, name, reps, warmup, C_, clock_fallback):
    F_, form, with_out, ctl_value = SHAPES[name]
    s = torch.cuda.current_stream()
    codec = torch.where(torch.arange(C_, device="cuda") % 2 == 0, 0, 8).to(torch.uint8)
    ctl = torch.full((C_,), ctl_value, dtype=torch.uint8, device="cuda")
    fc = F_ * C_
    sb = capi.NS_STATE.itemsize
    spec = [(fc * N, capi.IO_INPUT), (fc * N * 2 if form == "pcm" else 16, capi.IO_INPUT), (C_ * sb, capi.IO_RECORD), (fc * N * 2 if with_out else 16, capi.IO_RECORD),
            (fc * 16, capi.IO_RECORD), (fc * 16, capi.IO_RECORD)]
    ioset, (p_codes, p_pcm, p_state, p_out, p_rec, p_stats), rep = ctx.io_alloc(spec)
    ctx.gen_uniform(p_codes, fc * N, seed=1, stream=s.cuda_stream)
    if form == "pcm":
        ctx.decode_meter(p_codes, codec, C_, F_, N, p_stats, pcm=p_pcm, stream=s.cuda_stream)
    ctx.gen_uniform(p_state, C_ * sb, seed=3, stream=s.cuda_stream)        # no tag: every channel starts fresh
    torch.cuda.synchronize()
    g711 = form == "g711"
    p_out = p_out if with_out else None
    cfg = np.ascontiguousarray(capi.ns_cfg_default())
    mv = capi.internal("igdsp_internal_ns_move")

    def full():
        ctx.ns_run(p_state, C_, F_, N, g711=p_codes if g711 else None, codec=codec if g711 else None, pcm=None if g711 else p_pcm, ctl=ctl, cfg=cfg,
                   out=p_out, rec=p_rec, stats=p_stats, stream=s.cuda_stream)

    def move():
        rc = mv(ctx.h, p_codes if g711 else None, codec.data_ptr() if g711 else None, None if g711 else p_pcm, None, cfg.ctypes.data, C_, F_, N, p_state,
                p_out, p_rec, p_stats, s.cuda_stream)
        assert rc == 0, rc

    def meter():
        ctx.decode_meter(p_codes, codec, C_, F_, N, p_stats, stream=s.cuda_stream)

    t_full = timed(full, s, reps, warmup)
    clock = device_clock_mhz(clock_fallback, full)
    torch.cuda.synchronize()
    L = capi.load()
    rec = np.zeros(fc, capi.NS_REC)
    assert L.igdsp_copy_d2h(ctx.h, rec.ctypes.data, p_rec, fc * 16) == 0
    assert not (rec["flags"] & capi.NS_BYPASSED).any() and ((rec["flags"] & capi.NS_FROZEN) != 0).all() == (ctl_value == capi.NS_FREEZE)
    t_move = timed(move, s, reps, warmup)
    t_meter = timed(meter, s, reps, warmup)
    t_head = timed(meter, s, reps, warmup)                                 # the codes are uniform random already: the headline's input
    cus, clock_hz = torch.cuda.get_device_properties(0).multi_processor_count, clock[0] * 1e6
    waves_per_simd = max(1.0, (C_ / 4.0) / (4.0 * cus))                    # four channels a wave, one after another or side by side: the issue rate is the SIMD's
    per_hop = 7 * 4 * (VALU_PER_BUTTERFLY["forward"] + VALU_PER_BUTTERFLY["inverse"])
    floor_us = waves_per_simd * F_ * (N // HOP) * per_hop * ISSUE_CYCLES / clock_hz * 1e6
    aim = 1.5 * max(floor_us, t_move["median"])
    alg = fc * (N * (1 if g711 else 2) + (N * 2 if with_out else 0) + 16 + 16) + 2 * C_ * sb
    ioset.close()
    return {"case": name, "C": C_, "F": F_, "n": N, "form": form, "rows_out": with_out, "ctl": int(ctl_value), "us": t_full, "move_us": t_move,
            "decode_meter_us": t_meter, "headline_meter_us": t_head, "valu_floor_us": round(floor_us, 2), "valu_per_butterfly": VALU_PER_BUTTERFLY,
            "suppressing_share": round(float(((rec["flags"] & capi.NS_SUPPRESSING) != 0).mean()), 4), "clock_mhz": round(clock[0]), "clock_from": clock[1],
            "compute_units": cus, "aim_us": round(aim, 2), "over_aim": round(t_full["median"] / aim, 3), "aim": "met" if t_full["median"] <= aim else "missed",
            "ns_per_channel_frame": round(t_full["median"] * 1e3 / fc, 3), "algorithmic_bytes": alg,
            "share_of_8_TBps": round(alg / (t_full["median"] * 1e-6) / 8e12, 4),
            "shape": "16 lanes a channel, four channels a wave, the points in LDS, 64-bit products (the only one timed)", "bulk_spread": rep.get("bulk_spread"),
            "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=",".join(SHAPES))
    ap.add_argument("--channels", type=int, default=C_ALL)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="used only when the run cannot read the device's clock")
    a = ap.parse_args()
    assert a.reps >= 1
    assert not a.out or a.reps >= 20, "a result file holds medians of at least 20 launches: --out needs --reps >= 20"
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
