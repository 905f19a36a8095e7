"""igdsp_filt_run timing: microseconds per launch (device events on the launch stream; median, min and max of at least 20 launches after
warm-up) beside, in the same process, the compute-free yardstick igdsp_internal_filt_move, igdsp_decode_meter on the same codes, the
headline meter (igdsp_decode_meter, records only, on uniform random codes in the same buffers: nothing else moved; here the scene's codes
are those uniform codes already, so decode_meter_us and headline_meter_us are the same call timed twice) and a floor computed from the
kernel's own count of vector instructions per sample at the clock the run reports.

    python tools/filt_bench.py [--reps 20] [--warmup 3] [--out profiles/filt_bench.json] [--only G1,G2,...]

Shapes (n = 160, C = 65 536 channels, 128 frames unless said; rows, records and PCM records unless said; the codes, the PCM rows, the
state and the outputs come from one igdsp_io_alloc call; every channel runs the same plan from a RESET state):
    G1 G2 G4  from G.711 (mixed laws) at max_sections 1 (DC_BLOCK), 2 (CTCSS_HP) and 4 (CTCSS_HP then VOICE_BAND)
    P1 P2 P4  the same from PCM (the decoded codes)
    R2        G2 without d_out: records and PCM records only
    T2        1 frame of G2 (a live gateway's per-tick call)
The floor: k_filt's sample loop issues VALU_PER_SAMPLE[S] vector instructions per sample and lane (counted in the saved ISA of
k_filt<IN, S, false>: 35, 59 and 109 in the loop's body of two samples; tests/test_filt_resources_cpu.py recounts them from the .s file
with tools/kernel_resources.py's loop_valu_count and fails when a constant is stale); at 65 536 channels a SIMD holds one wave, which
issues a vector instruction every 4 cycles: floor = samples per lane x VALU_PER_SAMPLE[S] x 4 / clock.  The aim is 1.5 x the larger of
the yardstick and that floor.  Only the lane-per-channel shape with full waves (64 channels a block) and five v_mad_i32_i24 a section
exists and was timed."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libigdsp.so: one HIP runtime per process)

from igate4xsoftphonedsp_amd import capi  # noqa: E402

N, C_ALL = 160, 65536
VALU_PER_SAMPLE = {1: 17.5, 2: 29.5, 4: 54.5}   # tests/test_filt_resources_cpu.py counts the saved ISA's sample loops against these
ISSUE_CYCLES_ONE_WAVE = 4.0
SHAPES = {"G1": (128, "g711", 1, True), "G2": (128, "g711", 2, True), "G4": (128, "g711", 4, True), "P1": (128, "pcm", 1, True), "P2": (128, "pcm", 2, True),
          "P4": (128, "pcm", 4, True), "R2": (128, "g711", 2, False), "T2": (1, "g711", 2, True)}


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


def plan_for(sections):
    """one FILT_PLAN of 1, 2 or 4 sections from the presets"""
    if sections == 1:
        return capi.filt_plan_preset(capi.FILT_DC_BLOCK, 8000)
    plan = capi.filt_plan_preset(capi.FILT_CTCSS_HP, 8000)
    if sections == 4:
        plan["s"][2:4] = capi.filt_plan_preset(capi.FILT_VOICE_BAND, 8000)["s"][0:2]
        plan["n_sections"] = 4
    return plan


def run_case(ctx, name, reps, warmup, C_, clock_fallback):
    F_, form, sections, with_out = SHAPES[name]
    s = torch.cuda.current_stream()
    codec = torch.where(torch.arange(C_, device="cuda") % 2 == 0, 0, 8).to(torch.uint8)
    fc = F_ * C_
    sb = capi.FILT_STATE.itemsize
    spec = [(fc * N, capi.IO_INPUT), (fc * N * 2 if form == "pcm" else 16, capi.IO_INPUT), (C_ * sb, capi.IO_RECORD), (fc * N * 2 if with_out else 16, capi.IO_RECORD),
            (fc * 16, capi.IO_RECORD), (fc * 16, capi.IO_RECORD)]
    ioset, (p_codes, p_pcm, p_state, p_out, p_rec, p_stats), rep = ctx.io_alloc(spec)
    ctx.gen_uniform(p_codes, fc * N, seed=1, stream=s.cuda_stream)
    if form == "pcm":
        ctx.decode_meter(p_codes, codec, C_, F_, N, p_stats, pcm=p_pcm, stream=s.cuda_stream)
    ctx.gen_uniform(p_state, C_ * sb, seed=3, stream=s.cuda_stream)        # no tag: every channel starts from zero histories
    plan = plan_for(sections)
    assert capi.filt_plan_check(plan) == 0 and int(plan["n_sections"]) == sections
    d_plan = torch.from_numpy(np.frombuffer(plan.tobytes(), np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    g711 = form == "g711"
    p_out = p_out if with_out else None
    mv = capi.internal("igdsp_internal_filt_move")

    def full():
        ctx.filt_run(d_plan, 1, p_state, C_, F_, N, g711=p_codes if g711 else None, codec=codec if g711 else None, pcm=None if g711 else p_pcm,
                     max_sections=sections, out=p_out, rec=p_rec, stats=p_stats, stream=s.cuda_stream)

    def move():
        rc = mv(ctx.h, p_codes if g711 else None, codec.data_ptr() if g711 else None, None if g711 else p_pcm, None, d_plan.data_ptr(), 1, None, sections,
                C_, F_, N, p_state, p_out, p_rec, p_stats, s.cuda_stream)
        assert rc == 0, rc

    def meter():
        ctx.decode_meter(p_codes, codec, C_, F_, N, p_stats, stream=s.cuda_stream)

    t_full = timed(full, s, reps, warmup)
    clock = device_clock_mhz(clock_fallback, full)
    torch.cuda.synchronize()
    L = capi.load()
    rec = np.zeros(fc, capi.FILT_REC)
    assert L.igdsp_copy_d2h(ctx.h, rec.ctypes.data, p_rec, fc * 16) == 0
    assert (rec["n_sections"] == sections).all() and not (rec["flags"] & (capi.FILT_NO_PLAN | capi.FILT_BAD_PLAN | capi.FILT_BYPASSED)).any()
    t_move = timed(move, s, reps, warmup)
    t_meter = timed(meter, s, reps, warmup)
    t_head = timed(meter, s, reps, warmup)                                 # the codes are uniform random already: the headline's input
    cus, clock_hz = torch.cuda.get_device_properties(0).multi_processor_count, clock[0] * 1e6
    waves_per_simd = max(1.0, (C_ / 64.0) / (4.0 * cus))
    floor_us = F_ * N * VALU_PER_SAMPLE[sections] * max(ISSUE_CYCLES_ONE_WAVE, 2.0 * waves_per_simd) / clock_hz * 1e6
    aim = 1.5 * max(floor_us, t_move["median"])
    alg = fc * (N * (1 if g711 else 2) + (N * 2 if with_out else 0) + 16 + 16) + 2 * C_ * sb
    ioset.close()
    return {"case": name, "C": C_, "F": F_, "n": N, "form": form, "sections": sections, "rows_out": with_out, "us": t_full, "move_us": t_move,
            "decode_meter_us": t_meter, "headline_meter_us": t_head, "valu_floor_us": round(floor_us, 2), "valu_per_sample": VALU_PER_SAMPLE[sections],
            "clipped_share": round(float(((rec["flags"] & capi.FILT_CLIPPED) != 0).mean()), 4), "clock_mhz": round(clock[0]), "clock_from": clock[1],
            "compute_units": cus, "aim_us": round(aim, 2), "over_aim": round(t_full["median"] / aim, 3),
            "ns_per_channel_frame": round(t_full["median"] * 1e3 / fc, 3), "algorithmic_bytes": alg,
            "share_of_8_TBps": round(alg / (t_full["median"] * 1e-6) / 8e12, 4),
            "shape": "lane per channel, 64 channels a block, five v_mad_i32_i24 a section (the only one timed)", "bulk_spread": rep.get("bulk_spread"), "reps": reps}


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
