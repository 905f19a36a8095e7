"""igdsp_cng_run timing: microseconds per launch (device events on the launch stream; median, min and max of at least 20 launches after
warm-up) beside, in the same process, the compute-free yardstick igdsp_internal_cng_move, igdsp_decode_meter on the same codes, the
headline meter (igdsp_decode_meter, records only, on uniform random codes in the same buffers: nothing else moved; here the scene's codes
are those uniform codes already, so decode_meter_us and headline_meter_us are the same call timed twice) and a floor computed
from the kernel's own count of vector instructions per sample at the clock the run reports.

    python tools/cng_bench.py [--reps 20] [--warmup 3] [--out profiles/cng_bench.json] [--only N1,N2,N3,N4,N5]

Shapes (n = 160, C = 65 536 channels; rows, lengths, records and PCM records unless said; kinds, payloads, the voice rows, the state and
the outputs come from one igdsp_io_alloc call):
    N1  128 frames, voice rows as PCM: a SID of order 10 in frame 0, then NONE: every frame is generated
    N2  128 frames, voice rows as G.711 (mixed laws): talkspurts of 16 VOICE frames, 16 silent ones behind a SID, the channels' phases
        spread: half the frames are generated
    N3  N1 with a payload of order 0 (the lattice runs all ten stages with kq = 0)
    N4  N2 without d_len_out (d_out is required, so a launch for the records alone still writes the rows)
    N5  1 frame of N2 (a live gateway's per-tick call)
The floor: k_cng's sample loop issues VALU_PER_SAMPLE vector instructions per generated sample and lane (counted in the saved ISA of
k_cng<2, false>: 191 in the loop's body of two samples; tests/test_cng_resources_cpu.py recounts it from the .s file with
tools/kernel_resources.py's loop_valu_count and fails when the constant is stale); at 65 536 channels a SIMD holds one wave, which issues a vector instruction
every 4 cycles: floor = generated samples per lane x VALU_PER_SAMPLE x 4 / clock.  The aim is 1.5 x the larger of the yardstick and
that floor.  Only the lane-per-channel shape with full waves (64 channels a block) exists and was timed."""
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
VALU_PER_SAMPLE = 95.5                     # tests/test_cng_resources_cpu.py counts the saved ISA's sample loop against this
ISSUE_CYCLES_ONE_WAVE = 4.0
SHAPES = {"N1": (128, "pcm", False, 10), "N2": (128, "g711", True, 10), "N3": (128, "pcm", False, 0), "N4": (128, "g711", True, 10), "N5": (1, "g711", True, 10)}


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


def scene(F_, C_, talk, order):
    """kind [F][C] and sid [F][C][16] on the device: a SID in frame 0; with talkspurts 16 VOICE frames, a SID, 15 NONE, phases spread"""
    f = torch.arange(F_, device="cuda").view(-1, 1)
    c = torch.arange(C_, device="cuda").view(1, -1)
    kind = torch.zeros((F_, C_), dtype=torch.uint8, device="cuda")
    if talk:
        ph = (f + c * 7) % 32
        kind = torch.where(ph < 16, 1, torch.where(ph == 16, 2, 0)).to(torch.uint8)
    kind[0] = 2
    g = torch.Generator(device="cuda").manual_seed(2)
    sid = torch.zeros((F_, C_, 16), dtype=torch.uint8, device="cuda")
    sid[:, :, 0] = (30 + (c % 30)).to(torch.uint8)
    if order:
        sid[:, :, 1:1 + order] = (127 + torch.randn((F_, C_, order), device="cuda", generator=g) * 40).round().clamp(0, 254).to(torch.uint8)
    return kind.contiguous(), sid.contiguous(), order + 1


def run_case(ctx, name, reps, warmup, C_, clock_fallback):
    F_, form, talk, order = SHAPES[name]
    s = torch.cuda.current_stream()
    codec = torch.where(torch.arange(C_, device="cuda") % 2 == 0, 0, 8).to(torch.uint8)
    fc = F_ * C_
    sb = capi.CNG_STATE.itemsize
    spec = [(fc * N, capi.IO_INPUT), (fc * N * 2 if form == "pcm" else 16, capi.IO_INPUT), (fc, capi.IO_INPUT), (fc * 16, capi.IO_INPUT), (C_ * sb, capi.IO_RECORD),
            (fc * N * 2, capi.IO_RECORD), (fc * 2, capi.IO_RECORD), (fc * 16, capi.IO_RECORD), (fc * 16, capi.IO_RECORD)]
    ioset, (p_codes, p_pcm, p_kind, p_sid, p_state, p_out, p_len, p_rec, p_stats), rep = ctx.io_alloc(spec)
    kind, sid, sid_len = scene(F_, C_, talk, order)
    L = capi.load()                                                        # the scene goes into the io buffers through the library's copies
    h_kind, h_sid = np.ascontiguousarray(kind.cpu().numpy()), np.ascontiguousarray(sid.cpu().numpy())    # alive across the copies
    assert L.igdsp_copy_h2d(ctx.h, p_kind, h_kind.ctypes.data, fc) == 0
    assert L.igdsp_copy_h2d(ctx.h, p_sid, h_sid.ctypes.data, fc * 16) == 0
    del h_kind, h_sid, kind, sid
    ctx.gen_uniform(p_codes, fc * N, seed=1, stream=s.cuda_stream)
    if form == "pcm":
        ctx.decode_meter(p_codes, codec, C_, F_, N, p_stats, pcm=p_pcm, stream=s.cuda_stream)
    ctx.gen_uniform(p_state, C_ * sb, seed=3, stream=s.cuda_stream)        # no tag: every channel starts from RESET
    torch.cuda.synchronize()
    g711 = form == "g711"
    sl = torch.full((fc,), sid_len, dtype=torch.uint8, device="cuda")
    d_seed = torch.from_numpy(((np.arange(C_, dtype=np.uint64) * 2654435761) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).cuda()
    p_len = p_len if name != "N4" else None
    mv = capi.internal("igdsp_internal_cng_move")

    def full():
        ctx.cng_run(p_kind, p_sid, p_state, p_out, C_, F_, N, sid_len=sl, g711=p_codes if g711 else None, codec=codec if g711 else None,
                    pcm=None if g711 else p_pcm, seed=d_seed, len_out=p_len, rec=p_rec, stats=p_stats, stream=s.cuda_stream)

    def move():
        rc = mv(ctx.h, p_kind, p_sid, sl.data_ptr(), p_codes if g711 else None, codec.data_ptr() if g711 else None, None if g711 else p_pcm, None,
                d_seed.data_ptr(), C_, F_, N, p_state, p_out, p_len, p_rec, p_stats, s.cuda_stream)
        assert rc == 0, rc

    def meter():
        ctx.decode_meter(p_codes, codec, C_, F_, N, p_stats, stream=s.cuda_stream)

    t_full = timed(full, s, reps, warmup)
    clock = device_clock_mhz(clock_fallback, full)
    torch.cuda.synchronize()
    rec = np.zeros(fc, capi.CNG_REC)
    assert L.igdsp_copy_d2h(ctx.h, rec.ctypes.data, p_rec, fc * 16) == 0
    gen_share = float(((rec["flags"] & capi.CNG_F_GENERATED) != 0).mean())
    gen_per_lane = int(((rec["flags"].reshape(F_, C_) & capi.CNG_F_GENERATED) != 0).sum(axis=0).max()) * N
    t_move = timed(move, s, reps, warmup)
    t_meter = timed(meter, s, reps, warmup)
    t_head = timed(meter, s, reps, warmup)                                 # the codes are uniform random already: the headline's input
    cus, clock_hz = torch.cuda.get_device_properties(0).multi_processor_count, clock[0] * 1e6
    waves_per_simd = max(1.0, (C_ / 64.0) / (4.0 * cus))
    floor_us = gen_per_lane * VALU_PER_SAMPLE * max(ISSUE_CYCLES_ONE_WAVE, 2.0 * waves_per_simd) / clock_hz * 1e6
    aim = 1.5 * max(floor_us, t_move["median"])
    alg = fc * (1 + 16 + 1 + N * (1 if g711 else 2) + N * 2 + 2 + 16 + 16) + 2 * C_ * sb
    ioset.close()
    return {"case": name, "C": C_, "F": F_, "n": N, "form": form, "order": order, "talkspurts": talk, "us": t_full, "move_us": t_move,
            "decode_meter_us": t_meter, "headline_meter_us": t_head, "valu_floor_us": round(floor_us, 2), "valu_per_sample": VALU_PER_SAMPLE,
            "generated_share": round(gen_share, 4), "generated_samples_per_lane": gen_per_lane, "clock_mhz": round(clock[0]), "clock_from": clock[1],
            "compute_units": cus, "aim_us": round(aim, 2), "over_aim": round(t_full["median"] / aim, 3),
            "ns_per_channel_frame": round(t_full["median"] * 1e3 / fc, 3), "algorithmic_bytes": alg,
            "share_of_8_TBps": round(alg / (t_full["median"] * 1e-6) / 8e12, 4), "shape": "lane per channel, 64 channels a block (the only one timed)",
            "bulk_spread": rep.get("bulk_spread"), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="N1,N2,N3,N4,N5")
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
