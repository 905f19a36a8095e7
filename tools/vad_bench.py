"""igdsp_vad_run timing: microseconds per launch (device events on the launch stream; median, min and max of at least 20 launches after
warm-up) beside, in the same process, the compute-free yardstick igdsp_internal_vad_move, igdsp_decode_meter on the same codes, the
headline meter (igdsp_decode_meter, records only, on uniform random codes in the same buffers: nothing else moved) and a floor computed
from the kernel's own count of dot-product instructions at the clock the run reports.

    python tools/vad_bench.py [--reps 20] [--warmup 3] [--out profiles/vad_bench.json] [--only V1,V2,V3,V4,V5,V6]

Shapes (n = 160, C = 65 536 channels; kind, record, payload and control byte unless said; the codes, the PCM rows, the state and the
outputs come from one igdsp_io_alloc call):
    V1  128 frames of G.711 (mixed laws): noise on every channel at 33, 100 and 330 rms: every frame is non-raw, SIDs come by schedule
        (sid_every = 50)
    V2  128 frames of G.711: the same noise with bursts 21 dB above it, 16 frames on, 16 off, the channels' phases spread: about half the
        frames are raw, a SID at every OFFSET
    V3  V2's rows as PCM
    V4  V2, records only
    V5  1 frame of V2 (a live gateway's per-tick call)
    V6  V2 with the kind and the control byte only (a VOX leg: no record, so the level pass runs only in waves with a silent row)
The floor: k_vad issues per frame and wave (four channels) n / 2 v_dot2_i32_i16 (lane k sums lag k over the row, two samples an
instruction); a wave's instruction occupies its SIMD for four cycles, a CU has four SIMDs: floor = C F / 4 * (n / 2) * 4 / (4 CUs) /
clock.  The aim is 1.5 x the larger of the yardstick and that floor.  Only the transposed lag shape exists and was timed."""
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
ALL, REC, VOX = ("kind", "rec", "sid", "txctl"), ("rec",), ("kind", "txctl")
SHAPES = {"V1": (128, "g711", ALL, False), "V2": (128, "g711", ALL, True), "V3": (128, "pcm", ALL, True), "V4": (128, "g711", REC, True),
          "V5": (1, "g711", ALL, True), "V6": (128, "g711", VOX, True)}


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


def fill_codes(ctx, p_codes, codec, F_, C_, bursts, s):
    """the scene, encoded into the codes' buffer eight frames at a time (the whole scene in float would be 5 GB)"""
    g = torch.Generator(device="cuda").manual_seed(1)
    level = torch.tensor([33.0, 100.0, 330.0], device="cuda")[torch.arange(C_, device="cuda") % 3].view(1, C_, 1)
    phase = (torch.arange(C_, device="cuda") * 7) % 32
    for f0 in range(0, F_, 8):
        f1 = min(F_, f0 + 8)
        x = torch.randn((f1 - f0, C_, N), device="cuda", generator=g) * level
        if bursts:
            on = ((torch.arange(f0, f1, device="cuda").view(-1, 1) + phase.view(1, -1)) % 32 < 16).view(f1 - f0, C_, 1)
            x = torch.where(on, x * 11.2, x)
        pcm = x.round().clamp(-32768, 32767).to(torch.int16).contiguous()
        ctx.encode(pcm, codec, C_, f1 - f0, N, p_codes + f0 * C_ * N, stream=s.cuda_stream)
        torch.cuda.synchronize()


def run_case(ctx, name, reps, warmup, C_, clock_fallback):
    F_, form, which, bursts = SHAPES[name]
    s = torch.cuda.current_stream()
    codec = torch.where(torch.arange(C_, device="cuda") % 2 == 0, 0, 8).to(torch.uint8)
    fc = F_ * C_
    spec = [(fc * N, capi.IO_INPUT), (fc * N * 2 if form == "pcm" else 16, capi.IO_INPUT), (C_ * capi.VAD_STATE.itemsize, capi.IO_RECORD), (fc, capi.IO_RECORD),
            (fc * 16, capi.IO_RECORD), (fc * 16, capi.IO_RECORD), (fc, capi.IO_RECORD), (fc * 16, capi.IO_RECORD)]
    ioset, (p_codes, p_pcm, p_state, p_kind, p_rec, p_sid, p_tx, p_stats), rep = ctx.io_alloc(spec)
    fill_codes(ctx, p_codes, codec, F_, C_, bursts, s)
    if form == "pcm":
        ctx.decode_meter(p_codes, codec, C_, F_, N, p_stats, pcm=p_pcm, stream=s.cuda_stream)
    ctx.gen_uniform(p_state, C_ * capi.VAD_STATE.itemsize, seed=3, stream=s.cuda_stream)     # no tag: every channel starts from RESET
    torch.cuda.synchronize()
    g711 = form == "g711"
    cfg = capi.vad_cfg_default()
    if not bursts:
        cfg["sid_every"] = 50
    mv = capi.internal("igdsp_internal_vad_move")
    outs = {k: v for k, v in dict(kind=p_kind, rec=p_rec, sid=p_sid, txctl=p_tx).items() if k in which}

    def full():
        ctx.vad_run(p_state, C_, F_, N, g711=p_codes if g711 else None, codec=codec if g711 else None, pcm=None if g711 else p_pcm, cfg=cfg,
                    stream=s.cuda_stream, **outs)

    def move():
        rc = mv(ctx.h, p_codes if g711 else None, codec.data_ptr() if g711 else None, None if g711 else p_pcm, None, cfg.ctypes.data, C_, F_, N, 0, p_state,
                outs.get("kind"), outs.get("rec"), outs.get("sid"), outs.get("txctl"), None, 0, None, None, s.cuda_stream)
        assert rc == 0, rc

    def meter():
        ctx.decode_meter(p_codes, codec, C_, F_, N, p_stats, stream=s.cuda_stream)

    t_full = timed(full, s, reps, warmup)
    clock = device_clock_mhz(clock_fallback, full)
    t_move = timed(move, s, reps, warmup)
    t_meter = timed(meter, s, reps, warmup)
    ctx.gen_uniform(p_codes, fc * N, seed=1, stream=s.cuda_stream)
    t_head = timed(meter, s, reps, warmup)
    cus, clock_hz = torch.cuda.get_device_properties(0).multi_processor_count, clock[0] * 1e6
    dots = (fc / 4.0) * (N / 2)
    floor_us = dots * 4.0 / (4.0 * cus) / clock_hz * 1e6
    aim = 1.5 * max(floor_us, t_move["median"])
    alg = fc * (N * (1 if g711 else 2) + sum({"kind": 1, "rec": 16, "sid": 16, "txctl": 1}[k] for k in which)) + 2 * C_ * capi.VAD_STATE.itemsize
    ioset.close()
    return {"case": name, "C": C_, "F": F_, "n": N, "form": form, "outputs": "+".join(which), "bursts": bursts, "us": t_full, "move_us": t_move,
            "decode_meter_us": t_meter, "headline_meter_us": t_head, "dot_floor_us": round(floor_us, 2), "clock_mhz": round(clock[0]),
            "clock_from": clock[1], "compute_units": cus, "aim_us": round(aim, 2), "over_aim": round(t_full["median"] / aim, 3),
            "ns_per_channel_frame": round(t_full["median"] * 1e3 / fc, 3), "algorithmic_bytes": alg,
            "share_of_8_TBps": round(alg / (t_full["median"] * 1e-6) / 8e12, 4), "lag_shape": "transposed (the only one built and timed)",
            "bulk_spread": rep.get("bulk_spread"), "reps": reps}


def flag_shares(ctx, name, C_):
    """the shares of raw, VOICE and SID frames of a scene, from one launch of its own on plain buffers (a small slice of the channels)"""
    F_, form, _, bursts = SHAPES[name]
    C_ = min(C_, 3072)
    s = torch.cuda.current_stream()
    codec = torch.where(torch.arange(C_, device="cuda") % 2 == 0, 0, 8).to(torch.uint8)
    codes = torch.empty(F_ * C_ * N, dtype=torch.uint8, device="cuda")
    fill_codes(ctx, codes.data_ptr(), codec, F_, C_, bursts, s)
    state = torch.zeros(C_ * capi.VAD_STATE.itemsize, dtype=torch.uint8, device="cuda")
    rec = torch.empty(F_ * C_ * 16, dtype=torch.uint8, device="cuda")
    cfg = capi.vad_cfg_default()
    if not bursts:
        cfg["sid_every"] = 50
    for _ in range(2):                                                     # the second pass: a floor that has settled
        ctx.vad_run(state, C_, F_, N, g711=codes, codec=codec, cfg=cfg, rec=rec, stream=s.cuda_stream)
    torch.cuda.synchronize()
    fl = np.frombuffer(rec.cpu().numpy().tobytes(), capi.VAD_REC)["flags"]
    return {k: round(float(((fl & b) != 0).mean()), 4) for k, b in (("raw", capi.VAD_F_RAW), ("voice", capi.VAD_F_VOICE), ("sid", capi.VAD_F_SID))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="V1,V2,V3,V4,V5,V6")
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
            r["frame_shares"] = flag_shares(ctx, name, a.channels)
            print(json.dumps(r), flush=True)
            rows.append(r)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
