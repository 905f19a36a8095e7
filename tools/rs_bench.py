"""igdsp_resample timing: microseconds per launch (device events on the launch stream; median, min and max of --reps launches after a
warm-up), bytes read and written and the fraction of the 8 TB/s nominal HBM rate they represent, the packed dot products per second,
beside the compute-free yardstick (igdsp_internal_rs_copy: the same items in the same order, the same loads, tile traffic and stores,
an xor in place of the filter, zero records, no state) in the same process on the same buffers.  The buffers are plain device
allocations, one set for all cases.

    python tools/rs_bench.py [--reps 20] [--warmup 5] [--out profiles/rs_bench.json] [--only up6,down6] [--sweep up6,down6]

Shape: 65 536 channels x 128 frames x 160 narrow samples, the wide side in the row layout.  Cases: upR / downR for R = 2, 3, 4, 6 from
PCM with rows and records; upR_g711 from G.711 (both laws mixed per channel); up6_stats / down6_stats records only.
The figure judged is copy_over_entry, the yardstick's time over the entry's in the same run.  The entry's time includes k_rs_state (the
history write-back behind the kernel), which the yardstick does not run.
--sweep: the named cases once more with the grid sized for 1, 2, 3 and 4 blocks of 4 waves per CU (IGDSP_RS_BLOCKS, read by the
launcher at every call; the frames are cut to match), entry and yardstick in the same run: the wave-count sweep of DESIGN 3.18.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libigdsp.so: one HIP runtime per process)

from igate4xsoftphonedsp_amd import capi  # noqa: E402

C, F, N, PEAK = 65536, 128, 160, 8.0e12
CASES = {}
for _R in capi.RS_FACTORS:
    CASES[f"up{_R}"] = (capi.RS_UP, _R, False, True)
    CASES[f"down{_R}"] = (capi.RS_DOWN, _R, False, True)
    CASES[f"up{_R}_g711"] = (capi.RS_UP, _R, True, True)
CASES["up6_stats"] = (capi.RS_UP, 6, False, False)
CASES["down6_stats"] = (capi.RS_DOWN, 6, False, False)


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
    return float(np.median(t)), float(min(t)), float(max(t))


def run_case(ctx, name, bufs, reps, warmup):
    direction, R, g711, bulk = CASES[name]
    d_in, d_g711, d_codec, d_out, d_st, d_state = bufs
    s = torch.cuda.current_stream()
    n_in = N if direction == capi.RS_UP else N * R
    n_out = N * R if direction == capi.RS_UP else N
    in_bytes = C * F * n_in * (1 if g711 else 2)
    out_bytes, rec_bytes = C * F * n_out * 2, C * F * 16
    copy = capi.internal("igdsp_internal_rs_copy")
    payload, codec, pcm = (d_g711, d_codec, None) if g711 else (None, None, d_in)
    out = d_out if bulk else None

    def entry():
        ctx.resample(direction, R, d_state, C, F, N, payload=payload, codec=codec, pcm=pcm, out=out, stats=d_st, stream=s.cuda_stream)

    def yard():                                                            # the yardstick writes rows: records only has none of its own
        rc = copy(ctx.h, direction, R, capi.RS_ROWS, payload.data_ptr() if g711 else None, codec.data_ptr() if g711 else None,
                  None if g711 else pcm.data_ptr(), None, d_state.data_ptr(), C, F, N, 0, 0, d_out.data_ptr(), d_st.data_ptr(), s.cuda_stream)
        assert rc == 0, rc

    cus, cus_min, cus_max = timed(yard, s, reps, warmup) if bulk else (None, None, None)
    us, us_min, us_max = timed(entry, s, reps, warmup)
    moved = in_bytes + (out_bytes if bulk else 0) + rec_bytes
    dots = C * F * N * 12 * R                                              # lane operations of v_dot2c_i32_i16 in the filter
    row = {"case": name, "direction": "up" if direction == capi.RS_UP else "down", "R": R, "input": "g711" if g711 else "pcm",
           "outputs": "rows+records" if bulk else "records", "C": C, "F": F, "n": N, "us_per_launch": round(us, 1), "us_min": round(us_min, 1),
           "us_max": round(us_max, 1), "bytes_moved": moved, "frac_8TBps": round(moved / (us * 1e-6) / PEAK, 4),
           "gdot2_per_s": round(dots / (us * 1e-6) / 1e9, 1), "reps": reps}
    if bulk:
        cus2, _, _ = timed(yard, s, reps, 1)                               # once more after the entry: drift within the visit
        row.update({"copy_us": round(cus, 1), "copy_us_min": round(cus_min, 1), "copy_us_max": round(cus_max, 1), "copy_us_again": round(cus2, 1),
                    "copy_frac_8TBps": round(moved / (cus * 1e-6) / PEAK, 4), "copy_over_entry": round(cus / us, 3)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=",".join(CASES))
    ap.add_argument("--sweep", default="")
    a = ap.parse_args()
    assert a.reps >= 1
    torch.cuda.set_device(0)
    wide = C * F * N * 6
    d_in = torch.empty(wide, dtype=torch.int16, device="cuda")
    for k in range(0, wide, 1 << 28):                                      # speech-like levels: the clamp does not fire
        d_in[k:k + (1 << 28)].random_(-8000, 8000)
    d_g711 = torch.randint(0, 256, (C * F * N,), dtype=torch.uint8, device="cuda")
    d_codec = (torch.randint(0, 2, (C,), dtype=torch.uint8, device="cuda") * 8).contiguous()
    d_out = torch.empty(wide, dtype=torch.int16, device="cuda")
    d_st = torch.empty(C * F * 16, dtype=torch.uint8, device="cuda")
    d_state = torch.zeros(C * capi.RS_STATE.itemsize, dtype=torch.uint8, device="cuda")
    rows = []
    with capi.Context(device=0, max_channels=64) as ctx:
        for name in a.only.split(","):
            r = run_case(ctx, name, (d_in, d_g711, d_codec, d_out, d_st, d_state), a.reps, a.warmup)
            print(json.dumps(r), flush=True)
            rows.append(r)
        for name in [c for c in a.sweep.split(",") if c]:
            for blocks in (1, 2, 3, 4):
                os.environ["IGDSP_RS_BLOCKS"] = str(blocks)
                r = run_case(ctx, name, (d_in, d_g711, d_codec, d_out, d_st, d_state), a.reps, a.warmup)
                r.update({"case": f"{name}@{blocks}", "blocks_per_cu": blocks, "waves_per_cu_wanted": 4 * blocks})
                print(json.dumps(r), flush=True)
                rows.append(r)
            os.environ.pop("IGDSP_RS_BLOCKS", None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
