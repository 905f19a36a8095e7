"""igdsp_link_watch timing: microseconds per call (device events on the launch stream) beside its compute-free yardstick
(igdsp_internal_link_copy: the same passes and bytes, no state machine) timed in the same process on the same buffers, each with an
event list (count, scan and write passes) and without one (a single pass), and the ratios the design is judged by.

    python tools/link_bench.py [--reps 20] [--warmup 5] [--out profiles/r11_link_bench.json] [--only L1,L2,L3]

Shapes (65 536 legs, 1 arrival slot per tick, every slot holding a packet, kind bytes and a list of up to 65 536 events):
    L1  T = 128, healthy: every leg keeps sending keep-alives, no events after the warm-up
    L2  T = 128, 1 % of the legs change between audio and keep-alives in each tick
    L3  T = 2: the real-time shape (healthy), with igdsp_ptt_arbitrate's 2-frame launch (16 384 groups of 4, no audio) beside it for scale
Algorithmic bytes per call: 8 T C of records + T C kind bytes + 32 C of state in and out (read twice with a list).  Kernel times: run
this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libigdsp.so: one HIP runtime per process)

from igate4xsoftphonedsp_amd import capi  # noqa: E402

PEAK, C_, CAP = 8.0e12, 65536, 65536
CASES = {"L1": (128, 0.0), "L2": (128, 0.01), "L3": (2, 0.0)}


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
    T_, change = CASES[name]
    rng = np.random.default_rng(len(name) + C_ + T_)
    info = np.zeros((T_, C_), capi.RTP_INFO)
    info["pt"], info["flags"] = 123, capi.RTP_V2 | capi.RTP_KEEPALIVE
    if change:                                                           # a changing leg toggles between audio and keep-alives every tick
        legs = rng.random((T_, C_)) < change
        info["pt"] = np.where(legs & (np.arange(T_)[:, None] % 2 == 0), 8, 123)
        info["payload_len"] = np.where(info["pt"] == 8, 160, 0)
    info["ed137"] = rng.integers(0, 1 << 32, (T_, C_), dtype=np.uint64).astype(np.uint32)
    s = torch.cuda.current_stream()
    d_info = torch.from_numpy(info.view(np.uint8).reshape(-1)).cuda()
    state = torch.zeros(C_ * 16, dtype=torch.uint8, device="cuda")
    kind = torch.empty(T_ * C_, dtype=torch.uint8, device="cuda")
    events = torch.empty(CAP * 16, dtype=torch.uint8, device="cuda")
    count = torch.zeros(2, dtype=torch.int32, device="cuda")
    work = torch.empty(capi.link_work_bytes(C_, T_), dtype=torch.uint8, device="cuda")
    cp = capi.internal("igdsp_internal_link_copy")
    t0 = [1_000_000]

    def link(want_list=True):
        ctx.link_watch(d_info, state, C_, T_, 1, t0_ms=t0[0], tick_ms=20, kind=kind, events=events if want_list else None,
                       event_cap=CAP if want_list else 0, event_count=count if want_list else None, work=work if want_list else None,
                       stream=s.cuda_stream)
        t0[0] += 20 * T_

    def copy(want_list=True):
        rc = cp(ctx.h, d_info.data_ptr(), None, None, None, C_, T_, 1, t0[0], 20, 0, 0, state.data_ptr(), kind.data_ptr(),
                events.data_ptr() if want_list else None, CAP if want_list else 0, count.data_ptr() if want_list else None,
                work.data_ptr() if want_list else None, s.cuda_stream)
        assert rc == 0, rc

    link()                                                               # warm state: the calls are up
    link()
    torch.cuda.synchronize()
    n_events = int(count[0].item())
    us, us_min = timed(link, s, reps, warmup)
    us1, us1_min = timed(lambda: link(False), s, reps, warmup)
    cus, cus_min = timed(copy, s, reps, warmup)
    cus1, cus1_min = timed(lambda: copy(False), s, reps, warmup)
    us2, _ = timed(link, s, reps, 1)                                     # once more after the yardsticks: drift within the visit
    alg1 = T_ * C_ * 9 + 32 * C_
    row = {"case": name, "C": C_, "T": T_, "events_per_call": n_events, "us_list": round(us, 2), "us_list_min": round(us_min, 2),
           "us_list_again": round(us2, 2), "us_single": round(us1, 2), "us_single_min": round(us1_min, 2), "copy_us_list": round(cus, 2),
           "copy_us_list_min": round(cus_min, 2), "copy_us_single": round(cus1, 2), "copy_us_single_min": round(cus1_min, 2),
           "list_over_copy_list": round(us / cus, 3), "list_over_copy_single": round(us / cus1, 3), "single_over_copy_single": round(us1 / cus1, 3),
           "alg_bytes_single": alg1, "frac_8TBps_single": round(alg1 / (us1 * 1e-6) / PEAK, 4),
           "target": "list <= 2 x the yardstick's single pass", "target_met": bool(us <= 2.0 * cus1), "reps": reps}
    if T_ == 2:                                                          # igdsp_ptt_arbitrate's 2-frame launch on the same records, for scale
        G_ = C_ // 4
        d_ptr = torch.from_numpy(np.arange(0, C_ + 1, 4, dtype=np.uint32).view(np.int32)).cuda()
        d_mem = torch.arange(C_, dtype=torch.int32, device="cuda")
        pstate = torch.zeros(G_ * 4, dtype=torch.int32, device="cuda")
        pslots = torch.zeros(C_ * 2, dtype=torch.int32, device="cuda")
        sel = torch.empty(T_ * G_, dtype=torch.int32, device="cuda")
        tick = torch.empty(T_ * G_ * 2, dtype=torch.int32, device="cuda")
        pus, pus_min = timed(lambda: ctx.ptt_arbitrate(d_info, d_ptr, d_mem, C_, pstate, pslots, C_, G_, T_, 160, sel=sel, tick=tick,
                                                      stream=s.cuda_stream), s, reps, warmup)
        row.update(ptt_us=round(pus, 2), ptt_us_min=round(pus_min, 2), list_over_ptt=round(us / pus, 3))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="L1,L2,L3")
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
