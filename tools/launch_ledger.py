#!/usr/bin/env python3
"""The ledger of one launch of the headline kernel (k_meter_chunk64, 65 536 channels x F frames x 160 B) on placed buffers
(igdsp_io_alloc: payload INPUT, records RECORD, as bench.py allocates them), back-to-back launches with warm clocks:

    tools/launch_ledger.py [frames ...]        (default 64 128 256)

Per frame count, one markdown table row:
  ship   : event time per launch of the shipped instantiation with the launch aggregate (one event pair around N launches) — what
           bench.py reports as roofline.kernel_avg_ms;
  diag   : the same for the DIAG instantiation k_meter_chunk64<false, false, true>, whose stamps the other columns come from;
  span   : 100 MHz realtime, first wave begin -> last wave end of the LAST of those launches;
  outside: diag - span = what happens outside any wave's lifetime: dispatch + the boundary (write-back of dirty L2 lines);
  head   : wave begin -> prologue loads issued, and wave begin -> end of the barrier behind the LUT fill (shader cycles / clock);
  tail   : per block, its waves' last batch draw -> its last wave's end (median over blocks); chip-wide, the first draw that
           finds the device queue dry -> the last wave's end; and first wave end -> last wave end.
Then the line through the rows: slope (us per frame, fraction of 8 TB/s) between the two largest frame counts and the constant it
leaves at zero frames.  The stamps leave only through the diag buffer; the DIAG instantiation computes the same records."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from igate4xsoftphonedsp_amd import capi

C_, n = 65536, 160
FRAMES = [int(a) for a in sys.argv[1:]] or [64, 128, 256]
N_LAUNCH = 40
DW = 16                                             # kDiagWords
PEAK = 8.0e12

ctx = capi.Context(0, 1024)
L = ctx.L
L.igdsp_internal_diag_chunk32.restype = C.c_int
L.igdsp_internal_diag_chunk32.argtypes = [C.c_void_p] * 3 + [C.c_uint32] * 2 + [C.c_void_p] * 3
s = torch.cuda.current_stream().cuda_stream
nw = 256 * 16
d_cd = torch.zeros((C_,), dtype=torch.uint8, device="cuda")
d_dg = torch.zeros((nw * DW,), dtype=torch.int64, device="cuda")
d_agg = torch.zeros((capi.AGG_WORDS,), dtype=torch.int64, device="cuda")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps        # us per launch


rows = []
for F_ in FRAMES:
    nb_pl, nb_st = F_ * C_ * n, F_ * C_ * 16
    ioset, (p_pl, p_st), _ = ctx.io_alloc([(nb_pl, capi.IO_INPUT), (nb_st, capi.IO_RECORD)])
    d_pl, d_st = capi.as_tensor(p_pl, nb_pl), capi.as_tensor(p_st, nb_st)
    ctx.gen_uniform(d_pl, nb_pl, stream=s)
    ship = lambda: ctx.decode_meter(d_pl, d_cd, C_, F_, n, d_st, agg=d_agg, stream=s)
    diag = lambda: L.igdsp_internal_diag_chunk32(ctx.h, d_pl.data_ptr(), d_cd.data_ptr(), C_, F_, d_st.data_ptr(), d_dg.data_ptr(), s)
    timed(ship, max(20, 60 * 128 // F_))             # ~15 ms of load: steady clocks
    t_ship = min(timed(ship, N_LAUNCH) for _ in range(3))
    ref = d_st.clone()
    d_st.zero_()
    timed(diag, 10)
    t_diag = min(timed(diag, N_LAUNCH) for _ in range(3))
    torch.cuda.synchronize()
    assert torch.equal(ref, d_st), "the DIAG instantiation computes the same records"
    d = d_dg.cpu().numpy().view(np.uint64).reshape(nw, DW).astype(np.float64)
    d = d[d[:, 9] > 0]                               # waves that ran
    rt0, rt1 = d[:, 8], d[:, 9]
    begin, end = rt0.min(), rt1.max()
    span = (end - begin) / 100
    mhz = np.median((d[:, 2] - d[:, 0]) / (rt1 - rt0)) * 100
    ld = d[:, 12] > 0
    head_ld = np.median(d[ld, 12] - d[ld, 0]) / mhz
    head_bar = np.median(d[:, 1] - d[:, 0]) / mhz
    blk = d[:, 15].astype(np.int64)
    tails = []
    for b in np.unique(blk):
        m = blk == b
        draws = d[m, 13]
        draws = draws[draws >= begin]                # stamps of this launch only
        if draws.size:
            tails.append((rt1[m].max() - draws.max()) / 100)
    dry = d[:, 14]
    dry = dry[dry >= begin]
    rows.append(dict(F=F_, ship=t_ship, diag=t_diag, span=span, outside=t_diag - span, head_ld=head_ld, head_bar=head_bar,
                     begin_spread=(rt0.max() - begin) / 100, tail_blk=float(np.median(tails)) if tails else float("nan"),
                     tail_dry=(end - dry.min()) / 100 if dry.size else float("nan"), end_spread=(end - rt1.min()) / 100, mhz=mhz))
    ioset.close()

print(f"device {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}, {N_LAUNCH} back-to-back launches per figure (best of 3), shader clock {rows[-1]['mhz']:.0f} MHz")
print("| frames | ship us | diag us | span us | outside us | begin spread | head: loads issued | head: barrier end | tail: block draw->end | tail: queue dry->end | end spread |")
print("|---|---|---|---|---|---|---|---|---|---|---|")
for r in rows:
    print(f"| {r['F']} | {r['ship']:.1f} | {r['diag']:.1f} | {r['span']:.1f} | {r['outside']:.1f} | {r['begin_spread']:.1f} | {r['head_ld']:.2f} | {r['head_bar']:.2f} | "
          f"{r['tail_blk']:.1f} | {r['tail_dry']:.1f} | {r['end_spread']:.1f} |")
if len(rows) >= 2:
    a, b = rows[-2], rows[-1]
    for key in ("ship", "diag", "span"):
        slope = (b[key] - a[key]) / (b["F"] - a["F"])
        const = a[key] - slope * a["F"]
        print(f"{key}: slope {slope:.3f} us/frame = {C_ * (n + 16) / (slope * 1e-6) / 1e12:.2f} TB/s = {C_ * (n + 16) / (slope * 1e-6) / PEAK:.3f} of peak ({a['F']} -> {b['F']} frames); constant {const:.1f} us")
