"""igdsp_jb_receive timing: microseconds per call (device events on the launch stream), algorithmic bytes and the fraction of the 8 TB/s
nominal HBM rate they represent, beside igdsp_depayload over the same arrival arrays and the compute-free yardstick, all in one process.

    python tools/jb_bench.py [--reps 20] [--warmup 5] [--out profiles/r08_jb_bench.json] [--only J1,J4]
    python tools/jb_bench.py --adaptive [--only J1,J2,J3] [--out profiles/jb_adapt_bench.json]

Shapes (180-byte ED-137 packets: 20-byte header + 160 G.711 bytes, 180-byte slots, delay_frames 3; packets built on the device):
    J1  C = 65 536, 128 ticks, 1 slot per tick, in order, no loss
    J2  as J1 with 2 slots per tick: 3 % loss, 2 % reordered by one tick, 0.5 % duplicated, arrival jitter of +-80 RTP units
    J3  C = 65 536, 2 ticks, 1 slot per tick, as J1 (the flush tick's shape)
    J4  C = 4, 1 tick, 1 slot per tick, as J1 (the latency floor)
Every timed call continues the same stream of packets (the next call's arrays are built between the timed calls): the state and the
ring carry on, sequence numbers advance by T per call.
Algorithmic bytes per channel-tick: the S sizes and the arrived packets (180 each) read, payload + len + info + tick flag (171) written,
plus the 80-byte state and the 64 bytes of ring tags read and written once per channel and call.  Depayload does the same arrays with
S slots per tick (T x S frames out).  The yardstick (igdsp_internal_jb_copy) writes the rows of an in-order lossless call (slot 0 of
every tick copied as igdsp_depayload would) with no header walk, state machine or ring.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` in a run of its own.
--adaptive times igdsp_jb_receive_adaptive (default cfg, no d_delay_out) beside igdsp_jb_receive instead: the two entries take turns, call
by call, on the same stream of packets, the same state and ring and the same output buffers (the adaptive one with its igdsp_jb_adapt
beside them).  Its bar: the fixed entry's median plus the fixed entry's own max - min spread in that run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libigdsp.so: one HIP runtime per process)

from igate4xsoftphonedsp_amd import capi  # noqa: E402

N, STRIDE, HDR, DELAY, PEAK = 160, 180, 20, 3, 8.0e12
BARS = {"J1": 1.5, "J2": 2.0, "J3": 2.0, "J4": None}


def shape(name):
    """C, T, S"""
    return {"J1": (65536, 128, 1), "J2": (65536, 128, 2), "J3": (65536, 2, 1), "J4": (4, 1, 1)}[name]


class Traffic:
    """the sender side: packet seq0 + t of every channel, and the arrival arrays of one call (T ticks from tick t0)"""

    def __init__(self, C_, T, S, lossy, seed):
        self.C, self.T, self.S, self.lossy = C_, T, S, lossy
        self.g = torch.Generator(device="cuda").manual_seed(seed)
        self.seq0 = torch.randint(0, 65536, (C_,), device="cuda", generator=self.g)
        self.ssrc = torch.randint(0, 1 << 31, (C_,), device="cuda", generator=self.g)
        self.word = (1 << 28) | (torch.randint(0, 32, (C_,), device="cuda", generator=self.g) << 3)

    def sent(self, t0, T):
        """the packets of ticks t0 .. t0 + T - 1: [T][C][180]"""
        C_ = self.C
        pk = torch.randint(0, 256, (T, C_, STRIDE), dtype=torch.uint8, device="cuda", generator=self.g)
        t = torch.arange(t0, t0 + T, device="cuda")[:, None]
        seq = (self.seq0[None, :] + t) % 65536
        ts = (t * N) % (1 << 32) + torch.zeros_like(seq)

        def put(lo, v, nbytes):
            for i in range(nbytes):
                pk[:, :, lo + i] = ((v >> (8 * (nbytes - 1 - i))) & 0xFF).to(torch.uint8)

        pk[:, :, 0], pk[:, :, 1] = 0x90, 8
        put(2, seq, 2)
        put(4, ts, 4)
        put(8, self.ssrc[None, :].expand(T, C_), 4)
        pk[:, :, 12:16] = torch.tensor([0x01, 0x67, 0x00, 0x01], dtype=torch.uint8, device="cuda")
        put(16, self.word[None, :].expand(T, C_), 4)
        return pk, ts

    def arrivals(self, t0):
        """(packets [T*S][C][180], sizes [T*S][C] u16, arrival [T*S][C] u32)"""
        C_, T, S = self.C, self.T, self.S
        pk, ts = self.sent(t0, T + 1)                                      # packet T is the one held back from the previous call
        if not self.lossy:
            return pk[:T].reshape(T * S, C_, STRIDE).contiguous(), None, None
        r = torch.rand((3, T + 1, C_), device="cuda", generator=self.g)
        lost, late, dup = r[0] < 0.03, r[1] < 0.02, r[2] < 0.005
        # slot 0 of tick t: packet t unless lost or reordered; slot 1: packet t - 1 if it was reordered by one, else a duplicate of t
        out = torch.zeros((T, S, C_, STRIDE), dtype=torch.uint8, device="cuda")
        size = torch.zeros((T, S, C_), dtype=torch.int32, device="cuda")
        arr = torch.zeros((T, S, C_), dtype=torch.int64, device="cuda")
        jit = torch.randint(-80, 81, (T + 1, C_), device="cuda", generator=self.g)
        ok0 = ~lost[1:] & ~late[1:]
        out[:, 0] = torch.where(ok0[..., None], pk[1:], out[:, 0])
        size[:, 0] = ok0.int() * STRIDE
        arr[:, 0] = ts[1:] + jit[1:]
        prev = ~lost[:-1] & late[:-1]
        d1 = ok0 & dup[1:]
        out[:, 1] = torch.where(prev[..., None], pk[:-1], torch.where(d1[..., None], pk[1:], out[:, 1]))
        size[:, 1] = (prev | d1).int() * STRIDE
        arr[:, 1] = torch.where(prev, ts[:-1] + N + jit[:-1], ts[1:] + jit[1:] + 7)
        return (out.reshape(T * S, C_, STRIDE).contiguous(), size.reshape(T * S, C_).to(torch.int16).contiguous(),
                (arr.reshape(T * S, C_) % (1 << 32)).to(torch.int64).to(torch.int32).contiguous())


def timed(fn, s, reps, warmup, before=None):
    for _ in range(warmup):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        t.append(a.elapsed_time(b) * 1000.0)
    return float(np.median(t)), float(min(t))


def timed_pair(fns, s, reps, warmup, before):
    """the functions take turns, call by call; returns per function the sorted times in microseconds"""
    ts = [[] for _ in fns]
    for r in range(warmup + reps):
        for i, fn in enumerate(fns):
            before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            b.synchronize()
            if r >= warmup:
                ts[i].append(a.elapsed_time(b) * 1000.0)
    return [sorted(t) for t in ts]


def run_case(ctx, name, reps, warmup, adaptive=False):
    C_, T, S = shape(name)
    tr = Traffic(C_, T, S, name == "J2", seed=C_ + T + S)
    cur = [tr.arrivals(0)]
    radio = torch.ones(C_, dtype=torch.uint8, device="cuda")
    state = torch.zeros(C_ * capi.JB_STATE.itemsize, dtype=torch.uint8, device="cuda")
    ring = torch.zeros(capi.jb_ring_bytes(C_, N), dtype=torch.uint8, device="cuda")
    pay = torch.empty((T * S * C_ * N,), dtype=torch.uint8, device="cuda")   # room for depayload's T x S frames
    ln = torch.empty((T * S * C_,), dtype=torch.int16, device="cuda")
    inf = torch.empty((T * S * C_ * 8,), dtype=torch.uint8, device="cuda")
    fl = torch.empty((T * C_,), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()
    cp = capi.internal("igdsp_internal_jb_copy")
    k = [0]

    def args():
        return cur[0]

    def nxt():                                                             # the next call's arrivals (not timed): the stream goes on
        k[0] += 1
        cur[0] = None
        cur[0] = tr.arrivals(k[0] * T)

    def jb():
        pk, sz, ar = args()
        ctx.jb_receive(pk, radio, state, ring, pay, ln, inf, C_, T, S, STRIDE, N, DELAY, sizes=sz, arrival=ar, tick_flags=fl,
                       stream=s.cuda_stream)

    def copy():
        pk, sz, ar = args()
        rc = cp(ctx.h, pk.data_ptr(), None if sz is None else sz.data_ptr(), radio.data_ptr(), None, C_, T, S, STRIDE, N, DELAY,
                state.data_ptr(), ring.data_ptr(), pay.data_ptr(), ln.data_ptr(), inf.data_ptr(), fl.data_ptr(), None, s.cuda_stream)
        assert rc == 0, rc

    def dep():
        pk, sz, _ = args()
        ctx.depayload(pk, sz, radio, C_, T * S, STRIDE, N, pay, ln, inf, stream=s.cuda_stream)

    if adaptive:
        adapt = torch.zeros(C_ * capi.JB_ADAPT.itemsize, dtype=torch.uint8, device="cuda")

        def jba():
            pk, sz, ar = args()
            ctx.jb_receive_adaptive(pk, radio, state, ring, adapt, pay, ln, inf, C_, T, S, STRIDE, N, None, sizes=sz, arrival=ar, tick_flags=fl,
                                    stream=s.cuda_stream)

        tf, ta = timed_pair([jb, jba], s, reps, warmup, nxt)
        med_f, med_a, spread = float(np.median(tf)), float(np.median(ta)), tf[-1] - tf[0]
        return {"case": name, "C": C_, "T": T, "S": S, "fixed_us": round(med_f, 2), "fixed_min": round(tf[0], 2), "fixed_max": round(tf[-1], 2),
                "adaptive_us": round(med_a, 2), "adaptive_min": round(ta[0], 2), "adaptive_max": round(ta[-1], 2),
                "adaptive_over_fixed": round(med_a / med_f, 4), "bar_us": round(med_f + spread, 2), "bar_met": bool(med_a <= med_f + spread),
                "reps": reps}
    us, us_min = timed(jb, s, reps, warmup, nxt)
    st = state.cpu().numpy().view(capi.JB_STATE)
    played = float(st["played"].sum()) / max(1.0, float(st["played"].sum() + st["lost"].sum()))
    dus, _ = timed(dep, s, reps, warmup)
    cus, _ = timed(copy, s, reps, warmup)
    arrived = float(C_ * T * S) if cur[0][1] is None else float((cur[0][1] != 0).sum().item())
    alg = int(C_ * T * S * 2 + arrived * STRIDE + C_ * T * (N + 2 + 8 + 1) + 2 * C_ * (80 + 64))
    bar = BARS[name]
    return {"case": name, "C": C_, "T": T, "S": S, "played_frac": round(played, 4), "us_per_call": round(us, 2), "us_min": round(us_min, 2),
            "alg_bytes": alg, "frac_8TBps": round(alg / (us * 1e-6) / PEAK, 4), "depayload_us": round(dus, 2), "copy_us": round(cus, 2),
            "copy_frac_8TBps": round(alg / (cus * 1e-6) / PEAK, 4), "jb_over_depayload": round(us / dus, 3), "jb_over_copy": round(us / cus, 3),
            "bar": bar, "bar_met": None if bar is None else bool(us <= bar * dus), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--adaptive", action="store_true", help="igdsp_jb_receive_adaptive beside igdsp_jb_receive (J1, J2, J3)")
    a = ap.parse_args()
    a.only = a.only or ("J1,J2,J3" if a.adaptive else "J1,J2,J3,J4")
    torch.cuda.set_device(0)
    rows = []
    with capi.Context(device=0, max_channels=64) as ctx:
        for name in a.only.split(","):
            r = run_case(ctx, name, a.reps, a.warmup, a.adaptive)
            print(json.dumps(r), flush=True)
            rows.append(r)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
