"""igdsp_rtcp_build / igdsp_rtcp_parse / igdsp_srtcp_protect / igdsp_srtcp_unprotect timing: microseconds per launch (device events on
the launch stream; median, min and max of at least 20 launches after warm-up), in one process and on buffers of one igdsp_io_alloc
call per shape.

    python tools/rtcp_bench.py [--reps 20] [--warmup 3] [--out profiles/rtcp_bench.json] [--only R1,R16]

Shapes: C = 65 536 legs x 1 tick (R1: the real shape, one report per leg per interval) and x 16 ticks (R16), 152-byte slots.  Every
tick every leg sends an SR with one report block and an SDES with a 16-byte CNAME: 28 + 24 + 4 + 24 = 80 bytes.
    build, parse    beside their compute-free yardsticks igdsp_internal_rtcp_build_move / igdsp_internal_rtcp_parse_move (the same
                    loads, tile traffic and stores, no plan and no walk); the aim is 1.5 x the yardstick.
    SRTCP           protect of build's packets and unprotect of that (94 bytes), beside igdsp_srtp_protect / igdsp_srtp_unprotect at
                    the same legs, ticks and slots on 88-byte RTP packets (12-byte header): both take 5 AES blocks and 2 SHA-1
                    compressions a packet.  SRTCP should not be slower per packet: the margin is the spread (largest minus smallest
                    median) of five runs of the SRTP entry in this process, which is recorded.  The yardstick igdsp_internal_srtcp_move
                    stands beside them.
The states start over every launch through d_ctl = RESET on tick 0 (SRTP, SRTCP); build's and parse's state moves on, which changes
no packet's form (two source arrays alternate between launches, so the sender's packet count has always moved: an SR).  Parse and
protect read a copy of the built packets that igdsp_io_alloc placed as an input, as SRTP's packets are.  The headline meter
(igdsp_decode_meter, records only, uniform random codes, 128 frames) is timed after everything."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libigdsp.so: one HIP runtime per process)

from igate4xsoftphonedsp_amd import capi  # noqa: E402

C_ALL, STRIDE, CNAME_LEN, RTP_BYTES = 65536, 152, 16, 88
KEY = bytes(range(1, 31))
SHAPES = {"R1": 1, "R16": 16}


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


def run_case(ctx, name, reps, warmup, C_):
    F_ = SHAPES[name]
    s = torch.cuda.current_stream()
    L = capi.load()
    fc, sb = F_ * C_, capi.SRTP_STATE.itemsize
    spec = [(fc * STRIDE, capi.IO_RECORD), (fc * 2, capi.IO_RECORD), (fc * 8, capi.IO_RECORD), (C_ * 80, capi.IO_RECORD),      # built packets, sizes, records, state
            (fc * 32, capi.IO_RECORD), (C_ * 80, capi.IO_RECORD),                                                              # parse records, state
            (fc * STRIDE, capi.IO_RECORD), (fc * 2, capi.IO_RECORD), (fc * 8, capi.IO_RECORD), (C_ * sb, capi.IO_RECORD),      # protected
            (fc * STRIDE, capi.IO_RECORD), (fc * 2, capi.IO_RECORD), (C_ * sb, capi.IO_RECORD),                               # unprotected
            (fc * STRIDE, capi.IO_INPUT), (fc * 2, capi.IO_INPUT), (C_ * sb, capi.IO_RECORD), (C_ * sb, capi.IO_RECORD),      # RTP packets, sizes, two SRTP states
            (fc * STRIDE, capi.IO_INPUT), (fc * 2, capi.IO_INPUT)]                                                            # the built packets as an input of their own
    ioset, (p_pk, p_sz, p_brec, p_bst, p_prec, p_pst, p_pr, p_prsz, p_srec, p_tx, p_cl, p_clsz, p_rx, p_rtp, p_rtpsz, p_stx, p_srx, p_in, p_insz), rep = ctx.io_alloc(spec)

    def up(ptr, a):
        a = np.ascontiguousarray(a)
        assert L.igdsp_copy_h2d(ctx.h, ptr, a.ctypes.data, a.nbytes) == 0

    def down(ptr, dtype, n):
        a = np.zeros(n, dtype)
        assert L.igdsp_copy_d2h(ctx.h, a.ctypes.data, ptr, a.nbytes) == 0
        return a

    rng = np.random.default_rng(5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    jb = np.zeros(C_, capi.JB_STATE)
    jb["ssrc"], jb["base_seq"], jb["max_seq"], jb["received"], jb["jitter"], jb["flags"] = 0xB0000000 + np.arange(C_), 100, 1100, 990, 4000, 1
    src = np.zeros((F_, C_), capi.RTCP_SRC)
    src["ssrc"], src["packets"], src["rtp_ts"] = 0xA0000000 + np.arange(C_)[None], 50 * (1 + np.arange(F_))[:, None], 8000
    src["octets"] = src["packets"] * 160
    now = ((0x83AA7E80 + 5 * np.arange(F_, dtype=np.uint64)) << np.uint64(32)) | np.uint64(0x12345678)
    src2 = src.copy()
    src2["packets"] += 7                                                    # the launches alternate: a leg's packet count differs from the last one it reported
    d_ctl, d_jb, d_src, d_now = dev(np.full((F_, C_), capi.RTCP_REPORT, np.uint8)), dev(jb), [dev(src), dev(src2)], dev(now.astype("<u8"))
    turn = [0]
    d_cname, d_clen = dev(rng.integers(1, 256, (C_, 64), dtype=np.uint8)), dev(np.full(C_, CNAME_LEN, np.uint8))
    d_arrival, d_local = dev(np.full((F_, C_), 0x7E900000, "<u4")), dev(jb["ssrc"].astype("<u4"))
    up(p_bst, np.zeros(C_, capi.RTCP_STATE))
    up(p_pst, np.zeros(C_, capi.RTCP_STATE))
    st0 = np.repeat(capi.srtcp_derive(KEY)[None], C_)
    up(p_tx, st0)
    up(p_rx, st0)
    rst = np.zeros((F_, C_), np.uint8)
    rst[0] = capi.SRTP_RESET                                                # every timed launch starts the same stream over
    d_rst = dev(rst)
    rtp = np.zeros((F_, C_, STRIDE), np.uint8)
    rtp[:, :, 0], rtp[:, :, 1] = 0x80, 8
    seq = np.arange(F_, dtype=np.uint32)[:, None] + np.zeros((1, C_), np.uint32)
    rtp[:, :, 2], rtp[:, :, 3] = seq >> 8, seq & 255
    rtp[:, :, 8:12] = (0xA0000000 + np.arange(C_, dtype=np.uint32)).astype(">u4").view(np.uint8).reshape(1, C_, 4)
    rtp[:, :, 12:RTP_BYTES] = rng.integers(0, 256, (1, C_, RTP_BYTES - 12), dtype=np.uint8)
    up(p_rtp, rtp)
    up(p_rtpsz, np.full((F_, C_), RTP_BYTES, "<u2"))
    sst = np.repeat(capi.srtp_derive(KEY, 10)[None], C_)
    up(p_stx, sst)
    up(p_srx, sst)
    bm, pm, sm = (capi.internal(n) for n in ("igdsp_internal_rtcp_build_move", "igdsp_internal_rtcp_parse_move", "igdsp_internal_srtcp_move"))
    q = lambda t: t.data_ptr()

    def build():
        turn[0] ^= 1
        ctx.rtcp_build(d_ctl, d_src[turn[0]], d_now, C_, F_, p_bst, p_pk, STRIDE, p_sz, jb=d_jb, cname=d_cname, cname_len=d_clen, rec=p_brec, stream=s.cuda_stream)

    def build_move():
        assert bm(ctx.h, q(d_ctl), q(d_jb), q(d_src[0]), q(d_now), q(d_cname), q(d_clen), C_, F_, p_bst, p_cl, STRIDE, p_clsz, p_brec, s.cuda_stream) == 0

    def parse():
        ctx.rtcp_parse(p_in, p_insz, d_arrival, d_local, C_, F_, STRIDE, p_pst, rec=p_prec, stream=s.cuda_stream)

    def parse_move():
        assert pm(ctx.h, p_in, p_insz, q(d_arrival), q(d_local), C_, F_, STRIDE, p_pst, p_prec, s.cuda_stream) == 0

    def protect():
        ctx.srtcp_protect(p_tx, p_in, p_insz, C_, F_, STRIDE, p_pr, STRIDE, p_prsz, rec=p_srec, ctl=d_rst, stream=s.cuda_stream)

    def unprotect():
        ctx.srtcp_unprotect(p_rx, p_pr, p_prsz, C_, F_, STRIDE, p_cl, STRIDE, p_clsz, rec=p_srec, ctl=d_rst, stream=s.cuda_stream)

    def srtcp_move():
        assert sm(ctx.h, None, p_in, p_insz, C_, F_, STRIDE, p_tx, p_cl, STRIDE, p_clsz, p_srec, s.cuda_stream) == 0

    def srtp_protect():
        ctx.srtp_protect(p_stx, p_rtp, p_rtpsz, C_, F_, STRIDE, p_pr, STRIDE, p_prsz, rec=p_srec, ctl=d_rst, stream=s.cuda_stream)

    def srtp_unprotect():
        ctx.srtp_unprotect(p_srx, p_pr, p_prsz, C_, F_, STRIDE, p_cl, STRIDE, p_clsz, rec=p_srec, ctl=d_rst, stream=s.cuda_stream)

    out = {"case": name, "C": C_, "F": F_, "slot": STRIDE, "cname_len": CNAME_LEN, "rtp_bytes": RTP_BYTES, "reps": reps}
    out["build_us"] = timed(build, s, reps, warmup)
    torch.cuda.synchronize()
    sizes, brec = down(p_sz, "<u2", fc), down(p_brec, capi.RTCP_BUILT, fc)
    assert (sizes == 80).all() and (brec["flags"] == capi.RTCP_SR | capi.RTCP_HAS_BLOCK).all()
    out["rtcp_bytes"] = int(sizes[0])
    up(p_in, down(p_pk, np.uint8, fc * STRIDE))                             # parse and protect read them from input-class memory, as SRTP reads its packets
    up(p_insz, sizes)
    out["parse_us"] = timed(parse, s, reps, warmup)
    torch.cuda.synchronize()
    assert (down(p_prec, capi.RTCP_SEEN, fc)["flags"] == capi.RTCP_PARSED | capi.RTCP_GOT_SR | capi.RTCP_GOT_BLOCK).all()
    out["parse_move_us"] = timed(parse_move, s, reps, warmup)
    out["srtcp_protect_us"] = timed(protect, s, reps, warmup)
    torch.cuda.synchronize()
    assert (down(p_srec, capi.SRTP_REC, fc)["flags"] == capi.SRTP_OK).all() and (down(p_prsz, "<u2", fc) == 94).all()
    out["srtcp_unprotect_us"] = timed(unprotect, s, reps, warmup)
    torch.cuda.synchronize()
    assert (down(p_srec, capi.SRTP_REC, fc)["flags"] == capi.SRTP_OK).all()
    assert down(p_cl, np.uint8, C_ * STRIDE).reshape(C_, STRIDE)[:, :80].tobytes() == down(p_pk, np.uint8, C_ * STRIDE).reshape(C_, STRIDE)[:, :80].tobytes()
    out["srtcp_move_us"] = timed(srtcp_move, s, reps, warmup)
    out["build_move_us"] = timed(build_move, s, reps, warmup)              # (writes the clear buffers: after unprotect's check)
    runs_p = [timed(srtp_protect, s, reps, warmup) for _ in range(5)]
    torch.cuda.synchronize()
    assert ((down(p_srec, capi.SRTP_REC, fc)["flags"] & capi.SRTP_OK) != 0).all()
    runs_u = [timed(srtp_unprotect, s, reps, warmup) for _ in range(5)]
    torch.cuda.synchronize()
    assert ((down(p_srec, capi.SRTP_REC, fc)["flags"] & capi.SRTP_OK) != 0).all()
    for key, runs, mine in (("protect", runs_p, out["srtcp_protect_us"]), ("unprotect", runs_u, out["srtcp_unprotect_us"])):
        med = [r["median"] for r in runs]
        ref, spread = float(np.median(med)), round(max(med) - min(med), 2)
        out[f"srtp_{key}_us_five_runs"] = med
        out[f"srtp_{key}_spread_us"] = spread
        out[f"srtcp_{key}_over_srtp"] = round(mine["median"] / ref, 3)
        out[f"srtcp_{key}_not_slower"] = "met" if mine["median"] <= ref + spread else "missed"
        out[f"srtcp_{key}_ns_per_packet"] = round(mine["median"] * 1e3 / fc, 3)
    for key in ("build", "parse"):
        aim = 1.5 * out[f"{key}_move_us"]["median"]
        out[f"{key}_aim_us"] = round(aim, 2)
        out[f"{key}_over_aim"] = round(out[f"{key}_us"]["median"] / aim, 3)
        out[f"{key}_aim"] = "met" if out[f"{key}_us"]["median"] <= aim else "missed"
        out[f"{key}_ns_per_packet"] = round(out[f"{key}_us"]["median"] * 1e3 / fc, 3)
    out["bulk_spread"] = rep.get("bulk_spread")
    ioset.close()
    return out


def headline_meter(ctx, reps, warmup, C_):
    s = torch.cuda.current_stream()
    F_, N = 128, 160
    ioset, (p_codes, p_stats), _ = ctx.io_alloc([(F_ * C_ * N, capi.IO_INPUT), (F_ * C_ * 16, capi.IO_RECORD)])
    ctx.gen_uniform(p_codes, F_ * C_ * N, seed=1, stream=s.cuda_stream)
    codec = torch.zeros(C_, dtype=torch.uint8, device="cuda")
    t = timed(lambda: ctx.decode_meter(p_codes, codec, C_, F_, N, p_stats, stream=s.cuda_stream), s, reps, warmup)
    ioset.close()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=",".join(SHAPES))
    ap.add_argument("--channels", type=int, default=C_ALL)
    a = ap.parse_args()
    assert a.reps >= 1
    assert not a.out or a.reps >= 20, "a result file holds medians of at least 20 launches: --out needs --reps >= 20"
    torch.cuda.set_device(0)
    rows = []
    with capi.Context(device=0, max_channels=64) as ctx:
        for name in a.only.split(","):
            r = run_case(ctx, name, a.reps, a.warmup, a.channels)
            print(json.dumps(r), flush=True)
            rows.append(r)
            torch.cuda.empty_cache()
        meter = headline_meter(ctx, a.reps, a.warmup, a.channels)
        print(json.dumps({"headline_meter_after_us": meter}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows, "headline_meter_after_us": meter}, fh, indent=1)


if __name__ == "__main__":
    main()
