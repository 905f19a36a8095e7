"""igdsp_srtp_gcm_protect / igdsp_srtp_gcm_unprotect timing: microseconds per launch (device events on the launch stream; median, min and
max of at least 20 launches after warm-up), for both key sizes, beside, in the same process and on the same buffers, the compute-free
yardstick igdsp_internal_srtp_gcm_move, igdsp_srtp_protect / igdsp_srtp_unprotect (the SHA-1 suite, 80-bit tags) on the same packets
five times over (the spread of its five medians is the noise band of the GCM / HMAC ratio), the headline meter (igdsp_decode_meter,
records only, on uniform random codes) before and after, and a floor computed from the kernel's own count of vector instructions per
AES block and per GHASH multiply at the clock the run reports.

    python tools/srtp_gcm_bench.py [--reps 20] [--warmup 3] [--out profiles/srtp_gcm_bench.json] [--only S1,S2,...] [--keys 16,32]

Shapes: tools/srtp_bench.py's S1 to S5 (C = 65 536 legs; the packets, sizes, states and outputs come from one igdsp_io_alloc call), in
208-byte slots: a 180-byte ED-137 packet and its 16 tag bytes do not fit the 192-byte slot of the SRTP bench.
    S1  protect, 128 frames of 180-byte ED-137 packets (20-byte header, 160 samples)
    S2  unprotect of S1's output (196 bytes in the same slots); the states start fresh every launch through d_ctl = RESET on frame 0
    S3  S1 and S2 at one frame (a live gateway's per-tick call)
    S4  protect of 172-byte plain RTP (12-byte header)
    S5  S1 with 90 % of the legs sending 20-byte keep-alives
The floor: a packet of `end` bytes under the tag with an h-byte header takes ceil((end - h) / 16) + 1 AES blocks (the payload's and
J0's) and ceil(h / 16) + ceil((end - h) / 16) + 1 GHASH multiplies (AAD, ciphertext, lengths).  An AES-256 block is VALU_PER_AES vector
instructions from label to label; a wave whose legs all hold 128-bit keys branches over rounds 10..13 and their selects inside it,
VALU_AES_ROUNDS_10_13 of them.  A multiply is four trips of a loop of VALU_PER_GHASH_WORD.  All three were counted in the saved ISA
of k_srtp_gcm<0, false>; tests/test_srtp_gcm_resources_cpu.py recounts VALU_PER_AES and VALU_PER_GHASH_WORD from the .s file with
tools/kernel_resources.py and fails when one is stale (the run inside a block that a branch skips has no label of its own, so
VALU_AES_ROUNDS_10_13 is held only by being four of the fourteen rounds, the last of which is the cheapest, and four selects: above
3 / 14 of the block and below 4 / 13).
A wave is 64 legs, and a SIMD issues one vector instruction of one wave every 4 cycles however many waves it
holds: floor = waves per SIMD x frames x (AES blocks x VALU_PER_AES + multiplies x 4 x VALU_PER_GHASH_WORD) x 4 / clock.  It counts
those blocks alone (no header parse, index, alignment of keystream and GHASH blocks, tile traffic) and no LDS time, though an AES block
is 224 table reads and a multiply 160 LDS words.  Unprotect runs the same blocks.  The aim is 1.5 x the larger of the yardstick and
that floor.  Only the lane-per-leg shape with Te0, the round keys and Shoup's 4-bit tables in LDS exists and was timed; the bit-serial
multiply was counted in the saved ISA and not timed."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libigdsp.so: one HIP runtime per process)

from igate4xsoftphonedsp_amd import capi  # noqa: E402

C_ALL, STRIDE, N, TAG = 65536, 208, 160, 16
VALU_PER_AES = 635         # tests/test_srtp_gcm_resources_cpu.py counts the saved ISA's AES and GHASH blocks against these
VALU_AES_ROUNDS_10_13 = 192
VALU_PER_GHASH_WORD = 112
ISSUE_CYCLES = 4.0
KEY = bytes(range(1, 45))
#        frames, direction, header bytes, share of keep-alive legs
SHAPES = {"S1": (128, "protect", 20, 0.0), "S2": (128, "unprotect", 20, 0.0), "S3": (1, "both", 20, 0.0), "S4": (128, "protect", 12, 0.0),
          "S5": (128, "protect", 20, 0.9)}


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
    """(MHz, where it came from): the shader clock while `busy` keeps the device loaded, as the run can read it"""
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


def blocks_of(end, h):
    """(AES blocks, GHASH multiplies) of one packet"""
    ct = -(-(end - h) // 16)
    return ct + 1, -(-h // 16) + ct + 1


def run_case(ctx, name, keys, reps, warmup, C_, clock_fallback):
    F_, direction, hdr, ka_share = SHAPES[name]
    s = torch.cuda.current_stream()
    L = capi.load()
    fc = F_ * C_
    sb, gb = capi.SRTP_STATE.itemsize, capi.SRTP_GCM_STATE.itemsize
    spec = [(fc * N, capi.IO_INPUT), (fc * STRIDE, capi.IO_INPUT), (fc * 2, capi.IO_INPUT), (C_ * gb, capi.IO_RECORD), (fc * STRIDE, capi.IO_RECORD),
            (fc * 2, capi.IO_RECORD), (fc * 8, capi.IO_RECORD), (fc * STRIDE, capi.IO_RECORD), (fc * 2, capi.IO_RECORD), (C_ * gb, capi.IO_RECORD), (fc * 16, capi.IO_RECORD),
            (C_ * sb, capi.IO_RECORD), (C_ * sb, capi.IO_RECORD)]
    ioset, (p_codes, p_pk, p_sz, p_st, p_out, p_szo, p_rec, p_out2, p_szo2, p_st2, p_stats, p_hst, p_hst2), rep = ctx.io_alloc(spec)
    ctx.gen_uniform(p_codes, fc * N, seed=1, stream=s.cuda_stream)
    torch.cuda.synchronize()

    # ---- the clear packets: the library's own header layout around random codes, written on the host (what igdsp_tx_packetize emits
    # for a leg that sends every frame)
    rng = np.random.default_rng(5)
    sizes = np.full((F_, C_), hdr + N, np.uint16)
    quiet = rng.random(C_) < ka_share
    sizes[:, quiet] = 20
    pk = np.zeros((F_, C_, STRIDE), np.uint8)
    pk[:, :, 0] = 0x80 | (0x10 if hdr == 20 else 0)
    pk[:, :, 1] = 8
    seq = np.arange(F_, dtype=np.uint32)[:, None] + np.zeros((1, C_), np.uint32)
    pk[:, :, 2], pk[:, :, 3] = seq >> 8, seq & 255
    ssrc = (np.arange(C_, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    for k in range(4):
        pk[:, :, 8 + k] = (ssrc >> (24 - 8 * k)) & 255
    if hdr == 20:
        pk[:, :, 12:16] = np.array([0x01, 0x67, 0x00, 0x01], np.uint8)
    pk[:, quiet, 1] = 123
    pk[:, :, hdr:hdr + N] = rng.integers(0, 256, (1, C_, N), dtype=np.uint8)
    assert L.igdsp_copy_h2d(ctx.h, p_pk, pk.ctypes.data, pk.nbytes) == 0 and L.igdsp_copy_h2d(ctx.h, p_sz, sizes.ctypes.data, sizes.nbytes) == 0
    ctl = np.zeros((F_, C_), np.uint8)
    ctl[0] = capi.SRTP_RESET                                                # every timed launch starts the same stream over
    d_ctl = torch.from_numpy(ctl).cuda()
    mv = capi.internal("igdsp_internal_srtp_gcm_move")
    codec = torch.zeros(C_, dtype=torch.uint8, device="cuda")

    def meter():
        ctx.decode_meter(p_codes, codec, C_, F_, N, p_stats, stream=s.cuda_stream)

    def check(want_sizes):
        torch.cuda.synchronize()
        rec = np.zeros(fc, capi.SRTP_REC)
        assert L.igdsp_copy_d2h(ctx.h, rec.ctypes.data, p_rec, fc * 8) == 0
        assert ((rec["flags"] & capi.SRTP_OK) != 0).all() and (rec["size_out"] == want_sizes.reshape(-1)).all()

    def came_back():
        back = np.zeros((C_, STRIDE), np.uint8)                             # frame 0 comes back as it went in
        assert L.igdsp_copy_d2h(ctx.h, back.ctypes.data, p_out2, back.nbytes) == 0
        assert (back[:, :hdr + N] == pk[0, :, :hdr + N])[~quiet].all() and (back[quiet, :20] == pk[0, quiet, :20]).all()

    t_head0 = timed(meter, s, reps, warmup)

    # ---- the SHA-1 suite on the same packets and buffers, five times: its medians' spread is the noise band of the ratio
    h0 = np.repeat(capi.srtp_derive(KEY[:30], 10)[None], C_)
    assert L.igdsp_copy_h2d(ctx.h, p_hst, h0.ctypes.data, h0.nbytes) == 0 and L.igdsp_copy_h2d(ctx.h, p_hst2, h0.ctypes.data, h0.nbytes) == 0

    def hmac_protect():
        ctx.srtp_protect(p_hst, p_pk, p_sz, C_, F_, STRIDE, p_out, STRIDE, p_szo, rec=p_rec, ctl=d_ctl, stream=s.cuda_stream)

    def hmac_unprotect():
        ctx.srtp_unprotect(p_hst2, p_out, p_szo, C_, F_, STRIDE, p_out2, STRIDE, p_szo2, rec=p_rec, ctl=d_ctl, stream=s.cuda_stream)

    hmac = {"protect": [], "unprotect": []}
    for _ in range(5):
        hmac["protect"].append(timed(hmac_protect, s, reps, warmup)["median"])
        if direction in ("unprotect", "both"):
            hmac["unprotect"].append(timed(hmac_unprotect, s, reps, warmup)["median"])
    check(sizes) if direction in ("unprotect", "both") else check(sizes + 10)

    rows = []
    for kb in keys:
        st0 = np.repeat(capi.srtp_gcm_derive(KEY[:kb + 12])[None], C_)
        assert L.igdsp_copy_h2d(ctx.h, p_st, st0.ctypes.data, st0.nbytes) == 0 and L.igdsp_copy_h2d(ctx.h, p_st2, st0.ctypes.data, st0.nbytes) == 0

        def protect():
            ctx.srtp_gcm_protect(p_st, p_pk, p_sz, C_, F_, STRIDE, p_out, STRIDE, p_szo, rec=p_rec, ctl=d_ctl, stream=s.cuda_stream)

        def unprotect():
            ctx.srtp_gcm_unprotect(p_st2, p_out, p_szo, C_, F_, STRIDE, p_out2, STRIDE, p_szo2, rec=p_rec, ctl=d_ctl, stream=s.cuda_stream)

        def move():
            rc = mv(ctx.h, None, p_pk, p_sz, C_, F_, STRIDE, p_st, p_out2, STRIDE, p_szo2, p_rec, s.cuda_stream)
            assert rc == 0, rc

        out = {"case": name, "key_bytes": kb, "C": C_, "F": F_, "slot": STRIDE, "header": hdr, "keepalive_share": ka_share, "tag_len": TAG}
        t_prot = timed(protect, s, reps, warmup)
        check(sizes + TAG)
        clock = device_clock_mhz(clock_fallback, protect)
        torch.cuda.synchronize()
        if direction in ("protect", "both"):
            out["protect_us"] = t_prot
        if direction in ("unprotect", "both"):
            out["unprotect_us"] = timed(unprotect, s, reps, warmup)
            check(sizes)
            came_back()
        t_move = timed(move, s, reps, warmup)
        cus, clock_hz = torch.cuda.get_device_properties(0).multi_processor_count, clock[0] * 1e6
        waves_per_simd = max(1.0, (C_ / 64.0) / (4.0 * cus))                # 64 legs a wave, one after another or side by side: the issue rate is the SIMD's
        aes_v, mul_v = blocks_of(hdr + N, hdr)                              # a wave walks its longest packet: the voice packet where one leg sends one
        if ka_share >= 1.0:
            aes_v, mul_v = blocks_of(20, 20)
        per_aes = VALU_PER_AES - (VALU_AES_ROUNDS_10_13 if kb == 16 else 0)
        floor_us = waves_per_simd * F_ * (aes_v * per_aes + mul_v * 4 * VALU_PER_GHASH_WORD) * ISSUE_CYCLES / clock_hz * 1e6
        aim = 1.5 * max(floor_us, t_move["median"])
        out.update({"move_us": t_move, "valu_floor_us": round(floor_us, 2), "valu_per_aes_block": per_aes, "valu_per_ghash_multiply": 4 * VALU_PER_GHASH_WORD,
                    "aes_blocks": aes_v, "ghash_multiplies": mul_v, "clock_mhz": round(clock[0]), "clock_from": clock[1], "compute_units": cus, "aim_us": round(aim, 2)})
        for key in ("protect_us", "unprotect_us"):
            if key in out:
                t, side = out[key]["median"], key[:-3]
                out[side + "_over_aim"] = round(t / aim, 3)
                out[side + "_aim"] = "met" if t <= aim else "missed"
                out[side + "_ns_per_packet"] = round(t * 1e3 / fc, 3)
                out["hmac_sha1_" + side + "_us_five_medians"] = hmac[side]
                out["gcm_over_hmac_" + side] = round(t / float(np.median(hmac[side])), 3)
                out["hmac_noise_band_" + side] = round((max(hmac[side]) - min(hmac[side])) / float(np.median(hmac[side])), 4)
        rows.append(out)
    t_head1 = timed(meter, s, reps, warmup)
    for out in rows:
        out.update({"headline_meter_before_us": t_head0, "headline_meter_after_us": t_head1,
                    "shape": "a lane a leg, 64 legs a wave, pieces of 64 bytes through an LDS tile; Te0, the round keys and Shoup's 4-bit tables of H in LDS (the only one timed)",
                    "bulk_spread": rep.get("bulk_spread"), "reps": reps})
    ioset.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=",".join(SHAPES))
    ap.add_argument("--keys", default="16,32")
    ap.add_argument("--channels", type=int, default=C_ALL)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="used only when the run cannot read the device's clock")
    a = ap.parse_args()
    assert a.reps >= 1
    assert not a.out or a.reps >= 20, "a result file holds medians of at least 20 launches: --out needs --reps >= 20"
    torch.cuda.set_device(0)
    rows = []
    with capi.Context(device=0, max_channels=64) as ctx:
        for name in a.only.split(","):
            for r in run_case(ctx, name, [int(k) for k in a.keys.split(",")], a.reps, a.warmup, a.channels, a.clock_mhz):
                print(json.dumps(r), flush=True)
                rows.append(r)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
