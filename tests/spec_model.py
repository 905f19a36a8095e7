"""The spectrum rule (include/igdsp.h, "Spectrum") restated in numpy, in two precisions, and the comparison rule the CPU and the GPU
tests share.  Nothing of the rule comes from the library: the window is built here, the transform is numpy's (one input, the ring
tone, is made by the library's tone generator).

    float64   the reference: the formulas evaluated in double
    float32   the same steps in single, with numpy's own float32 FFT (numpy >= 2: the result dtype is asserted): what a correct
              single-precision implementation deviates from the reference by

Comparison rule.  At each hop M = {k : P64[k] >= 1e-6 * sum(P64)}: the bins within 60 dB of the frame's total.  On M, for raw, for the
averaged array (M intersected over the sequence's hops) and for peak_db, two bounds hold:
  (a) |delta| <= 0.05 dB: the worst-case FFT bound ||err||_2 <= log2(N) * eta * ||X||_2 with eta ~ 6.7 * 2^-24 puts 0.049 dB at the mask's
      edge; the average is a convex combination and adds only rounding.
  (b) |delta| <= 32 * E32, E32 the largest deviation of the float32 model from the float64 model on the sequence's masked bins, computed at
      run time (raw and peak_db: over the raw arrays of all hops; the averaged array: over the averaged arrays after every hop) and never
      taken below half a float32 ulp of the largest value compared (half_ulp32): the margin covers another radix and FMA order than
      pocketfft's and a 2-ulp log10f.
Bins outside M may not exceed the float64 value by more than 3 dB where that value is above -120 dBFS (tone inputs)."""
import numpy as np

from tests import rs_model

N, BINS, FLOOR_DB = 1024, 512, -70.0
HOP = 1                                 # record flag
POW_FLOOR = 1e-20
BOUND_A, MARGIN_B, MASK_REL = 0.05, 32.0, 1e-6


def window(dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).astype(dtype)


def decode(payload, codec):
    """[F][C][n] G.711 codes -> int16, the law from codec[c] (8 A-law, anything else mu-law)"""
    return rs_model.decode(payload, codec).astype(np.int16)


def transform(x, mode):
    """x: int16 [1024], oldest first -> (raw [512] in dBFS, P [512]) in the mode's precision"""
    if mode == "f64":
        X = np.fft.rfft(x.astype(np.float64) * window())[:BINS]
        P = (X.real ** 2 + X.imag ** 2) * 2.0 ** -46
        return 10.0 * np.log10(P + POW_FLOOR), P
    X = np.fft.rfft(x.astype(np.float32) * window(np.float32))[:BINS]
    assert X.dtype == np.complex64, "numpy's float32 FFT is needed (numpy >= 2)"
    P = (X.real * X.real + X.imag * X.imag) * np.float32(2.0 ** -46)
    raw = np.float32(10.0) * np.log10(P + np.float32(POW_FLOOR))
    assert raw.dtype == np.float32
    return raw, P


def new_state():
    return dict(hist=np.zeros(N, np.int16), avg=None, since=0, hops=0)


def run(rows, hop=1, alpha=0.25, mode="f64", state=None):
    """rows: int16 [F][n] of one channel.  Returns dict(flags [F], peak_bin [F], peak_db [F], hop_frames: the frames that hopped,
    raw [H][512], P [H][512], avg [H][512] (the averaged array after each hop), avg_final [512], state)."""
    ft = np.float64 if mode == "f64" else np.float32
    st = new_state() if state is None else state
    F_ = len(rows)
    avg = np.full(BINS, FLOOR_DB, ft) if st["avg"] is None else np.asarray(st["avg"], ft).copy()
    since = min(st["since"], hop - 1)
    flags, peak_bin, peak_db = np.zeros(F_, np.uint16), np.zeros(F_, np.uint16), np.zeros(F_, ft)
    hops, raws, Ps, avgs = [], [], [], []
    a = ft(alpha)
    for f in range(F_):
        n = len(rows[f])
        st["hist"] = np.concatenate([st["hist"][n:], np.asarray(rows[f], np.int16)])
        since += 1
        if since == hop:
            since = 0
            raw, P = transform(st["hist"], mode)
            avg = avg + a * (raw - avg)
            assert avg.dtype == ft
            st["hops"] += 1
            flags[f], peak_bin[f], peak_db[f] = HOP, int(np.argmax(raw)), raw.max()       # argmax: the lowest bin on a tie
            hops.append(f)
            raws.append(raw)
            Ps.append(P)
            avgs.append(avg.copy())
    st["since"], st["avg"] = since, avg
    z = np.zeros((0, BINS), ft)
    return dict(flags=flags, peak_bin=peak_bin, peak_db=peak_db, hop_frames=np.array(hops, np.int64), raw=np.array(raws, ft) if raws else z,
                P=np.array(Ps, ft) if Ps else z, avg=np.array(avgs, ft) if avgs else z, avg_final=avg, state=st)


def half_ulp32(v):
    """half a float32 ulp of the largest magnitude in v: what rounding a float64 value to float32 can move it by.  E32 is at least this:
    the float32 model's deviation is a sample of the format's rounding and comes out as 0 only by coincidence (silence: numpy's log10f of
    1e-20f is exactly -20, so the model's -200 is exact, while a 1-ulp log10f gives -200.00002)."""
    return float(np.spacing(np.float32(np.abs(v).max()))) / 2.0


def reference(rows, hop=1, alpha=0.25, state64=None, state32=None):
    """both models over one channel's rows, the masks, and E32"""
    r64, r32 = run(rows, hop, alpha, "f64", state64), run(rows, hop, alpha, "f32", state32)
    M = r64["P"] >= MASK_REL * r64["P"].sum(axis=1, keepdims=True)                      # [H][512]
    e32 = max(float(np.abs(r32["raw"].astype(np.float64) - r64["raw"])[M].max()), half_ulp32(r64["raw"][M])) if M.any() else 0.0
    Mall = M.all(axis=0) if len(M) else np.zeros(BINS, bool)
    e32_avg = max(float(np.abs(r32["avg"].astype(np.float64) - r64["avg"])[:, Mall].max()), half_ulp32(r64["avg"][:, Mall])) if Mall.any() else 0.0
    return dict(r64=r64, r32=r32, M=M, e32=e32, e32_avg=e32_avg)


def check(ref, got_raw, got_avg_final, got_rec, what=""):
    """The comparison rule.  ref: reference(); got_raw: {hop index h: raw [512]} for the hops whose raw array is known (any subset);
    got_avg_final [512] or None; got_rec: dict(flags, peak_bin, peak_db) per frame or None.  Returns the figures: the largest deviations
    seen (raw, avg, peak) and the two bounds."""
    r64, M, e32 = ref["r64"], ref["M"], ref["e32"]
    bound = min(BOUND_A, MARGIN_B * e32)
    fig = dict(e32=e32, bound_b=MARGIN_B * e32, bound=bound, raw=0.0, avg=0.0, peak=0.0)
    for h, raw in got_raw.items():
        d = np.abs(np.asarray(raw, np.float64) - r64["raw"][h])
        fig["raw"] = max(fig["raw"], float(d[M[h]].max()))
        over = ~M[h] & (r64["raw"][h] > -120.0)
        assert np.all(np.asarray(raw, np.float64)[over] <= r64["raw"][h][over] + 3.0), f"{what}: a bin outside the mask is more than 3 dB above the reference (hop {h})"
    if got_avg_final is not None and len(M):
        Mall = M.all(axis=0)
        fig["avg"] = float(np.abs(np.asarray(got_avg_final, np.float64) - r64["avg_final"])[Mall].max()) if Mall.any() else 0.0
    elif got_avg_final is not None:                                                     # no hop: the array is as it was
        np.testing.assert_array_equal(got_avg_final, r64["avg_final"].astype(np.float32), err_msg=what)
    if got_rec is not None:
        np.testing.assert_array_equal(got_rec["flags"], r64["flags"], err_msg=what)
        idle = r64["flags"] == 0
        assert not np.asarray(got_rec["peak_bin"])[idle].any() and not np.asarray(got_rec["peak_db"])[idle].view(np.uint32).any(), f"{what}: a frame without a hop has a non-zero record"
        for h, f in enumerate(r64["hop_frames"]):
            fig["peak"] = max(fig["peak"], abs(float(got_rec["peak_db"][f]) - float(r64["peak_db"][f])))
            order = np.argsort(-r64["raw"][h], kind="stable")
            lead, second = order[0], order[1]
            ok = {int(lead)} if r64["raw"][h][lead] - r64["raw"][h][second] > 0.01 else {int(lead), int(second)}
            assert int(got_rec["peak_bin"][f]) in ok, f"{what}: peak_bin {got_rec['peak_bin'][f]} at frame {f}, the reference's {sorted(ok)}"
    fig["e32_avg"] = ref["e32_avg"]
    print(f"spec {what}: e32 {e32:.3e} e32_avg {ref['e32_avg']:.3e} bound {bound:.3e} raw {fig['raw']:.3e} avg {fig['avg']:.3e} peak {fig['peak']:.3e}")
    for k in ("raw", "avg", "peak"):
        e = ref["e32_avg"] if k == "avg" else e32                        # the averaged array against the float32 model's averaged arrays
        assert fig[k] <= BOUND_A, f"{what}: {k} deviates by {fig[k]:.3e} dB, bound (a) {BOUND_A}"
        assert fig[k] <= MARGIN_B * e, f"{what}: {k} deviates by {fig[k]:.3e} dB, bound (b) 32 x E32 = {MARGIN_B * e:.3e}"
    return fig


def mask_share(ref):
    """the share of bins the mask keeps: per hop (the smallest) and over all hops"""
    M = ref["M"]
    return (float(M.mean(axis=1).min()), float(M.all(axis=0).mean())) if len(M) else (1.0, 1.0)


# ---- inputs: rows [F][n] int16 of one channel
def noise_codes(seed, F_, n):
    return np.random.default_rng(seed).integers(0, 256, (F_, n), dtype=np.uint8)


def lsb_noise(seed, F_, n):
    return np.random.default_rng(seed).integers(-1, 2, (F_, n)).astype(np.int16)


def sine(k, F_, n, amp=32767.0, phase=0.0):
    """a line on the centre of bin k, continuous over the rows"""
    t = np.arange(F_ * n, dtype=np.float64)
    return np.round(amp * np.sin(2.0 * np.pi * k * t / N + phase)).clip(-32768, 32767).astype(np.int16).reshape(F_, n)


def square16(F_, n):
    t = np.arange(F_ * n)
    return np.where((t // 8) % 2 == 0, 32767, -32768).astype(np.int16).reshape(F_, n)


def ring_tone(F_, n):
    """440 + 480 Hz, the ring plan's ON phase, from the library's own host tone generator (igdsp_tone_frame)"""
    from igate4xsoftphonedsp_amd import capi

    plan, st = capi.tone_plan_build([(440, 480, 2000, 1000)]), np.zeros((), capi.TONE_STATE)
    rows = np.stack([capi.tone_frame(plan, st, n, capi.TONE_CMD_REWIND if f == 0 else 0)[0] for f in range(F_)]).astype(np.int16)
    assert np.abs(rows).max() > 10000
    return rows
