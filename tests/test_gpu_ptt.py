"""-m gpu: igdsp_ptt_arbitrate (include/igdsp.h, "PTT priority arbitration") bit for bit against tests/ptt_model.py — sel, tick, ctl_out,
out, stats (rms within 1e-5 relative), the final state and the final slots: a fuzz over the three input forms with groups of 0 to 300
members, a bad table and start states that are not zero; split invariance on the device; a garbage state; guard bytes around every
output; the outputs without audio; a group wider than the ops window; every argument path; two streams; the chains from
igdsp_depayload and into igdsp_tx_packetize; one chip-filling shape."""
import functools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import bss_model as bm  # noqa: E402
from tests import conf_model as cm  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import host_util as hu  # noqa: E402
from tests import ptt_model as pm  # noqa: E402
from tests import tx_model as tm  # noqa: E402

GUARD = 256
GAINS = np.array([0, 13, 64, 128, 256, 65535], np.uint16)
PART = 128                                                            # kPttPart
SIZES = (4, 0, 1, 2, 17, 65, 300)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def _dev(a):
    a = np.ascontiguousarray(a)
    return gu.to_dev(a if a.size else np.zeros(4, np.uint8))


class Guarded:
    """a device buffer of nbytes between two guard zones"""

    def __init__(self, nbytes, fill, init=None):
        self.n, self.fill = int(nbytes), fill
        raw = np.full(self.n + 2 * GUARD, fill, np.uint8)
        if init is not None:
            raw[GUARD:GUARD + self.n] = np.ascontiguousarray(init).view(np.uint8).reshape(-1)
        self.t = gu.to_dev(raw)
        self.ptr = self.t.data_ptr() + GUARD

    def take(self, what):
        raw = self.t.cpu().numpy()
        assert np.all(raw[:GUARD] == self.fill) and np.all(raw[GUARD + self.n:] == self.fill), f"guard bytes around {what} written"
        return raw[GUARD:GUARD + self.n].copy()


def run_ptt(ctx, info, ptr, mem, C_, G_, n, state, slots, payload=None, codec=None, pcm=None, length=None, gain=None, rxonly=None, rf=0,
            sel=True, tick=True, ctl=True, out=True, stats=True, stream=None, entry=None, fill=None, raw=None):
    """igdsp_ptt_arbitrate through the C ABI with guard bytes around every output, the state and the slots; returns (sel, tick, ctl, out,
    stats, state, slots) (None where not asked for).  entry: through that yardstick of capi.INTERNAL_TWIN instead; fill: the byte every
    output and its guards hold before the launch; raw: a dict that takes the output buffers' bytes, guards included, after it."""
    torch = gu.torch_cuda()
    F_, nm = info.shape[0], len(mem)
    audio = payload is not None or pcm is not None
    f5 = (0x3C, 0x4D, 0x2B, 0xA5, 0x5A) if fill is None else (fill,) * 5
    b_sel = Guarded(F_ * G_ * 4, f5[0]) if sel else None
    b_tick = Guarded(F_ * G_ * 8, f5[1]) if tick else None
    b_ctl = Guarded(F_ * G_, f5[2]) if ctl else None
    b_out = Guarded(F_ * G_ * n * 2, f5[3]) if out and audio else None
    b_st = Guarded(F_ * G_ * 16, f5[4]) if stats and audio else None
    b_state = Guarded(G_ * 16, 0x77, state)
    b_slots = Guarded(nm * 8, 0x66, slots)
    keep = [_dev(x) if x is not None else None for x in (info, ptr, mem if nm else None, payload, codec, pcm, length, gain, rxonly)]
    d_info, d_ptr, d_mem, d_pl, d_cd, d_pcm, d_len, d_gain, d_rx = keep
    p = lambda b: b.ptr if b is not None else None                  # noqa: E731
    (ctx.via(entry) if entry else ctx).ptt_arbitrate(
        d_info, d_ptr, d_mem, nm, b_state.ptr, b_slots.ptr if nm else None, C_, G_, F_, n, payload=d_pl, codec=d_cd, pcm=d_pcm, length=d_len,
        gain=d_gain, rxonly=d_rx, release_frames=rf, sel=p(b_sel), tick=p(b_tick), ctl_out=p(b_ctl), out=p(b_out), stats=p(b_st), stream=stream)
    if stream is None:
        torch.cuda.synchronize()
    else:
        ctx.sync(stream)
    s = b_sel.take("d_sel").view("<i4").reshape(F_, G_) if sel else None
    t = b_tick.take("d_tick").view(capi.PTT_TICK).reshape(F_, G_) if tick else None
    c = b_ctl.take("d_ctl_out").reshape(F_, G_) if ctl else None
    o = b_out.take("d_out").view("<i2").reshape(F_, G_, n) if b_out is not None else None
    r = b_st.take("d_stats").view(capi.FRAME_STATS).reshape(F_, G_) if b_st is not None else None
    st = b_state.take("d_state").view(capi.PTT_STATE)
    sl = b_slots.take("d_slots").view(capi.PTT_SLOT)
    if raw is not None:
        raw.update({k: b.t.cpu().numpy() for k, b in (("sel", b_sel), ("tick", b_tick), ("ctl_out", b_ctl), ("out", b_out), ("stats", b_st))
                    if b is not None})
    return s, t, c, o, r, st, sl


def check(got, exp, x=None, n=None, gain=None, length=None):
    """got: run_ptt's tuple; exp: pm.arbitrate's (sel, tick, state, slots)"""
    s, t, c, o, r, st, sl = got
    es, et, est, esl = exp
    if s is not None:
        np.testing.assert_array_equal(s, es)
    if t is not None:
        for k in capi.PTT_TICK.names:
            np.testing.assert_array_equal(t[k], et[k], err_msg=k)
    if c is not None:
        np.testing.assert_array_equal(c, et["ctl"])
    np.testing.assert_array_equal(st.view(np.uint8), est.view(np.uint8))
    np.testing.assert_array_equal(sl.view(np.uint8), esl.view(np.uint8))
    if x is not None:
        eo, ers = bm.emit(es, x, n, gain, length)
        np.testing.assert_array_equal(o, eo)
        gu.assert_stats_equal(r, ers)


def random_info(rng, F_, C_, p_key=0.4):
    """PTT types held for runs of frames with short drops inside (bridged releases); PTs that store and that do not; runts"""
    typ = np.zeros((F_, C_), np.int64)
    hold = rng.integers(1, 20, (F_, C_))
    val = np.where(rng.random((F_, C_)) < p_key, rng.choice([1, 1, 2, 2, 3, 5], (F_, C_)), 0)
    for c in range(C_):
        t = 0
        while t < F_:
            typ[t:t + hold[t, c], c] = val[t, c]
            t += hold[t, c]
    typ[rng.random((F_, C_)) < 0.05] = 0                              # one-frame drops
    info = np.zeros((F_, C_), capi.RTP_INFO)
    info["ed137"] = (typ.astype(np.uint32) << 29) | (rng.integers(0, 64, (F_, C_)).astype(np.uint32) << 22) | rng.integers(0, 1 << 22, (F_, C_)).astype(np.uint32)
    info["pt"] = rng.choice([0, 8, 18, 96, 123], (F_, C_), p=[0.65, 0.15, 0.05, 0.05, 0.10])
    info["flags"] = np.where(rng.random((F_, C_)) < 0.05, bm.RTP_RUNT, 0)
    info["payload_len"] = 160
    return info


def small_table(rng, C_, G_):
    sizes = rng.integers(0, 7, G_)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    return ptr, rng.integers(0, C_, int(ptr[-1])).astype(np.uint32)


def garbage(rng, G_, nm):
    st = np.zeros(G_, capi.PTT_STATE)
    st["level"] = rng.choice([0, 1, 3, 7, 9, 0xFFFFFFFF], G_)
    st["holder"] = rng.choice([0, 1, 2, 5, 400, 0xFFFFFFFF], G_)
    st["takeovers"] = rng.integers(0, 2**32, G_, dtype=np.uint64)
    st["reserved"] = rng.integers(0, 2**32, G_, dtype=np.uint64)
    sl = rng.integers(0, 256, nm * 8).astype(np.uint8).view(capi.PTT_SLOT).copy()
    sl["pressed"] = rng.choice([0, 1, 0x37], nm)
    sl["release_cnt"] = rng.choice([0, 1, 11, 254, 255], nm)
    return st, sl


FUZZ_F = (1, 7, PART + 2)
FUZZ_C = 64


@functools.lru_cache(maxsize=None)
def fuzz_case(case):
    """the fuzz's table, info, start state and model result of case 0 .. 2, shared by the three forms and left unchanged: groups of
    SIZES members, a descending group_ptr pair (group 1, so group 0 runs into group 2's slots), a group_ptr past n_members, members
    >= n_channels, and 389 slots over 64 channels (every channel sits in several groups)"""
    rng = np.random.default_rng(6124 + case)
    F_, C_, G_ = FUZZ_F[case], FUZZ_C, len(SIZES)
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint32)
    nm = int(ptr[-1])
    mem = rng.integers(0, C_, nm).astype(np.uint32)
    mem[rng.random(nm) < 0.08] = C_ + rng.integers(0, 5)
    ptr[1] = ptr[2] + 2                                               # descending: group 1 (already empty) and an overlap
    ptr[-1] = nm + 7                                                  # clamped
    info = random_info(rng, F_, C_)
    st0, sl0 = garbage(rng, G_, nm) if case == 1 else (np.zeros(G_, capi.PTT_STATE), np.zeros(nm, capi.PTT_SLOT))
    rxonly = (rng.random(C_) < 0.1).astype(np.uint8) if case else None
    rf = (0, 3, 5)[case]
    exp = pm.arbitrate(info, ptr, mem, nm, C_, G_, st0, sl0, rxonly, rf)
    for a in (ptr, mem, info, st0, sl0) + tuple(exp):
        a.setflags(write=False)
    return info, ptr, mem, st0, sl0, rxonly, rf, exp


@pytest.mark.parametrize("form", ["g711", "pcm", "none"])
@pytest.mark.parametrize("case", range(3))
def test_fuzz(ctx, orc, form, case):
    info, ptr, mem, st0, sl0, rxonly, rf, exp = fuzz_case(case)
    rng = np.random.default_rng(200 + case)
    F_, C_, G_ = info.shape[0], FUZZ_C, len(SIZES)
    n = (160, 24, 163)[case]
    gain = GAINS[rng.integers(0, len(GAINS), C_)] if case != 0 else None
    length = rng.integers(0, n + 3, (F_, C_)).astype(np.uint16) if case == 1 else None
    x, kw = None, {}
    if form == "g711":
        payload = orc.gen_uniform(F_ * C_ * n, seed=case).reshape(F_, C_, n)
        codec = np.where(rng.random(C_) < 0.5, 8, 0).astype(np.uint8)
        x, kw = cm.decode(payload, codec, orc), dict(payload=payload, codec=codec)
    elif form == "pcm":
        pcm = rng.integers(-32768, 32768, (F_, C_, n)).astype(np.int16)
        x, kw = pcm.astype(np.int64), dict(pcm=pcm)
    got = run_ptt(ctx, info, ptr, mem, C_, G_, n, st0, sl0, length=length, gain=gain, rxonly=rxonly, rf=rf, **kw)
    check(got, exp, x, n, gain, length)
    if form == "none":
        assert got[3] is None and got[4] is None
    if F_ > 1:
        assert (exp[0] >= 0).any() and (exp[0] < 0).any() and (exp[1]["flags"] & pm.TAKEOVER).any() and (exp[1]["flags"] & pm.RELEASE).any()


def test_split_invariance_on_the_device(ctx, orc):
    rng = np.random.default_rng(21)
    C_, G_, F_, n = 32, 10, 40, 160
    info = random_info(rng, F_, C_)
    ptr, mem = small_table(rng, C_, G_)
    payload = orc.gen_uniform(F_ * C_ * n, seed=9).reshape(F_, C_, n)
    codec = np.zeros(C_, np.uint8)
    z = np.zeros(G_, capi.PTT_STATE), np.zeros(len(mem), capi.PTT_SLOT)
    whole = run_ptt(ctx, info, ptr, mem, C_, G_, n, *z, payload=payload, codec=codec, rf=4)
    check(whole, pm.arbitrate(info, ptr, mem, len(mem), C_, G_, *z, None, 4), cm.decode(payload, codec, orc), n)
    st, sl = z
    parts = []
    for f in range(F_):
        r = run_ptt(ctx, info[f:f + 1], ptr, mem, C_, G_, n, st, sl, payload=payload[f:f + 1], codec=codec, rf=4)
        st, sl = r[5], r[6]
        parts.append(r)
    for i, what in enumerate(("sel", "tick", "ctl_out", "out", "stats")):
        np.testing.assert_array_equal(np.concatenate([p[i] for p in parts]).view(np.uint8), whole[i].view(np.uint8), err_msg=what)
    np.testing.assert_array_equal(st.view(np.uint8), whole[5].view(np.uint8))
    np.testing.assert_array_equal(sl.view(np.uint8), whole[6].view(np.uint8))


def test_two_parts_and_two_passes_in_one_launch(ctx):
    """more frames than one part (kPttPart = 128) and 64 slots per wave (two passes of 64 frames a part): state and slots carried"""
    rng = np.random.default_rng(31)
    C_, G_, F_ = 80, 20, 300
    info = random_info(rng, F_, C_)
    ptr = np.arange(0, C_ + 1, 4, dtype=np.uint32)
    mem = rng.permutation(C_).astype(np.uint32)
    z = np.zeros(G_, capi.PTT_STATE), np.zeros(C_, capi.PTT_SLOT)
    got = run_ptt(ctx, info, ptr, mem, C_, G_, 160, *z, rf=3)
    check(got, pm.arbitrate(info, ptr, mem, C_, C_, G_, *z, None, 3))


def test_garbage_state_and_slots(ctx):
    rng = np.random.default_rng(77)
    C_, G_, F_ = 24, 12, 30
    info = random_info(rng, F_, C_)
    ptr, mem = small_table(rng, C_, G_)
    mem[::7] = C_ + 3
    st0, sl0 = garbage(rng, G_, len(mem))
    got = run_ptt(ctx, info, ptr, mem, C_, G_, 160, st0, sl0)
    exp = pm.arbitrate(info, ptr, mem, len(mem), C_, G_, st0, sl0)
    check(got, exp)
    assert (exp[2]["level"] <= 7).all() and (exp[2]["holder"] <= (np.diff(ptr.astype(np.int64)))).all()
    dropped = mem >= C_
    np.testing.assert_array_equal(got[6][dropped].view(np.uint8), sl0[dropped].view(np.uint8))      # frozen
    np.testing.assert_array_equal(got[5]["reserved"], st0["reserved"])


def test_outputs_without_audio_each_alone(ctx):
    rng = np.random.default_rng(7)
    C_, G_, F_ = 20, 6, 30
    info = random_info(rng, F_, C_)
    ptr, mem = small_table(rng, C_, G_)
    z = np.zeros(G_, capi.PTT_STATE), np.zeros(len(mem), capi.PTT_SLOT)
    exp = pm.arbitrate(info, ptr, mem, len(mem), C_, G_, *z, None, 2)
    for only in ("sel", "tick", "ctl", None):
        kw = {k: k == only for k in ("sel", "tick", "ctl")}
        got = run_ptt(ctx, info, ptr, mem, C_, G_, 160, *z, rf=2, **kw)
        assert got[3] is None and got[4] is None
        check(got, exp)


def test_group_wider_than_the_ops_window(ctx):
    """one group of 4 100 slots (more than kPttOps = 4 096: a frame at a time, two windows) next to a group of 3"""
    rng = np.random.default_rng(4100)
    C_, G_, F_ = 512, 2, 3
    ptr = np.array([0, 4100, 4103], np.uint32)
    mem = rng.integers(0, C_, 4103).astype(np.uint32)
    info = random_info(rng, F_, C_, p_key=0.02)
    info["pt"] = 0
    z = np.zeros(G_, capi.PTT_STATE), np.zeros(4103, capi.PTT_SLOT)
    got = run_ptt(ctx, info, ptr, mem, C_, G_, 160, *z, rf=1)
    exp = pm.arbitrate(info, ptr, mem, 4103, C_, G_, *z, None, 1)
    check(got, exp)
    assert (exp[1]["flags"][:, 0] & pm.TAKEOVER).any()


def test_chip_filling_shape(ctx, orc):
    """65 536 legs in 16 384 groups of 4 x 8 frames, G.711: sel, tick, ctl, state and slots everywhere, out and records on one frame"""
    torch = gu.torch_cuda()
    rng = np.random.default_rng(65536)
    C_, m, F_, n = 65536, 4, 8, 160
    G_ = C_ // m
    info = random_info(rng, F_, C_, p_key=0.6)
    ptr = np.arange(0, C_ + 1, m, dtype=np.uint32)
    mem = np.arange(C_, dtype=np.uint32)
    codec = np.where(np.arange(C_) % 3 == 0, 8, 0).astype(np.uint8)
    d_pl = torch.randint(0, 256, (F_ * C_ * n,), dtype=torch.uint8, device="cuda")
    d_sel, d_tick, d_ctl = gu.dev_zeros(F_ * G_ * 4), gu.dev_zeros(F_ * G_ * 8), gu.dev_zeros(F_ * G_)
    d_out, d_st = gu.dev_zeros(F_ * G_ * n * 2), gu.dev_zeros(F_ * G_ * 16)
    d_state, d_slots = gu.dev_zeros(G_ * 16), gu.dev_zeros(C_ * 8)
    ctx.ptt_arbitrate(gu.to_dev(info), gu.to_dev(ptr), gu.to_dev(mem), C_, d_state, d_slots, C_, G_, F_, n, payload=d_pl, codec=gu.to_dev(codec),
                      release_frames=2, sel=d_sel, tick=d_tick, ctl_out=d_ctl, out=d_out, stats=d_st)
    torch.cuda.synchronize()
    es, et, est, esl = pm.arbitrate(info, ptr, mem, C_, C_, G_, np.zeros(G_, capi.PTT_STATE), np.zeros(C_, capi.PTT_SLOT), None, 2)
    np.testing.assert_array_equal(gu.to_host(d_sel, "<i4", (F_, G_)), es)
    np.testing.assert_array_equal(gu.to_host(d_tick, np.uint8), et.view(np.uint8).reshape(-1))
    np.testing.assert_array_equal(gu.to_host(d_ctl, np.uint8, (F_, G_)), et["ctl"])
    np.testing.assert_array_equal(gu.to_host(d_state, np.uint8), est.view(np.uint8).reshape(-1))
    np.testing.assert_array_equal(gu.to_host(d_slots, np.uint8), esl.view(np.uint8).reshape(-1))
    assert 0.3 < (es >= 0).mean() < 1.0
    f, g1 = 7, 2048                                                   # the emit on a slice of one frame
    pl = d_pl[f * C_ * n:(f + 1) * C_ * n].cpu().numpy().reshape(1, C_, n)
    eo, er = bm.emit(es[f:f + 1, :g1], cm.decode(pl, codec, orc), n)
    np.testing.assert_array_equal(d_out[f * G_ * n * 2:(f * G_ + g1) * n * 2].cpu().numpy().view("<i2").reshape(1, g1, n), eo)
    gu.assert_stats_equal(d_st[f * G_ * 16:(f * G_ + g1) * 16].cpu().numpy().view(capi.FRAME_STATS).reshape(1, g1), er)


def test_chain_depayload_ptt(ctx, orc):
    """ED-137 packets with PTT words, R2S keep-alives (PT 123, no payload) and gaps (size 0) through igdsp_depayload"""
    torch = gu.torch_cuda()
    C_, F_, n, stride = 24, 40, 160, 192
    rng = np.random.default_rng(4)
    radio = np.ones(C_, np.uint8)
    codec = np.where(np.arange(C_) % 2 == 0, 8, 0).astype(np.uint8)
    pk = np.zeros((F_, C_, stride), np.uint8)
    sizes = np.zeros((F_, C_), np.uint16)
    body = orc.gen_uniform(F_ * C_ * n, seed=6).reshape(F_, C_, n)
    typ = random_info(rng, F_, C_, p_key=0.5)["ed137"]
    for f in range(F_):
        for c in range(C_):
            kind = rng.choice(3, p=[0.75, 0.15, 0.1])                 # audio, keep-alive, gap
            if kind == 2:
                continue
            pkt = hu.rtp_packet(123 if kind == 1 else int(codec[c]), f, b"" if kind == 1 else bytes(body[f, c]), True, int(typ[f, c]))
            pk[f, c, :len(pkt)] = np.frombuffer(pkt, np.uint8)
            sizes[f, c] = len(pkt)
    d_pl, d_len, d_info = gu.dev_zeros(F_ * C_ * n), gu.dev_zeros(F_ * C_ * 2), gu.dev_zeros(F_ * C_ * 8)
    ctx.depayload(gu.to_dev(pk), gu.to_dev(sizes), gu.to_dev(radio), C_, F_, stride, n, d_pl, d_len, d_info)
    torch.cuda.synchronize()
    info = gu.to_host(d_info, capi.RTP_INFO, (F_, C_))
    G_ = C_ // 3
    ptr = np.arange(0, C_ + 1, 3, dtype=np.uint32)
    mem = np.arange(C_, dtype=np.uint32)
    d_sel, d_tick, d_out, d_st = gu.dev_zeros(F_ * G_ * 4), gu.dev_zeros(F_ * G_ * 8), gu.dev_zeros(F_ * G_ * n * 2), gu.dev_zeros(F_ * G_ * 16)
    ctx.ptt_arbitrate(d_info, gu.to_dev(ptr), gu.to_dev(mem), C_, gu.dev_zeros(G_ * 16), gu.dev_zeros(C_ * 8), C_, G_, F_, n, payload=d_pl,
                      codec=gu.to_dev(codec), length=d_len, release_frames=2, sel=d_sel, tick=d_tick, out=d_out, stats=d_st)
    torch.cuda.synchronize()
    epl, elen, _ = orc.depayload(pk, sizes, radio, n)
    assert (info["flags"] & bm.RTP_RUNT).any() and (info["pt"] == 123).any()
    es, et, _, _ = pm.arbitrate(info, ptr, mem, C_, C_, G_, np.zeros(G_, capi.PTT_STATE), np.zeros(C_, capi.PTT_SLOT), None, 2)
    np.testing.assert_array_equal(gu.to_host(d_sel, "<i4", (F_, G_)), es)
    np.testing.assert_array_equal(gu.to_host(d_tick, np.uint8), et.view(np.uint8).reshape(-1))
    assert (es >= 0).any()
    eo, er = bm.emit(es, cm.decode(epl, codec, orc), n, None, elen)
    np.testing.assert_array_equal(gu.to_host(d_out, "<i2", (F_, G_, n)), eo)
    gu.assert_stats_equal(gu.to_host(d_st, capi.FRAME_STATS, (F_, G_)), er)


def test_chain_ptt_into_tx_packetize(ctx, orc):
    """d_ctl_out [F][G] passed as igdsp_tx_packetize's d_ctl [F][C] with C = G: the transmitters' PTT follows ON frame for frame"""
    torch = gu.torch_cuda()
    rng = np.random.default_rng(8)
    C_, G_, F_, n, stride, t0 = 32, 8, 24, 160, 192, 1_700_000_000_000
    info = random_info(rng, F_, C_, p_key=0.3)
    ptr = np.arange(0, C_ + 1, 4, dtype=np.uint32)
    mem = np.arange(C_, dtype=np.uint32)
    payload = orc.gen_uniform(F_ * C_ * n, seed=12).reshape(F_, C_, n)
    codec = np.zeros(C_, np.uint8)
    d_ctl, d_out = gu.dev_zeros(F_ * G_, 0x55), gu.dev_zeros(F_ * G_ * n * 2)
    ctx.ptt_arbitrate(gu.to_dev(info), gu.to_dev(ptr), gu.to_dev(mem), C_, gu.dev_zeros(G_ * 16), gu.dev_zeros(C_ * 8), C_, G_, F_, n,
                      payload=gu.to_dev(payload), codec=gu.to_dev(codec), release_frames=2, ctl_out=d_ctl, out=d_out)
    st = np.zeros(G_, capi.TX_CHAN)
    for g in range(G_):
        st[g] = tm.chan_init("Tx", False, 0, 0x1000 + g, 7 * g, 1000 * g, now_ms=t0)[()]
    last = np.zeros((G_, n), np.uint8)
    d_st, d_last = gu.to_dev(st), gu.to_dev(last)
    d_pk, d_sz, d_inf = gu.dev_zeros(F_ * G_ * stride, 0xA5), gu.dev_zeros(F_ * G_ * 2), gu.dev_zeros(F_ * G_ * 8)
    ctx.tx_packetize(d_st, d_last, d_pk, stride, d_sz, d_inf, G_, F_, n, t0, 20, pcm=d_out, ctl=d_ctl, variant=capi.ENC_G191)
    torch.cuda.synchronize()
    es, et, _, _ = pm.arbitrate(info, ptr, mem, C_, C_, G_, np.zeros(G_, capi.PTT_STATE), np.zeros(C_, capi.PTT_SLOT), None, 2)
    ctl = gu.to_host(d_ctl, np.uint8, (F_, G_))
    np.testing.assert_array_equal(ctl, et["ctl"])
    on = (et["flags"] & pm.ON) != 0
    assert on.any() and (~on).any()
    np.testing.assert_array_equal(ctl, np.where(on, 0x81, 0x80))
    eo, _ = bm.emit(es, cm.decode(payload, codec, orc), n)
    tab = orc.encode_table(0, capi.ENC_G191)
    g711 = tab[eo.astype(np.int32) + 32768]
    epk = np.full((F_, G_, stride), 0xA5, np.uint8)
    esz, einf = tm.packetize(st, last, g711, epk, ctl, t0, 20)
    np.testing.assert_array_equal(gu.to_host(d_sz, np.uint16, (F_, G_)), esz)
    assert np.array_equal(gu.to_host(d_inf, capi.TX_INFO, (F_, G_)), einf)
    np.testing.assert_array_equal(gu.to_host(d_pk, np.uint8, (F_, G_, stride)), epk)
    got_st = gu.to_host(d_st, capi.TX_CHAN)
    np.testing.assert_array_equal(got_st["ptt"], on[-1].astype(np.uint8))       # the transmitter's PTT is the last tick's ON
    np.testing.assert_array_equal(got_st["sql"], 0)                             # ctl holds sql at 0


def test_two_streams_disjoint_state(ctx, orc):
    torch = gu.torch_cuda()
    C_, G_, F_, n = 40, 10, 24, 160
    cases = []
    for i in range(2):
        rng = np.random.default_rng(40 + i)
        cases.append((random_info(rng, F_, C_),) + small_table(rng, C_, G_))
    payload = orc.gen_uniform(F_ * C_ * n, seed=13).reshape(F_, C_, n)
    codec = np.full(C_, 8, np.uint8)
    results, errors = [None, None], []

    def worker(i):
        try:
            s = torch.cuda.Stream()
            info, ptr, mem = cases[i]
            for _ in range(3):
                results[i] = run_ptt(ctx, info, ptr, mem, C_, G_, n, np.zeros(G_, capi.PTT_STATE), np.zeros(len(mem), capi.PTT_SLOT),
                                     payload=payload, codec=codec, rf=2, stream=s.cuda_stream)
        except Exception as e:                                      # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    x = cm.decode(payload, codec, orc)
    for i in range(2):
        info, ptr, mem = cases[i]
        exp = pm.arbitrate(info, ptr, mem, len(mem), C_, G_, np.zeros(G_, capi.PTT_STATE), np.zeros(len(mem), capi.PTT_SLOT), None, 2)
        check(results[i], exp, x, n)


def test_arguments(ctx):
    torch = gu.torch_cuda()
    C_, G_, F_, n = 8, 2, 2, 160
    info = _dev(np.zeros((F_, C_), capi.RTP_INFO))
    ptr, mem = _dev(np.array([0, 4, 8], np.uint32)), _dev(np.arange(8, dtype=np.uint32))
    state, slots = gu.dev_zeros(G_ * 16), gu.dev_zeros(8 * 8)
    pl, cd, pcm = gu.dev_zeros(F_ * C_ * n), gu.dev_zeros(C_), gu.dev_zeros(F_ * C_ * n * 2)
    out, st, sel = gu.dev_zeros(F_ * G_ * n * 2 + 8), gu.dev_zeros(F_ * G_ * 16 + 8), gu.dev_zeros(F_ * G_ * 4 + 8)
    tick, ctl = gu.dev_zeros(F_ * G_ * 8 + 8), gu.dev_zeros(F_ * G_ + 8)
    L, h = ctx.L, ctx.h

    def call(**kw):
        a = dict(info=info, payload=pl, codec=cd, pcm=None, length=None, gain=None, ptr=ptr, mem=mem, nm=8, rx=None, C=C_, G=G_, F=F_, n=n,
                 rf=0, state=state, slots=slots, sel=sel, tick=tick, ctl=ctl, out=out, stats=st)
        a.update(kw)
        p = capi._ptr
        return L.igdsp_ptt_arbitrate(h, p(a["info"]), p(a["payload"]), p(a["codec"]), p(a["pcm"]), p(a["length"]), p(a["gain"]), p(a["ptr"]),
                                     p(a["mem"]), a["nm"], p(a["rx"]), a["C"], a["G"], a["F"], a["n"], a["rf"], p(a["state"]), p(a["slots"]),
                                     p(a["sel"]), p(a["tick"]), p(a["ctl"]), p(a["out"]), p(a["stats"]), None)

    EINVAL = -22
    assert call() == 0
    assert call(payload=None, codec=None, pcm=pcm) == 0
    assert call(payload=None, codec=None, out=None, stats=None) == 0                 # no audio
    assert call(sel=None, tick=None, ctl=None, out=None, stats=None) == 0            # state only
    assert call(rf=1) == 0 and call(rf=255) == 0
    assert call(G=0) == 0 and call(F=0) == 0 and call(G=0, info=None) == 0           # nothing to do
    assert call(G=0, n=0) == EINVAL and call(F=0, n=257) == EINVAL                   # n and n_members are always checked
    assert call(F=0, nm=(1 << 24) + 1) == EINVAL
    assert call(info=None) == EINVAL
    assert call(ptr=None) == EINVAL
    assert call(state=None) == EINVAL
    assert call(mem=None) == EINVAL and call(slots=None) == EINVAL
    assert call(nm=0, mem=None, slots=None) == 0
    assert call(nm=(1 << 24) + 1) == EINVAL
    assert call(rf=256) == EINVAL
    assert call(pcm=pcm) == EINVAL                                                   # two input forms
    assert call(codec=None) == EINVAL
    assert call(payload=None, codec=None) == EINVAL                                  # out / stats without audio
    assert call(n=0) == EINVAL and call(n=257) == EINVAL
    assert call(stats=capi._ptr(st) + 4) == EINVAL
    assert call(out=capi._ptr(out) + 1) == EINVAL
    assert call(sel=capi._ptr(sel) + 2) == EINVAL
    assert call(tick=capi._ptr(tick) + 2) == EINVAL
    assert call(ctl=capi._ptr(ctl) + 1) == 0                                         # bytes: any address
    assert call(info=capi._ptr(info) + 2) == EINVAL
    assert call(slots=capi._ptr(slots) + 2) == EINVAL
    with pytest.raises(capi.IgdspError):
        ctx.ptt_arbitrate(info, ptr, mem, 8, None, slots, C_, G_, F_, n)
    torch.cuda.synchronize()


# ---- the compute-free yardstick (igdsp_internal_ptt_copy, tools/ptt_bench.py) against its promise in csrc/igdsp_capi.hip: "the same
# traversal (info records, ops passes, the first member of every group emitted undecoded), the same bytes in and out, no debounce,
# arbitration, decode or records; the group state is not touched, the slots are stepped as by a launch, and sel / out / stats hold raw
# bytes (tick and ctl_out are not written)"

def _yard_inputs(rng, form, F_, C_, n):
    if form == "g711":
        return dict(payload=rng.integers(0, 256, (F_, C_, n), dtype=np.uint8), codec=np.where(rng.random(C_) < 0.5, 8, 0).astype(np.uint8))
    return dict(pcm=rng.integers(-32768, 32768, (F_, C_, n)).astype(np.int16)) if form == "pcm" else {}


def _yard_table(rng, C_, G_, wide=False):
    """groups of 1 .. 6 members; wide: one of 70 (more than the 64 slots of an ops window: two passes)"""
    sizes = rng.integers(1, 7, G_)
    if wide:
        sizes[G_ // 2] = 70
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    return ptr, rng.integers(0, C_, int(ptr[-1])).astype(np.uint32)


@pytest.mark.parametrize("form", ["g711", "pcm", "none"])
@pytest.mark.parametrize("F_", [3, 131])
def test_yardstick_footprint_and_independence(ctx, form, F_):
    """igdsp_internal_ptt_copy, group counts around a wave's (G = 17 with a group of 70 slots: two passes), one part and two, the three
    input forms: it stores the bytes igdsp_ptt_arbitrate stores in sel, out and stats, nothing in d_tick and d_ctl_out, leaves the slots
    as the entry does and the group state as it was; whether that holds zeros or garbage, the outputs are the same bytes"""
    rng = np.random.default_rng(840 + F_ + len(form))
    C_, n = 48, 160
    for G_ in (1, 15, 17, 65):
        info = random_info(rng, F_, C_)
        ptr, mem = _yard_table(rng, C_, G_, wide=G_ == 17)
        kw = _yard_inputs(rng, form, F_, C_, n)
        _, sl0 = garbage(rng, G_, len(mem))
        got = {}

        def launch(entry):
            def run(fill):
                raw = {}
                st0 = np.full(G_ * 16, fill, np.uint8).view(capi.PTT_STATE) if entry else np.zeros(G_, capi.PTT_STATE)
                got[entry, fill] = run_ptt(ctx, info, ptr, mem, C_, G_, n, st0, sl0, entry=entry, fill=fill, raw=raw, **kw)
                return raw
            return run

        yard, real = gu.written_mask(launch("ptt_copy")), gu.written_mask(launch(None))
        assert all(real[k][GUARD:-GUARD].all() for k in real if k in ("sel", "out", "stats"))
        gu.assert_same_footprint(yard, real, not_written=("tick", "ctl_out"))
        zero = run_ptt(ctx, info, ptr, mem, C_, G_, n, np.zeros(G_, capi.PTT_STATE), sl0, entry="ptt_copy", fill=gu.FILL_A, **kw)
        a, b = got["ptt_copy", gu.FILL_A], got["ptt_copy", gu.FILL_B]
        assert (a[5].view(np.uint8) == gu.FILL_A).all() and (b[5].view(np.uint8) == gu.FILL_B).all() and not zero[5].view(np.uint8).any()
        for x in (b, zero):
            assert all(p is None or p.tobytes() == q.tobytes() for p, q in zip((x[0], x[3], x[4]), (a[0], a[3], a[4])))
            assert x[6].tobytes() == got[None, gu.FILL_A][6].tobytes()                                            # the slots as the entry's
        np.testing.assert_array_equal(a[0], np.broadcast_to(mem[ptr[:-1]].astype(np.int64), (F_, G_)))           # sel: the first member


@pytest.mark.parametrize("form", ["g711", "pcm"])
def test_yardstick_reads_the_first_members_rows(ctx, form):
    """one channel's whole row of one frame replaced by fresh random bytes: out (and the raw bytes in the record) of exactly the groups
    whose first member it is change, in that frame; every other output byte is the same.  One d_info record replaced: every output
    byte is the same and the launch completes — the promise says the records are read, but nothing the yardstick stores in sel, out or
    stats depends on them (the kernel keeps the loads alive through a fold it compares with a constant), and a load that was dropped
    cannot be seen from outside, so this is as far as a test can go."""
    rng = np.random.default_rng(860 + len(form))
    C_, G_, F_, n, f = 48, 65, 3, 160, 1
    info = random_info(rng, F_, C_)
    ptr, mem = _yard_table(rng, C_, G_, wide=True)
    kw = _yard_inputs(rng, form, F_, C_, n)
    st0, sl0 = np.zeros(G_, capi.PTT_STATE), np.zeros(len(mem), capi.PTT_SLOT)
    c = int(mem[ptr[G_ // 2]])                                             # the wide group's first member
    consumers = [g for g in range(G_) if mem[ptr[g]] == c]
    base = run_ptt(ctx, info, ptr, mem, C_, G_, n, st0, sl0, entry="ptt_copy", **kw)
    key = "payload" if form == "g711" else "pcm"
    rows = kw[key].copy()
    rows[f, c] = rng.integers(0, 256, n, dtype=np.uint8) if form == "g711" else rng.integers(-32768, 32768, n).astype(np.int16)
    got = run_ptt(ctx, info, ptr, mem, C_, G_, n, st0, sl0, entry="ptt_copy", **{**kw, key: rows})
    want = np.zeros((F_, G_), bool)
    want[f, consumers] = True
    np.testing.assert_array_equal((got[3] != base[3]).any(axis=2), want)
    rec = lambda r: np.ascontiguousarray(r).view(np.uint8).reshape(F_, G_, 16)   # noqa: E731
    assert got[0].tobytes() == base[0].tobytes() and not (rec(got[4]) != rec(base[4])).any(axis=2)[~want].any()
    info2 = info.copy()
    info2[f, c] = random_info(rng, 1, 1)[0, 0]
    info2["ed137"][f, c] ^= 0x5A5A5A5A
    got = run_ptt(ctx, info2, ptr, mem, C_, G_, n, st0, sl0, entry="ptt_copy", **kw)
    assert all(p.tobytes() == q.tobytes() for p, q in zip((got[0], got[3], got[4]), (base[0], base[3], base[4])))
