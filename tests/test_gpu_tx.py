"""-m gpu: igdsp_tx_packetize against tests/tx_model.py — packets over [0, size), the 0xA5 sentinel past size and in unsent slots,
sizes, info, final state and send buffers; split launches; the round trip through igdsp_depayload; two streams at once."""
import numpy as np
import pytest

from igate4xsoftphonedsp_amd import capi
from tests import tx_model as tm
from tests.gpu_util import dev_zeros, to_dev, to_host, torch_cuda

pytestmark = pytest.mark.gpu
N, STRIDE = 160, 180
CALLTYPES = ["Tx", "Rx", "Rxonly", "TRx", "Idle", "RxTx", "Foo", "IdleTx"]


def rand_states(rng, C_, pt, t0):
    st = np.zeros((C_,), capi.TX_CHAN)
    for c in range(C_):
        st[c] = tm.chan_init(CALLTYPES[rng.integers(len(CALLTYPES))], bool(rng.integers(2)), int(pt[c]), int(rng.integers(1 << 32)),
                             int(rng.integers(1 << 16)), int(rng.integers(1 << 32)), int(rng.choice([200, 60, 0, -1, 1000])),
                             int(t0 + rng.integers(-100, 400)))
    st["first_r2s"] = rng.random(C_) < 0.5
    st["packet_cnt"] = np.where(st["first_r2s"], rng.integers(0, 31, C_), 30)
    for k in ("tx_slave", "rx_slave", "tx_slave_changed", "rx_slave_changed", "ptt", "sql", "call_recorder"):
        st[k] = rng.integers(0, 2, C_)
    st["slave_count"] = rng.integers(0, 6, C_)
    st["pttid"], st["pttpriority"], st["bssi"] = rng.integers(0, 256, C_), rng.integers(0, 256, C_), rng.integers(0, 256, C_)
    st["tx_run"] = rng.integers(-5, 32767, C_)
    st["level"] = rng.integers(0, 256, C_)
    return st


def rand_ctl(rng, F_, C_, p_set=0.05):
    ctl = (rng.random((F_, C_)) < p_set).astype(np.uint8) * capi.TX_CTL_SET
    ctl |= rng.integers(0, 8, (F_, C_)).astype(np.uint8)
    return ctl


def rand_pcm(rng, F_, C_, n):
    pcm = rng.integers(-32768, 32768, (F_, C_, n), dtype=np.int16)
    sil = rng.random((F_, C_)) < 0.3                       # silence frames: the probe bytes 0xD5 (A-law) / 0xFF (mu-law)
    pcm[sil] = rng.integers(-2, 3, (int(sil.sum()), n), dtype=np.int16)
    return pcm


def encode_np(orc, pcm, pt, variant):
    tabs = {p: orc.encode_table(p, variant) for p in (0, 8)}
    out = np.empty(pcm.shape, np.uint8)
    law = np.broadcast_to((pt == 8)[:, None], pcm.shape[1:])
    for f in range(pcm.shape[0]):                            # frame by frame: no full-size temporaries
        idx = pcm[f].astype(np.int32) + 32768
        out[f] = np.where(law, tabs[8][idx], tabs[0][idx])
    return out


class Dev:
    """device copies of one packetizer's buffers"""

    def __init__(self, st, last, F_, C_, n, stride):
        self.st, self.last = to_dev(st), to_dev(last)
        self.pk = dev_zeros(F_ * C_ * stride, 0xA5)
        self.sizes = dev_zeros(F_ * C_ * 2)
        self.info = dev_zeros(F_ * C_ * 8)
        self.F, self.C, self.n, self.stride = F_, C_, n, stride

    def run(self, ctx, pcm=None, g711=None, ctl=None, t0=0, frame_ms=20, variant=capi.ENC_G191, f0=0, nf=None, stream=None, c0=0, nc=None):
        """frames [f0, f0 + nf) of channels [c0, c0 + nc): sub-views of the time-major arrays only where they are contiguous"""
        torch = torch_cuda()
        nf = self.F if nf is None else nf
        nc = self.C if nc is None else nc
        assert nc == self.C or nf == 1             # a channel sub-range is contiguous only within one frame
        ctx.tx_packetize(self.st.data_ptr() + 64 * c0, self.last.data_ptr() + c0 * self.n,
                         self.pk.data_ptr() + (f0 * self.C + c0) * self.stride, self.stride,
                         self.sizes.data_ptr() + 2 * (f0 * self.C + c0), self.info.data_ptr() + 8 * (f0 * self.C + c0), nc, nf, self.n,
                         t0 + f0 * frame_ms, frame_ms,
                         pcm=None if pcm is None else pcm.data_ptr() + 2 * (f0 * self.C + c0) * self.n,
                         g711=None if g711 is None else g711.data_ptr() + (f0 * self.C + c0) * self.n,
                         ctl=None if ctl is None else ctl.data_ptr() + f0 * self.C + c0, variant=variant, stream=stream)

    def host(self):
        torch_cuda().cuda.synchronize()
        F_, C_ = self.F, self.C
        return (to_host(self.st, capi.TX_CHAN), to_host(self.last, np.uint8, (C_, self.n)), to_host(self.pk, np.uint8, (F_, C_, self.stride)),
                to_host(self.sizes, np.uint16, (F_, C_)), to_host(self.info, capi.TX_INFO, (F_, C_)))


def model(st, last, g711, ctl, t0, frame_ms, stride):
    F_, C_, n = g711.shape
    st, last = st.copy(), last.copy()
    pk = np.full((F_, C_, stride), 0xA5, np.uint8)
    sizes, info = tm.packetize(st, last, g711, pk, ctl, t0, frame_ms)
    return st, last, pk, sizes, info


def check(got, exp, what=""):
    gst, glast, gpk, gsz, ginf = got
    est, elast, epk, esz, einf = exp
    assert np.array_equal(gsz, esz), what + ": sizes"
    assert np.array_equal(ginf, einf), what + ": info"
    bad = np.argwhere(gpk != epk)
    assert bad.size == 0, (what + ": packets", bad[:5], gsz[tuple(bad[0][:2])] if bad.size else None)
    assert np.array_equal(glast, elast), what + ": send buffers"
    assert gst.tobytes() == est.tobytes(), (what + ": state", [k for k in capi.TX_CHAN.names if not np.array_equal(gst[k], est[k])])


@pytest.mark.parametrize("form", ["pcm", "g711"])
@pytest.mark.parametrize("variant", [capi.ENC_G191, capi.ENC_SUN16])
def test_fuzz_4096x64(orc, form, variant):
    rng = np.random.default_rng(7 + variant + (form == "pcm") * 10)
    C_, F_, t0 = 4096, 64, 1_700_000_000_000
    pt = np.where(rng.random(C_) < 0.5, 8, 0).astype(np.uint8)            # both laws
    st = rand_states(rng, C_, pt, t0)
    last = rng.integers(0, 256, (C_, N)).astype(np.uint8)
    pcm = rand_pcm(rng, F_, C_, N)
    g711 = encode_np(orc, pcm, pt, variant)
    ctl = rand_ctl(rng, F_, C_)
    exp = model(st, last, g711, ctl, t0, 20, STRIDE)
    with capi.Context(device=0, max_channels=64) as ctx:
        d = Dev(st, last, F_, C_, N, STRIDE)
        d_ctl = to_dev(ctl)
        if form == "pcm":
            d.run(ctx, pcm=to_dev(pcm), ctl=d_ctl, t0=t0, variant=variant)
        else:
            d.run(ctx, g711=to_dev(g711), ctl=d_ctl, t0=t0)
        check(d.host(), exp, f"{form}/{variant}")
    # the fuzz covered every branch
    f = exp[4]["flags"]
    for b in (capi.TX_SENT, capi.TX_KEEPALIVE_PT, capi.TX_MARKER, capi.TX_STALE_PAYLOAD, capi.TX_LEVEL_VALID):
        assert (f & b).any(), b
    assert (exp[3] == 0).any() and (exp[3] == 20).any() and (exp[3] == 180).any()


@pytest.mark.parametrize("n,stride", [(13, 36), (48, 68), (50, 72), (161, 184)])
def test_odd_geometry(orc, n, stride):
    rng = np.random.default_rng(n)
    C_, F_, t0 = 300, 19, 5000
    pt = np.where(rng.random(C_) < 0.5, 8, 0).astype(np.uint8)
    st = rand_states(rng, C_, pt, t0)
    last = rng.integers(0, 256, (C_, n)).astype(np.uint8)
    pcm = rand_pcm(rng, F_, C_, n)
    g711 = encode_np(orc, pcm, pt, capi.ENC_G191)
    ctl = rand_ctl(rng, F_, C_, 0.2)
    exp = model(st, last, g711, ctl, t0, 20, stride)
    with capi.Context(device=0, max_channels=64) as ctx:
        for form in ("pcm", "g711"):
            d = Dev(st, last, F_, C_, n, stride)
            d.run(ctx, **({"pcm": to_dev(pcm)} if form == "pcm" else {"g711": to_dev(g711)}), ctl=to_dev(ctl), t0=t0)
            check(d.host(), exp, f"n={n} {form}")


def test_tuned_shape_65536x128(orc):
    rng = np.random.default_rng(3)
    C_, F_, t0 = 65536, 128, 10_000
    pt = np.where(np.arange(C_) & 1, 8, 0).astype(np.uint8)
    st = rand_states(rng, C_, pt, t0)
    last = np.zeros((C_, N), np.uint8)
    pcm = rand_pcm(rng, F_, C_, N)
    g711 = encode_np(orc, pcm, pt, capi.ENC_G191)
    ctl = rand_ctl(rng, F_, C_, 0.02)
    exp = model(st, last, g711, ctl, t0, 20, STRIDE)
    with capi.Context(device=0, max_channels=64) as ctx:
        d = Dev(st, last, F_, C_, N, STRIDE)
        d.run(ctx, pcm=to_dev(pcm), ctl=to_dev(ctl), t0=t0)
        check(d.host(), exp, "65536x128")


def test_split_launches(orc):
    rng = np.random.default_rng(11)
    C_, F_, t0 = 1000, 128, 777
    pt = np.where(rng.random(C_) < 0.5, 8, 0).astype(np.uint8)
    st = rand_states(rng, C_, pt, t0)
    last = rng.integers(0, 256, (C_, N)).astype(np.uint8)
    pcm = rand_pcm(rng, F_, C_, N)
    g711 = encode_np(orc, pcm, pt, capi.ENC_SUN16)
    ctl = rand_ctl(rng, F_, C_)
    exp = model(st, last, g711, ctl, t0, 20, STRIDE)
    with capi.Context(device=0, max_channels=64) as ctx:
        d_pcm, d_ctl = to_dev(pcm), to_dev(ctl)
        for parts in (1, 4, 128):
            d = Dev(st, last, F_, C_, N, STRIDE)
            step = F_ // parts
            for f0 in range(0, F_, step):
                d.run(ctx, pcm=d_pcm, ctl=d_ctl, t0=t0, variant=capi.ENC_SUN16, f0=f0, nf=step)
            check(d.host(), exp, f"{parts} parts")


def test_roundtrip_through_depayload(orc):
    torch = torch_cuda()
    rng = np.random.default_rng(5)
    C_, F_, t0 = 2048, 32, 100_000
    pt = np.where(rng.random(C_) < 0.5, 8, 0).astype(np.uint8)
    st = rand_states(rng, C_, pt, t0)
    last = rng.integers(0, 256, (C_, N)).astype(np.uint8)
    pcm = rand_pcm(rng, F_, C_, N)
    g711 = encode_np(orc, pcm, pt, capi.ENC_G191)
    ctl = rand_ctl(rng, F_, C_)
    est, elast, epk, esz, einf = model(st, last, g711, ctl, t0, 20, STRIDE)
    with capi.Context(device=0, max_channels=64) as ctx:
        d = Dev(st, last, F_, C_, N, STRIDE)
        d.run(ctx, pcm=to_dev(pcm), ctl=to_dev(ctl), t0=t0)
        pl, ln, inf = dev_zeros(F_ * C_ * N), dev_zeros(F_ * C_ * 2), dev_zeros(F_ * C_ * 8)
        radio = to_dev(np.ones(C_, np.uint8))
        ctx.depayload(d.pk, d.sizes, radio, C_, F_, STRIDE, N, pl, ln, inf)
        torch.cuda.synchronize()
        rinfo = to_host(inf, capi.RTP_INFO, (F_, C_))
        rpl = to_host(pl, np.uint8, (F_, C_, N))
    sent = esz > 0
    assert np.array_equal(rinfo["ed137"][sent], einf["ed137"][sent])
    assert np.array_equal((rinfo["flags"][sent] & capi.RTP_KEEPALIVE) != 0, (epk[..., 1][sent] & 0x7F) == 123)
    assert np.all(rinfo["flags"][sent] & capi.RTP_ED137_OK)
    # a metered packet (full size, G.711 PT) carries encode(pcm) of its own frame or of the stale source
    met = (esz == 180) & ((epk[..., 1] & 0x7F) != 123)
    assert met.any()
    assert np.array_equal(rpl[met], epk[..., 20:180][met])
    own = met & ((einf["flags"] & capi.TX_STALE_PAYLOAD) == 0)
    assert np.array_equal(rpl[own], g711[own])


def test_two_streams_disjoint_halves(orc):
    torch = torch_cuda()
    rng = np.random.default_rng(9)
    C_, F_, t0 = 4096, 32, 50_000
    pt = np.where(rng.random(C_) < 0.5, 8, 0).astype(np.uint8)
    st = rand_states(rng, C_, pt, t0)
    last = rng.integers(0, 256, (C_, N)).astype(np.uint8)
    g711 = rng.integers(0, 256, (F_, C_, N)).astype(np.uint8)
    ctl = rand_ctl(rng, F_, C_)
    exp = model(st, last, g711, ctl, t0, 20, STRIDE)
    h = C_ // 2
    with capi.Context(device=0, max_channels=64) as ctx:
        d = Dev(st, last, F_, C_, N, STRIDE)
        d_g, d_ctl = to_dev(g711), to_dev(ctl)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        # a launch over channels [c0, c0 + h) of the time-major arrays: one frame per launch (rows of a frame are contiguous)
        for f in range(F_):
            d.run(ctx, g711=d_g, ctl=d_ctl, t0=t0, f0=f, nf=1, c0=0, nc=h, stream=s1.cuda_stream)
            d.run(ctx, g711=d_g, ctl=d_ctl, t0=t0, f0=f, nf=1, c0=h, nc=h, stream=s2.cuda_stream)
        torch.cuda.synchronize()
        check(d.host(), exp, "two streams")


# ---- the compute-free packet writer (igdsp_internal_tx_copy, tools/tx_bench.py --ab) against its promise in csrc/igdsp_capi.hip and
# csrc/igdsp_k_tx.hip: "the same traversal and the same bytes moved as an all-audio igdsp_tx_packetize launch — every packet 20 + n bytes,
# its payload read from the frame's input — no encoder (PCM: the low byte of each sample is stored) and no records"

def run_tx_copy(ctx, C_, F_, n, stride, pcm=None, g711=None, fill=0xA5, guard=256):
    """one launch; returns the packet buffer's bytes with `guard` bytes ahead of and behind the F * C slots"""
    torch = torch_cuda()
    d_pk = dev_zeros(F_ * C_ * stride + 2 * guard, fill)
    d_in = to_dev(pcm if pcm is not None else g711)
    assert d_pk.data_ptr() % 256 == 0 and d_in.data_ptr() % 256 == 0
    rc = capi.internal("tx_copy")(ctx.h, d_in.data_ptr() if pcm is not None else None, d_in.data_ptr() if g711 is not None else None, C_, F_, n,
                                  d_pk.data_ptr() + guard, stride, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return d_pk.cpu().numpy()


@pytest.mark.parametrize("form", ["g711", "pcm"])
@pytest.mark.parametrize("n", [4, 160, 236])
def test_yardstick_packets(n, form):
    """channels at and around a wave's 16 and a block's four groups, frames at and around a chunk's 8, the slot stride 256 and the
    smallest multiple of 4 that holds a packet: the bytes stored are exactly [0, 20 + n) of every slot (nothing past a packet, nothing
    around the buffer); the five header dwords are row * 0x9E3779B9 + o, the payload the G.711 bytes or the low byte of each sample"""
    rng = np.random.default_rng(900 + n + len(form))
    guard = 256
    with capi.Context(device=0, max_channels=64) as ctx:
        _yardstick_packets(ctx, rng, n, form, guard)


def _yardstick_packets(ctx, rng, n, form, guard):
    from tests import gpu_util as gu

    for C_ in (15, 16, 17, 63, 64, 65):
        for F_ in (7, 8, 9):
            for stride in (256, (20 + n + 3) // 4 * 4):
                pcm = rng.integers(-32768, 32768, (F_, C_, n)).astype(np.int16) if form == "pcm" else None
                g711 = rng.integers(0, 256, (F_, C_, n), dtype=np.uint8) if form == "g711" else None
                got = {}

                def run(fill):
                    got[fill] = run_tx_copy(ctx, C_, F_, n, stride, pcm, g711, fill, guard)
                    return {"packets": got[fill]}

                mask = gu.written_mask(run)["packets"]
                assert not mask[:guard].any() and not mask[-guard:].any(), "bytes around the packets written"
                mask = mask[guard:-guard].reshape(F_ * C_, stride)
                assert mask[:, :20 + n].all(), "a packet byte was not stored"
                assert not mask[:, 20 + n:].any(), "bytes past 20 + n of a slot written"
                row = np.arange(F_ * C_, dtype=np.uint64)
                hdr = ((row[:, None] * np.uint64(0x9E3779B9) + np.arange(5, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)).astype("<u4")
                pay = (g711 if pcm is None else (pcm & 0xFF).astype(np.uint8)).reshape(F_ * C_, n)
                for fill in (gu.FILL_A, gu.FILL_B):
                    pk = got[fill][guard:-guard].reshape(F_ * C_, stride)
                    np.testing.assert_array_equal(pk[:, :20].copy().view("<u4"), hdr)
                    np.testing.assert_array_equal(pk[:, 20:20 + n], pay)
