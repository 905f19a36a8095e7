"""-m gpu: igdsp_conf_mix (include/igdsp.h, "Conference mix") bit for bit against tests/conf_model.py: both input forms, ragged
lengths, every gain class, bad tables, the narrow and the wide (block-split) form, full-size shapes with a second statement computed
on the device by torch, the depayload -> mix chain, two streams at once, guard bytes and every argument path."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import conf_model as cm  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import host_util as hu  # noqa: E402

GUARD = 256
GAINS = np.array([0, 13, 64, 128, 256, 65535], np.uint16)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def _dev(a):
    a = np.ascontiguousarray(a)
    return gu.to_dev(a if a.size else np.zeros(4, np.uint8))


def run_mix(ctx, C_, P_, F_, n, gain, ptr, mem, payload=None, codec=None, pcm=None, length=None, n_members=None, out=True, stats=True,
            stream=None, entry=None, fill=None, raw=None):
    """igdsp_conf_mix through the C ABI with guard bytes after both outputs; returns (out [F][P][n] | None, stats [F][P] | None).
    entry: through that yardstick of capi.INTERNAL_TWIN instead; fill: the byte both outputs and their guards hold before the launch;
    raw: a dict that takes the whole output buffers' bytes after it."""
    torch = gu.torch_cuda()
    nm = len(mem) if n_members is None else n_members
    fo, fs = (0xA5, 0x5A) if fill is None else (fill, fill)
    d_out = gu.dev_zeros(F_ * P_ * n * 2 + GUARD, fo) if out else None
    d_st = gu.dev_zeros(F_ * P_ * 16 + GUARD, fs) if stats else None
    args = dict(payload=_dev(payload) if payload is not None else None, codec=_dev(codec) if codec is not None else None,
                pcm=_dev(pcm) if pcm is not None else None, length=_dev(length) if length is not None else None)
    (ctx.via(entry) if entry else ctx).conf_mix(_dev(gain), _dev(ptr), _dev(mem) if nm else None, nm, C_, P_, F_, n, out=d_out, stats=d_st,
                                                stream=stream, **args)
    if stream is None:
        torch.cuda.synchronize()
    else:
        ctx.sync(stream)
    o = s = None
    if out:
        b = d_out.cpu().numpy()
        assert np.all(b[F_ * P_ * n * 2:] == fo), "guard bytes after d_out written"
        o = b[:F_ * P_ * n * 2].view("<i2").reshape(F_, P_, n)
    if stats:
        b = d_st.cpu().numpy()
        assert np.all(b[F_ * P_ * 16:] == fs), "guard bytes after d_stats written"
        s = b[:F_ * P_ * 16].view(capi.FRAME_STATS).reshape(F_, P_)
    if raw is not None:
        raw.update({k: t.cpu().numpy() for k, t in (("out", d_out), ("stats", d_st)) if t is not None})
    return o, s


def check(o, s, eo, es, frames=None):
    fr = slice(None) if frames is None else frames
    if o is not None:
        np.testing.assert_array_equal(o[fr], eo)
    if s is not None:
        s = s[fr]
        for k in ("sumsq", "peak", "byte_mean", "flags"):
            np.testing.assert_array_equal(s[k], es[k], err_msg=k)
        ref = es["rms"].astype(np.float64)
        assert np.all(np.abs(s["rms"].astype(np.float64) - ref) <= 1e-5 * ref + 1e-30)


def _decode_any(orc, payload, codec, pcm):
    return cm.decode(payload, codec, orc) if payload is not None else pcm.astype(np.int64)


def _bad_table(rng, C_, P_):
    """ragged ports incl. empty ones, a wide port (> kConfWideMin members), duplicates, members >= C, a descending port_ptr and
    port_ptr values past n_members"""
    sizes = rng.integers(0, 9, P_)
    sizes[rng.integers(0, P_)] = 0
    sizes[1] = 300                                                      # the block-split form
    mem = np.concatenate([rng.integers(0, C_ + 6, s) for s in sizes]).astype(np.uint32)   # members >= C included
    mem[:4] = mem[0]                                                    # a duplicate
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    ptr[P_ - 2] = ptr[P_ - 1] + 3                                       # port P-3 longer, port P-2 descending
    ptr[P_] = ptr[P_] + 50                                              # clamped to n_members
    return ptr, mem


@pytest.mark.parametrize("n", [1, 80, 160, 164, 256])
@pytest.mark.parametrize("form", ["g711", "pcm"])
def test_fuzz_vs_model(ctx, orc, n, form):
    rng = np.random.default_rng(n * 7 + len(form))
    C_, P_, F_ = 48, 12, 5
    codec = np.where(rng.integers(0, 2, C_) == 1, 8, 0).astype(np.uint8)
    payload = pcm = None
    if form == "g711":
        payload = rng.integers(0, 256, (F_, C_, n), dtype=np.uint8)
    else:
        pcm = rng.integers(-32768, 32768, (F_, C_, n)).astype(np.int16)
        pcm.reshape(-1)[::17] = -32768
        pcm.reshape(-1)[::19] = 32767
    length = np.where(rng.integers(0, 4, (F_, C_)) == 0, rng.integers(0, n + 1, (F_, C_)), n).astype(np.uint16)
    length[:, 5] = 0                                                    # keep-alive zeros
    length[2, :] = 0                                                    # a frame of nothing but keep-alives
    gain = GAINS[rng.integers(0, len(GAINS), C_)]
    ptr, mem = _bad_table(rng, C_, P_)
    x = _decode_any(orc, payload, codec, pcm)
    eo, es = cm.mix(x, gain, ptr, mem, len(mem), P_, length)
    assert (es["flags"] & cm.FLAG_SATURATED).any() and (es["flags"] & cm.FLAG_EMPTY).any()
    o, s = run_mix(ctx, C_, P_, F_, n, gain, ptr, mem, payload=payload, codec=codec, pcm=pcm, length=length)
    check(o, s, eo, es)
    # without d_len every member is full length; each output alone
    eo, es = cm.mix(x, gain, ptr, mem, len(mem), P_)
    o, _ = run_mix(ctx, C_, P_, F_, n, gain, ptr, mem, payload=payload, codec=codec, pcm=pcm, stats=False)
    _, s = run_mix(ctx, C_, P_, F_, n, gain, ptr, mem, payload=payload, codec=codec, pcm=pcm, out=False)
    check(o, s, eo, es)


def test_truncation_and_clamps_on_device(ctx):
    # the hand cases of tests/test_conf_cpu.py, through the kernel: -3 * 13 / 128 -> 0, -129 * 1 / 128 -> -1; 2 x 32767 at 256 -> 32767
    n, C_ = 4, 6
    pcm = np.array([[[-3, 3, -129, 129], [-129, -128, 127, 0], [32767, 32767, -32768, 1], [32767, 32767, -32768, 1],
                     [-32768, -32768, 0, 0], [-32768, -32768, 0, 0]]], np.int16)
    gain = np.array([13, 1, 256, 256, 128, 128], np.uint16)
    ptr = np.array([0, 1, 2, 4, 6], np.uint32)
    mem = np.arange(6, dtype=np.uint32)
    o, s = run_mix(ctx, C_, 4, 1, n, gain, ptr, mem, pcm=pcm)
    assert o[0, 0].tolist() == [0, 0, -13, 13]
    assert o[0, 1].tolist() == [-1, -1, 0, 0]
    assert o[0, 2].tolist() == [32767, 32767, -32768, 4]
    assert s[0, 2]["flags"] & capi.FLAG_SATURATED and s[0, 2]["peak"] == 32768
    assert o[0, 3].tolist() == [-32768, -32768, 0, 0] and s[0, 3]["flags"] & capi.FLAG_SATURATED   # only the final clamp fired
    assert not s[0, 0]["flags"] & capi.FLAG_SATURATED


def test_identity_equals_decode_meter(ctx, orc):
    torch = gu.torch_cuda()
    C_, F_, n = 128, 6, 160
    codec = np.where(np.arange(C_) % 3 == 0, 8, 0).astype(np.uint8)
    payload = orc.gen_uniform(F_ * C_ * n).reshape(F_, C_, n)
    d_st, d_pcm = gu.dev_zeros(F_ * C_ * 16), gu.dev_zeros(F_ * C_ * n * 2)
    ctx.decode_meter(gu.to_dev(payload), gu.to_dev(codec), C_, F_, n, d_st, pcm=d_pcm)
    torch.cuda.synchronize()
    pcm = gu.to_host(d_pcm, "<i2", (F_, C_, n))
    dst = gu.to_host(d_st, capi.FRAME_STATS, (F_, C_))
    o, s = run_mix(ctx, C_, C_, F_, n, np.full(C_, 128, np.uint16), np.arange(C_ + 1, dtype=np.uint32), np.arange(C_, dtype=np.uint32),
                   payload=payload, codec=codec)
    assert o.tobytes() == pcm.tobytes()
    for k in ("sumsq", "peak"):
        np.testing.assert_array_equal(s[k], dst[k], err_msg=k)
    # rms: the definition sqrtf((float)sumsq / n) here; the tuned n == 160 meter evaluates it as sqrt(sumsq / 16 * 0.1f), within
    # 4e-7 of the definition (csrc/igdsp_device.h pack_stats160) — both inside the 1e-5 contract
    ref = np.sqrt(dst["sumsq"].astype(np.float64) / n)
    assert np.all(np.abs(s["rms"] - ref) <= 1e-5 * ref) and np.all(np.abs(s["rms"] - dst["rms"]) <= 1e-6 * ref)


def _torch_sumsq(payload, codec, gain, ptr, mem, P_, orc, chunk=4):
    """second statement on the device: decode, scale, index_add_ per port in int64, clamp, sum of squares — [F][P] uint64"""
    torch = gu.torch_cuda()
    F_, C_, n = payload.shape
    tab = torch.from_numpy(np.stack([orc.decode_table(0), orc.decode_table(8)]).astype(np.int64)).cuda()
    law = torch.from_numpy((codec == 8).astype(np.int64)).cuda()
    g = torch.from_numpy(gain.astype(np.int64)).cuda()
    cnt = np.diff(np.minimum(ptr.astype(np.int64), len(mem)))
    port_of = torch.from_numpy(np.repeat(np.arange(P_), np.maximum(cnt, 0))).cuda()
    m = torch.from_numpy(mem.astype(np.int64)).cuda()
    d_pl = torch.from_numpy(payload).cuda()
    res = []
    for f0 in range(0, F_, chunk):
        pl = d_pl[f0:f0 + chunk].long()                                  # [f][C][n]
        x = tab[law[None, :, None].expand_as(pl), pl]
        a = torch.clamp(torch.div(x * g[None, :, None], 128, rounding_mode="trunc"), -32768, 32767)
        S = torch.zeros((pl.shape[0], P_, n), dtype=torch.int64, device="cuda")
        S.index_add_(1, port_of, a[:, m, :])
        o = torch.clamp(S, -32768, 32767)
        res.append((o * o).sum(dim=2).cpu().numpy())
        del pl, x, a, S, o
    return np.concatenate(res).astype(np.uint64)


def _shape(name, rng):
    """the measured shapes of tools/conf_bench.py (B1-B5): (C, P, F, channel list, port list)"""
    if name == "B1":
        C_, P_ = 65536, 8192
        return C_, P_, 128, np.arange(C_), np.arange(C_) // 8
    if name == "B2":
        C_, P_ = 65536, 8192
        return C_, P_, 128, rng.permutation(C_), np.arange(C_) // 8
    if name == "B3":
        C_, P_ = 65536, 16384
        ch = np.concatenate([np.arange(C_), np.arange(C_)])
        return C_, P_, 128, ch, np.concatenate([np.arange(C_) // 8, (np.arange(C_) // 8 + P_ // 2) % P_])
    if name == "B4":
        C_, P_ = 65536, 16
        return C_, P_, 128, np.arange(C_), np.arange(C_) // 4096
    return 4, 5, 2, np.repeat(np.arange(4), 5), np.tile(np.arange(5), 4)   # B5


@pytest.mark.parametrize("name", ["B1", "B2", "B3", "B4", "B5"])
def test_full_size_shapes(orc, name):
    rng = np.random.default_rng(ord(name[1]))
    C_, P_, F_, ch, pt = _shape(name, rng)
    n = 160
    ptr, mem = capi.conf_build(ch, pt, C_, P_)
    codec = np.where(rng.integers(0, 2, C_) == 1, 8, 0).astype(np.uint8)
    gain = GAINS[1:][rng.integers(0, len(GAINS) - 1, C_)]
    gain[::7] = 0
    payload = orc.gen_uniform(F_ * C_ * n, seed=0x5EED + ord(name[1])).reshape(F_, C_, n)
    with capi.Context(device=0, max_channels=64) as c:
        o, s = run_mix(c, C_, P_, F_, n, gain, ptr, mem, payload=payload, codec=codec)
    frames = sorted({0, F_ // 2, F_ - 1})
    x = cm.decode(payload[frames], codec, orc)
    eo, es = cm.mix(x, gain, ptr, mem, len(mem), P_)
    check(o, s, eo, es, frames=frames)
    np.testing.assert_array_equal(s["sumsq"], _torch_sumsq(payload, codec, gain, ptr, mem, P_, orc))


def test_skew_one_port_of_everything_and_a_random_wide_port(ctx, orc):
    C_, F_, n = 65536, 3, 160
    payload = np.full((F_, C_, n), 0x80, np.uint8)                      # mu-law +32124 everywhere
    payload[1, :, ::2] = 0x00                                           # -32124 on even samples of frame 1
    codec = np.zeros(C_, np.uint8)
    gain = np.full(C_, 128, np.uint16)
    with capi.Context(device=0, max_channels=64) as c:
        o, s = run_mix(c, C_, 1, F_, n, gain, np.array([0, C_], np.uint32), np.arange(C_, dtype=np.uint32), payload=payload, codec=codec)
    assert np.all(o[0] == 32767) and np.all(s["flags"] & capi.FLAG_SATURATED)
    assert np.all(o[1, 0, ::2] == -32768) and s[0, 0]["sumsq"] == 160 * 32767 ** 2
    rng = np.random.default_rng(9)
    mem = rng.permutation(C_)[:4096].astype(np.uint32)
    payload = orc.gen_uniform(F_ * C_ * n, seed=77).reshape(F_, C_, n)
    codec = np.where(rng.integers(0, 2, C_) == 1, 8, 0).astype(np.uint8)
    gain = GAINS[rng.integers(0, len(GAINS), C_)]
    ptr = np.array([0, 3, 4096], np.uint32)                             # a narrow port and a wide one, random order
    o, s = run_mix(ctx, C_, 2, F_, n, gain, ptr, mem, payload=payload, codec=codec)
    eo, es = cm.mix(cm.decode(payload, codec, orc), gain, ptr, mem, len(mem), 2)
    check(o, s, eo, es)


def test_chain_depayload_keepalives_then_mix(ctx, orc):
    torch = gu.torch_cuda()
    C_, F_, n, stride = 40, 6, 160, 192
    rng = np.random.default_rng(3)
    radio = (np.arange(C_) % 2).astype(np.uint8)
    codec = np.where(np.arange(C_) % 3 == 0, 8, 0).astype(np.uint8)
    pk = np.zeros((F_, C_, stride), np.uint8)
    sizes = np.zeros((F_, C_), np.uint16)
    body = orc.gen_uniform(F_ * C_ * n, seed=5).reshape(F_, C_, n)
    for f in range(F_):
        for c in range(C_):
            keep = rng.integers(0, 4) == 0
            pkt = hu.rtp_packet(123 if keep else int(codec[c]), f, b"" if keep else bytes(body[f, c]), bool(radio[c]), 1234 + c)
            pk[f, c, :len(pkt)] = np.frombuffer(pkt, np.uint8)
            sizes[f, c] = len(pkt)
    d_pl, d_len, d_info = gu.dev_zeros(F_ * C_ * n), gu.dev_zeros(F_ * C_ * 2), gu.dev_zeros(F_ * C_ * 8)
    ctx.depayload(gu.to_dev(pk), gu.to_dev(sizes), gu.to_dev(radio), C_, F_, stride, n, d_pl, d_len, d_info)
    gain = GAINS[rng.integers(0, len(GAINS), C_)]
    ptr, mem = capi.conf_build(np.arange(C_), np.arange(C_) // 5, C_, 8)
    d_out, d_st = gu.dev_zeros(F_ * 8 * n * 2), gu.dev_zeros(F_ * 8 * 16)
    ctx.conf_mix(gu.to_dev(gain), gu.to_dev(ptr), gu.to_dev(mem), len(mem), C_, 8, F_, n, out=d_out, stats=d_st, payload=d_pl, codec=gu.to_dev(codec),
                 length=d_len)
    torch.cuda.synchronize()
    epl, elen, _ = orc.depayload(pk, sizes, radio, n)
    assert (elen == 0).any()
    eo, es = cm.mix(cm.decode(epl, codec, orc), gain, ptr, mem, len(mem), 8, elen)
    check(gu.to_host(d_out, "<i2", (F_, 8, n)), gu.to_host(d_st, capi.FRAME_STATS, (F_, 8)), eo, es)


def test_two_streams_two_tables(ctx, orc):
    torch = gu.torch_cuda()
    C_, F_, n = 64, 20, 160
    payload = orc.gen_uniform(F_ * C_ * n, seed=11).reshape(F_, C_, n)
    codec = np.where(np.arange(C_) & 1, 8, 0).astype(np.uint8)
    x = cm.decode(payload, codec, orc)
    tables = [capi.conf_build(np.arange(C_), np.arange(C_) // 4, C_, 16), capi.conf_build(np.arange(C_)[::-1], np.arange(C_) % 3, C_, 3)]
    gains = [np.full(C_, 256, np.uint16), np.full(C_, 13, np.uint16)]
    results, errors = [None, None], []

    def worker(i):
        try:
            s = torch.cuda.Stream()
            ptr, mem = tables[i]
            P_ = len(ptr) - 1
            for _ in range(3):
                results[i] = run_mix(ctx, C_, P_, F_, n, gains[i], ptr, mem, payload=payload, codec=codec, stream=s.cuda_stream)
        except Exception as e:                                          # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for i in range(2):
        ptr, mem = tables[i]
        eo, es = cm.mix(x, gains[i], ptr, mem, len(mem), len(ptr) - 1)
        check(*results[i], eo, es)


def test_argument_paths(ctx):
    torch = gu.torch_cuda()
    L, h = ctx.L, ctx.h
    C_, P_, F_, n = 8, 2, 2, 160
    pl, cd, pcm = gu.dev_zeros(F_ * C_ * n), gu.dev_zeros(C_), gu.dev_zeros(F_ * C_ * n * 2)
    g, ptr, mem = gu.to_dev(np.full(C_, 128, np.uint16)), gu.to_dev(np.array([0, 4, 8], np.uint32)), gu.to_dev(np.arange(C_, dtype=np.uint32))
    out, st = gu.dev_zeros(F_ * P_ * n * 2 + 64, 0xA5), gu.dev_zeros(F_ * P_ * 16 + 64, 0x5A)
    P = lambda t, o=0: t.data_ptr() + o                                 # noqa: E731

    def call(ctx_h=h, payload=P(pl), codec=P(cd), pcm_=None, length=None, gain=P(g), pp=P(ptr), mm=P(mem), nm=8, c=C_, p=P_, f=F_, nn=n,
             o=P(out), s=P(st)):
        return L.igdsp_conf_mix(ctx_h, payload, codec, pcm_, length, gain, pp, mm, nm, c, p, f, nn, o, s, None)

    assert call() == 0
    assert call(ctx_h=None) == -22
    assert call(pcm_=P(pcm)) == -22                                     # both inputs
    assert call(payload=None) == -22                                    # neither
    assert call(codec=None) == -22                                      # G.711 without codec
    assert call(o=None, s=None) == -22
    assert call(gain=None) == -22 and call(pp=None) == -22 and call(mm=None) == -22
    assert call(nn=0) == -22 and call(nn=257) == -22
    assert call(o=P(out, 1)) == -22 and call(s=P(st, 4)) == -22 and call(pp=P(ptr, 2)) == -22 and call(mm=P(mem, 1)) == -22
    assert call(payload=None, codec=None, pcm_=P(pcm, 1)) == -22 and call(gain=P(g, 1)) == -22 and call(length=P(out, 1)) == -22
    assert call(c=0x10000, f=0x10000) == -34 and call(p=0x10000, f=0x10000) == -34
    torch.cuda.synchronize()
    before = (out.cpu().numpy().copy(), st.cpu().numpy().copy())
    # no-ops: nothing to write, whatever the pointers
    assert call(p=0) == 0 and call(f=0) == 0
    assert call(p=0, payload=None, codec=None, gain=None, pp=None, mm=None, o=None, s=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), before[0]) and np.array_equal(st.cpu().numpy(), before[1])
    # n_members == 0 with NULL members: every port empty
    assert call(mm=None, nm=0) == 0
    torch.cuda.synchronize()
    s = gu.to_host(st, capi.FRAME_STATS)[:F_ * P_]
    assert np.all(s["flags"] == capi.FLAG_EMPTY) and np.all(gu.to_host(out, "<i2")[:F_ * P_ * n] == 0)
    # C == 0: no member is a channel
    assert call(c=0) == 0
    torch.cuda.synchronize()
    assert np.all(gu.to_host(st, capi.FRAME_STATS)[:F_ * P_]["flags"] == capi.FLAG_EMPTY)
    assert np.all(out.cpu().numpy()[F_ * P_ * n * 2:] == 0xA5) and np.all(st.cpu().numpy()[F_ * P_ * 16:] == 0x5A)


# ---- the compute-free yardstick (igdsp_internal_conf_copy, tools/conf_bench.py) against its promise in csrc/igdsp_capi.hip: "the
# same traversal, the same bytes read and written, no decode / scale / clamp / stats"

def _yard_case(rng, C_, P_, F_, n, form, wide=None):
    """a table of unique members (every port lists 0 .. 6 channels, port `wide` 130), full gains but for two muted channels, d_len with
    short and empty rows"""
    sizes = rng.integers(0, 7, P_)
    if wide is not None:
        sizes[wide] = 130
    chan = np.concatenate([rng.choice(C_, k, replace=False) for k in sizes] + [np.zeros(0, np.int64)]).astype(np.uint32)
    port = np.repeat(np.arange(P_), sizes).astype(np.uint32)
    ptr, mem = cm.build(chan, port, C_, P_)
    gain = GAINS[rng.integers(1, len(GAINS), C_)]
    gain[[C_ // 3, C_ // 2]] = 0
    length = np.where(rng.integers(0, 4, (F_, C_)) == 0, rng.integers(0, n + 1, (F_, C_)), n).astype(np.uint16)
    codec = np.where(rng.integers(0, 2, C_) == 1, 8, 0).astype(np.uint8)
    kw = dict(payload=rng.integers(0, 256, (F_, C_, n), dtype=np.uint8), codec=codec) if form == "g711" else \
        dict(pcm=rng.integers(-32768, 32768, (F_, C_, n)).astype(np.int16))
    return gain, ptr, mem, length, kw


YARD_ITEMS = [(1, 1), (5, 3), (16, 1), (17, 1), (11, 3)]                   # P x F = 1, 15, 16, 17, 33 items: a block takes 16 at a time


@pytest.mark.parametrize("form", ["g711", "pcm"])
@pytest.mark.parametrize("n", [1, 160, 164])
def test_yardstick_footprint(ctx, n, form):
    """igdsp_internal_conf_copy stores exactly the bytes igdsp_conf_mix stores on the same arguments: every port-frame's row and record,
    narrow ports and a block-wide one, and nothing behind them"""
    rng = np.random.default_rng(500 + n + len(form))
    for P_, F_ in YARD_ITEMS + [(3, 2)]:
        C_ = 140
        gain, ptr, mem, length, kw = _yard_case(rng, C_, P_, F_, n, form, wide=1 if (P_, F_) == (3, 2) else None)

        def launch(entry):
            def run(fill):
                raw = {}
                run_mix(ctx, C_, P_, F_, n, gain, ptr, mem, length=length, entry=entry, fill=fill, raw=raw, **kw)
                return raw
            return run

        yard, real = gu.written_mask(launch("conf_copy")), gu.written_mask(launch(None))
        assert real["out"][:F_ * P_ * n * 2].all() and real["stats"][:F_ * P_ * 16].all()
        gu.assert_same_footprint(yard, real)


@pytest.mark.parametrize("form", ["g711", "pcm"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_yardstick_reads_every_member_row(ctx, form, wide):
    """one member channel's whole row of one frame replaced by fresh random bytes (not complemented: the fold is an xor): the output
    rows of exactly the ports that list the channel change, in that frame; every other output byte is the same.  Once through the
    narrow form, once for a port of 130 members (> kConfWideMin: the block splits the list)"""
    rng = np.random.default_rng(520 + len(form) + wide)
    C_, P_, F_, n = 140, 11, 3, 160
    gain, ptr, mem, length, kw = _yard_case(rng, C_, P_, F_, n, form, wide=4 if wide else None)
    f = 1
    lists = [mem[ptr[p]:ptr[p + 1]] for p in range(P_)]
    pool = lists[4] if wide else np.concatenate([lists[p] for p in range(P_) if p != 4])
    c = int(next(x for x in pool if gain[x] and (wide or x not in lists[4])))
    length[f, c] = n
    consumers = [p for p in range(P_) if c in lists[p]]
    assert consumers and (4 in consumers) == wide and (len(lists[4]) == 130) == wide
    base = run_mix(ctx, C_, P_, F_, n, gain, ptr, mem, length=length, entry="conf_copy", **kw)
    key = "payload" if form == "g711" else "pcm"
    rows = kw[key].copy()
    rows[f, c] = rng.integers(0, 256, n, dtype=np.uint8) if form == "g711" else rng.integers(-32768, 32768, n).astype(np.int16)
    assert (rows[f, c] != kw[key][f, c]).any()
    got = run_mix(ctx, C_, P_, F_, n, gain, ptr, mem, length=length, entry="conf_copy", **{**kw, key: rows})
    changed = (got[0] != base[0]).any(axis=2)
    want = np.zeros((F_, P_), bool)
    want[f, consumers] = True
    np.testing.assert_array_equal(changed, want)
    assert got[1].tobytes() == base[1].tobytes()                            # the records do not depend on the samples
    again = run_mix(ctx, C_, P_, F_, n, gain, ptr, mem, length=length, entry="conf_copy", **kw)
    assert again[0].tobytes() == base[0].tobytes() and again[1].tobytes() == base[1].tobytes()
