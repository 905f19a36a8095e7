"""-m gpu: igdsp_bss_select (include/igdsp.h, "Best signal selection") bit for bit against tests/bss_model.py — sel, out, stats, the
final state and the final words: fuzz over both input forms, ragged lengths, every gain class, group sizes 1-8 and one of more than
64 members, bad tables, d_mute and start states that are not zero; split invariance on the device; the full-size shape; the chain
from packets through igdsp_depayload; the chain into igdsp_conf_mix; two streams at once; guard bytes and every argument path."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import bss_model as bm  # noqa: E402
from tests import conf_model as cm  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import host_util as hu  # noqa: E402

GUARD = 256
GAINS = np.array([0, 13, 64, 128, 256, 65535], np.uint16)
W = bm.word


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def _dev(a):
    a = np.ascontiguousarray(a)
    return gu.to_dev(a if a.size else np.zeros(4, np.uint8))


def run_bss(ctx, info, ptr, mem, C_, G_, n, state, words, payload=None, codec=None, pcm=None, length=None, gain=None, mute=None, vf=0,
            sel=True, out=True, stats=True, stream=None, F_=None, entry=None, fill=None, raw=None):
    """igdsp_bss_select through the C ABI with guard bytes after every output; returns (sel, out, stats, state, words) (None where not
    asked for).  entry: through that yardstick of capi.INTERNAL_TWIN instead; fill: the byte every output and its guard hold before the
    launch; raw: a dict that takes the whole output buffers' bytes after it."""
    torch = gu.torch_cuda()
    F_ = info.shape[0] if F_ is None else F_
    nm = len(mem)
    audio = payload is not None or pcm is not None
    fsel, fout, fst = (0x3C, 0xA5, 0x5A) if fill is None else (fill,) * 3
    d_sel = gu.dev_zeros(F_ * G_ * 4 + GUARD, fsel) if sel else None
    d_out = gu.dev_zeros(F_ * G_ * n * 2 + GUARD, fout) if out and audio else None
    d_st = gu.dev_zeros(F_ * G_ * 16 + GUARD, fst) if stats and audio else None
    d_state = _dev(np.concatenate([np.ascontiguousarray(state, np.uint32).reshape(-1).view(np.uint8), np.full(GUARD, 0x77, np.uint8)]))
    d_words = _dev(np.concatenate([np.ascontiguousarray(words, np.uint32).view(np.uint8), np.full(GUARD, 0x66, np.uint8)]))
    # (the inputs are named so that they live until the launch is through: a temporary is freed when the call returns, and with
    # two threads the other one's next allocation may take its memory while this launch still reads it)
    d_info, d_ptr, d_mem = _dev(info), _dev(ptr), _dev(mem) if nm else None
    ins = {k: _dev(v) if v is not None else None for k, v in (("payload", payload), ("codec", codec), ("pcm", pcm), ("length", length),
                                                               ("gain", gain), ("mute", mute))}
    (ctx.via(entry) if entry else ctx).bss_select(d_info, d_ptr, d_mem, nm, d_state, d_words if nm else None, C_, G_, F_, n, vote_frames=vf,
                                                  sel=d_sel, out=d_out, stats=d_st, stream=stream, **ins)
    if stream is None:
        torch.cuda.synchronize()
    else:
        ctx.sync(stream)

    def take(d, nbytes, fill, what):
        raw = d.cpu().numpy()
        assert np.all(raw[nbytes:] == fill), f"guard bytes after {what} written"
        return raw[:nbytes]

    s = take(d_sel, F_ * G_ * 4, fsel, "d_sel").view("<i4").reshape(F_, G_) if sel else None
    o = take(d_out, F_ * G_ * n * 2, fout, "d_out").view("<i2").reshape(F_, G_, n) if d_out is not None else None
    r = take(d_st, F_ * G_ * 16, fst, "d_stats").view(capi.FRAME_STATS).reshape(F_, G_) if d_st is not None else None
    st = take(d_state, G_ * 16, 0x77, "d_state").view("<u4").reshape(G_, 4)
    wd = take(d_words, nm * 4, 0x66, "d_words").view("<u4").copy()
    if raw is not None:
        raw.update({k: t.cpu().numpy() for k, t in (("sel", d_sel), ("out", d_out), ("stats", d_st)) if t is not None})
    return s, o, r, st, wd


def random_info(rng, F_, C_, p_open=0.6, nq=32):
    info = np.zeros((F_, C_), capi.RTP_INFO)
    sq = rng.random((F_, C_)) < p_open
    q = rng.integers(0, nq, (F_, C_))
    info["ed137"] = (sq.astype(np.uint32) << 28) | (q.astype(np.uint32) << 3) | rng.integers(0, 8, (F_, C_)).astype(np.uint32) << 29
    info["pt"] = rng.choice([0, 8, 18, 96, 123], (F_, C_), p=[0.6, 0.15, 0.05, 0.05, 0.15])
    info["flags"] = np.where(rng.random((F_, C_)) < 0.08, bm.RTP_RUNT, 0)
    info["payload_len"] = 160
    return info


def random_table(rng, C_, G_, bad=False, wide=False):
    sizes = rng.integers(1, 9, G_)
    if wide:
        sizes[G_ // 2] = 70                                          # one group of more than 64 members
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    mem = rng.integers(0, C_, int(ptr[-1])).astype(np.uint32)
    if bad:
        mem[rng.random(len(mem)) < 0.1] = C_ + rng.integers(0, 5)   # members >= C
        i = int(rng.integers(1, G_ - 1))
        ptr[i] = ptr[i + 1] + 2 if ptr[i + 1] + 2 <= ptr[-1] else ptr[i]   # a descending range
        ptr[-1] = len(mem) + 7                                      # past n_members: clamped
    return ptr, mem


def start_state(rng, G_, ptr, nm):
    st = np.zeros((G_, 4), np.uint32)
    st[:, 0] = rng.choice([0, 1, 7, 0xFFFFFFFF], G_)
    st[:, 1] = rng.integers(0, 10, G_)                              # some name no member of their group
    st[:, 2] = rng.choice([0, 1, 5], G_)
    st[:, 3] = rng.integers(0, 2**32, G_, dtype=np.uint64)
    wd = rng.integers(0, 2**32, nm, dtype=np.uint64).astype(np.uint32)
    return st, wd


@pytest.mark.parametrize("form", ["g711", "pcm"])
@pytest.mark.parametrize("case", range(4))
def test_fuzz(ctx, orc, form, case):
    rng = np.random.default_rng(100 + case + (50 if form == "pcm" else 0))
    C_, G_, F_ = 48, 24, 37
    n = [160, 80, 37, 256][case]
    info = random_info(rng, F_, C_, nq=[32, 2, 32, 4][case])
    ptr, mem = random_table(rng, C_, G_, bad=case >= 2, wide=case in (1, 3))
    st0, wd0 = start_state(rng, G_, ptr, len(mem)) if case % 2 else (np.zeros((G_, 4), np.uint32), np.zeros(len(mem), np.uint32))
    gain = GAINS[rng.integers(0, len(GAINS), C_)] if case != 0 else None
    length = rng.integers(0, n + 3, (F_, C_)).astype(np.uint16) if case in (1, 2) else None
    mute = (rng.random(G_) < 0.2).astype(np.uint8) if case >= 1 else None
    vf = [0, 1, 3, 5][case]
    if form == "g711":
        payload = orc.gen_uniform(F_ * C_ * n, seed=case).reshape(F_, C_, n)
        codec = np.where(rng.random(C_) < 0.5, 8, 0).astype(np.uint8)
        x, kw = cm.decode(payload, codec, orc), dict(payload=payload, codec=codec)
    else:
        pcm = rng.integers(-32768, 32768, (F_, C_, n)).astype(np.int16)
        x, kw = pcm.astype(np.int64), dict(pcm=pcm)
    s, o, r, st, wd = run_bss(ctx, info, ptr, mem, C_, G_, n, st0, wd0, length=length, gain=gain, mute=mute, vf=vf, **kw)
    es, est, ewd = bm.select(info, ptr, mem, len(mem), C_, G_, st0, wd0, vf, mute)
    np.testing.assert_array_equal(s, es)
    np.testing.assert_array_equal(st, est)
    np.testing.assert_array_equal(wd, ewd)
    assert (es >= 0).any() and (es < 0).any()
    eo, ers = bm.emit(es, x, n, gain, length)
    np.testing.assert_array_equal(o, eo)
    gu.assert_stats_equal(r, ers)


def test_sel_only_without_audio(ctx):
    rng = np.random.default_rng(7)
    C_, G_, F_ = 20, 6, 30
    info = random_info(rng, F_, C_)
    ptr, mem = random_table(rng, C_, G_)
    z = np.zeros((G_, 4), np.uint32), np.zeros(len(mem), np.uint32)
    s, o, r, st, wd = run_bss(ctx, info, ptr, mem, C_, G_, 160, *z, vf=2)
    es, est, ewd = bm.select(info, ptr, mem, len(mem), C_, G_, *z, 2)
    assert o is None and r is None
    np.testing.assert_array_equal(s, es)
    np.testing.assert_array_equal(st, est)
    np.testing.assert_array_equal(wd, ewd)


def test_split_invariance_on_the_device(ctx, orc):
    rng = np.random.default_rng(21)
    C_, G_, F_, n = 32, 10, 128, 160
    info = random_info(rng, F_, C_, p_open=0.7, nq=3)
    ptr, mem = random_table(rng, C_, G_)
    payload = orc.gen_uniform(F_ * C_ * n, seed=9).reshape(F_, C_, n)
    codec = np.zeros(C_, np.uint8)
    z = np.zeros((G_, 4), np.uint32), np.zeros(len(mem), np.uint32)
    whole = run_bss(ctx, info, ptr, mem, C_, G_, n, *z, payload=payload, codec=codec, vf=4)
    es, est, ewd = bm.select(info, ptr, mem, len(mem), C_, G_, *z, 4)
    np.testing.assert_array_equal(whole[0], es)
    np.testing.assert_array_equal(whole[3], est)
    for cuts in ([1] * F_, [3, 7, 118]):
        st, wd = z
        sels, outs, recs = [], [], []
        f0 = 0
        for k in cuts:
            s, o, r, st, wd = run_bss(ctx, info[f0:f0 + k], ptr, mem, C_, G_, n, st, wd, payload=payload[f0:f0 + k], codec=codec, vf=4)
            sels.append(s), outs.append(o), recs.append(r)
            f0 += k
        np.testing.assert_array_equal(np.concatenate(sels), whole[0])
        np.testing.assert_array_equal(np.concatenate(outs), whole[1])
        np.testing.assert_array_equal(np.concatenate(recs).view(np.uint8), whole[2].view(np.uint8))
        np.testing.assert_array_equal(st, whole[3])
        np.testing.assert_array_equal(wd, whole[4])


def test_two_parts_in_one_launch(ctx):
    """more frames than one part (kBssPart = 128): the state and the words are carried between the parts"""
    rng = np.random.default_rng(31)
    C_, G_, F_ = 16, 4, 300
    info = random_info(rng, F_, C_, p_open=0.8, nq=2)
    ptr = np.arange(0, C_ + 1, 4, dtype=np.uint32)
    mem = np.arange(C_, dtype=np.uint32)
    z = np.zeros((G_, 4), np.uint32), np.zeros(C_, np.uint32)
    s, _, _, st, wd = run_bss(ctx, info, ptr, mem, C_, G_, 160, *z, vf=3)
    es, est, ewd = bm.select(info, ptr, mem, C_, C_, G_, *z, 3)
    np.testing.assert_array_equal(s, es)
    np.testing.assert_array_equal(st, est)
    np.testing.assert_array_equal(wd, ewd)


def test_full_size(ctx, orc):
    """65 536 channels in 16 384 groups of 4 x 128 frames, G.711: sel, state and words everywhere, out and records on sampled frames"""
    torch = gu.torch_cuda()
    rng = np.random.default_rng(65536)
    C_, m, F_, n = 65536, 4, 128, 160
    G_ = C_ // m
    info = random_info(rng, F_, C_, p_open=0.9, nq=4)
    ptr = np.arange(0, C_ + 1, m, dtype=np.uint32)
    mem = np.arange(C_, dtype=np.uint32)
    codec = np.where(np.arange(C_) % 3 == 0, 8, 0).astype(np.uint8)
    d_pl = torch.randint(0, 256, (F_ * C_ * n,), dtype=torch.uint8, device="cuda")
    d_sel = torch.zeros(F_ * G_, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(F_ * G_ * n, dtype=torch.int16, device="cuda")
    d_st = torch.zeros(F_ * G_ * 16, dtype=torch.uint8, device="cuda")
    d_state = torch.zeros(G_ * 4, dtype=torch.int32, device="cuda")
    d_words = torch.zeros(C_, dtype=torch.int32, device="cuda")
    ctx.bss_select(gu.to_dev(info), gu.to_dev(ptr), gu.to_dev(mem), C_, d_state, d_words, C_, G_, F_, n, payload=d_pl, codec=gu.to_dev(codec),
                   vote_frames=4, sel=d_sel, out=d_out, stats=d_st)
    torch.cuda.synchronize()
    es, est, ewd = bm.select_uniform(info, m, np.zeros((G_, 4), np.uint32), np.zeros(C_, np.uint32), 4)
    np.testing.assert_array_equal(d_sel.cpu().numpy().reshape(F_, G_), es)
    np.testing.assert_array_equal(d_state.cpu().numpy().view(np.uint32).reshape(G_, 4), est)
    np.testing.assert_array_equal(d_words.cpu().numpy().view(np.uint32), ewd)
    assert 0.3 < (es >= 0).mean() < 1.0
    for f in (0, 3, 4, 64, 127):
        pl = d_pl[f * C_ * n:(f + 1) * C_ * n].cpu().numpy().reshape(1, C_, n)
        x = cm.decode(pl, codec, orc)
        eo, er = bm.emit(es[f:f + 1], x, n)
        np.testing.assert_array_equal(d_out[f * G_ * n:(f + 1) * G_ * n].cpu().numpy().reshape(1, G_, n), eo)
        gu.assert_stats_equal(d_st[f * G_ * 16:(f + 1) * G_ * 16].cpu().numpy().view(capi.FRAME_STATS).reshape(1, G_), er)


def test_chain_packets_depayload_bss(ctx, orc):
    """ED-137 packets with squelch / BSS words, R2S keep-alives (PT 123, no payload) and gaps (size 0) through igdsp_depayload"""
    torch = gu.torch_cuda()
    C_, F_, n, stride = 24, 40, 160, 192
    rng = np.random.default_rng(4)
    radio = np.ones(C_, np.uint8)
    codec = np.where(np.arange(C_) % 2 == 0, 8, 0).astype(np.uint8)
    pk = np.zeros((F_, C_, stride), np.uint8)
    sizes = np.zeros((F_, C_), np.uint16)
    body = orc.gen_uniform(F_ * C_ * n, seed=6).reshape(F_, C_, n)
    for f in range(F_):
        for c in range(C_):
            kind = rng.choice(3, p=[0.75, 0.15, 0.1])                 # audio, keep-alive, gap
            if kind == 2:
                continue
            wd = W(rng.random() < 0.7, int(rng.integers(0, 4)))
            pkt = hu.rtp_packet(123 if kind == 1 else int(codec[c]), f, b"" if kind == 1 else bytes(body[f, c]), True, wd)
            pk[f, c, :len(pkt)] = np.frombuffer(pkt, np.uint8)
            sizes[f, c] = len(pkt)
    d_pl, d_len, d_info = gu.dev_zeros(F_ * C_ * n), gu.dev_zeros(F_ * C_ * 2), gu.dev_zeros(F_ * C_ * 8)
    ctx.depayload(gu.to_dev(pk), gu.to_dev(sizes), gu.to_dev(radio), C_, F_, stride, n, d_pl, d_len, d_info)
    torch.cuda.synchronize()
    info = gu.to_host(d_info, capi.RTP_INFO, (F_, C_))
    G_ = C_ // 3
    ptr = np.arange(0, C_ + 1, 3, dtype=np.uint32)
    mem = np.arange(C_, dtype=np.uint32)
    z = np.zeros((G_, 4), np.uint32), np.zeros(C_, np.uint32)
    d_sel, d_out, d_st = gu.dev_zeros(F_ * G_ * 4), gu.dev_zeros(F_ * G_ * n * 2), gu.dev_zeros(F_ * G_ * 16)
    d_state, d_words = _dev(z[0]), _dev(z[1])
    ctx.bss_select(d_info, gu.to_dev(ptr), gu.to_dev(mem), C_, d_state, d_words, C_, G_, F_, n, payload=d_pl, codec=gu.to_dev(codec), length=d_len,
                   vote_frames=2, sel=d_sel, out=d_out, stats=d_st)
    torch.cuda.synchronize()
    epl, elen, _ = orc.depayload(pk, sizes, radio, n)
    assert (info["flags"] & bm.RTP_RUNT).any() and (info["pt"] == 123).any()
    es, _, _ = bm.select(info, ptr, mem, C_, C_, G_, *z, 2)
    np.testing.assert_array_equal(gu.to_host(d_sel, "<i4", (F_, G_)), es)
    eo, er = bm.emit(es, cm.decode(epl, codec, orc), n, None, elen)
    np.testing.assert_array_equal(gu.to_host(d_out, "<i2", (F_, G_, n)), eo)
    gu.assert_stats_equal(gu.to_host(d_st, capi.FRAME_STATS, (F_, G_)), er)


def test_chain_bss_into_conf_mix(ctx, orc):
    """voted groups (PCM out of igdsp_bss_select) mixed into consoles by igdsp_conf_mix with d_pcm"""
    torch = gu.torch_cuda()
    rng = np.random.default_rng(8)
    C_, G_, F_, n = 32, 8, 20, 160
    info = random_info(rng, F_, C_, p_open=0.8, nq=3)
    ptr = np.arange(0, C_ + 1, 4, dtype=np.uint32)
    mem = np.arange(C_, dtype=np.uint32)
    payload = orc.gen_uniform(F_ * C_ * n, seed=12).reshape(F_, C_, n)
    codec = np.zeros(C_, np.uint8)
    z = np.zeros((G_, 4), np.uint32), np.zeros(C_, np.uint32)
    d_out = gu.dev_zeros(F_ * G_ * n * 2)
    ctx.bss_select(gu.to_dev(info), gu.to_dev(ptr), gu.to_dev(mem), C_, _dev(z[0]), _dev(z[1]), C_, G_, F_, n, payload=gu.to_dev(payload),
                   codec=gu.to_dev(codec), vote_frames=2, out=d_out)
    cptr, cmem = capi.conf_build(np.arange(G_), np.arange(G_) // 4, G_, 2)
    cgain = np.full(G_, 128, np.uint16)
    d_mix, d_mst = gu.dev_zeros(F_ * 2 * n * 2), gu.dev_zeros(F_ * 2 * 16)
    ctx.conf_mix(gu.to_dev(cgain), gu.to_dev(cptr), gu.to_dev(cmem), len(cmem), G_, 2, F_, n, out=d_mix, stats=d_mst, pcm=d_out)
    torch.cuda.synchronize()
    es, _, _ = bm.select(info, ptr, mem, C_, C_, G_, *z, 2)
    eo, _ = bm.emit(es, cm.decode(payload, codec, orc), n)
    emix, emst = cm.mix(eo.astype(np.int64), cgain, cptr, cmem, len(cmem), 2)
    np.testing.assert_array_equal(gu.to_host(d_mix, "<i2", (F_, 2, n)), emix)
    gu.assert_stats_equal(gu.to_host(d_mst, capi.FRAME_STATS, (F_, 2)), emst)


def test_two_streams_disjoint_state(ctx, orc):
    torch = gu.torch_cuda()
    C_, G_, F_, n = 40, 10, 24, 160
    cases = []
    for i in range(2):
        rng = np.random.default_rng(40 + i)
        info = random_info(rng, F_, C_, nq=3)
        ptr, mem = random_table(rng, C_, G_)
        cases.append((info, ptr, mem))
    payload = orc.gen_uniform(F_ * C_ * n, seed=13).reshape(F_, C_, n)
    codec = np.full(C_, 8, np.uint8)
    results, errors = [None, None], []

    def worker(i):
        try:
            s = torch.cuda.Stream()
            info, ptr, mem = cases[i]
            for _ in range(3):
                results[i] = run_bss(ctx, info, ptr, mem, C_, G_, n, np.zeros((G_, 4), np.uint32), np.zeros(len(mem), np.uint32),
                                     payload=payload, codec=codec, vf=2, stream=s.cuda_stream)
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
        es, est, ewd = bm.select(info, ptr, mem, len(mem), C_, G_, np.zeros((G_, 4), np.uint32), np.zeros(len(mem), np.uint32), 2)
        s, o, r, st, wd = results[i]
        np.testing.assert_array_equal(s, es)
        np.testing.assert_array_equal(st, est)
        np.testing.assert_array_equal(wd, ewd)
        eo, er = bm.emit(es, x, n)
        np.testing.assert_array_equal(o, eo)
        gu.assert_stats_equal(r, er)


def test_arguments(ctx):
    torch = gu.torch_cuda()
    C_, G_, F_, n = 8, 2, 2, 160
    info = _dev(np.zeros((F_, C_), capi.RTP_INFO))
    ptr, mem = _dev(np.array([0, 4, 8], np.uint32)), _dev(np.arange(8, dtype=np.uint32))
    state, words = gu.dev_zeros(G_ * 16), gu.dev_zeros(8 * 4)
    pl, cd, pcm = gu.dev_zeros(F_ * C_ * n), gu.dev_zeros(C_), gu.dev_zeros(F_ * C_ * n * 2)
    out, st, sel = gu.dev_zeros(F_ * G_ * n * 2 + 8), gu.dev_zeros(F_ * G_ * 16 + 8), gu.dev_zeros(F_ * G_ * 4 + 8)
    L, h = ctx.L, ctx.h

    def call(**kw):
        a = dict(info=info, payload=pl, codec=cd, pcm=None, length=None, gain=None, ptr=ptr, mem=mem, nm=8, mute=None, C=C_, G=G_, F=F_, n=n,
                 vf=0, state=state, words=words, sel=sel, out=out, stats=st)
        a.update(kw)
        p = capi._ptr
        return L.igdsp_bss_select(h, p(a["info"]), p(a["payload"]), p(a["codec"]), p(a["pcm"]), p(a["length"]), p(a["gain"]), p(a["ptr"]),
                                  p(a["mem"]), a["nm"], p(a["mute"]), a["C"], a["G"], a["F"], a["n"], a["vf"], p(a["state"]), p(a["words"]),
                                  p(a["sel"]), p(a["out"]), p(a["stats"]), None)

    EINVAL = -22
    assert call() == 0
    assert call(payload=None, codec=None, pcm=pcm) == 0
    assert call(payload=None, codec=None, out=None, stats=None) == 0                 # sel only
    assert call(sel=None, out=None, stats=None) == 0                                 # state only
    assert call(G=0) == 0 and call(F=0) == 0 and call(G=0, info=None) == 0           # nothing to do
    assert call(info=None) == EINVAL
    assert call(ptr=None) == EINVAL
    assert call(state=None) == EINVAL
    assert call(mem=None) == EINVAL and call(words=None) == EINVAL
    assert call(nm=0, mem=None, words=None) == 0
    assert call(nm=(1 << 24) + 1) == EINVAL
    assert call(pcm=pcm) == EINVAL                                                   # two input forms
    assert call(codec=None) == EINVAL
    assert call(payload=None, codec=None) == EINVAL                                  # out / stats without audio
    assert call(n=0) == EINVAL and call(n=257) == EINVAL
    assert call(stats=capi._ptr(st) + 4) == EINVAL
    assert call(out=capi._ptr(out) + 1) == EINVAL
    assert call(sel=capi._ptr(sel) + 2) == EINVAL
    assert call(info=capi._ptr(info) + 2) == EINVAL
    with pytest.raises(capi.IgdspError):
        ctx.bss_select(info, ptr, mem, 8, None, words, C_, G_, F_, n)
    torch.cuda.synchronize()


# ---- the compute-free yardstick (igdsp_internal_bss_copy, tools/bss_bench.py) against its promise in csrc/igdsp_capi.hip: "the same
# traversal, the same bytes read and written, no decode / scale / clamp / stats / state machine (every non-empty group selects its first
# member); the group state is not touched, the stored words are written as by a launch, and sel / out / stats hold raw bytes"

def _yard_inputs(rng, form, F_, C_, n):
    if form == "g711":
        return dict(payload=rng.integers(0, 256, (F_, C_, n), dtype=np.uint8), codec=np.where(rng.random(C_) < 0.5, 8, 0).astype(np.uint8))
    return dict(pcm=rng.integers(-32768, 32768, (F_, C_, n)).astype(np.int16)) if form == "pcm" else {}


@pytest.mark.parametrize("form", ["g711", "pcm", "none"])
@pytest.mark.parametrize("F_", [3, 131])
def test_yardstick_footprint_and_independence(ctx, form, F_):
    """igdsp_internal_bss_copy, group counts around a wave's, one part and two, the three input forms: it stores the bytes
    igdsp_bss_select stores in sel, out and stats and leaves the stored words as the entry does; the group state is not written, and
    whether it holds zeros or garbage the outputs are the same bytes"""
    rng = np.random.default_rng(800 + F_ + len(form))
    C_, n = 48, 160
    for G_ in (1, 15, 17, 65):
        info = random_info(rng, F_, C_)
        ptr, mem = random_table(rng, C_, G_)
        kw = _yard_inputs(rng, form, F_, C_, n)
        _, wd0 = start_state(rng, G_, ptr, len(mem))
        got = {}

        def launch(entry):
            def run(fill):
                raw = {}
                st0 = np.full((G_, 4), fill * 0x01010101, np.uint32) if entry else np.zeros((G_, 4), np.uint32)
                got[entry, fill] = run_bss(ctx, info, ptr, mem, C_, G_, n, st0, wd0, entry=entry, fill=fill, raw=raw, **kw)
                return raw
            return run

        yard, real = gu.written_mask(launch("bss_copy")), gu.written_mask(launch(None))
        assert all(real[k][:-GUARD].all() for k in real)
        gu.assert_same_footprint(yard, real)
        zero = run_bss(ctx, info, ptr, mem, C_, G_, n, np.zeros((G_, 4), np.uint32), wd0, entry="bss_copy", fill=gu.FILL_A, **kw)
        a, b = got["bss_copy", gu.FILL_A], got["bss_copy", gu.FILL_B]
        assert (a[3].view(np.uint8) == gu.FILL_A).all() and (b[3].view(np.uint8) == gu.FILL_B).all() and not zero[3].any()    # the state as it was
        for x in (b, zero):
            assert all(p is None or p.tobytes() == q.tobytes() for p, q in zip(x[:3], a[:3]))
            np.testing.assert_array_equal(x[4], got[None, gu.FILL_A][4])                                          # the words as the entry's
        first = np.where(ptr[1:] > ptr[:-1], mem[np.minimum(ptr[:-1], len(mem) - 1)].astype(np.int64), -1)
        np.testing.assert_array_equal(a[0], np.broadcast_to(first, (F_, G_)))                                    # sel: the first member


@pytest.mark.parametrize("form", ["g711", "pcm"])
def test_yardstick_reads_the_first_members_rows(ctx, form):
    """one channel's whole row of one frame replaced by fresh random bytes: out (and the raw bytes in the record) of exactly the groups
    whose first member it is change, in that frame; every other output byte is the same.  One d_info record replaced: every output
    byte is the same and the launch completes — the promise says the records are read, but nothing the yardstick stores depends on
    them (the kernel keeps the loads alive through a fold it compares with a constant), and a load that was dropped cannot be seen
    from outside, so this is as far as a test can go."""
    rng = np.random.default_rng(820 + len(form))
    C_, G_, F_, n, f = 48, 65, 3, 160, 1
    info = random_info(rng, F_, C_)
    ptr, mem = random_table(rng, C_, G_)
    kw = _yard_inputs(rng, form, F_, C_, n)
    st0, wd0 = np.zeros((G_, 4), np.uint32), np.zeros(len(mem), np.uint32)
    c = int(mem[ptr[G_ // 2]])
    consumers = [g for g in range(G_) if mem[ptr[g]] == c]
    base = run_bss(ctx, info, ptr, mem, C_, G_, n, st0, wd0, entry="bss_copy", **kw)
    key = "payload" if form == "g711" else "pcm"
    rows = kw[key].copy()
    rows[f, c] = rng.integers(0, 256, n, dtype=np.uint8) if form == "g711" else rng.integers(-32768, 32768, n).astype(np.int16)
    got = run_bss(ctx, info, ptr, mem, C_, G_, n, st0, wd0, entry="bss_copy", **{**kw, key: rows})
    want = np.zeros((F_, G_), bool)
    want[f, consumers] = True
    np.testing.assert_array_equal((got[1] != base[1]).any(axis=2), want)
    rec = lambda r: np.ascontiguousarray(r).view(np.uint8).reshape(F_, G_, 16)   # noqa: E731
    assert got[0].tobytes() == base[0].tobytes() and not (rec(got[2]) != rec(base[2])).any(axis=2)[~want].any()
    info2 = info.copy()
    info2[f, c] = random_info(rng, 1, 1)[0, 0]
    info2["ed137"][f, c] ^= 0x5A5A5A5A
    got = run_bss(ctx, info2, ptr, mem, C_, G_, n, st0, wd0, entry="bss_copy", **kw)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(got[:3], base[:3]))
