"""-m gpu: igdsp_snd_combine / igdsp_snd_split (include/igdsp.h, "Sound-card splitter / combiner") against tests/snd_model.py: bulk data,
sumsq, peak and flags bit for bit, rms at 1e-5 relative against float64.  Every small shape in both directions (the vector form, its
tail where K * n * 2 is no multiple of 16, the general form), misaligned views, the single-output forms, the round trip on the device,
the chains with igdsp_depayload / igdsp_conf_mix / igdsp_hold_update, one full-chip shape per direction against a second statement
computed on the device with torch, two streams at once, guard bytes behind every output and every argument clause."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import conf_model as cm  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import host_util as hu  # noqa: E402
from tests import snd_model as sm  # noqa: E402

GUARD = 256
KS = [1, 2, 3, 5, 6, 7, 8]
NS = [1, 2, 80, 160, 164, 255, 256]
DS = [1, 3, 65, 257]
FS = [1, 3]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def make_pcm(rng, F_, rows, n):
    """random int16 over the full range with rows of all -32768, all 0 and all +-8 planted"""
    pcm = rng.integers(-32768, 32768, (F_, rows, n)).astype(np.int16)
    flat = pcm.reshape(F_ * rows, n)
    if len(flat) >= 4:
        flat[len(flat) // 2] = -32768
        flat[len(flat) // 3] = 0
        flat[-1] = np.where(np.arange(n) & 1, -8, 8)
    return pcm


def run_snd(ctx, direction, src, D_, K_, F_, n, bulk=True, stats=True, in_off=0, out_off=0, stream=None, entry=None, fill=None, raw=None):
    """One direction through the C ABI with guard bytes behind both outputs and the buffers offset by in_off / out_off bytes from a
    256-byte aligned base.  src: the input as int16 (any shape).  Returns (bulk int16 flat | None, stats [F][D * K] | None).  entry:
    through that yardstick of capi.INTERNAL_TWIN instead; fill: the byte both outputs and their surroundings hold before the launch;
    raw: a dict that takes the whole output buffers' bytes after it."""
    torch = gu.torch_cuda()
    nb = F_ * D_ * K_ * n * 2
    fb, fs = (0xA5, 0x5A) if fill is None else (fill, fill)
    d_in = gu.dev_zeros(nb + 64)
    d_in[in_off:in_off + nb] = gu.to_dev(src)
    d_out = gu.dev_zeros(nb + 64 + GUARD, fb) if bulk else None
    d_st = gu.dev_zeros(F_ * D_ * K_ * 16 + GUARD, fs) if stats else None
    assert d_in.data_ptr() % 256 == 0 and (d_out is None or d_out.data_ptr() % 256 == 0)
    c = ctx.via(entry) if entry else ctx
    fn = c.snd_combine if direction == "combine" else c.snd_split
    kw = {("frames" if direction == "combine" else "pcm"): (d_out.data_ptr() + out_off if bulk else None)}
    fn(d_in.data_ptr() + in_off, D_, K_, F_, n, stats=d_st, stream=stream, **kw)
    if stream is None:
        torch.cuda.synchronize()
    else:
        ctx.sync(stream)
    o = s = None
    if bulk:
        b = d_out.cpu().numpy()
        assert np.all(b[:out_off] == fb) and np.all(b[out_off + nb:] == fb), "bytes around the bulk output written"
        o = b[out_off:out_off + nb].copy().view("<i2")
    if stats:
        b = d_st.cpu().numpy()
        assert np.all(b[F_ * D_ * K_ * 16:] == fs), "guard bytes after d_stats written"
        s = b[:F_ * D_ * K_ * 16].view(capi.FRAME_STATS).reshape(F_, D_ * K_)
    if raw is not None:
        raw.update({k: t.cpu().numpy() for k, t in (("bulk", d_out), ("stats", d_st)) if t is not None})
    return o, s


def check_dir(ctx, direction, pcm, D_, K_, **kw):
    """pcm [F][D * K][n]: combine takes it, split takes the model's frames of it; both give the model's other side and records"""
    F_, _, n = pcm.shape
    frames = sm.combine(pcm, D_, K_)
    src, want = (pcm, frames) if direction == "combine" else (frames, pcm)
    o, s = run_snd(ctx, direction, src, D_, K_, F_, n, **kw)
    if o is not None:
        np.testing.assert_array_equal(o, want.reshape(-1))
    if s is not None:
        gu.assert_stats_equal(s, sm.records(pcm))


@pytest.mark.parametrize("K_", KS)
@pytest.mark.parametrize("direction", ["combine", "split"])
def test_small_shapes_vs_model(ctx, direction, K_):
    rng = np.random.default_rng(100 + K_)
    for n in NS:
        for D_ in DS:
            for F_ in FS:
                check_dir(ctx, direction, make_pcm(rng, F_, D_ * K_, n), D_, K_)


def test_shapes_cover_every_form():
    forms = {("general" if (n * k) & 1 else ("vector" if (n * k * 2) % 16 == 0 else "tail")) for n in NS for k in KS}
    assert forms == {"general", "vector", "tail"}


@pytest.mark.parametrize("direction", ["combine", "split"])
def test_alignment(ctx, direction):
    rng = np.random.default_rng(7)
    for K_, n in ((6, 160), (8, 160), (3, 2), (6, 164)):
        pcm = make_pcm(rng, 2, 5 * K_, n)
        for in_off, out_off in ((2, 0), (4, 0), (8, 0), (0, 2), (0, 4), (0, 8), (2, 2), (4, 4), (8, 8), (2, 8), (4, 2)):
            check_dir(ctx, direction, pcm, 5, K_, in_off=in_off, out_off=out_off)
    for K_, n in ((6, 159), (8, 255), (1, 7), (5, 1)):                   # a 16-byte aligned base with an odd n
        check_dir(ctx, direction, make_pcm(rng, 3, 9 * K_, n), 9, K_)


@pytest.mark.parametrize("direction", ["combine", "split"])
def test_single_output_forms(ctx, direction):
    rng = np.random.default_rng(8)
    for K_, n in ((6, 160), (5, 255), (7, 2)):
        pcm = make_pcm(rng, 3, 70 * K_, n)
        check_dir(ctx, direction, pcm, 70, K_, stats=False)               # run_snd checks the guard of what is given
        check_dir(ctx, direction, pcm, 70, K_, bulk=False)


def test_round_trip_on_the_device(ctx):
    torch = gu.torch_cuda()
    rng = np.random.default_rng(9)
    for K_, n, D_, F_ in ((6, 160, 130, 3), (8, 256, 65, 2), (3, 255, 65, 2), (7, 2, 257, 3)):
        pcm = make_pcm(rng, F_, D_ * K_, n)
        nb = pcm.nbytes
        d_x, d_fr, d_y = gu.to_dev(pcm), gu.dev_zeros(nb), gu.dev_zeros(nb)
        d_so, d_si = gu.dev_zeros(F_ * D_ * K_ * 16), gu.dev_zeros(F_ * D_ * K_ * 16, 0xFF)
        ctx.snd_combine(d_x, D_, K_, F_, n, frames=d_fr, stats=d_so)
        ctx.snd_split(d_fr, D_, K_, F_, n, pcm=d_y, stats=d_si)
        torch.cuda.synchronize()
        assert torch.equal(d_x, d_y)
        assert torch.equal(d_so, d_si)                                     # the out VU equals the in VU, byte for byte


def test_chain_depayload_mix_combine(ctx, orc):
    torch = gu.torch_cuda()
    C_, F_, n, stride, D_, K_ = 40, 6, 160, 192, 2, 6
    P_ = D_ * K_
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
    gain = np.array([13, 64, 128, 256], np.uint16)[rng.integers(0, 4, C_)]
    ptr, mem = capi.conf_build(np.arange(C_), np.arange(C_) % (P_ - 1), C_, P_)       # the last port has no members: zeros
    d_mix, d_fr, d_st = gu.dev_zeros(F_ * P_ * n * 2), gu.dev_zeros(F_ * P_ * n * 2 + GUARD, 0xA5), gu.dev_zeros(F_ * P_ * 16)
    ctx.conf_mix(gu.to_dev(gain), gu.to_dev(ptr), gu.to_dev(mem), len(mem), C_, P_, F_, n, out=d_mix, payload=d_pl, codec=gu.to_dev(codec), length=d_len)
    ctx.snd_combine(d_mix, D_, K_, F_, n, frames=d_fr, stats=d_st)
    torch.cuda.synchronize()
    epl, elen, _ = orc.depayload(pk, sizes, radio, n)
    eo, _ = cm.mix(cm.decode(epl, codec, orc), gain, ptr, mem, len(mem), P_, elen)
    raw = d_fr.cpu().numpy()
    assert np.all(raw[F_ * P_ * n * 2:] == 0xA5)
    np.testing.assert_array_equal(raw[:F_ * P_ * n * 2].view("<i2"), sm.combine(eo, D_, K_).reshape(-1))
    gu.assert_stats_equal(gu.to_host(d_st, capi.FRAME_STATS, (F_, P_)), sm.records(eo))
    assert np.all(eo[:, P_ - 1] == 0)


def test_chain_split_mix_and_hold(ctx, orc):
    torch = gu.torch_cuda()
    D_, K_, F_, n = 7, 6, 9, 160
    C_, P_ = D_ * K_, 5
    rng = np.random.default_rng(4)
    mic = make_pcm(rng, F_, C_, n)
    mic[:, 3] //= 4096                                                   # a quiet microphone: SILENT records
    frames = sm.combine(mic, D_, K_)
    d_pcm, d_st = gu.dev_zeros(mic.nbytes), gu.dev_zeros(F_ * C_ * 16)
    ctx.snd_split(gu.to_dev(frames), D_, K_, F_, n, pcm=d_pcm, stats=d_st)
    gain = np.array([13, 64, 128, 256], np.uint16)[rng.integers(0, 4, C_)]
    ptr, mem = capi.conf_build(np.arange(C_), np.arange(C_) % P_, C_, P_)
    d_out, d_ost = gu.dev_zeros(F_ * P_ * n * 2), gu.dev_zeros(F_ * P_ * 16)
    ctx.conf_mix(gu.to_dev(gain), gu.to_dev(ptr), gu.to_dev(mem), len(mem), C_, P_, F_, n, out=d_out, stats=d_ost, pcm=d_pcm)
    d_hold = gu.to_dev(gu.new_hold(C_))
    ctx.hold_update(d_st, C_, F_, n, d_hold)
    torch.cuda.synchronize()
    st = gu.to_host(d_st, capi.FRAME_STATS, (F_, C_))
    gu.assert_stats_equal(st, sm.records(mic))
    assert (st["flags"] & sm.FLAG_SILENT).any()
    eo, es = cm.mix(mic.astype(np.int64), gain, ptr, mem, len(mem), P_)
    np.testing.assert_array_equal(gu.to_host(d_out, "<i2", (F_, P_, n)), eo)
    np.testing.assert_array_equal(gu.to_host(d_ost, capi.FRAME_STATS, (F_, P_))["sumsq"], es["sumsq"])
    # the in VU through the PTT window: the records (checked above) folded by the hold model
    eh = orc.hold_new(C_)
    orc.hold_update(np.ascontiguousarray(st), n, eh)
    gh = gu.to_host(d_hold, capi.CHAN_HOLD)
    for f in capi.CHAN_HOLD.names:
        assert np.array_equal(gh[f], eh[f]), f


@pytest.mark.parametrize("direction", ["combine", "split"])
def test_full_chip_shape(direction):
    """D = 16 384 cards of 6 channels, 4 frames of 160 samples: 63 MB each way, several draws of the persistent loop.  Second
    statement on the device with torch: permute, and integer reductions over the mono rows."""
    torch = gu.torch_cuda()
    D_, K_, F_, n = 16384, 6, 4, 160
    g = torch.Generator(device="cuda").manual_seed(12 if direction == "combine" else 13)
    pcm = torch.randint(-32768, 32768, (F_, D_, K_, n), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
    pcm[0, 5, 2] = -32768
    pcm[1, 7, 0] = 0
    pcm[F_ - 1, D_ - 1, K_ - 1, ::2] = 8
    pcm[F_ - 1, D_ - 1, K_ - 1, 1::2] = -8
    frames = pcm.permute(0, 1, 3, 2).contiguous()
    src, want = (pcm, frames) if direction == "combine" else (frames, pcm)
    nb = pcm.numel() * 2
    d_out = gu.dev_zeros(nb + GUARD, 0xA5)
    d_st = gu.dev_zeros(F_ * D_ * K_ * 16 + GUARD, 0x5A)
    with capi.Context(device=0, max_channels=64) as c:
        (c.snd_combine if direction == "combine" else c.snd_split)(src, D_, K_, F_, n, d_out, d_st)
        torch.cuda.synchronize()
    assert torch.equal(d_out[:nb].view(torch.int16), want.reshape(-1))
    assert bool((d_out[nb:] == 0xA5).all()) and bool((d_st[F_ * D_ * K_ * 16:] == 0x5A).all())
    x = pcm.reshape(F_, D_ * K_, n).to(torch.int64)
    st = d_st[:F_ * D_ * K_ * 16].cpu().numpy().view(capi.FRAME_STATS).reshape(F_, D_ * K_)
    sumsq = (x * x).sum(dim=2).cpu().numpy()
    peak = x.abs().amax(dim=2).cpu().numpy()
    np.testing.assert_array_equal(st["sumsq"], sumsq.astype(np.uint64))
    np.testing.assert_array_equal(st["peak"], peak.astype(np.uint16))
    np.testing.assert_array_equal(st["flags"], np.where(peak <= 8, sm.FLAG_SILENT, 0).astype(np.uint8))
    assert np.all(st["byte_mean"] == 0)
    ref = np.sqrt(sumsq.astype(np.float64) / n)
    assert np.all(np.abs(st["rms"].astype(np.float64) - ref) <= 1e-5 * ref + 1e-30)
    assert st[0, 5 * K_ + 2]["peak"] == 32768 and st[0, 5 * K_ + 2]["sumsq"] == n * 32768 ** 2
    assert st[1, 7 * K_]["flags"] == sm.FLAG_SILENT and st[F_ - 1, -1]["flags"] == sm.FLAG_SILENT and st[F_ - 1, -1]["peak"] == 8


def test_two_streams_from_two_threads(ctx):
    torch = gu.torch_cuda()
    rng = np.random.default_rng(11)
    D_, K_, F_, n = 300, 6, 4, 160
    pcms = [make_pcm(rng, F_, D_ * K_, n) for _ in range(2)]
    dirs = ["combine", "split"]
    srcs = [pcms[0], sm.combine(pcms[1], D_, K_)]
    serial = [run_snd(ctx, dirs[i], srcs[i], D_, K_, F_, n) for i in range(2)]
    results, errors = [None, None], []

    def worker(i):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(3):
                    results[i] = run_snd(ctx, dirs[i], srcs[i], D_, K_, F_, n, stream=s.cuda_stream)
        except Exception as e:                                          # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for i in range(2):
        assert results[i][0].tobytes() == serial[i][0].tobytes() and results[i][1].tobytes() == serial[i][1].tobytes()
    np.testing.assert_array_equal(serial[0][0], sm.combine(pcms[0], D_, K_).reshape(-1))
    np.testing.assert_array_equal(serial[1][0], pcms[1].reshape(-1))


# every clause of the argument rule (csrc/igdsp_args.h: snd_rule), in order, through the library: (overrides, code, error text or None)
ARG_ROWS = [
    (dict(), 0, None),
    (dict(ctx=None), -22, None),
    (dict(src=None), -22, None),
    (dict(bulk=None, st=None), -22, None),
    (dict(bulk=None), 0, None),
    (dict(st=None), 0, None),
    (dict(K=0), -22, None),
    (dict(K=9), -22, None),
    (dict(n=0), -22, None),
    (dict(n=257), -22, None),
    (dict(D=0x10000000, F=3), -34, None),                               # D * K * F = 18 * 2^28: past the row limit
    (dict(D=0x80000000, K=8, F=1), -34, None),                          # D * K alone wraps 32 bits
    (dict(D=0x10000000, F=3, n=0), -22, None),                          # a bad n wins over too many rows
    (dict(D=0x10000000, F=3, K=9), -22, None),                          # and so does a bad K
    (dict(src_off=1), -22, None),
    (dict(bulk_off=1), -22, None),
    (dict(st_off=4), -22, None),
    (dict(D=0x10000000, F=3, src_off=1), -34, None),                    # too many rows wins over the alignment
    (dict(alias=True), -22, "the output must not be the input"),
    (dict(alias=True, st_off=4), -22, None),                            # the alignment wins over the aliasing
    # nothing to do, whatever the rest
    (dict(D=0), 0, None),
    (dict(F=0), 0, None),
    (dict(D=0, src=None, bulk=None, st=None, K=0, n=0), 0, None),
    (dict(F=0, alias=True, K=99), 0, None),
]


@pytest.mark.parametrize("entry", ["igdsp_snd_combine", "igdsp_snd_split", "igdsp_internal_snd_copy"])
def test_argument_clauses(ctx, entry):
    """(the yardstick takes igdsp_snd_combine's rule and name, and also rejects a NULL bulk output)"""
    if entry == "igdsp_internal_snd_copy":
        return _argument_clauses(ctx, capi.internal(entry), "igdsp_snd_combine", [(o, -22 if o == dict(bulk=None) else c, t) for o, c, t in ARG_ROWS])
    return _argument_clauses(ctx, getattr(ctx.L, entry), entry, ARG_ROWS)


def _argument_clauses(ctx, fn, entry, rows):
    torch = gu.torch_cuda()
    L = ctx.L
    D_, K_, F_, n = 3, 6, 2, 160
    nb = F_ * D_ * K_ * n * 2
    src = gu.dev_zeros(nb + 64, 1)
    out, st = gu.dev_zeros(nb + 64, 0xA5), gu.dev_zeros(F_ * D_ * K_ * 16 + 64, 0x5A)
    for over, code, text in rows:
        a = dict(ctx=ctx.h, src=src.data_ptr(), bulk=out.data_ptr(), st=st.data_ptr(), D=D_, K=K_, F=F_, n=n, src_off=0, bulk_off=0, st_off=0, alias=False)
        a.update(over)
        p_src = a["src"] + a["src_off"] if a["src"] else None
        p_bulk = p_src if a["alias"] else (a["bulk"] + a["bulk_off"] if a["bulk"] else None)
        p_st = a["st"] + a["st_off"] if a["st"] else None
        launches = code == 0 and a["D"] and a["F"] and a["ctx"]
        if not launches:
            torch.cuda.synchronize()
            before = (src.cpu().numpy().copy(), out.cpu().numpy().copy(), st.cpu().numpy().copy())
        rc = fn(a["ctx"], p_src, a["D"], a["K"], a["F"], a["n"], p_bulk, p_st, None)
        assert rc == code, (entry, over, rc)
        if text is not None:
            assert L.igdsp_last_error(ctx.h).decode() == f"{entry}: {text}", over
        torch.cuda.synchronize()
        if not launches:                                                  # a rejected call, or nothing to do, writes nothing
            after = (src.cpu().numpy(), out.cpu().numpy(), st.cpu().numpy())
            assert all(np.array_equal(x, y) for x, y in zip(before, after)), over
    assert np.all(out.cpu().numpy()[nb:] == 0xA5) and np.all(st.cpu().numpy()[F_ * D_ * K_ * 16:] == 0x5A)


def test_snd_vu_of_device_records(ctx):
    rng = np.random.default_rng(21)
    pcm = make_pcm(rng, 2, 12, 160)
    _, s = run_snd(ctx, "combine", pcm, 2, 6, 2, 160, bulk=False)
    for rec in s.reshape(-1):
        vu = capi.snd_vu(rec)
        p, db = sm.snd_vu(rec["rms"])
        assert vu["percent"] == p and abs(vu["db"] - db) <= 1e-9


# ---- the compute-free yardstick (igdsp_internal_snd_copy, tools/snd_bench.py) against its promise in csrc/igdsp_capi_snd.hip: "the
# same items, the same bytes read and written in memory order, no transpose and no records; d_out is required and d_stats is not
# written"

@pytest.mark.parametrize("K_", KS)
@pytest.mark.parametrize("direction", ["combine", "split"])
def test_yardstick_footprint_and_values(ctx, direction, K_):
    """igdsp_internal_snd_copy with the arguments of either direction, D x F = 1, 31, 33, 65 items (a block takes 32), n of the vector
    form, its tail and (K n odd) the general form: it stores the bulk bytes the direction stores, none of d_stats, and the bulk output is
    the input, byte for byte"""
    rng = np.random.default_rng(300 + K_)
    for D_, F_ in ((1, 1), (31, 1), (11, 3), (65, 1)):
        for n in (160, 164, 3):
            src = make_pcm(rng, F_, D_ * K_, n)
            got = {}

            def yard(fill):
                raw = {}
                got[fill] = run_snd(ctx, direction, src, D_, K_, F_, n, entry="snd_copy", fill=fill, raw=raw)
                return raw

            def real(fill):
                raw = {}
                run_snd(ctx, direction, src, D_, K_, F_, n, fill=fill, raw=raw)
                return raw

            gu.assert_same_footprint(gu.written_mask(yard), gu.written_mask(real), not_written=("stats",))
            for fill in (gu.FILL_A, gu.FILL_B):
                np.testing.assert_array_equal(got[fill][0], src.reshape(-1))
    for in_off, out_off in ((2, 0), (0, 2), (8, 8)):                      # misaligned bases: the general form and the tail
        src = make_pcm(rng, 2, 5 * K_, 160)
        o, s = run_snd(ctx, direction, src, 5, K_, 2, 160, entry="snd_copy", in_off=in_off, out_off=out_off, fill=0xEE)
        np.testing.assert_array_equal(o, src.reshape(-1))
        assert (s.view(np.uint8) == 0xEE).all()
