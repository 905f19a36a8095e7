"""-m gpu: igdsp_resample (include/igdsp.h, "Rate converter") against tests/rs_model.py through the C ABI: outputs, sumsq, peak, flags and
the state bit for bit, rms at 1e-5 relative against float64.  Shapes around the kernel's ownership units (UP: a wave owns 16 channels,
a block 64; DOWN: a wave 4, a block 16), frames so that the history spans several rows, every factor, both directions, both layouts,
both forms (16-byte pieces; the sample-granular one for odd n and 2-byte aligned bases), G.711 of both laws, short and empty rows, row
strides with canaries, the single-output forms, one launch against split launches, the argument clauses, full-chip shapes (the only
ones where a wave keeps a channel for several frames) and the chain into igdsp_conf_mix beside a 16 kHz tone port."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import conf_model as cm  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import rs_model as rm  # noqa: E402
from tests import tone_model as tm  # noqa: E402

GUARD = 256
EINVAL, ERANGE = -22, -34
SIZES = (1, 7, 8, 23, 24, 25, 160, 255, 256)
UP_CH, DOWN_CH = (1, 15, 16, 17, 63, 64, 65), (1, 3, 4, 5, 15, 16, 17)     # +-1 around a wave's and a block's channels


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def strided(rows, stride):
    """rows [frames][C][len] -> [frames][stride][len] of the same type with 0xEE bytes in the foreign rows"""
    fr, C_, ln = rows.shape
    buf = np.empty((fr, stride, ln), rows.dtype)
    buf.view(np.uint8)[:] = 0xEE
    buf[:, :C_] = rows
    return buf


def run_rs(ctx, direction, R, layout, rows, n, codec=None, length=None, hist=None, rn=0, rw=0, off=0, out=True, stats=True, d_state=None,
           entry=None, fill=0xEE, raw=None):
    """One launch through the C ABI (entry: through that yardstick of capi.INTERNAL_TWIN instead; fill: the byte the outputs and their
    surroundings hold before the launch; raw: a dict that takes the whole output buffers' bytes after it).  rows: the input as laid out ([F][C][n] int16 or G.711 uint8 for UP; the wide side for DOWN).  The
    input rows, d_len and the output sit in strided buffers whose foreign rows and surroundings hold 0xEE, the input and the output
    `off` bytes behind a 256-byte aligned base.  Returns (out as laid out [frames][C][len] | None, stats | None, state [C], the state
    tensor)."""
    torch = gu.torch_cuda()
    fr_in, C_, len_in = rows.shape
    F_ = fr_in // (R if direction == rm.DOWN and layout == rm.SUBFRAMES else 1)
    g711 = rows.dtype == np.uint8
    s_in, s_out = ((rn, rw) if direction == rm.UP else (rw, rn))
    s_in, s_out = s_in or C_, s_out or C_
    fr_out = F_ * (R if direction == rm.UP and layout == rm.SUBFRAMES else 1)
    len_out = n * R if direction == rm.UP and layout == rm.ROWS else n
    d_in = gu.dev_zeros(fr_in * s_in * len_in * rows.itemsize + 64, 0xEE)
    d_in[off:off + fr_in * s_in * len_in * rows.itemsize] = gu.to_dev(strided(rows, s_in))
    d_len = gu.to_dev(strided(np.asarray(length, np.uint16)[:, :, None], s_in)) if length is not None else None
    d_codec = gu.to_dev(np.asarray(codec, np.uint8)) if g711 else None
    if d_state is None:
        st = np.zeros(C_, capi.RS_STATE)
        if hist is not None:
            st["hist"] = hist
        st["flags"], st["frames"] = 0xA5, 0xFFFFFFFE
        d_state = gu.to_dev(st)
    nb = fr_out * s_out * len_out * 2
    d_out = gu.dev_zeros(nb + 64 + GUARD, fill) if out else None
    d_st = gu.dev_zeros(fr_out * C_ * 16 + GUARD, fill) if stats else None
    assert d_in.data_ptr() % 256 == 0 and (d_out is None or d_out.data_ptr() % 256 == 0)
    (ctx.via(entry) if entry else ctx).resample(direction, R, d_state, C_, F_, n, layout=layout, payload=d_in.data_ptr() + off if g711 else None, codec=d_codec,
                 pcm=None if g711 else d_in.data_ptr() + off, length=d_len, rows_narrow=rn, rows_wide=rw,
                 out=d_out.data_ptr() + off if out else None, stats=d_st)
    torch.cuda.synchronize()
    o = s = None
    if out:
        b = d_out.cpu().numpy()
        assert np.all(b[:off] == fill) and np.all(b[off + nb:] == fill), "bytes around the rows written"
        o = b[off:off + nb].copy().view("<i2").reshape(fr_out, s_out, len_out)
        assert np.all(o[:, C_:].view(np.uint8) == fill), "rows outside [0, C) written"
        o = o[:, :C_]
    if stats:
        b = d_st.cpu().numpy()
        assert np.all(b[fr_out * C_ * 16:] == fill), "bytes after d_stats written"
        s = b[:fr_out * C_ * 16].view(capi.FRAME_STATS).reshape(fr_out, C_)
    if raw is not None:
        raw.update({k: t.cpu().numpy() for k, t in (("out", d_out), ("stats", d_st), ("state", d_state)) if t is not None})
    return o, s, d_state.cpu().numpy().view(capi.RS_STATE), d_state


def make_input(rng, direction, R, layout, C_, F_, n, g711=False, loud=False):
    """(rows as laid out, the same decoded to int64, codec | None)"""
    if direction == rm.UP:
        shape = (F_, C_, n)
    else:
        shape = (F_ * R, C_, n) if layout == rm.SUBFRAMES else (F_, C_, n * R)
    if g711:
        rows = rng.integers(0, 256, shape).astype(np.uint8)
        codec = rng.choice([0, 8, 8, 0, 96], C_).astype(np.uint8)
        return rows, rm.decode(rows, codec), codec
    rows = (rng.choice([-32768, 32767], shape) if loud else rng.integers(-32768, 32768, shape)).astype(np.int16)
    return rows, rows.astype(np.int64), None


def check_launch(ctx, rng, direction, R, layout, C_, F_, n, g711=False, loud=False, with_len=False, **kw):
    rows, dec, codec = make_input(rng, direction, R, layout, C_, F_, n, g711, loud)
    length = None
    if with_len:
        length = rng.integers(0, rows.shape[2] + 40, rows.shape[:2])      # short rows, rows past their size, and
        length[rng.random(rows.shape[:2]) < 0.2] = 0                        # empty ones
    hist = rng.integers(-32768, 32768, (C_, 144)).astype(np.int16)
    o, s, st, _ = run_rs(ctx, direction, R, layout, rows, n, codec=codec, length=length, hist=hist, **kw)
    eo, es, eh = rm.launch(direction, R, layout, dec, hist, length)
    if o is not None:
        np.testing.assert_array_equal(o, eo)
    if s is not None:
        gu.assert_stats_equal(s, es)
    np.testing.assert_array_equal(st["hist"], eh)
    assert (st["frames"] == (0xFFFFFFFE + F_) % 2 ** 32).all() and (st["flags"] == 0xA5).all()
    return s


@pytest.mark.parametrize("R", rm.FACTORS)
@pytest.mark.parametrize("direction", (rm.UP, rm.DOWN), ids=("up", "down"))
def test_small_shapes_vs_model(ctx, direction, R):
    """every n, both layouts, channels around a wave's and a block's, F in 1 / 2 / 3 / 7: at small n the history of a frame spans
    several earlier rows and the state"""
    rng = np.random.default_rng(10 * R + direction)
    chans = UP_CH if direction == rm.UP else DOWN_CH
    k = 0
    for n in SIZES:
        for layout in (rm.ROWS, rm.SUBFRAMES):
            for F_ in (1, 2, 3, 7):
                check_launch(ctx, rng, direction, R, layout, chans[k % len(chans)], F_, n)
                k += 1
    for C_ in chans:                                                       # and every channel count at the sizes of both forms
        check_launch(ctx, rng, direction, R, rm.SUBFRAMES, C_, 3, 160)
        check_launch(ctx, rng, direction, R, rm.ROWS, C_, 2, 25)


@pytest.mark.parametrize("R", rm.FACTORS)
def test_g711_input_both_laws(ctx, R):
    rng = np.random.default_rng(20 + R)
    for n, C_, F_, layout in ((160, 17, 3, rm.ROWS), (8, 65, 7, rm.SUBFRAMES), (255, 5, 2, rm.ROWS), (1, 16, 7, rm.SUBFRAMES), (24, 33, 3, rm.ROWS)):
        check_launch(ctx, rng, rm.UP, R, layout, C_, F_, n, g711=True)
        check_launch(ctx, rng, rm.UP, R, layout, C_, F_, n, g711=True, with_len=True)


@pytest.mark.parametrize("R", rm.FACTORS)
@pytest.mark.parametrize("direction", (rm.UP, rm.DOWN), ids=("up", "down"))
def test_len_strides_offsets_and_loud_input(ctx, direction, R):
    """short and empty rows; row strides on both sides; bases 2, 8 and 16 bytes off (the first two take the sample-granular form);
    full-scale input"""
    rng = np.random.default_rng(30 * R + direction)
    for layout in (rm.ROWS, rm.SUBFRAMES):
        for n in (160, 25, 8):
            check_launch(ctx, rng, direction, R, layout, 19, 3, n, with_len=True)
            check_launch(ctx, rng, direction, R, layout, 19, 2, n, rn=23, rw=31)
            check_launch(ctx, rng, direction, R, layout, 5, 2, n, rn=5, rw=6, with_len=True, off=2)
        check_launch(ctx, rng, direction, R, layout, 17, 2, 160, off=8)
        check_launch(ctx, rng, direction, R, layout, 17, 2, 160, off=16, rn=18)
        check_launch(ctx, rng, direction, R, layout, 9, 3, 160, loud=True)
        check_launch(ctx, rng, direction, R, layout, 9, 2, 7, loud=True)


@pytest.mark.parametrize("R", rm.FACTORS)
def test_saturating_input_sets_the_flag(ctx, R):
    """the taps' signs times +-32767 in a window: the output clamps at either end and the row's record says so; the other rows do not"""
    up, down = rm.up_table(R), rm.down_table(R)
    p = int(np.abs(up).sum(axis=1).argmax())
    for direction, layout, n in ((rm.UP, rm.ROWS, 160), (rm.UP, rm.SUBFRAMES, 25), (rm.DOWN, rm.ROWS, 160), (rm.DOWN, rm.SUBFRAMES, 25)):
        n_in = n if direction == rm.UP else n * R
        x = np.zeros((2, 3, n_in), np.int64)                              # [F][C][n_in] in the row layout; channel 1 stays silent
        g = n - 1
        if direction == rm.UP:
            x[1, 0, g - np.arange(24)] = np.where(up[p] < 0, -32767, 32767)
            x[1, 2, g - np.arange(24)] = -np.where(up[p] < 0, -32767, 32767)
        else:
            w = np.where(down < 0, -32767, 32767)
            stream = np.zeros((3, 2 * n_in), np.int64)
            stream[0, n_in + g * R + R - 1 - np.arange(24 * R)] = w
            stream[2, n_in + g * R + R - 1 - np.arange(24 * R)] = -w
            x = stream.reshape(3, 2, n_in).transpose(1, 0, 2)
        rows = x.astype(np.int16)
        if direction == rm.DOWN and layout == rm.SUBFRAMES:
            rows = rm.rows_to_sub(rows, R)
        o, s, _, _ = run_rs(ctx, direction, R, layout, rows, n)
        eo, es, _ = rm.launch(direction, R, layout, rows.astype(np.int64))
        np.testing.assert_array_equal(o, eo)
        gu.assert_stats_equal(s, es)
        sat = (s["flags"] & rm.FLAG_SATURATED) != 0
        assert sat[:, 0].any() and sat[:, 2].any() and not sat[:, 1].any()
        assert o.max() == 32767 and o.min() == -32768


def test_single_output_forms(ctx):
    rng = np.random.default_rng(40)
    for direction, R, layout, n in ((rm.UP, 2, rm.SUBFRAMES, 160), (rm.DOWN, 6, rm.ROWS, 160), (rm.UP, 3, rm.ROWS, 7), (rm.DOWN, 4, rm.SUBFRAMES, 25)):
        check_launch(ctx, rng, direction, R, layout, 21, 3, n, stats=False)
        check_launch(ctx, rng, direction, R, layout, 21, 3, n, out=False)


def test_one_launch_against_split_launches(ctx):
    rng = np.random.default_rng(50)
    for direction, R, layout, n in ((rm.UP, 2, rm.SUBFRAMES, 160), (rm.UP, 6, rm.ROWS, 8), (rm.DOWN, 3, rm.ROWS, 25), (rm.DOWN, 6, rm.SUBFRAMES, 160),
                                    (rm.DOWN, 4, rm.SUBFRAMES, 1)):
        C_, F_ = 21, 9
        rows, _, _ = make_input(rng, direction, R, layout, C_, F_, n)
        hist = rng.integers(-32768, 32768, (C_, 144)).astype(np.int16)
        whole = run_rs(ctx, direction, R, layout, rows, n, hist=hist)
        per = R if direction == rm.DOWN and layout == rm.SUBFRAMES else 1     # input rows per frame
        for cuts in ((1, 8), (4, 5), (1,) * 9, (2, 3, 4)):
            d_state, outs, recs, at = None, [], [], 0
            for k in cuts:
                o, s, st, d_state = run_rs(ctx, direction, R, layout, rows[at * per:(at + k) * per], n, hist=hist, d_state=d_state)
                outs.append(o), recs.append(s)
                at += k
            np.testing.assert_array_equal(np.concatenate(outs), whole[0])
            assert np.concatenate(recs).tobytes() == whole[1].tobytes()
            np.testing.assert_array_equal(st["hist"], whole[2]["hist"])
            assert (st["frames"] == whole[2]["frames"]).all()


def test_argument_errors(ctx):
    L = capi.load()
    d_state = gu.dev_zeros(4 * 296 + 64)
    d_pcm, d_len, d_cd = gu.dev_zeros(2 * 4 * 960 * 2 + 64), gu.dev_zeros(64), gu.dev_zeros(64)
    d_out, d_st = gu.dev_zeros(2 * 4 * 960 * 2 + 64, 0xEE), gu.dev_zeros(2 * 4 * 6 * 16, 0xEE)
    stt, pcm, ln, cd, out, st = (t.data_ptr() for t in (d_state, d_pcm, d_len, d_cd, d_out, d_st))

    def call(direction=0, R=2, layout=0, payload=None, codec=None, pcm_=pcm, len_=None, state=stt, C_=4, F_=2, n=160, rn=0, rw=0, out_=out, st_=st, h=ctx.h):
        return L.igdsp_resample(h, direction, R, layout, payload, codec, pcm_, len_, state, C_, F_, n, rn, rw, out_, st_, None)

    assert call(h=None) == EINVAL
    for kw in (dict(direction=2), dict(R=1), dict(R=5), dict(R=0), dict(R=8), dict(layout=2)):          # checked even with nothing to do
        assert call(**kw) == EINVAL and call(C_=0, **kw) == EINVAL, kw
    assert call(C_=0, pcm_=None, state=None, out_=None, st_=None, n=0) == 0 and call(F_=0, n=999) == 0  # nothing to do comes next
    for kw in (dict(pcm_=None), dict(payload=pcm, codec=cd), dict(payload=pcm, pcm_=None), dict(direction=1, payload=pcm, codec=cd, pcm_=None),
               dict(direction=1, payload=pcm, codec=cd), dict(state=None), dict(out_=None, st_=None), dict(rn=3), dict(rw=3), dict(n=0), dict(n=257),
               dict(pcm_=pcm + 1), dict(len_=ln + 1), dict(out_=out + 1), dict(st_=st + 4), dict(state=stt + 2), dict(out_=pcm), dict(out_=stt),
               dict(st_=stt), dict(len_=out)):
        assert call(**kw) == EINVAL, kw
    assert call(C_=0x10000000, F_=16) == ERANGE and call(rw=0x10000000, F_=16) == ERANGE and call(rn=0x10000000, F_=16) == ERANGE
    assert call(C_=0x08000000, F_=16, layout=1) == ERANGE and call(C_=0x10000000, F_=16, n=0) == EINVAL
    assert call(out_=pcm) == EINVAL and b"an output must not be an input or the state" in (L.igdsp_last_error(ctx.h) or b"")
    gu.torch_cuda().cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xEE).all() and (d_st.cpu().numpy() == 0xEE).all() and not d_state.cpu().numpy().any()   # nothing written
    assert call(payload=pcm, codec=cd, pcm_=None) == 0 and call(direction=1, R=6, layout=1) == 0 and call(len_=ln, out_=None) == 0
    gu.torch_cuda().cuda.synchronize()


FULL_CHIP = [  # (direction, R, layout, n, F, G.711 input, d_len, row strides)
    (rm.UP, 2, rm.SUBFRAMES, 160, 7, False, False, False), (rm.UP, 6, rm.ROWS, 8, 9, False, False, False), (rm.UP, 3, rm.ROWS, 7, 9, True, True, False),
    (rm.UP, 4, rm.SUBFRAMES, 24, 9, True, True, True), (rm.DOWN, 6, rm.SUBFRAMES, 160, 7, False, False, False),
    (rm.DOWN, 2, rm.ROWS, 8, 9, False, False, False), (rm.DOWN, 3, rm.SUBFRAMES, 25, 7, False, True, False), (rm.DOWN, 4, rm.ROWS, 16, 9, False, True, True),
]


@pytest.mark.parametrize("direction,R,layout,n,F_,g711,with_len,strides", FULL_CHIP)
def test_full_chip(ctx, direction, R, layout, n, F_, g711, with_len, strides):
    """2 051 / 2 058 channel groups, a sixth of the items rs_route wants on 256 CUs (fewer CUs: fewer cuts), so the frames are cut into
    chunks of two or more: a wave keeps its channels for several frames and moves the tile's tail to its front; with n = 7 .. 25 the
    tail spans several rows.  Every factor; G.711, d_len and row strides ride along in some.  The channels repeat 509 rows of data (a
    prime: no ownership unit divides it)."""
    rng = np.random.default_rng(60 + R)
    C_ = 2048 * (16 if direction == rm.UP else 4) + 37
    base, dec, codec = make_input(rng, direction, R, layout, 509, F_, n, g711=g711)
    hist = rng.integers(-32768, 32768, (509, 144)).astype(np.int16)
    length = None
    if with_len:
        length = rng.integers(0, base.shape[2] + 9, base.shape[:2])
        length[rng.random(base.shape[:2]) < 0.2] = 0
    idx = np.arange(C_) % 509
    o, s, st, _ = run_rs(ctx, direction, R, layout, base[:, idx], n, codec=codec[idx] if g711 else None, length=length[:, idx] if with_len else None,
                         hist=hist[idx], rn=C_ + 3 if strides else 0, rw=C_ + 5 if strides else 0)
    eo, es, eh = rm.launch(direction, R, layout, dec, hist, length)
    np.testing.assert_array_equal(o, eo[:, idx])
    gu.assert_stats_equal(s, es[:, idx])
    np.testing.assert_array_equal(st["hist"], eh[idx])


def test_up_beside_a_16k_tone_into_conf_mix(ctx):
    """the chain at a 16 kHz bridge, one tick of 160 narrow samples = 2 sub-frames of 160 wide samples: the calls' G.711 rows go UP by 2 in
    the sub-frame layout into rows [0, C) of a [2][C + P][160] array, a tone port built at 16 000 Hz with samples_per_frame 160 writes
    rows [C, C + P) of the same array, igdsp_conf_mix reads it with n_channels = C + P and F = 2: the composition of the three models"""
    torch = gu.torch_cuda()
    rng = np.random.default_rng(70)
    C_, P_, n, R = 6, 2, 160, 2
    rows, dec, codec = make_input(rng, rm.UP, R, rm.SUBFRAMES, C_, 1, n, g711=True)
    hist = rng.integers(-32768, 32768, (C_, 144)).astype(np.int16)
    plan = tm.plan_build([(440, 480, 2000, 1000)], 16000)
    pos = np.array([0, 31900])
    d_all, d_len = gu.dev_zeros(2 * (C_ + P_) * n * 2, 0xEE), gu.to_dev(np.full((2, C_ + P_), n, np.uint16))
    st = np.zeros(C_, capi.RS_STATE)
    st["hist"] = hist
    ctx.resample(rm.UP, R, gu.to_dev(st), C_, 1, n, layout=rm.SUBFRAMES, payload=gu.to_dev(rows), codec=gu.to_dev(codec), rows_wide=C_ + P_, out=d_all)
    ts = np.zeros(P_, capi.TONE_STATE)
    ts["pos"], ts["flags"] = pos, tm.PLAYING
    d_plan = gu.to_dev(np.array([tm.plan_record(plan, capi.TONE_PLAN)], capi.TONE_PLAN))
    ctx.tone_generate(d_plan, 1, gu.to_dev(ts), P_, 2, n, rows_per_frame=C_ + P_, pcm=d_all.data_ptr() + C_ * n * 2)
    chan = np.array([0, 1, 2, 3, 4, 5, C_, C_ + 1, 0], np.uint32)          # consoles 0, 1 hear a call and a tone; 2 .. 5 a call; 6 two calls
    port = np.array([0, 1, 2, 3, 4, 5, 0, 1, 6], np.uint32)
    chan, port = np.append(chan, 1).astype(np.uint32), np.append(port, 6).astype(np.uint32)
    ptr, mem = cm.build(chan, port, C_ + P_, 7)
    gain = np.full(C_ + P_, 128, np.uint16)
    d_out, d_st = gu.dev_zeros(2 * 7 * n * 2), gu.dev_zeros(2 * 7 * 16)
    ctx.conf_mix(gu.to_dev(gain), gu.to_dev(ptr), gu.to_dev(mem), len(mem), C_ + P_, 7, 2, n, out=d_out, stats=d_st, pcm=d_all, length=d_len)
    torch.cuda.synchronize()
    wide, _, _ = rm.launch(rm.UP, R, rm.SUBFRAMES, dec, hist)             # [2][C][160]
    tone_rows, _, _, _, _ = tm.generate([plan], None, None, pos, np.full(P_, tm.PLAYING), 2, n)
    both = np.concatenate([wide, tone_rows], axis=1)
    np.testing.assert_array_equal(d_all.cpu().numpy().view("<i2").reshape(2, C_ + P_, n), both)
    eo, es = cm.mix(both.astype(np.int64), gain, ptr, mem, len(mem), 7, length=np.full((2, C_ + P_), n))
    np.testing.assert_array_equal(d_out.cpu().numpy().view("<i2").reshape(2, 7, n), eo)
    s = d_st.cpu().numpy().view(capi.FRAME_STATS).reshape(2, 7)
    for k in ("sumsq", "peak", "flags"):
        np.testing.assert_array_equal(s[k], es[k], err_msg=k)


# ---- the compute-free yardstick (igdsp_internal_rs_copy, tools/rs_bench.py) against its promise: csrc/igdsp_capi_rs.hip and the head
# of csrc/igdsp_k_rs.hip.  "The same items, loads, tile traffic and stores, an xor in place of the filter, zero records; d_out is
# required, the state is neither read nor written."

def rs_chunk_frames(direction, R, C_, F_, cus, blocks=None):
    """rs_route's frames per chunk (csrc/igdsp_route.h), restated: a wave keeps its channels for this many frames"""
    up = direction == rm.UP
    ch, u = (16, 1) if up else (4, R)
    lds = 4 * ch * ((24 * u + 256 * u) * 2 + R * 16) + (1024 if up else 0)
    per_cu = blocks if blocks is not None and 1 <= blocks <= 8 else min(3, 163840 // (lds + 16))
    want, groups = max(1, cus) * per_cu * 4 * 4, -(-C_ // ch)
    cuts = 1 if groups >= want else min(F_, -(-want // groups))
    return -(-F_ // cuts)


def rs_copy_model(direction, R, layout, rows, n, length=None, codec=None, chunk_frames=1, vec=True):
    """What the yardstick stores, from the input rows as laid out.  Per channel and frame the tile holds the 24 (UP) / 24 R (DOWN)
    samples ahead of the frame, the frame's samples and zeros up to the last unit's end; unit q folds the 32 (32 R) tile samples from
    8 q (8 R q) on: x[d & 3] ^= E[d] over its dwords, i.e. output sample i of the unit is the xor of the tile samples i, i + 8, ...; UP
    stores the eight samples R times.  The samples ahead of a chunk's first frame are the earlier rows' (decoded, cut at d_len; zeros
    ahead of the launch), those ahead of a later frame are the tile's own tail.  A G.711 row in the vector form is not decoded: its 8
    code bytes are stored as 4 samples, twice."""
    up = direction == rm.UP
    u = 1 if up else R
    SI = R if (not up and layout == rm.SUBFRAMES) else 1
    fr_in, C_, LI = rows.shape
    F_, n_in, HIST, pieces, g711 = fr_in // SI, n * u, 24 * u, (n + 7) // 8, rows.dtype == np.uint8
    valid = np.arange(LI)[None, None, :] < (np.full(rows.shape[:2], LI) if length is None else np.asarray(length))[:, :, None]
    D = W = np.where(valid, rm.decode(rows, codec) if g711 else rows.astype(np.int64), 0)
    if g711 and vec:
        b = rows.astype(np.int64)
        w = (b[..., 0::2] | b[..., 1::2] << 8).reshape(fr_in, C_, LI // 8, 4)
        W = np.where(valid, np.concatenate([w, w], axis=-1).reshape(fr_in, C_, LI), 0)
    stream = lambda x: (x.reshape(F_, SI, C_, LI).transpose(0, 2, 1, 3).reshape(F_, C_, n_in) & 0xFFFF).astype(np.uint16)   # noqa: E731
    D, W = stream(D), stream(W)
    n_rep = R if up else 1
    y = np.zeros((F_, C_, pieces * 8 * n_rep), np.uint16)
    tile = None
    for f in range(F_):
        if f % chunk_frames == 0:
            ahead = np.concatenate([np.zeros((C_, HIST), np.uint16)] + [D[g] for g in range(max(0, f - HIST), f)], axis=1)[:, -HIST:]
        else:
            ahead = tile[:, n_in:n_in + HIST]
        tile = np.concatenate([ahead, W[f], np.zeros((C_, pieces * 8 * u - n_in), np.uint16)], axis=1)
        for q in range(pieces):
            fold = np.bitwise_xor.reduce(tile[:, q * 8 * u:q * 8 * u + 32 * u].reshape(C_, 4 * u, 8), axis=1)
            y[f, :, q * 8 * n_rep:(q + 1) * 8 * n_rep] = np.tile(fold, (1, n_rep))
    n_out = n * R if up else n
    SO = R if (up and layout == rm.SUBFRAMES) else 1
    y = np.ascontiguousarray(y[:, :, :n_out]).view(np.int16)
    return y.reshape(F_, C_, SO, n_out // SO).transpose(0, 2, 1, 3).reshape(F_ * SO, C_, n_out // SO)


def yardstick_case(ctx, rng, direction, R, layout, C_, F_, n, g711=False, with_len=False, chunk_frames=1, **kw):
    """footprint, values and independence of one yardstick launch"""
    rows, _, codec = make_input(rng, direction, R, layout, C_, F_, n, g711)
    length = None
    if with_len:
        length = rng.integers(0, rows.shape[2] + 40, rows.shape[:2])
        length[rng.random(rows.shape[:2]) < 0.2] = 0
    got = {}

    def yard(fill):                                                       # the state holds the fill: garbage the yardstick must not read
        raw = {}
        got[fill] = run_rs(ctx, direction, R, layout, rows, n, codec=codec, length=length, d_state=gu.dev_zeros(C_ * 296, fill), entry="rs_copy",
                           fill=fill, raw=raw, **kw)[:2]
        return raw

    def real(fill):
        raw = {}
        run_rs(ctx, direction, R, layout, rows, n, codec=codec, length=length, fill=fill, raw=raw, **kw)
        return {k: raw[k] for k in ("out", "stats")}

    ym = gu.written_mask(yard)
    gu.assert_same_footprint(ym, gu.written_mask(real), not_written=("state",))       # (a) rows and records as the entry's, no state
    off = kw.get("off", 0)
    vec = n % 8 == 0 and off % 16 == 0
    exp = rs_copy_model(direction, R, layout, rows, n, length, codec, chunk_frames, vec)
    for fill in (gu.FILL_A, gu.FILL_B):                                   # (c) the fold of the right tile dwords; zero records
        np.testing.assert_array_equal(got[fill][0], exp)
        assert not got[fill][1].tobytes().strip(b"\0")
    o, s, st, _ = run_rs(ctx, direction, R, layout, rows, n, codec=codec, length=length, entry="rs_copy", **kw)   # (b) a zero state
    np.testing.assert_array_equal(o, exp)
    assert not s.tobytes().strip(b"\0") and not st["hist"].any() and (st["flags"] == 0xA5).all() and (st["frames"] == 0xFFFFFFFE).all()


@pytest.mark.parametrize("R", rm.FACTORS)
@pytest.mark.parametrize("direction", (rm.UP, rm.DOWN), ids=("up", "down"))
def test_yardstick_footprint_values_independence(ctx, direction, R):
    """igdsp_internal_rs_copy at F = 3, every n of (8, 25, 160) (25: the general form), both layouts and the channel counts around a
    wave's and a block's: it stores the bytes igdsp_resample stores and none of the state (which holds garbage, other garbage, or
    zeros: the rows are the same), the records are zero, and every output piece is the xor fold of its unit's tile dwords"""
    rng = np.random.default_rng(80 + 10 * R + direction)
    cus = ctx.device_info()["compute_units"]
    for layout in (rm.ROWS, rm.SUBFRAMES):
        for n in (8, 25, 160):
            for C_ in ((1, 17, 65) if direction == rm.UP else (1, 5, 17)):
                assert rs_chunk_frames(direction, R, C_, 3, cus) == 1
                yardstick_case(ctx, rng, direction, R, layout, C_, 3, n)
                if direction == rm.UP and C_ == 17:
                    yardstick_case(ctx, rng, direction, R, layout, C_, 3, n, g711=True)
        yardstick_case(ctx, rng, direction, R, layout, 17, 3, 160, off=2)                                   # a base 2 bytes off: the general form
        yardstick_case(ctx, rng, direction, R, layout, 5, 3, 160, with_len=True, rn=7, rw=9)                # d_len and row strides
        yardstick_case(ctx, rng, direction, R, layout, 5, 3, 25, with_len=True, rn=6, rw=5, off=2, g711=direction == rm.UP)


@pytest.mark.parametrize("direction,R", [(rm.UP, 2), (rm.DOWN, 3)], ids=("up", "down"))
def test_yardstick_wave_keeps_its_channels_for_two_frames(ctx, monkeypatch, direction, R):
    """one block per CU in the grid and a sixth of the groups rs_route wants: the frames are cut into chunks of two, so from a chunk's
    second frame on the samples ahead of the row are the tile's own tail, moved to its front"""
    assert rs_chunk_frames(rm.UP, 2, 32805, 9, 256) == 2 and rs_chunk_frames(rm.DOWN, 2, 8229, 7, 256) == 2            # rows of the route
    assert rs_chunk_frames(rm.UP, 6, 65536, 128, 256, 1) == 128 and rs_chunk_frames(rm.UP, 6, 65536, 128, 256, 2) == 64   # table
    monkeypatch.setenv("IGDSP_RS_BLOCKS", "1")
    cus, ch = ctx.device_info()["compute_units"], 16 if direction == rm.UP else 4
    C_ = (cus * 16 // 6 + 1) * ch - 3
    cf = rs_chunk_frames(direction, R, C_, 9, cus, 1)
    assert cf >= 2, (cus, C_, cf)
    yardstick_case(ctx, np.random.default_rng(90 + direction), direction, R, rm.ROWS, C_, 9, 8, chunk_frames=cf)


def test_yardstick_argument_rules(ctx):
    """igdsp_internal_rs_copy rejects what igdsp_resample rejects, and a NULL d_out, with nothing written"""
    fn = capi.internal("rs_copy")
    d_state, d_pcm = gu.dev_zeros(4 * 296 + 64, 0xEE), gu.dev_zeros(2 * 4 * 960 * 2 + 64)
    d_out, d_st = gu.dev_zeros(2 * 4 * 960 * 2 + 64, 0xEE), gu.dev_zeros(2 * 4 * 6 * 16, 0xEE)
    stt, pcm, out, st = (t.data_ptr() for t in (d_state, d_pcm, d_out, d_st))

    def call(direction=0, R=2, layout=0, pcm_=pcm, state=stt, C_=4, F_=2, n=160, out_=out, st_=st, h=ctx.h):
        return fn(h, direction, R, layout, None, None, pcm_, None, state, C_, F_, n, 0, 0, out_, st_, None)

    for kw in (dict(h=None), dict(direction=2), dict(R=5), dict(layout=2), dict(pcm_=None), dict(state=None), dict(n=257), dict(out_=out + 1),
               dict(out_=pcm), dict(out_=None)):
        assert call(**kw) == EINVAL, kw
    gu.torch_cuda().cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xEE).all() and (d_st.cpu().numpy() == 0xEE).all() and (d_state.cpu().numpy() == 0xEE).all()
    assert call() == 0
    gu.torch_cuda().cuda.synchronize()
    rec = d_st.cpu().numpy()
    assert (d_state.cpu().numpy() == 0xEE).all() and not rec[:2 * 4 * 16].any() and (rec[2 * 4 * 16:] == 0xEE).all()
