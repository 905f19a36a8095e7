"""-m gpu: igdsp_tone_generate (include/igdsp.h, "Tone generator") against tests/tone_model.py: rows, lengths, sumsq, peak, flags and the
state bit for bit, rms at 1e-5 relative against float64.  Small shapes around every geometry edge (a wave owns 16 ports, a block 256),
both forms (16-byte pieces; the sample-granular one for odd n and 2-byte aligned bases), plans whose edges fall mid-frame, the wrap and
the end of a plan inside a launch, mixed plans, every cmd bit, the single-output forms, a row stride with canaries, one launch against
split launches, the argument clauses, one full-chip shape and the chain into igdsp_conf_mix."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import conf_model as cm  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import tone_model as tm  # noqa: E402

GUARD = 256
EINVAL, ERANGE = -22, -34
RING = tm.plan_build([(440, 480, 2000, 1000)])                           # the reference's ring: 24 000 samples
EDGES = tm.plan_build([(440, 480, 30, 10)])                              # 240 on / 80 off: a cycle of 320, every edge inside a frame of 160
EIGHT = tm.plan_build([(350, 440, 37, 5), (480, 620, 20, 0), (1000, 0, 13, 7), (1400, 0, 5, 1), (697, 1209, 50, 50, 32767), (3999, 1, 9, 3, 1),
                       (2600, 0, 0, 11), (941, 1633, 2, 2, 20000)])
ONCE = tm.plan_build([(440, 480, 100, 25)], 8000, 0)                     # does not loop: 1 000 samples, ends inside frame 6 of 160
ONCE_EDGE = tm.plan_build([(697, 0, 35, 5)], 8000, tm.NO_FADE)          # does not loop: 320 samples, ends on a frame edge


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def plan_array(plans):
    return np.array([tm.plan_record(p, capi.TONE_PLAN) for p in plans], capi.TONE_PLAN)


def run_tone(ctx, plans, pos, flags, F_, n, plan_of=None, cmd=None, rpf=0, pcm=True, length=True, stats=True, off=0, d_state=None, entry=None,
             fill=0xEE, raw=None):
    """One launch through the C ABI.  The rows and lengths sit in buffers filled with 0xEE (the canary of foreign rows and of the bytes
    around), the rows `off` bytes behind a 256-byte aligned base.  Returns (pcm [F][R][n] | None, len [F][R] | None, stats [F][P] | None,
    state [P], the state tensor).  entry: through that yardstick of capi.INTERNAL_TWIN instead; fill: another canary byte; raw: a dict
    that takes the whole output buffers' bytes after the launch."""
    torch = gu.torch_cuda()
    P_ = len(pos)
    R_ = rpf or P_
    st = np.zeros(P_, capi.TONE_STATE)
    st["pos"], st["flags"] = pos, flags
    d_plans = gu.to_dev(plans if isinstance(plans, np.ndarray) else plan_array(plans))
    d_state = gu.to_dev(st) if d_state is None else d_state
    d_of = gu.to_dev(np.asarray(plan_of, np.uint16)) if plan_of is not None else None
    d_cmd = gu.to_dev(np.asarray(cmd, np.uint8)) if cmd is not None else None
    nb = F_ * R_ * n * 2
    d_pcm = gu.dev_zeros(nb + 64 + GUARD, fill) if pcm else None
    d_len = gu.dev_zeros(F_ * R_ * 2 + GUARD, fill) if length else None
    d_st = gu.dev_zeros(F_ * P_ * 16 + GUARD, fill) if stats else None
    assert d_pcm is None or d_pcm.data_ptr() % 256 == 0
    (ctx.via(entry) if entry else ctx).tone_generate(d_plans, len(plans), d_state, P_, F_, n, plan_of=d_of, cmd=d_cmd, rows_per_frame=rpf,
                                                     pcm=d_pcm.data_ptr() + off if pcm else None, length=d_len, stats=d_st)
    torch.cuda.synchronize()
    o = ln = s = None
    if pcm:
        b = d_pcm.cpu().numpy()
        assert np.all(b[:off] == fill) and np.all(b[off + nb:] == fill), "bytes around the rows written"
        o = b[off:off + nb].copy().view("<i2").reshape(F_, R_, n)
    if length:
        b = d_len.cpu().numpy()
        assert np.all(b[F_ * R_ * 2:] == fill), "bytes after d_len written"
        ln = b[:F_ * R_ * 2].view("<u2").reshape(F_, R_)
    if stats:
        b = d_st.cpu().numpy()
        assert np.all(b[F_ * P_ * 16:] == fill), "bytes after d_stats written"
        s = b[:F_ * P_ * 16].view(capi.FRAME_STATS).reshape(F_, P_)
    if raw is not None:
        raw.update({k: t.cpu().numpy() for k, t in (("pcm", d_pcm), ("len", d_len), ("stats", d_st), ("state", d_state)) if t is not None})
    return o, ln, s, d_state.cpu().numpy().view(capi.TONE_STATE), d_state


def check_launch(ctx, plans, pos, flags, F_, n, plan_of=None, cmd=None, **kw):
    """a launch equals the model: the rows [0, P) of every frame, the canaries in the others, lengths, records, state"""
    P_ = len(pos)
    o, ln, s, st, _ = run_tone(ctx, plans, pos, flags, F_, n, plan_of=plan_of, cmd=cmd, **kw)
    eo, eln, es, epos, eflags = tm.generate(plans, plan_of, cmd, pos, flags, F_, n)
    if o is not None:
        np.testing.assert_array_equal(o[:, :P_], eo)
        assert np.all(o[:, P_:].view(np.uint16) == 0xEEEE), "rows outside [0, P) written"
    if ln is not None:
        np.testing.assert_array_equal(ln[:, :P_], eln)
        assert np.all(ln[:, P_:] == 0xEEEE), "lengths outside [0, P) written"
    if s is not None:
        gu.assert_stats_equal(s, es)
    np.testing.assert_array_equal(st["pos"], epos)
    np.testing.assert_array_equal(st["flags"], eflags)
    return eo, eln


def spread(rng, plan, P_):
    """positions spread over the cycle, its first and last sample among them"""
    pos = rng.integers(0, plan["cycle"], P_)
    pos[0] = 0
    pos[-1] = plan["cycle"] - 1
    return pos


@pytest.mark.parametrize("n", [1, 160, 255, 256])
def test_small_shapes_vs_model(ctx, n):
    """P: one port, three, one more than a wave owns (16), one more than a block owns (256); both forms by n"""
    rng = np.random.default_rng(n)
    for P_ in (1, 3, 17, 257):
        for F_ in (1, 5, 7):
            for plan in (EDGES, RING, EIGHT):
                check_launch(ctx, [plan], spread(rng, plan, P_), np.full(P_, tm.PLAYING), F_, n)


def test_ring_plan_edges(ctx):
    """the ring plan at its four edges: the fade-in at 0, the fade-out before 16 000, the start of the pause, the wrap at 24 000"""
    pos = np.array([0, 1, 7, 8, 15800, 15983, 15984, 15999, 16000, 16001, 23839, 23840, 23999, 12345, 20000, 15840, 15841])
    eo, _ = check_launch(ctx, [RING], pos, np.full(len(pos), tm.PLAYING), 3, 160)
    assert not eo[:, 14].any() and eo[0, 0, 0] == 0 and eo[0, 0, 9] != 0


def test_loop_wrap_inside_a_launch(ctx):
    """cycle 320, 7 frames of 160 and of 256: every port wraps several times, some inside a row"""
    for n in (160, 256, 255):
        check_launch(ctx, [EDGES], np.arange(0, 320, 9), np.full(36, tm.PLAYING), 7, n)
    tiny = tm.plan_build([(1000, 0, 1, 1)])                               # a cycle of 16 samples: 10 wraps per row
    check_launch(ctx, [tiny], np.arange(16), np.full(16, tm.PLAYING), 5, 160)


def test_non_looping_end_inside_a_launch(ctx):
    """the end mid-frame and on a frame edge, and every frame after it: EMPTY, PLAYING cleared, pos = cycle"""
    pos = np.array([0, 1, 159, 160, 500, 999, 1000, 3000, 839, 840, 841])
    eo, eln = check_launch(ctx, [ONCE], pos, np.full(len(pos), tm.PLAYING), 9, 160)
    assert eln[:, 0].tolist() == [160] * 7 + [0, 0] and eln[:, 6].tolist() == [0] * 9 and not eo[6, 0, 40:].any()
    pos = np.array([0, 160, 319, 320, 1])
    _, eln = check_launch(ctx, [ONCE_EDGE], pos, np.full(5, tm.PLAYING), 5, 160)
    assert eln[:, 0].tolist() == [160, 160, 0, 0, 0]
    check_launch(ctx, [ONCE], pos, np.full(5, tm.PLAYING), 7, 255)


def test_mixed_plans_and_missing_plans(ctx):
    rng = np.random.default_rng(5)
    plans = [RING, EDGES, EIGHT, ONCE]
    P_ = 83
    plan_of = rng.integers(0, 6, P_)                                      # 4 and 5: no such plan
    plan_of[:6] = [0, 1, 2, 3, 4, 65535]
    pos = np.array([rng.integers(0, plans[i]["cycle"]) if i < 4 else rng.integers(0, 2 ** 32) for i in plan_of])
    flags = np.where(rng.random(P_) < 0.8, tm.PLAYING, 0)
    cmd = np.where(plan_of >= 4, rng.integers(0, 8, P_), 0)               # a port without a plan still takes its cmd
    eo, eln = check_launch(ctx, plans, pos, flags, 6, 160, plan_of=plan_of, cmd=cmd)
    assert not eln[:, plan_of >= 4].any() and not eo[:, plan_of >= 4].any()
    # a plan nobody built (all zero: cycle 0) plays nothing and leaves the state; one with a cycle and no segment is silence
    raw = np.zeros(2, capi.TONE_PLAN)
    raw[1]["cycle"], raw[1]["options"], raw[1]["n_tones"] = 1000, tm.LOOP, 99
    o, ln, s, st, _ = run_tone(ctx, raw, [5, 5], [tm.PLAYING, tm.PLAYING], 3, 160, plan_of=[0, 1])
    assert not o.any() and ln.tolist() == [[0, 160]] * 3 and s["flags"].tolist() == [[tm.FLAG_EMPTY, tm.FLAG_SILENT]] * 3
    assert st["pos"].tolist() == [5, 485] and st["flags"].tolist() == [tm.PLAYING, tm.PLAYING]


def test_every_cmd_bit(ctx):
    rng = np.random.default_rng(6)
    P_ = 8 * 3 * 2
    cmd = np.repeat(np.arange(8), 6)
    flags = np.tile(np.repeat([0, tm.PLAYING, tm.PLAYING | 0x100], 2), 8)
    for plan in (EDGES, ONCE):
        pos = rng.integers(0, plan["cycle"], P_)
        check_launch(ctx, [plan], pos, flags, 4, 160, cmd=cmd)
        check_launch(ctx, [plan], pos, flags, 1, 255, cmd=cmd)


def test_single_output_forms(ctx):
    rng = np.random.default_rng(7)
    for n in (160, 255):
        pos = spread(rng, EDGES, 70)
        fl = np.full(70, tm.PLAYING)
        check_launch(ctx, [EDGES], pos, fl, 3, n, stats=False)           # run_tone checks the canaries of what is given
        check_launch(ctx, [EDGES], pos, fl, 3, n, pcm=False, length=False)
        check_launch(ctx, [EDGES], pos, fl, 3, n, length=False)
        check_launch(ctx, [EDGES], pos, fl, 3, n, pcm=False)


def test_row_stride_leaves_foreign_rows(ctx):
    """rows_per_frame > P: the tone rows of each frame beside other rows; those and everything behind the end keep their 0xEE"""
    rng = np.random.default_rng(8)
    for P_, rpf, n in ((3, 4, 160), (17, 40, 160), (5, 6, 255), (33, 64, 8), (1, 2, 1)):
        check_launch(ctx, [EDGES], spread(rng, EDGES, P_), np.full(P_, tm.PLAYING), 5, n, rpf=rpf)


def test_two_byte_aligned_base_takes_the_general_form(ctx):
    rng = np.random.default_rng(9)
    for off in (2, 4, 8, 14):
        for n in (160, 256, 8):
            check_launch(ctx, [EIGHT], spread(rng, EIGHT, 19), np.full(19, tm.PLAYING), 3, n, off=off)


def test_one_launch_equals_split_launches(ctx):
    rng = np.random.default_rng(10)
    for plan, n in ((EDGES, 160), (EIGHT, 255), (ONCE, 160), (RING, 256)):
        P_, F_ = 37, 9
        pos, fl = spread(rng, plan, P_), np.where(rng.random(P_) < 0.9, tm.PLAYING, 0)
        whole = run_tone(ctx, [plan], pos, fl, F_, n)
        for cuts in ((1, 8), (4, 5), (1, 1, 1, 1, 1, 1, 1, 1, 1), (2, 3, 4)):
            d_state, rows, lens, recs = None, [], [], []
            for k in cuts:
                o, ln, s, st, d_state = run_tone(ctx, [plan], pos, fl, k, n, d_state=d_state)
                rows.append(o), lens.append(ln), recs.append(s)
            np.testing.assert_array_equal(np.concatenate(rows), whole[0])
            np.testing.assert_array_equal(np.concatenate(lens), whole[1])
            assert np.concatenate(recs).tobytes() == whole[2].tobytes() and st.tobytes() == whole[3].tobytes()


def test_argument_errors(ctx):
    L = capi.load()
    d_plans, d_state = gu.to_dev(plan_array([EDGES])), gu.dev_zeros(64)
    d_pcm, d_len, d_st = gu.dev_zeros(4 * 160 * 2 * 2 + 64), gu.dev_zeros(64), gu.dev_zeros(4 * 16 * 2)
    pl, stt, pcm, ln, st = (t.data_ptr() for t in (d_plans, d_state, d_pcm, d_len, d_st))

    def call(plans=pl, n_plans=1, plan_of=None, cmd=None, state=stt, P_=4, F_=2, n=160, rpf=0, pcm_=pcm, len_=ln, st_=st, h=ctx.h):
        return L.igdsp_tone_generate(h, plans, n_plans, plan_of, cmd, state, P_, F_, n, rpf, pcm_, len_, st_, None)

    assert call() == 0
    assert call(h=None) == EINVAL
    assert call(P_=0, plans=None, state=None, pcm_=None, st_=None, n=0) == 0 and call(F_=0, n=999) == 0      # nothing to do comes first
    for kw in (dict(plans=None), dict(state=None), dict(n_plans=0), dict(pcm_=None, st_=None), dict(rpf=3), dict(n=0), dict(n=257),
               dict(pcm_=pcm + 1), dict(len_=ln + 1), dict(st_=st + 4), dict(state=stt + 2), dict(plans=pl + 2), dict(plan_of=ln + 1),
               dict(pcm_=stt), dict(st_=stt), dict(len_=pl)):
        assert call(**kw) == EINVAL, kw
    assert call(P_=0x10000000, F_=16) == ERANGE and call(rpf=0x10000000, F_=16) == ERANGE
    assert call(P_=0x10000000, F_=16, n=0) == EINVAL
    assert call(pcm_=stt) == EINVAL and b"an output must not be an input or the state" in (L.igdsp_last_error(ctx.h) or b"")
    gu.torch_cuda().cuda.synchronize()
    assert not d_state.cpu().numpy()[32:].any()                           # nothing past the four ports' state was written


def test_full_chip(ctx):
    """ports >= CUs x waves per CU x ports per wave (256 x 16 x 16), and 17 more: the grid-stride loop takes a second item, the kernel
    writes the state itself (no frame chunks).  Mixed plans, positions over the cycle, a tenth of the ports stopped or held."""
    rng = np.random.default_rng(11)
    P_, F_ = 256 * 16 * 16 + 17, 2
    plans = [RING, EDGES, ONCE]
    plan_of = rng.integers(0, 3, P_)
    pos = (rng.random(P_) * np.array([p["cycle"] for p in plans])[plan_of]).astype(np.int64)
    flags = np.where(rng.random(P_) < 0.95, tm.PLAYING, 0)
    cmd = np.where(rng.random(P_) < 0.05, rng.integers(0, 8, P_), 0)
    check_launch(ctx, plans, pos, flags, F_, 160, plan_of=plan_of, cmd=cmd)


def test_ring_into_conf_mix(ctx):
    """F = 1, one array [1][C + P][n]: the calls' PCM rows, then the tone rows written in place by igdsp_tone_generate (no stride needed
    at one frame); igdsp_conf_mix over n_channels = C + P equals conf_model over the model's rows.  Console k listens to call k and,
    while its ring is connected, to tone row k: it hears clamp16(call + tone)."""
    torch = gu.torch_cuda()
    rng = np.random.default_rng(12)
    C_, P_, n = 6, 4, 160
    calls = rng.integers(-32768, 32768, (1, C_, n)).astype(np.int16)
    calls[0, 1] = 32000                                                    # call + tone clamps
    pos = np.array([0, 8000, 15900, 17000])                               # the last one is in the pause: silence, but a live row
    tone_rows, tone_len, _, _, _ = tm.generate([RING], None, None, pos, np.full(P_, tm.PLAYING), 1, n)
    d_all = gu.dev_zeros((C_ + P_) * n * 2)
    d_all[:C_ * n * 2] = gu.to_dev(calls)
    d_len = gu.to_dev(np.full(C_ + P_, n, np.uint16))
    st = np.zeros(P_, capi.TONE_STATE)
    st["pos"], st["flags"] = pos, tm.PLAYING
    d_state, d_plans = gu.to_dev(st), gu.to_dev(plan_array([RING]))
    ctx.tone_generate(d_plans, 1, d_state, P_, 1, n, pcm=d_all.data_ptr() + C_ * n * 2, length=d_len.data_ptr() + C_ * 2)
    # consoles 0 .. 3: (call k, tone k); console 2 has its ring disconnected; console 4 hears a tone alone
    chan = np.array([0, 1, 2, 3, C_ + 0, C_ + 1, C_ + 3, C_ + 2], np.uint32)
    port = np.array([0, 1, 2, 3, 0, 1, 3, 4], np.uint32)
    ptr, mem = cm.build(chan, port, C_ + P_, 5)
    gain = np.full(C_ + P_, 128, np.uint16)
    d_out, d_st = gu.dev_zeros(5 * n * 2), gu.dev_zeros(5 * 16)
    ctx.conf_mix(gu.to_dev(gain), gu.to_dev(ptr), gu.to_dev(mem), len(mem), C_ + P_, 5, 1, n, out=d_out, stats=d_st, pcm=d_all, length=d_len)
    torch.cuda.synchronize()
    rows = np.concatenate([calls, tone_rows], axis=1)
    np.testing.assert_array_equal(d_all.cpu().numpy().view("<i2").reshape(1, C_ + P_, n), rows)
    np.testing.assert_array_equal(d_len.cpu().numpy().view("<u2"), np.concatenate([np.full(C_, n), tone_len[0]]))
    eo, es = cm.mix(rows.astype(np.int64), gain, ptr, mem, len(mem), 5, length=np.full((1, C_ + P_), n))
    o = d_out.cpu().numpy().view("<i2").reshape(1, 5, n)
    np.testing.assert_array_equal(o, eo)
    np.testing.assert_array_equal(o[0, 0], np.clip(calls[0, 0].astype(int) + tone_rows[0, 0], -32768, 32767))
    np.testing.assert_array_equal(o[0, 2], calls[0, 2])
    np.testing.assert_array_equal(o[0, 4], tone_rows[0, 2])
    s = d_st.cpu().numpy().view(capi.FRAME_STATS).reshape(1, 5)
    for k in ("sumsq", "peak", "flags"):
        np.testing.assert_array_equal(s[k], es[k], err_msg=k)
    assert s["flags"][0, 1] & cm.FLAG_SATURATED


# ---- the compute-free yardstick (igdsp_internal_tone_fill, tools/tone_bench.py) against its promise in csrc/igdsp_capi_tone.hip: "the
# same items in the same order, the same rows, lengths and records stored, no plan, no state, no oscillator; d_pcm is required, the
# state is neither read nor written, the rows hold a pattern and the records are the len-0 record"

@pytest.mark.parametrize("n", [1, 160, 255])
def test_yardstick_footprint_values_independence(ctx, n):
    """igdsp_internal_tone_fill at F = 3 with P = 1, 17, 65 ports, a row stride, a base 2 bytes off: it stores the bytes
    igdsp_tone_generate stores in the rows, lengths and records (foreign rows and the surroundings stay), none of the state, which may
    hold anything; the lengths are those of a launch whose ports all play, the records the len-0 record"""
    from tests import record_model

    rng = np.random.default_rng(400 + n)
    for P_, kw in ((1, {}), (17, {}), (65, {}), (17, dict(rpf=23)), (5, dict(off=2)), (17, dict(rpf=19, off=2))):
        pos, fl = spread(rng, RING, P_), np.full(P_, tm.PLAYING)
        got = {}

        def yard(fill):
            raw = {}
            got[fill] = run_tone(ctx, [RING], pos, fl, 3, n, d_state=gu.dev_zeros(P_ * 8, fill), entry="tone_fill", fill=fill, raw=raw, **kw)
            return raw

        def real(fill):
            raw = {}
            got["real", fill] = run_tone(ctx, [RING], pos, fl, 3, n, fill=fill, raw=raw, **kw)
            return {k: v for k, v in raw.items() if k != "state"}

        gu.assert_same_footprint(gu.written_mask(yard), gu.written_mask(real), not_written=("state",))
        zero = run_tone(ctx, [RING], np.zeros(P_, np.int64), np.zeros(P_, np.int64), 3, n, entry="tone_fill", cmd=np.full(P_, 7, np.uint8), **kw)
        empty = record_model.records(np.zeros((3, P_, n), np.int64), live=np.zeros((3, P_), bool))
        for o, ln, st, _, _ in (got[gu.FILL_A], got[gu.FILL_B], zero):
            np.testing.assert_array_equal(o[:, :P_], got[gu.FILL_A][0][:, :P_])
            np.testing.assert_array_equal(ln[:, :P_], got["real", gu.FILL_A][1][:, :P_])
            assert (ln[:, :P_] == n).all()
            gu.assert_stats_equal(st, empty)
            assert (st["rms"] == 0).all()
        assert not zero[3].tobytes().strip(b"\0")


def test_yardstick_argument_rules(ctx):
    """igdsp_internal_tone_fill rejects what igdsp_tone_generate rejects, and a NULL d_pcm, with nothing written"""
    fn = capi.internal("tone_fill")
    d_plans, d_state = gu.to_dev(plan_array([EDGES])), gu.dev_zeros(64, 0xEE)
    d_pcm, d_len, d_st = gu.dev_zeros(4 * 160 * 2 * 2 + 64, 0xEE), gu.dev_zeros(64, 0xEE), gu.dev_zeros(4 * 16 * 2, 0xEE)
    pl, stt, pcm, ln, st = (t.data_ptr() for t in (d_plans, d_state, d_pcm, d_len, d_st))

    def call(plans=pl, n_plans=1, state=stt, P_=4, F_=2, n=160, rpf=0, pcm_=pcm, len_=ln, st_=st, h=ctx.h):
        return fn(h, plans, n_plans, None, None, state, P_, F_, n, rpf, pcm_, len_, st_, None)

    for kw in (dict(h=None), dict(plans=None), dict(state=None), dict(n_plans=0), dict(rpf=3), dict(n=257), dict(pcm_=pcm + 1), dict(st_=st + 4),
               dict(pcm_=stt), dict(pcm_=None), dict(pcm_=None, len_=None)):
        assert call(**kw) == EINVAL, kw
    gu.torch_cuda().cuda.synchronize()
    assert all((t.cpu().numpy() == 0xEE).all() for t in (d_state, d_pcm, d_len, d_st))
    assert call() == 0
    gu.torch_cuda().cuda.synchronize()
    assert (d_state.cpu().numpy() == 0xEE).all()
