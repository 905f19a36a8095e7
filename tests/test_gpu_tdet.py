"""-m gpu: igdsp_tone_detect (include/igdsp.h, "Tone detector") through the C ABI against tests/tdet_model.py, bit for bit: records,
state, events and counts.  Shapes around the kernel's ownership units (16 lanes own a channel, a wave four, a block 32; n / 2 odd takes
the kernel's other instantiation): (C, F, n) in (1, 1, 160), (3, 7, 24), (4, 5, 164), (5, 2, 160), (67, 5, 160), (5, 3, 256), (3, 4, 2),
each from mu-law, A-law (mixed per channel) and PCM, with the DTMF plan alone and with the DTMF, the 8 + 8 and the 1-tone plan mixed
through d_plan_of so that every plan occurs at every shape (one index out of range; at C = 1 a launch per plan), channels of the 1-tone
plan hearing its tone.  Every launch starts from the state the model reached over three earlier frames of the
scene, so digits are up and candidates are running at frame 0.  Bit for bit as well: one launch against the same frames in several,
the same channel at another position and channel count, G.711 against its decoded PCM.  Every optional output absent in turn, an
event_cap below the count, guard bytes behind every buffer and behind the state, a garbage state, the argument clauses, the yardstick against its written
promise, and igdsp_tone_generate -> igdsp_tone_detect on the device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import tdet_model as tm  # noqa: E402

GUARD = 256
EINVAL, ERANGE = -22, -34
SB = capi.TDET_STATE.itemsize
SHAPES = ((1, 1, 160), (3, 7, 24), (4, 5, 164), (5, 2, 160), (67, 5, 160), (5, 3, 256), (3, 4, 2))
PRE = 3
PLANS3 = np.array([tm.plan_dtmf(), tm.plan_8x8(), tm.plan_single()])


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def mixed_laws(C_):
    return np.where(np.arange(C_) % 3 == 1, 8, 0).astype(np.uint8)


def mixed_plans(C_):
    """C >= 3: all three plans in one launch: one channel each first (three plans in one wave), then runs of two, and one index out of
    range when there is room for it.  C < 3: None (the caller makes one launch per plan)"""
    if C_ < 3:
        return None
    po = np.concatenate([np.arange(3), (np.arange(C_ - 3) // 2) % 3]).astype(np.uint16)
    if C_ >= 5:
        po[3] = 7
    assert set(po.tolist()) >= {0, 1, 2}
    return po


STATE_GUARD = 0xA5


def state_dev(state):
    """the state records on the device with GUARD bytes of STATE_GUARD behind them"""
    b = np.ascontiguousarray(state).view(np.uint8).reshape(-1)
    return gu.to_dev(np.concatenate([b, np.full(GUARD, STATE_GUARD, np.uint8)]))


def run_tdet(ctx, x, plans, codec=None, plan_of=None, state=None, d_state=None, outputs=("rec", "list"), cap=None, mask=0, fill=0xEE, entry=None,
             raw_bytes=None):
    """One launch through the C ABI (entry: through that yardstick instead).  x [F][C][n]: uint8 codes (with codec [C]) or int16 PCM;
    plans a TDET_PLAN array; state [C] or None (reset), or d_state carried from an earlier launch.  outputs: "rec", "list" (events, counts
    and work; cap None: room for every (f, c)).  Returns the outputs, the state records and the state tensor."""
    torch = gu.torch_cuda()
    F_, C_, n = x.shape
    g711 = x.dtype == np.uint8
    d_x = gu.to_dev(x if g711 else np.asarray(x, "<i2"))
    d_codec = gu.to_dev(np.asarray(codec, np.uint8)) if g711 else None
    plans = np.atleast_1d(np.asarray(plans, capi.TDET_PLAN))
    d_plans = gu.to_dev(plans)
    d_po = gu.to_dev(np.asarray(plan_of, "<u2")) if plan_of is not None else None
    if d_state is None:
        d_state = state_dev(np.zeros(C_, capi.TDET_STATE) if state is None else state)
    cap = F_ * C_ if cap is None else cap
    sizes = {}
    if "rec" in outputs:
        sizes["rec"] = F_ * C_ * 8
    if "list" in outputs:
        sizes.update(events=cap * 16, count=8, work=capi.tdet_work_bytes(C_, F_, "rec" in outputs))
    bufs = {k: gu.dev_zeros(v + GUARD, fill) for k, v in sizes.items()}
    p = lambda k: bufs[k].data_ptr() if k in bufs else None
    if entry:
        rc = capi.internal(entry)(ctx.h, d_x.data_ptr() if g711 else None, d_codec.data_ptr() if g711 else None, None if g711 else d_x.data_ptr(),
                                  d_plans.data_ptr(), len(plans), None if d_po is None else d_po.data_ptr(), C_, F_, n, mask, d_state.data_ptr(), p("rec"),
                                  p("events") if cap else None, cap, p("count"), p("work"), None)
        assert rc == 0, rc
    else:
        ctx.tone_detect(d_plans, d_state, C_, F_, n, g711=d_x if g711 else None, codec=d_codec, pcm=None if g711 else d_x, n_plans=len(plans),
                        plan_of=d_po, event_mask=mask, rec=bufs.get("rec"), events=bufs.get("events") if cap else None, event_cap=cap,
                        event_count=bufs.get("count"), work=bufs.get("work"))
    torch.cuda.synchronize()
    host = {k: t.cpu().numpy() for k, t in bufs.items()}
    for k, b in host.items():
        assert np.all(b[sizes[k]:] == fill), f"bytes after d_{k} written"
    sbytes = d_state.cpu().numpy()
    assert len(sbytes) == C_ * SB + GUARD and np.all(sbytes[C_ * SB:] == STATE_GUARD), "bytes after d_state written"
    res = dict(d_state=d_state, state=sbytes[:C_ * SB].view(capi.TDET_STATE).copy())
    if "rec" in host:
        res["rec"] = host["rec"][:sizes["rec"]].view(capi.TDET_REC).reshape(F_, C_)
    if "list" in outputs:
        res["count"] = host["count"][:8].view("<u4").copy()
        res["events"] = host["events"][:cap * 16].view(capi.TDET_EVENT)
        res["events_raw"] = host["events"][:cap * 16]
    if raw_bytes is not None:
        raw_bytes.update({k: v for k, v in host.items() if k != "work"})
        raw_bytes["state"] = sbytes[:C_ * SB]
    return res


def pcm_of(x, codec):
    return tm.decode(x, codec) if x.dtype == np.uint8 else np.asarray(x, np.int16)


def check(got, x, plans, codec=None, plan_of=None, state=None, mask=0, cap=None, fill=0xEE):
    """a launch against the model: records, state, counts, the stored events, and the bytes of d_events past them"""
    rec, st = tm.detect(list(np.atleast_1d(plans)), pcm_of(x, codec), state, plan_of)
    if "rec" in got:
        assert got["rec"].tobytes() == rec.tobytes(), np.argwhere(got["rec"].view("<u8") != rec.view("<u8"))[:8]
    assert got["state"].tobytes() == st.tobytes(), [k for k in st.dtype.names if not np.array_equal(got["state"][k], st[k])]
    if "count" in got:
        ev, cnt = tm.events(rec, mask, cap)
        assert tuple(got["count"]) == tuple(cnt), (got["count"], cnt)
        assert got["events"][:cnt[1]].tobytes() == ev.tobytes()
        assert np.all(got["events_raw"][cnt[1] * 16:] == fill), "an event slot past the stored ones written"
    return rec, st


def scene_with_state(C_, F_, n, seed, plans, plan_of=None, law=None, tones=()):
    """the scene's last F frames and the model's state after its first PRE; law "u8": as codes of mixed laws; tones: channels that play
    the 1-tone plan's 1 000 Hz whatever the scene gives them"""
    x = tm.scene(C_, F_ + PRE, n, seed, tones=tones)
    codec = None
    if law:
        codec = mixed_laws(C_)
        x = tm.encode(x, codec)
    _, st = tm.detect(list(np.atleast_1d(plans)), pcm_of(x[:PRE], codec), None, plan_of)
    return x[PRE:], codec, st


# ---- 1. the shapes, from codes and from PCM, one plan and three
@pytest.mark.parametrize("law", ("g711", "pcm"))
@pytest.mark.parametrize("C_,F_,n", SHAPES)
def test_shapes(ctx, C_, F_, n, law):
    po3 = mixed_plans(C_)
    cases = [(PLANS3[:1], None), (PLANS3, po3)] if po3 is not None else [(PLANS3[k:k + 1], None) for k in range(3)]     # C < 3: a launch per plan
    for plans, po in cases:
        # every other channel of the 1-tone plan hears its tone (channel 0 when that plan has the launch to itself)
        tones = [c for c in range(C_) if (po[c] == 2 if po is not None else plans is not PLANS3[:1] and plans[0] == PLANS3[2])][::2]
        x, codec, st = scene_with_state(C_, F_, n, 10 + n + C_, plans, po, law == "g711", tones)
        got = run_tdet(ctx, x, plans, codec, po, state=st)
        rec, _ = check(got, x, plans, codec, po, st)
        if (C_, n) == (67, 160):
            assert tm.events(rec)[1][0] >= 20 and len(np.unique(rec["code"])) >= 8, "the large case carries events of many digits"


# ---- 2. launches split
def test_split_launches(ctx):
    C_, F_, n = 9, 8, 160
    po = mixed_plans(C_)
    x, codec, st = scene_with_state(C_, F_, n, 21, PLANS3, po, True)
    one = run_tdet(ctx, x, PLANS3, codec, po, state=st)
    check(one, x, PLANS3, codec, po, st)
    for cuts in ((3, 8), (1, 2, 5, 8), tuple(range(1, 9))):
        d_state, f0, recs, evs = state_dev(st), 0, [], []
        for f1 in cuts:
            got = run_tdet(ctx, x[f0:f1], PLANS3, codec, po, d_state=d_state)
            d_state = got["d_state"]
            recs.append(got["rec"])
            e = got["events"][:got["count"][1]].copy()
            e["frame"] += f0
            evs.append(e)
            f0 = f1
        assert np.concatenate(recs).tobytes() == one["rec"].tobytes()
        assert got["state"].tobytes() == one["state"].tobytes()
        assert np.concatenate(evs).tobytes() == one["events"][:one["count"][1]].tobytes()


# ---- 3. position and channel count
def test_position_independence(ctx):
    C_, F_, n = 67, 5, 160
    x, codec, st = scene_with_state(C_, F_, n, 31, PLANS3[:1], None, True)
    full = run_tdet(ctx, x, PLANS3[:1], codec, state=st)
    for pick in ([66], [5, 40, 2], list(range(30, 65))):
        got = run_tdet(ctx, np.ascontiguousarray(x[:, pick]), PLANS3[:1], codec[pick], state=st[pick])
        assert got["rec"].tobytes() == np.ascontiguousarray(full["rec"][:, pick]).tobytes()
        assert got["state"].tobytes() == full["state"][pick].tobytes()


# ---- 4. codes against their decoded PCM
@pytest.mark.parametrize("n", (160, 2, 24))
def test_g711_equals_decoded_pcm(ctx, n):
    C_, F_ = 6, 6
    po = mixed_plans(C_)
    x, codec, st = scene_with_state(C_, F_, n, 41, PLANS3, po, True)
    a, b = run_tdet(ctx, x, PLANS3, codec, po, state=st), run_tdet(ctx, tm.decode(x, codec), PLANS3, None, po, state=st)
    for k in ("rec", "state", "events", "count"):
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- 5. optional outputs, the cap, the mask
def test_optional_outputs_absent_in_turn(ctx):
    C_, F_, n = 7, 6, 160
    x, codec, st = scene_with_state(C_, F_, n, 51, PLANS3[:1], None, True)
    full = run_tdet(ctx, x, PLANS3[:1], codec, state=st)
    check(full, x, PLANS3[:1], codec, None, st)
    assert full["count"][0] >= 4
    for outs in (("rec",), ("list",), ()):
        got = run_tdet(ctx, x, PLANS3[:1], codec, state=st, outputs=outs)
        check(got, x, PLANS3[:1], codec, None, st)
        for k in ("rec", "events", "count", "state"):
            if k in got:
                assert got[k].tobytes() == full[k].tobytes(), (outs, k)


@pytest.mark.parametrize("with_rec", (True, False))
def test_event_cap_and_mask(ctx, with_rec):
    C_, F_, n = 67, 5, 160
    x, codec, st = scene_with_state(C_, F_, n, 61, PLANS3[:1], None, False)
    outs = ("rec", "list") if with_rec else ("list",)
    total = run_tdet(ctx, x, PLANS3[:1], state=st, outputs=outs)["count"][0]
    assert total >= 8
    for cap in (0, 1, int(total) - 1, int(total)):
        got = run_tdet(ctx, x, PLANS3[:1], state=st, outputs=outs, cap=cap)
        check(got, x, PLANS3[:1], None, None, st, cap=cap)
        assert tuple(got["count"]) == (total, cap)
    for mask in (capi.TDET_ON0 | capi.TDET_ON1, capi.TDET_OFF0 | capi.TDET_OFF1, capi.TDET_OFF1):
        got = run_tdet(ctx, x, PLANS3[:1], state=st, outputs=outs, mask=mask)
        check(got, x, PLANS3[:1], None, None, st, mask=mask)
        assert 0 < got["count"][0] < total


def test_footprint(ctx):
    C_, F_, n = 7, 6, 160                                                                            # four events, room for three
    x, codec, st = scene_with_state(C_, F_, n, 51, PLANS3[:1], None, True)

    def launch(fill):
        raw = {}
        run_tdet(ctx, x, PLANS3[:1], codec, state=st, fill=fill, raw_bytes=raw, cap=3)
        raw.pop("state")
        return raw

    mask = gu.written_mask(launch)
    assert mask["rec"][:F_ * C_ * 8].all() and not mask["rec"][F_ * C_ * 8:].any()
    assert mask["events"][:48].all() and not mask["events"][48:].any()
    assert mask["count"][:8].all() and not mask["count"][8:].any()


# ---- 6. garbage state
def test_garbage_state(ctx):
    C_, F_, n = 9, 5, 160
    rng = np.random.default_rng(6)
    state = np.frombuffer(rng.integers(0, 256, C_ * SB, dtype=np.uint8).tobytes(), capi.TDET_STATE).copy()
    po = mixed_plans(C_)
    x = tm.encode(tm.scene(C_, F_, n, 81), mixed_laws(C_))
    got = run_tdet(ctx, x, PLANS3, mixed_laws(C_), po, state=state)
    check(got, x, PLANS3, mixed_laws(C_), po, state)
    live = po < 3
    assert not got["state"]["reserved"][live].any() and got["state"][~live].tobytes() == state[~live].tobytes()


# ---- 7. clauses
def test_argument_errors(ctx):
    L = capi.load()
    C_, F_, n = 4, 2, 160
    d_state = gu.dev_zeros(C_ * SB + 64)
    d_g, d_cd, d_pcm = gu.dev_zeros(F_ * C_ * n + 64), gu.dev_zeros(64), gu.dev_zeros(F_ * C_ * n * 2 + 64)
    d_plans, d_po = gu.to_dev(PLANS3), gu.dev_zeros(64)
    d_rec, d_ev, d_cnt, d_work = (gu.dev_zeros(k + 64, 0xEE) for k in (F_ * C_ * 8, 8 * 16, 8, capi.tdet_work_bytes(C_, F_, False)))
    g, cd, pc, pl, po, stt, rec, ev, cnt, wk = (t.data_ptr() for t in (d_g, d_cd, d_pcm, d_plans, d_po, d_state, d_rec, d_ev, d_cnt, d_work))

    def call(g_=g, cd_=cd, pcm_=None, pl_=pl, np_=3, po_=po, C=C_, F=F_, n_=n, state=stt, rec_=rec, ev_=ev, cap=8, cnt_=cnt, wk_=wk, h=ctx.h):
        return L.igdsp_tone_detect(h, g_, cd_, pcm_, pl_, np_, po_, C, F, n_, 0, state, rec_, ev_, cap, cnt_, wk_, None)

    assert call(h=None) == EINVAL
    for kw in (dict(n_=0), dict(n_=161), dict(n_=1), dict(n_=258)):
        assert call(**kw) == EINVAL and call(C=0, **kw) == EINVAL, kw                                # checked even with nothing to do
    assert call(C=0, g_=None, state=None, cnt_=None) == 0 and call(F=0, pcm_=pc, cnt_=None, wk_=None) == 0     # nothing to do comes next
    for kw in (dict(g_=None), dict(pcm_=pc), dict(cd_=None), dict(state=None), dict(pl_=None), dict(np_=0), dict(g_=None, cd_=None, pcm_=pc + 1), dict(g_=None, cd_=None, pcm_=pc + 2), dict(g_=g + 1), dict(ev_=ev + 8),
               dict(po_=po + 1), dict(state=stt + 2), dict(pl_=pl + 2), dict(rec_=rec + 4), dict(ev_=ev + 4), dict(cnt_=cnt + 2), dict(wk_=wk + 8),
               dict(wk_=None), dict(ev_=None), dict(state=g), dict(rec_=g + 8), dict(rec_=stt + SB), dict(ev_=rec), dict(cnt_=rec), dict(wk_=rec + 16),
               dict(rec_=pl + 8), dict(state=po)):
        assert call(**kw) == EINVAL, kw
    assert call(C=0x10000000, F=16) == ERANGE and call(C=0x10000000, F=16, n_=0) == EINVAL
    assert call(rec_=g + 8) == EINVAL and b"must not overlap an input" in (L.igdsp_last_error(ctx.h) or b"")
    assert call(ev_=rec) == EINVAL and b"must not overlap each other" in (L.igdsp_last_error(ctx.h) or b"")
    gu.torch_cuda().cuda.synchronize()
    for t in (d_rec, d_ev, d_cnt, d_work):
        assert (t.cpu().numpy() == 0xEE).all()                                                       # nothing written
    assert not d_state.cpu().numpy().any()
    assert call() == 0 and call(rec_=None, ev_=None, cap=0, cnt_=None, wk_=None) == 0 and call(ev_=None, cap=0) == 0 and call(po_=None, np_=1) == 0
    assert call(C=0) == 0                                                                            # nothing to do with a list: the counts are 0
    gu.torch_cuda().cuda.synchronize()
    assert tuple(d_cnt.cpu().numpy()[:8].view("<u4")) == (0, 0)


# ---- 8. yardstick
def test_yardstick_footprint_and_rules(ctx):
    """igdsp_internal_tdet_move stores exactly the bytes igdsp_tone_detect stores: every record all-zero, the state's history as by
    igdsp_tone_detect, the debounce fields as they were (reserved 0), both counts 0; it rejects what its twin rejects"""
    C_, F_, n = 5, 4, 160
    x, codec, st = scene_with_state(C_, F_, n, 91, PLANS3[:1], None, True)

    def launch(entry):
        def go(fill):
            raw = {}
            go.res = run_tdet(ctx, x, PLANS3[:1], codec, state=st, fill=fill, entry=entry, raw_bytes=raw, cap=0)
            return raw
        return go

    real, yard = launch(None), launch("igdsp_internal_tdet_move")
    gu.assert_same_footprint(gu.written_mask(yard), gu.written_mask(real))
    np.testing.assert_array_equal(yard.res["state"]["hist"], real.res["state"]["hist"])
    for k in ("cur", "cand", "run", "off", "len"):
        np.testing.assert_array_equal(yard.res["state"][k], st[k])
    assert not yard.res["state"]["reserved"].any() and not yard.res["rec"].view(np.uint8).any() and tuple(yard.res["count"]) == (0, 0)
    fn = capi.internal("tdet_move")
    d_state, d_g, d_cd, d_pl = gu.dev_zeros(4 * SB, 0xEE), gu.dev_zeros(2 * 4 * 160 + 64), gu.dev_zeros(64), gu.to_dev(PLANS3)
    stt, g, cd, pl = (t.data_ptr() for t in (d_state, d_g, d_cd, d_pl))

    def call(g_=g, cd_=cd, C=4, F=2, n_=160, state=stt, pl_=pl, h=ctx.h):
        return fn(h, g_, cd_, None, pl_, 3, None, C, F, n_, 0, state, None, None, 0, None, None, None)

    for kw in (dict(h=None), dict(n_=0), dict(n_=3), dict(g_=None), dict(cd_=None), dict(state=None), dict(state=stt + 2), dict(pl_=None), dict(state=g)):
        assert call(**kw) == EINVAL, kw
    assert call(C=0x10000000, F=16) == ERANGE
    gu.torch_cuda().cuda.synchronize()
    assert (d_state.cpu().numpy() == 0xEE).all()


# ---- 9. the generator into the detector, on the device
def test_generate_then_detect(ctx):
    """67 tone ports play staggered digit plans (60 ms on, 60..66 ms off); igdsp_tone_detect on the rows
    igdsp_tone_generate wrote gives the model's records and events on the same rows, and every port's digit string comes back"""
    torch = gu.torch_cuda()
    P_, F_, n = 67, 30, 160
    strings = ["".join(tm.DIGITS[(p + 5 * i) % 16] for i in range(4)) for p in range(P_)]
    plans = np.zeros(P_, capi.TONE_PLAN)
    for p, s in enumerate(strings):
        tones = [(tm.DTMF_LO[tm.DIGITS.index(ch) // 4], tm.DTMF_HI[tm.DIGITS.index(ch) % 4], 60, 60 + p % 7, 8000) for ch in s]   # staggered
        plans[p] = capi.tone_plan_build(tones, 8000, 0)
    d_plans, d_po = gu.to_dev(plans), gu.to_dev(np.arange(P_, dtype="<u2"))
    d_cmd = gu.to_dev(np.full(P_, capi.TONE_CMD_REWIND, np.uint8))
    d_tstate, d_pcm = gu.dev_zeros(P_ * 8), gu.dev_zeros(F_ * P_ * n * 2)
    ctx.tone_generate(d_plans, P_, d_tstate, P_, F_, n, plan_of=d_po, cmd=d_cmd, pcm=d_pcm)
    torch.cuda.synchronize()
    pcm = d_pcm.cpu().numpy().view("<i2").reshape(F_, P_, n)
    got = run_tdet(ctx, pcm, PLANS3[:1])
    rec, _ = check(got, pcm, PLANS3[:1])
    for p in range(P_):
        assert tm.digits_of(got["rec"][:, p]) == strings[p], p
