"""-m "not gpu": the tone detector on the host.  igdsp_tdet_frame (csrc/igdsp_tdet.h, the code the kernel runs) against
tests/tdet_model.py bit for bit: plan, table, records and state at n in {160, 164, 24, 2, 256}, the DTMF plan, a single-group plan of one
tone and an 8 + 8 plan, G.711-decoded and PCM rows, a garbage state, and the overflow bound (PCM of all -32768 against a frequency one
below Nyquist at n = 256).  Then what the rule promises, measured with the model while igdsp_tdet_frame runs the same rows and must give the same bytes: every digit once, twist, frequency offset, talk-off, noise, duration.

Figures (the model, the default thresholds, n = 160 at 8 kHz, 1 200 clean digits per length at random start offsets and phases): the first
length always detected is 36 ms, the last never detected 22 ms (23 ms: 1 of 1 200); the tests hold 40 ms and 20 ms."""
import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import tdet_model as tm

N = 160
PLANS = {"dtmf": tm.plan_dtmf(), "one": tm.plan_single(), "8x8": tm.plan_8x8()}


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


def host_run(plan, rows, state=None):
    """igdsp_tdet_frame over one channel's rows [F][n] -> (records [F], the state after)"""
    st = np.zeros((), capi.TDET_STATE) if state is None else np.array(state, capi.TDET_STATE)
    recs = np.zeros(len(rows), capi.TDET_REC)
    for f, row in enumerate(rows):
        recs[f] = capi.tdet_frame(np.asarray(plan, capi.TDET_PLAN), st, row)
    return recs, st


def model_events(plan, signals, n=N, host=True):
    """signals [C][S] -> per channel the list of (kind, code, evaluation, len) by the model; host: igdsp_tdet_frame runs the same rows
    and gives the same records and state, so what the model shows holds for the C rule the kernel runs"""
    x = tm.frames(np.asarray(signals), n)
    rec, st = tm.detect(plan, x)
    if host:
        for c in range(x.shape[1]):
            r, s = host_run(plan, x[:, c])
            assert r.tobytes() == rec[:, c].tobytes() and s.tobytes() == st[c].tobytes(), f"igdsp_tdet_frame differs from the model on signal {c}"
    return [tm.on_off(rec[:, c]) for c in range(rec.shape[1])]


def one_clean_pair(ev, d):
    return [k for k, *_ in ev] == ["on", "off"] and tm.digit(ev[0][1]) == d and ev[1][1] == ev[0][1]


def burst(d, on, amp_lo, amp_hi=None, lead=200, tail=800, **kw):
    return np.concatenate([np.zeros(lead), tm.dtmf(d, on, amp_lo, amp_hi, **kw), np.zeros(tail)])


# ---- 1. the host function is the model, bit for bit
def test_plans_tables_digits(lib):
    assert capi.tdet_plan_dtmf().tobytes() == PLANS["dtmf"].tobytes()
    assert capi.tdet_plan_build(tm.LO8, tm.HI8).tobytes() == PLANS["8x8"].tobytes()
    assert capi.tdet_plan_build((1000,)).tobytes() == PLANS["one"].tobytes()
    thr = np.array((500, 900, 700, 1500, 200, 4, 5), capi.TDET_THR)
    assert capi.tdet_plan_build((350, 440), (480,), 16000, thr).tobytes() == tm.plan_build((350, 440), (480,), 16000, **{k: int(thr[k]) for k in thr.dtype.names}).tobytes()
    for name, plan in PLANS.items():
        for n in (160, 164, 24, 2, 256):
            t = capi.tdet_table(np.asarray(plan, capi.TDET_PLAN), n)
            assert np.array_equal(t, tm.table(plan, n)), (name, n)
            assert t.min() >= -2047 and t.max() <= 2047
    assert PLANS["dtmf"]["step"][0] == ((697 << 32) + 4000) // 8000                                  # the generator's formula
    assert "".join(capi.tdet_digit(c) for c in range(1, 17)) == tm.DIGITS and capi.tdet_digit(0) == "" and capi.tdet_digit(17) == ""
    for bad in (dict(freq_lo=()), dict(freq_lo=(0,)), dict(freq_lo=(4000,)), dict(freq_lo=(1000,) * 9), dict(freq_lo=(1000,), freq_hi=(1200,) * 9),
                dict(freq_lo=(1000,), clock_rate=8001), dict(freq_lo=(1000,), clock_rate=7000),
                dict(freq_lo=(1000,), thr=np.array((7, 1024, 643, 1615, 218, 2, 2), capi.TDET_THR)),
                dict(freq_lo=(1000,), thr=np.array((400, 1024, 643, 1615, 218, 0, 2), capi.TDET_THR)),
                dict(freq_lo=(1000,), thr=np.array((400, 0, 643, 1615, 218, 2, 2), capi.TDET_THR))):
        with pytest.raises(capi.IgdspError):
            capi.tdet_plan_build(**bad)
    st = np.zeros((), capi.TDET_STATE)
    for n in (0, 1, 161, 258):
        with pytest.raises(capi.IgdspError):
            capi.tdet_frame(np.asarray(PLANS["dtmf"], capi.TDET_PLAN), st, np.zeros(n, np.int16))
        if n:
            with pytest.raises(capi.IgdspError):
                capi.tdet_table(np.asarray(PLANS["dtmf"], capi.TDET_PLAN), n)


@pytest.mark.parametrize("law", ("g711", "pcm"))
@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("n", (160, 164, 24, 2, 256))
def test_frame_matches_model(lib, n, plan, law):
    C_, F_ = 9, max(6, 1600 // n) if n > 2 else 60
    x = tm.scene(C_, F_, n, 100 + n)
    if law == "g711":
        codec = np.where(np.arange(C_) % 3 == 1, 8, 0).astype(np.uint8)
        x = tm.decode(tm.encode(x, codec), codec)
    rec, st = tm.detect(PLANS[plan], x)
    for c in range(C_):
        r, s = host_run(PLANS[plan], x[:, c])
        assert r.tobytes() == rec[:, c].tobytes(), (c, np.nonzero(r.view("<u8") != rec[:, c].view("<u8"))[0][:4])
        assert s.tobytes() == st[c].tobytes()
    if n >= 160 and plan != "one":
        assert rec["flags"].any(), "the scene raises events at this shape"


def test_garbage_state(lib):
    rng = np.random.default_rng(7)
    state = np.frombuffer(rng.integers(0, 256, 6 * capi.TDET_STATE.itemsize, dtype=np.uint8).tobytes(), capi.TDET_STATE).copy()
    x = tm.scene(6, 6, N, 3)
    for name, plan in PLANS.items():
        rec, st = tm.detect(plan, x, state.view(tm.STATE))
        for c in range(6):
            r, s = host_run(plan, x[:, c], state[c])
            assert r.tobytes() == rec[:, c].tobytes() and s.tobytes() == st[c].tobytes(), (name, c)
            assert s["reserved"] == 0


def test_overflow_bound(lib):
    """PCM of all -32768 (v = -4096) against 3 999 Hz, one below Nyquist, at n = 256: the largest |I|, |Q| the rule can meet stay below
    2^31, and host and model agree"""
    assert 4096 * 2047 * 256 < 2 ** 31
    plan = tm.plan_build((3999,), ())
    tab = tm.table(plan, 256)
    assert np.abs(tab).max() <= 2047 and 4096 * int(np.abs(tab[0]).sum(1).max()) < 2 ** 31
    x = np.full((4, 1, 256), -32768, np.int16)
    x[2, 0, 1::2] = 32767                                                                            # and the alternating extreme
    rec, st = tm.detect(plan, x)
    r, s = host_run(plan, x[:, 0])
    assert r.tobytes() == rec[:, 0].tobytes() and s.tobytes() == st[0].tobytes()
    assert s["hist"].min() == -4096


# ---- 2. what the rule promises
@pytest.mark.parametrize("amp", (450, 20000))
def test_all_16_digits(lib, amp):
    """each digit 100 ms on / 100 ms off: exactly one ON with the right code and one OFF"""
    sigs = [burst(d, 800, amp, tail=800) for d in tm.DIGITS]
    for d, ev in zip(tm.DIGITS, model_events(PLANS["dtmf"], sigs)):
        assert one_clean_pair(ev, d), (d, ev)
        assert 6 <= ev[1][3] <= 10, "a 100 ms digit is 6 to 10 evaluations of 10 ms long"


def test_twist(lib):
    """the high tone relative to the low one: -7 .. +3.9 dB is detected, -8.5 and +4.5 dB are not (every digit)"""
    for db in (-7.0, -4.0, 0.0, 3.0, 3.9):
        for d, ev in zip(tm.DIGITS, model_events(PLANS["dtmf"], [burst(d, 800, 5000, 5000 * 10 ** (db / 20)) for d in tm.DIGITS])):
            assert one_clean_pair(ev, d), (db, d, ev)
    for db in (-8.5, 4.5):
        for d, ev in zip(tm.DIGITS, model_events(PLANS["dtmf"], [burst(d, 800, 5000, 5000 * 10 ** (db / 20)) for d in tm.DIGITS])):
            assert ev == [], (db, d, ev)


def test_frequency_offset(lib):
    """both tones off by the same ratio: up to +-1.5 % is detected, +-3.0 % and beyond is not (every digit)"""
    for pct in (-1.5, -1.0, -0.5, 0.5, 1.0, 1.5):
        for d, ev in zip(tm.DIGITS, model_events(PLANS["dtmf"], [burst(d, 800, 5000, f_scale=1 + pct / 100) for d in tm.DIGITS])):
            assert one_clean_pair(ev, d), (pct, d, ev)
    for pct in (-4.0, -3.5, -3.0, 3.0, 3.5, 4.0):
        for d, ev in zip(tm.DIGITS, model_events(PLANS["dtmf"], [burst(d, 800, 5000, f_scale=1 + pct / 100) for d in tm.DIGITS])):
            assert ev == [], (pct, d, ev)


def test_talk_off(lib):
    """a single tone of either group, and 10 s of Gaussian noise at sigma = 3 000, give no event"""
    t = np.arange(8000) / 8000.0
    for ev in model_events(PLANS["dtmf"], [10000 * np.sin(2 * np.pi * f * t) for f in tm.DTMF_LO + tm.DTMF_HI]):
        assert ev == []
    noise = np.random.default_rng(11).normal(0, 3000, (4, 80000))
    for ev in model_events(PLANS["dtmf"], noise):
        assert ev == []


@pytest.mark.parametrize("amp", (1000, 10000))
def test_noise(lib, amp):
    """white noise 10 dB below each tone leaves each digit one clean ON / OFF pair"""
    rng = np.random.default_rng(13)
    sigma = amp / np.sqrt(2) / np.sqrt(10)
    sigs = [burst(d, 800, amp) + rng.normal(0, sigma, 1800) for d in tm.DIGITS]
    for d, ev in zip(tm.DIGITS, model_events(PLANS["dtmf"], sigs)):
        assert one_clean_pair(ev, d), (d, ev)


def _duration_trials(ms, trials, seed):
    rng = np.random.default_rng(seed)
    L = ms * 8
    sigs = []
    for t in range(trials):
        off = int(rng.integers(160, 480))
        sigs.append(np.concatenate([np.zeros(off), tm.dtmf(tm.DIGITS[t % 16], L, 5000, phase=rng.uniform(0, 2 * np.pi, 2)), np.zeros(1440 - off - L)]))
    return sum(1 for ev in model_events(PLANS["dtmf"], sigs) if any(k == "on" for k, *_ in ev))


@pytest.mark.parametrize("ms,always", ((40, True), (45, True), (60, True), (20, False), (15, False), (10, False)))
def test_duration(lib, ms, always):
    """clean digits at random start offsets and phases, 208 per length (13 of every digit): always detected at 40 ms and longer, never at
    20 ms and shorter.  Measured edges (the module's docstring): 36 ms and 22 ms; the bounds here keep that margin."""
    hits = _duration_trials(ms, 208, 1000 + ms)
    assert hits == (208 if always else 0), (ms, hits)


def test_generator_to_detector(lib):
    """igdsp_tone_frame plays "159D" at 60 ms on / 60 ms off into igdsp_tdet_frame: the digit string comes back"""
    tones = [(tm.DTMF_LO[tm.DIGITS.index(ch) // 4], tm.DTMF_HI[tm.DIGITS.index(ch) % 4], 60, 60, 8000) for ch in "159D"]
    tplan = capi.tone_plan_build(tones, 8000, 0)
    tst, st = np.zeros((), capi.TONE_STATE), np.zeros((), capi.TDET_STATE)
    plan = capi.tdet_plan_dtmf()
    out, recs = "", []
    for f in range(30):
        row, ln = capi.tone_frame(tplan, tst, N, capi.TONE_CMD_REWIND if f == 0 else 0)
        rec = capi.tdet_frame(plan, st, row if ln else np.zeros(N, np.int16))
        recs.append(rec)
    recs = np.array(recs, capi.TDET_REC)
    assert tm.digits_of(recs.view(tm.REC)) == "159D"
    assert [k for k, *_ in tm.on_off(recs.view(tm.REC))] == ["on", "off"] * 4


def test_ring_tone_plan(lib):
    """INTEGRATION 18's ring-tone plan, low group {440}, high group {480}: the dual tone raises code 1 for its length, the generator's
    ring tone (igdsp_tone_frame, 440 + 480 Hz) does, 440 Hz or 480 Hz alone raise nothing, nor does a 420 + 500 Hz pair.  Its limit, as
    the document states it: at 160 samples and 8 kHz a bin is 50 Hz wide and the two tones are 40 Hz apart, so one tone between them
    (450 .. 470 Hz) fills both bins alike and reads as the ring tone too"""
    plan = tm.plan_build((440,), (480,))
    t = np.arange(4000) / 8000.0
    sig = lambda *fs: np.concatenate([np.zeros(200), sum(4000 * np.sin(2 * np.pi * f * t) for f in fs), np.zeros(800)])
    ev = model_events(plan, [sig(440, 480), sig(440), sig(480), sig(420, 500), sig(460)])
    assert [k for k, *_ in ev[0]] == ["on", "off"] and ev[0][0][1] == 1 and 47 <= ev[0][1][3] <= 51, ev[0]      # 500 ms: 50 evaluations, up to 3 lost at the edges, 1 gained
    assert ev[1] == [] and ev[2] == [] and ev[3] == []
    assert [k for k, *_ in ev[4]] == ["on", "off"], "the stated limit: a single tone midway reads as the pair"
    tplan, tst, st = capi.tone_plan_build([(440, 480, 400, 200)], 8000, 0), np.zeros((), capi.TONE_STATE), np.zeros((), capi.TDET_STATE)
    recs = []
    for f in range(30):
        row, ln = capi.tone_frame(tplan, tst, N, capi.TONE_CMD_REWIND if f == 0 else 0)
        recs.append(capi.tdet_frame(np.asarray(plan, capi.TDET_PLAN), st, row if ln else np.zeros(N, np.int16)))
    on = tm.on_off(np.array(recs, capi.TDET_REC).view(tm.REC))
    assert [k for k, *_ in on] == ["on", "off"] and on[0][1] == 1 and 37 <= on[1][3] <= 41, on      # 400 ms on


def test_yardstick_is_listed():
    """igdsp_internal_tdet_move is a yardstick with igdsp_tone_detect's arguments, listed beside the other *_move entries"""
    res, args = capi.INTERNAL_MORE["igdsp_internal_tdet_move"]
    pub = {name: (r, a) for name, r, a in capi.PROTOTYPES}["igdsp_tone_detect"]
    assert (res, list(args)) == (pub[0], list(pub[1])) and capi.INTERNAL_MORE_TWIN["igdsp_internal_tdet_move"] == "igdsp_tone_detect"
    assert "igdsp_internal_tdet_move" not in capi.INTERNAL


def test_host_mirror_dtmf_receiver(lib):
    """DtmfReceiver (host/igdsp_host.h) through its C shims: the generator's "159D" comes back digit by digit, a new call empties the
    string, bad shapes give no receiver"""
    import ctypes

    H = ctypes.CDLL(igbuild.HOST_LIB)
    vp, u, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    for name, res, args in (("igdsp_host_dtmf_new", vp, [u, u]), ("igdsp_host_dtmf_free", None, [vp]), ("igdsp_host_dtmf_feed", i, [vp, vp]),
                            ("igdsp_host_dtmf_digits", ctypes.c_char_p, [vp]), ("igdsp_host_dtmf_new_call", None, [vp])):
        fn = getattr(H, name)
        fn.restype, fn.argtypes = res, args
    tones = [(tm.DTMF_LO[tm.DIGITS.index(ch) // 4], tm.DTMF_HI[tm.DIGITS.index(ch) % 4], 60, 60, 8000) for ch in "159D"]
    tplan, tst = capi.tone_plan_build(tones, 8000, 0), np.zeros((), capi.TONE_STATE)
    r = H.igdsp_host_dtmf_new(N, 8000)
    assert r
    try:
        got = []
        for f in range(30):
            row, ln = capi.tone_frame(tplan, tst, N, capi.TONE_CMD_REWIND if f == 0 else 0)
            row = np.ascontiguousarray(row if ln else np.zeros(N, np.int16))
            got.append(H.igdsp_host_dtmf_feed(r, row.ctypes.data))
        assert "".join(chr(g) for g in got if g) == "159D" and H.igdsp_host_dtmf_digits(r) == b"159D"
        H.igdsp_host_dtmf_new_call(r)
        assert H.igdsp_host_dtmf_digits(r) == b"" and H.igdsp_host_dtmf_feed(r, None) == -22 and H.igdsp_host_dtmf_feed(None, row.ctypes.data) == -22
    finally:
        H.igdsp_host_dtmf_free(r)
    for bad in ((0, 8000), (161, 8000), (258, 8000), (160, 7000)):
        assert not H.igdsp_host_dtmf_new(*bad)
