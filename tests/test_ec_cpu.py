"""igdsp_ec_frame (csrc/igdsp_ec.h through the C ABI, no GPU) against tests/ec_model.py, bit for bit: output, record, state; then what
the rule is worth, each property stated against a reference run on the same input and each asserting the model's bytes first.
The rule is the library's own, UNVERIFIED against ITU-T G.168 and against any other canceller: what these tests show is what is promised."""
import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import ec_model as em
from tests import tdet_model

TAILS = (128, 256)
SEEDS = (0, 1, 2)
LAW_OF_SEED = {0: 0, 1: 8, 2: 0}                                           # mu-law, A-law, mu-law


@pytest.fixture(scope="module", autouse=True)
def lib():
    igbuild.build()
    return capi.load()


def ccfg(cfg):
    return np.asarray(cfg).view(capi.EC_CFG)


def host_frames(cfg, near, far, ctl=None, state=None):
    """igdsp_ec_frame over near [F][C][n] / far [F][P][n] (row c of far, None: no far end), as em.cancel walks them"""
    F_, C_, n = near.shape
    st = np.zeros(C_, capi.EC_STATE) if state is None else np.array(state).view(capi.EC_STATE).copy()
    out = np.zeros((F_, C_, n), np.int16)
    rec = np.zeros((F_, C_), capi.EC_REC)
    for c in range(C_):
        k = em.RUN if ctl is None else int(ctl[c])
        s = st[c:c + 1].reshape(())
        for f in range(F_):
            out[f, c], rec[f, c] = capi.ec_frame(ccfg(cfg), s, near[f, c], None if far is None or c >= far.shape[1] else far[f, c], k)
            if k == em.RESET or k > 3:
                k = em.RUN
    return out, rec, st


def same(host, model):
    (o, r, s), (mo, mr, _, ms) = host, model
    assert np.array_equal(o, mo), np.argwhere(o != mo)[:4]
    assert r.tobytes() == mr.tobytes(), [(k, r[k][r[k] != mr[k]][:3], mr[k][r[k] != mr[k]][:3]) for k in mr.dtype.names if not np.array_equal(r[k], mr[k])]
    assert s.tobytes() == ms.tobytes(), [k for k in ms.dtype.names if not np.array_equal(s[k], ms[k])]


def test_layouts_and_defaults():
    assert capi.EC_CFG.itemsize == em.CFG.itemsize == 12 and capi.EC_STATE.itemsize == em.STATE.itemsize == 1552 <= 1664
    assert capi.EC_REC.itemsize == em.REC.itemsize == 16
    for a, b in ((capi.EC_CFG, em.CFG), (capi.EC_STATE, em.STATE), (capi.EC_REC, em.REC)):
        assert a.names == b.names and [a.fields[k][1] for k in a.names] == [b.fields[k][1] for k in b.names]
    for L in TAILS:
        assert capi.ec_cfg_default(L).tobytes() == em.cfg_default(L).tobytes()
    assert (capi.EC_RUN, capi.EC_FREEZE, capi.EC_BYPASS, capi.EC_RESET) == (em.RUN, em.FREEZE, em.BYPASS, em.RESET)
    assert (capi.EC_ADAPTED, capi.EC_DOUBLETALK, capi.EC_FAR_ACTIVE, capi.EC_W_SATURATED, capi.EC_BYPASSED) == (1, 2, 4, 8, 16)


def test_rejects():
    st, x = np.zeros((), capi.EC_STATE), np.zeros(160, np.int16)
    L = capi.load()
    p = lambda a: a.ctypes.data
    for n in (0, 1, 3, 161, 258):
        assert L.igdsp_ec_frame(None, p(st), p(np.zeros(300, np.int16)), None, n, 0, None, None) == -22
    for bad in (dict(tail=64), dict(tail=255), dict(tail=512), dict(mu_shift=7)):
        c = em.cfg_default(128)
        for k, v in bad.items():
            c[k] = v
        assert L.igdsp_ec_frame(p(c), p(st), p(x), p(x), 160, 0, None, None) == -22
    assert L.igdsp_ec_frame(None, None, p(x), p(x), 160, 0, None, None) == -22
    assert L.igdsp_ec_frame(None, p(st), None, p(x), 160, 0, None, None) == -22
    assert L.igdsp_ec_frame(None, p(st), p(x), p(x), 160, 0, None, None) == 0       # out and rec optional, cfg NULL: tail 128
    assert int(st["tag"]) == capi.EC_TAG | 128


@pytest.mark.parametrize("n", (160, 164, 24, 2, 256))
@pytest.mark.parametrize("L", TAILS)
def test_frame_matches_model(L, n):
    """a fresh and a garbage state, PCM and both laws' decoded values; the scene adapts, fires the detector and runs the hang"""
    C_, F_ = 4, 6
    cfg = em.cfg_default(L)
    near, far = em.small_scene(C_, F_, n, seed=n + L)
    tot = np.zeros(3, np.int64)
    for law in (None, 0, 8):
        if law is not None:
            codec = np.full(C_, law, np.uint8)
            near_l = tdet_model.decode(tdet_model.encode(near, codec), codec)
        else:
            near_l = near
        for st0 in (None, em.garbage_state(C_, L, n)):
            m = em.cancel(cfg, near_l, far, state=st0)
            same(host_frames(cfg, near_l, far, state=st0), m)
            tot += (int(m[1]["n_adapt"].sum()), int(m[1]["n_dt"].sum()), int((m[1]["flags"] & em.FAR_ACTIVE).astype(bool).sum()))
    assert np.all(tot > 0), tot                                            # the scene exercises adaptation, the detector and pmin


@pytest.mark.parametrize("L", TAILS)
def test_every_ctl_and_a_missing_far_end(L):
    C_, F_, n = 6, 3, 24
    cfg = em.cfg_default(L, hang=2, dmin=0)
    near, far = em.small_scene(C_, F_, n, seed=3, P_=5)                    # channel 5 has no far row
    ctl = np.array([200, em.FREEZE, em.BYPASS, em.RESET, em.RUN, em.RUN], np.uint8)       # 200: as RUN
    st0 = em.garbage_state(C_, L, 1)
    st0["hang"] = 0
    m = em.cancel(cfg, near, far, ctl=ctl, state=st0)
    same(host_frames(cfg, near, far, ctl, st0), m)
    out, rec, _, st = m
    assert np.array_equal(st["w"][1], np.where(np.arange(256) < L, st0["w"][1], 0)) and not rec["n_adapt"][:, 1].any()   # FREEZE leaves w
    for c in (2, 5):                                                       # BYPASS and no far end: the near row, the weights as they were
        assert np.array_equal(out[:, c], near[:, c]) and np.all(rec["flags"][:, c] == em.BYPASSED)
        assert np.array_equal(st["w"][c, :L], st0["w"][c, :L]) and np.all(rec["near_e"][:, c] == rec["out_e"][:, c])
    assert F_ * n < L and np.array_equal(st["hist"][2, :L], np.concatenate([np.clip(st0["hist"][2, :L], -8192, 8191)[F_ * n:],
                                                                            far[:, 2].reshape(-1) >> 2]))   # BYPASS: the history still advances
    assert np.all(st["hist"][5, :L][-F_ * n:] == 0)                        # no far end: zeros pass through the history
    fresh = em.cancel(cfg, near[:, 3:4], far[:, 3:4])                      # RESET from garbage equals a fresh state
    assert np.array_equal(out[:, 3], fresh[0][:, 0]) and st[3].tobytes() == fresh[3][0].tobytes() and rec[:, 3].tobytes() == fresh[1][:, 0].tobytes()
    # a state of another tail's tag, or of no tag, starts as the reset state too
    other = em.garbage_state(1, 384 - L, 2)
    a = em.cancel(cfg, near[:, :1], far[:, :1], state=other)
    same(host_frames(cfg, near[:, :1], far[:, :1], state=other), a)
    b = em.cancel(cfg, near[:, :1], far[:, :1])
    assert np.array_equal(a[0], b[0]) and a[3].tobytes() == b[3].tobytes()
    assert rec["n_adapt"][:, 0].sum() > 0 and rec["n_adapt"][:, 3].sum() > 0


@pytest.mark.parametrize("L", TAILS)
def test_overflow_bound(L):
    """full-scale rows against a saturated garbage state, the detector unable to hold the update (hang 0) and the largest step: every
    lane-sized sum reaches the bound igdsp_ec.h asserts, weights clip at both ends"""
    C_, F_, n = 3, 3, 164
    rng = np.random.default_rng(9)
    near = np.where(rng.integers(0, 2, (F_, C_, n)) == 1, 32767, -32768).astype(np.int16)
    far = near.copy()
    far[:, 1] = -32768                                                     # xs = -8192 throughout: P = L 2^26, the products all of one sign
    far[:, 2] = 32767
    near[:, 2] = -32768
    for mu in (0, 6):
        cfg = em.cfg_default(L, hang=0, mu_shift=mu, pmin=0)
        st0 = em.garbage_state(C_, L, 4, saturated=True)
        st0["w"][1] = -(1 << 31)                                           # wh = -8192 against xs = -8192: acc = L 2^26
        m = em.cancel(cfg, near, far, state=st0)
        same(host_frames(cfg, near, far, state=st0), m)
        assert m[1]["n_adapt"].min() == (n + 7) // 8
        if mu == 0:
            assert np.all(m[1]["flags"][0] & em.W_SATURATED) and np.all(m[3]["flags"] == em.W_SATURATED) and m[1]["wmax"].max() == 8192
    assert L * (1 << 26) <= 1 << 34 and 16 * (1 << 26) <= 1 << 30


def test_split_at_every_point():
    L, C_, F_, n = 128, 3, 5, 24
    cfg = em.cfg_default(L, hang=3, dmin=0)
    near, far = em.small_scene(C_, F_, n, seed=8)
    whole = em.cancel(cfg, near, far)
    same(host_frames(cfg, near, far), whole)
    for k in range(1, F_):
        a = em.cancel(cfg, near[:k], far[:k])
        b = em.cancel(cfg, near[k:], far[k:], state=a[3])
        assert np.array_equal(np.concatenate([a[0], b[0]]), whole[0]) and np.concatenate([a[1], b[1]]).tobytes() == whole[1].tobytes()
        assert b[3].tobytes() == whole[3].tobytes()
        same(host_frames(cfg, near[k:], far[k:], state=a[3]), b)


@pytest.mark.parametrize("L", TAILS)
def test_silent_far_end_changes_nothing(L):
    C_, F_, n = 2, 3, 160
    near, _ = em.small_scene(C_, F_, n, seed=2)
    far = np.zeros((F_, C_, n), np.int16)
    far[:, 1] = 3                                                          # xs = 0 as well
    cfg = em.cfg_default(L, dmin=0)
    st0 = em.garbage_state(C_, L, 6)
    st0["hist"], st0["hang"], st0["flags"] = 0, 0, 0
    m = em.cancel(cfg, near, far, state=st0)
    same(host_frames(cfg, near, far, state=st0), m)
    assert not m[1]["n_adapt"].any() and not (m[1]["flags"] & (em.ADAPTED | em.FAR_ACTIVE)).any()
    assert np.array_equal(m[3]["w"][:, :L], st0["w"][:, :L]) and not m[3]["hist"].any()
    assert np.array_equal(m[0], near)                                      # a zero history under any weights predicts zero


# ---- what the rule is worth.  One run per (seed, L, scene), shared; the host function over the same rows must give the model's bytes
def _run_model(cfg, far, near, n=160):
    F_ = len(near) // n
    return em.cancel(cfg, near.reshape(F_, 1, n), far.reshape(F_, 1, n))


def _run_host(cfg, far, near, n=160):
    F_ = len(near) // n
    return host_frames(cfg, near.reshape(F_, 1, n), far.reshape(F_, 1, n))


def _run_f64(cfg, far, near, n=160, detector=True):
    st = em.fresh_f64(int(cfg["tail"]))
    return np.concatenate([em.frame_f64(cfg, st, near[i:i + n], far[i:i + n], detector) for i in range(0, len(near), n)])


@pytest.fixture(scope="module")
def single():
    res = {}
    for L in TAILS:
        for seed in SEEDS:
            far, near, _ = em.echo_scene(seed, law=LAW_OF_SEED[seed])
            cfg = em.cfg_default(L)
            h = _run_host(cfg, far, near)
            same(h, _run_model(cfg, far, near))
            res[L, seed] = (near, h[0].reshape(-1), _run_f64(cfg, far, near))
    return res


def test_integer_loss(single):
    """the integer rule against the float64 statement of the same algorithm: at most 0.5 dB of ERLE lost in any second (measured: at most
    0.07 dB over these runs)"""
    for (L, seed), (near, out, f64) in single.items():
        loss = em.erle_db(near, f64) - em.erle_db(near, out)
        print(f"L {L} seed {seed}: ERLE lost per second {np.round(loss, 3).tolist()}")
        assert loss.max() <= 0.5, (L, seed, loss)


# measured with this model and generator, eighth second, seeds 0 1 2: L = 256: 19.20 21.35 21.90 dB; L = 128: 20.45 21.84 22.37 dB.
# The floor is 2 dB under the minimum (and not below 15 / 17 dB)
SINGLE_FLOOR = {256: 17.2, 128: 18.4}


def test_single_talk(single):
    assert SINGLE_FLOOR[256] >= 15.0 and SINGLE_FLOOR[128] >= 17.0
    for (L, seed), (near, out, _) in single.items():
        e = em.erle_db(near, out)
        print(f"L {L} seed {seed}: ERLE per second {np.round(e, 2).tolist()}")
        assert e[-1] >= SINGLE_FLOOR[L], (L, seed, e)


@pytest.mark.parametrize("L", TAILS)
def test_double_talk(L):
    """a talker of the far end's level through the sixth second.  First, on seed 1 at L = 128: without the hold (hang 0 adapts through the
    talker) the ERLE of the second after the burst falls below 0 dB, so the condition can fail.  Then with the defaults: the talker's
    energy is kept within 1 dB and the ERLE of the second after the burst is at least 10 dB (measured: kept within 0.11 dB, 16.8 dB and more)"""
    if L == 128:
        far, near, _ = em.echo_scene(1, law=LAW_OF_SEED[1], talk=(5, 6))
        c0 = em.cfg_default(L, hang=0)
        h0 = _run_host(c0, far, near)
        same(h0, _run_model(c0, far, near))
        e0 = em.erle_db(near, h0[0].reshape(-1))
        print(f"hang 0, seed 1: ERLE per second {np.round(e0, 2).tolist()}")
        assert e0[6] < 0.0, e0
    cfg = em.cfg_default(L)
    for seed in SEEDS:
        far, near, talker = em.echo_scene(seed, law=LAW_OF_SEED[seed], talk=(5, 6))
        h = _run_host(cfg, far, near)
        same(h, _run_model(cfg, far, near))
        out = h[0].reshape(-1).astype(np.float64)
        e = em.erle_db(near, out)
        keep = 10.0 * np.log10((out[40000:48000] ** 2).sum() / (talker[40000:48000] ** 2).sum())
        print(f"L {L} seed {seed}: talker kept within {keep:+.2f} dB, ERLE per second {np.round(e, 2).tolist()}")
        assert abs(keep) <= 1.0 and e[6] >= 10.0, (L, seed, keep, e)


def test_yardstick_is_bound_like_the_entry():
    res, args = capi.INTERNAL_MORE["igdsp_internal_ec_move"]
    pub = {name: (r, a) for name, r, a in capi.PROTOTYPES}["igdsp_echo_cancel"]
    assert (res, list(args)) == (pub[0], list(pub[1])) and capi.INTERNAL_MORE_TWIN["igdsp_internal_ec_move"] == "igdsp_echo_cancel"
    assert "igdsp_internal_ec_move" not in capi.INTERNAL


def test_host_mirror_echo_canceller():
    """EchoCanceller (host/igdsp_host.h) through its C shims: the frames of a scene give igdsp_ec_frame's bytes, the record and the ERLE
    of the last frame are readable, reset forgets the filter, bad shapes give no canceller"""
    import ctypes

    H = ctypes.CDLL(igbuild.HOST_LIB)
    vp, u, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    for name, res, args in (("igdsp_host_ec_new", vp, [u, u]), ("igdsp_host_ec_free", None, [vp]), ("igdsp_host_ec_cancel", i, [vp, vp, vp, vp, u]),
                            ("igdsp_host_ec_rec", i, [vp, vp]), ("igdsp_host_ec_erle_db", ctypes.c_float, [vp]), ("igdsp_host_ec_reset", None, [vp])):
        fn = getattr(H, name)
        fn.restype, fn.argtypes = res, args
    n, L = 160, 256
    far, near, _ = em.echo_scene(0, seconds=1)
    cfg = em.cfg_default(L)
    want = _run_model(cfg, far, near, n)
    e = H.igdsp_host_ec_new(n, L)
    assert e
    try:
        out, rec = np.zeros(n, np.int16), np.zeros((), capi.EC_REC)
        for f in range(len(near) // n):
            a, b = np.ascontiguousarray(near[f * n:(f + 1) * n]), np.ascontiguousarray(far[f * n:(f + 1) * n])
            assert H.igdsp_host_ec_cancel(e, a.ctypes.data, b.ctypes.data, out.ctypes.data, em.RUN) == 0
            assert np.array_equal(out, want[0][f, 0]) and H.igdsp_host_ec_rec(e, rec.ctypes.data) == 0 and rec.tobytes() == want[1][f, 0].tobytes()
        assert abs(H.igdsp_host_ec_erle_db(e) - 10.0 * np.log10(float(rec["near_e"]) / float(rec["out_e"]))) < 1e-3 and rec["wmax"] > 0
        assert H.igdsp_host_ec_cancel(e, a.ctypes.data, None, out.ctypes.data, em.RUN) == 0 and np.array_equal(out, a)      # nothing was played
        H.igdsp_host_ec_reset(e)
        assert H.igdsp_host_ec_cancel(e, a.ctypes.data, b.ctypes.data, out.ctypes.data, em.FREEZE) == 0 and np.array_equal(out, a)   # no filter left
        assert H.igdsp_host_ec_cancel(e, None, b.ctypes.data, out.ctypes.data, 0) == -22 and H.igdsp_host_ec_cancel(None, a.ctypes.data, None, out.ctypes.data, 0) == -22
    finally:
        H.igdsp_host_ec_free(e)
    for bad in ((0, 128), (161, 128), (258, 256), (160, 64), (160, 0)):
        assert not H.igdsp_host_ec_new(*bad)


@pytest.mark.parametrize("L", TAILS)
def test_detector_edges(L):
    """the double-talk test at its two edges.  Equality does not fire: 2 dmax == xmax holds the hang down, one more fires.  xmax looks
    L + b values back: a far peak that has left the filter's L values but not the block's first sample still holds the detector off"""
    n = 8
    cfg = em.cfg_default(L, hang=1, dmin=0)
    far = np.full((4, 1, n), 4000, np.int16)                               # xs = 1000: xmax = 4000
    for level, fires in ((2000, False), (2001, True), (-2000, False), (-2001, True)):
        near = np.full((4, 1, n), level, np.int16)
        m = em.cancel(cfg, near, far)
        same(host_frames(cfg, near, far), m)
        assert bool(m[1]["n_dt"].any()) == fires and np.all((m[1]["n_dt"] == 1) == fires), (level, m[1]["n_dt"])
    F_ = L // 8 + 3
    far = np.full((F_, 1, n), 400, np.int16)                               # xmax = 400 without the peak
    far[0, 0, 4] = 32000                                                   # xs = 8000 at sample 4
    near = np.full((F_, 1, n), 1000, np.int16)                             # 2 dmax = 2000: fires unless the peak is in sight
    m = em.cancel(cfg, near, far)
    same(host_frames(cfg, near, far), m)
    # the block of frame f ends at 8 f + 8 and sees samples 8 f - L .. 8 f + 7: sample 4 is in sight up to f = L / 8
    assert m[1]["n_dt"][:, 0].tolist() == [0] * (L // 8 + 1) + [1, 1]
