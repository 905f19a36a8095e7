"""-m "not gpu": best signal selection without a device — tests/bss_model.py against the host mirror's BssVoter (the reference's
four-radio block restated literally), hand-derived cases citing roip_ed137.cpp, split invariance of the model with the state carried,
and the C entry's NULL-context rule."""
import ctypes

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import build as igbuild
from igate4xsoftphonedsp_amd import capi
from tests import bss_model as bm

W = bm.word
EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    igbuild.build()
    return capi.load()


@pytest.fixture(scope="module")
def host(lib):
    H = ctypes.CDLL(igbuild.HOST_LIB)
    vp, i = ctypes.c_void_p, ctypes.c_int
    for name, res, args in (("igdsp_host_bss_new", vp, [i, i]), ("igdsp_host_bss_free", None, [vp]),
                            ("igdsp_host_bss_tick", i, [vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(i), i]),
                            ("igdsp_host_bss_state", i, [vp, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(ctypes.c_uint)])):
        getattr(H, name).restype = res
        getattr(H, name).argtypes = args
    return H


def infos(rows):
    """RTP_INFO [F][C] from rows of (word, pt, flags) per channel; a bare int is a PT-0 packet carrying that word"""
    F_, C_ = len(rows), len(rows[0])
    a = np.zeros((F_, C_), capi.RTP_INFO)
    for f, row in enumerate(rows):
        for c, x in enumerate(row):
            w, pt, fl = (x, 0, 0) if isinstance(x, int) else x
            a[f, c] = (w, 160, pt, fl)
    return a


def run(rows, group_ptr=(0, 4), members=(0, 1, 2, 3), C_=None, vf=3, state=None, words=None, mute=None):
    info = infos(rows)
    C_ = info.shape[1] if C_ is None else C_
    G_ = len(group_ptr) - 1
    st = np.zeros((G_, 4), np.uint32) if state is None else state
    wd = np.zeros(len(members), np.uint32) if words is None else words
    return bm.select(info, np.array(group_ptr), np.array(members), len(members), C_, G_, st, wd, vf, mute)


# ---------------------------------------------------------------- the model equals the host mirror (4 radios, 5 ticks)
def test_model_equals_bss_voter(host):
    rng = np.random.default_rng(137)
    for trial in range(12):
        T = 600
        p_open = rng.uniform(0.2, 0.9)
        sq = rng.random((T, 4)) < p_open
        # squelch runs: hold each radio's state for a few ticks so that votes, latches and re-votes all happen
        hold = rng.integers(1, 12, (T, 4))
        for r in range(4):
            t = 0
            while t < T:
                sq[t:t + hold[t, r], r] = sq[t, r]
                t += hold[t, r]
        q = rng.integers(0, 32, (T, 4)) if trial % 3 else rng.integers(0, 3, (T, 4))     # few BSS values: many ties
        up = rng.random((T, 4)) < (0.97 if trial % 2 else 1.0)
        mute = rng.random(T) < (0.03 if trial % 4 == 1 else 0.0)
        v = host.igdsp_host_bss_new(5, 0)
        try:
            got = []
            for t in range(T):
                ws = (ctypes.c_uint32 * 4)(*[W(sq[t, r], int(q[t, r]), ptt_type=int(rng.integers(0, 8))) for r in range(4)])
                cu = (ctypes.c_int * 4)(*[int(x) for x in up[t]])
                got.append(host.igdsp_host_bss_tick(v, ws, cu, int(mute[t])))
            cnt, on, votes = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint()
            assert host.igdsp_host_bss_state(v, ctypes.byref(cnt), ctypes.byref(on), ctypes.byref(votes)) == 0
        finally:
            host.igdsp_host_bss_free(v)
        # the same ticks through the model: one frame per tick, one group of 4 members; a dropped call is member >= C (remapped)
        exp = []
        st = np.zeros((1, 4), np.uint32)
        wd = np.zeros(4, np.uint32)
        for t in range(T):
            words_t = [W(sq[t, r], int(q[t, r])) for r in range(4)]
            info = infos([[x for x in words_t] + [0]])
            members = np.array([r if up[t, r] else 4 + 1 for r in range(4)], np.uint32)      # 5 >= C = 5: the call is not up
            s, st, wd = bm.select(info, np.array([0, 4]), members, 4, 5, 1, st, wd, 5, np.array([int(mute[t])]))
            exp.append(int(s[0, 0]))
        # the model's sel is a channel (= radio index here), the mirror's result a radio index
        assert got == exp, f"trial {trial}: first difference at tick {next(i for i in range(T) if got[i] != exp[i])}"
        assert (cnt.value, on.value, votes.value) == (int(st[0, 0]), int(st[0, 2]), int(st[0, 3]))


def test_bss_voter_null_handle(host):
    ws = (ctypes.c_uint32 * 4)()
    cu = (ctypes.c_int * 4)()
    assert host.igdsp_host_bss_tick(None, ws, cu, 0) == EINVAL
    assert host.igdsp_host_bss_state(None, None, None, None) == EINVAL


def test_bss_voter_stale_last_rx_quirk(host):
    """with the reference's stale lastRx a dropped call keeps the count running (roip_ed137.cpp:6027: lastRx > 0 of any radio)"""
    v = host.igdsp_host_bss_new(2, 1)
    try:
        open1 = (ctypes.c_uint32 * 4)(W(1, 3), 0, 0, 0)
        up = (ctypes.c_int * 4)(1, 1, 1, 1)
        down = (ctypes.c_int * 4)(0, 1, 1, 1)
        assert host.igdsp_host_bss_tick(v, open1, up, 0) == -1
        assert host.igdsp_host_bss_tick(v, open1, up, 0) == 0                    # voted at the 2nd tick
        assert host.igdsp_host_bss_tick(v, open1, down, 0) == -1                 # call down: vote dropped (:5987-5996)
        cnt = ctypes.c_int()
        host.igdsp_host_bss_state(v, ctypes.byref(cnt), None, None)
        assert cnt.value == 1                                                    # ... but its stale lastRx counts on
    finally:
        host.igdsp_host_bss_free(v)


# ---------------------------------------------------------------- hand-derived cases
def test_vote_lands_on_the_threshold_frame():
    """sqlStatusCount++ then >= 5 (here vote_frames 3) and !sqlStatusOn (roip_ed137.cpp:6027-6031)"""
    sel, st, _ = run([[W(1, 4), 0, 0, 0]] * 4, vf=3)
    assert sel[:, 0].tolist() == [-1, -1, 0, 0]
    assert st[0].tolist() == [4, 1, 1, 1]


def test_latch_stronger_receiver_does_not_take_over():
    """once sqlStatusOn, the chain at :6047-6110 is not re-entered"""
    rows = [[W(1, 4), 0, 0, 0]] * 3 + [[W(1, 4), W(1, 30), 0, 0]] * 3
    sel, st, _ = run(rows, vf=3)
    assert sel[:, 0].tolist() == [-1, -1, 0, 0, 0, 0]
    assert st[0, 3] == 1


def test_tie_goes_to_the_first_member():
    """rssi >= every other and lastRx: the first branch of the if/else chain (:6047) wins a tie"""
    sel, _, _ = run([[0, W(1, 9), W(1, 9), W(1, 9)]] * 3, vf=3)
    assert sel[2, 0] == 1
    # member order, not channel order, is the tie order
    sel, _, _ = run([[0, W(1, 9), W(1, 9), W(1, 9)]] * 3, members=(3, 2, 1, 0), vf=3)
    assert sel[2, 0] == 3


def test_highest_bss_wins_the_vote():
    sel, _, _ = run([[W(1, 2), W(1, 7), W(1, 31), W(1, 30)]] * 3, vf=3)
    assert sel[2, 0] == 2


def test_revote_after_the_voted_receiver_closes():
    """the voted radio closes (:5989-5993: count 0, on false), others open: count++ makes it 1 in that same tick (:6029)"""
    rows = [[W(1, 20), W(1, 5), 0, 0]] * 3 + [[W(0, 20), W(1, 5), 0, 0]] * 4
    sel, st, _ = run(rows, vf=3)
    assert sel[:, 0].tolist() == [-1, -1, 0, -1, -1, 1, 1]
    _, st4, _ = run(rows[:4], vf=3)
    assert st4[0].tolist() == [1, 0, 0, 1]                                     # count 1 in the closing frame
    assert st[0].tolist() == [4, 2, 1, 2]


def test_reset_when_all_close():
    """no lastRx at all: sqlStatusCount 0, sqlStatusOn false, no radio voted (:6111-6117)"""
    rows = [[W(1, 3), W(1, 3), 0, 0]] * 3 + [[0, 0, 0, 0]] + [[W(1, 3), 0, 0, 0]] * 2
    sel, st, _ = run(rows, vf=3)
    assert sel[:, 0].tolist() == [-1, -1, 0, -1, -1, -1]
    assert st[0].tolist() == [2, 0, 0, 1]


def test_word_sticks_across_runts_and_other_payload_types():
    """transport_rtp_cb stores the word for PT 0 / 8 / 18 / 123 only (TransportAdapter.cpp:247-256); a runt (no packet) keeps it"""
    runt = (0, 0, bm.RTP_RUNT)
    pt96 = (0, 96, 0)
    rows = [[W(1, 6), 0, 0, 0], [runt, 0, 0, 0], [pt96, 0, 0, 0], [(0, 123, 0), 0, 0, 0]]
    sel, _, words = run(rows, vf=3)
    assert sel[:, 0].tolist() == [-1, -1, 0, -1]                               # open through the runt and PT 96, closed by the keep-alive
    assert words[0] == 0
    # PT 18 (G.729) updates the word
    sel, _, words = run([[W(1, 6), 0, 0, 0], [(W(0, 0), 18, 0), 0, 0, 0]], vf=1)
    assert sel[:, 0].tolist() == [0, -1]
    # an all-zero record is a PT-0 packet carrying word 0: it closes the receiver
    sel, _, _ = run([[W(1, 6), 0, 0, 0], [0, 0, 0, 0]], vf=1)
    assert sel[:, 0].tolist() == [0, -1]


def test_mute_closes_the_group():
    """forceMuteSqlOn / group PTT under MUTEALL forces sqlon false (roip_ed137.cpp:5630-5642)"""
    sel, st, words = run([[W(1, 6), W(1, 2), 0, 0]] * 4, vf=1, mute=np.array([1]))
    assert (sel == -1).all() and st[0].tolist() == [0, 0, 0, 0]
    assert words.tolist()[:2] == [W(1, 6), W(1, 2)]                             # the words are still stored


def test_members_past_c_are_calls_that_are_not_up():
    sel, _, words = run([[W(1, 6), W(1, 31)]] * 2, group_ptr=(0, 3), members=(0, 7, 1), C_=2, vf=1)
    assert sel[:, 0].tolist() == [1, 1]
    assert words.tolist() == [W(1, 6), 0, W(1, 31)]


def test_voted_member_past_c_in_a_start_state_resets():
    st0 = np.array([[9, 2, 1, 4]], np.uint32)
    sel, st, _ = run([[W(1, 6), 0]], group_ptr=(0, 2), members=(0, 5), C_=2, vf=5, state=st0)
    assert sel[0, 0] == -1 and st[0].tolist() == [1, 0, 0, 4]


def test_reversed_group_ptr_is_an_empty_group():
    rows = [[W(1, 6), W(1, 9), W(1, 1), W(1, 2)]] * 2
    sel, st, _ = run(rows, group_ptr=(0, 2, 1, 4), members=(0, 1, 2, 3), vf=1)
    assert sel[:, 0].tolist() == [1, 1]                                        # group 0: members 0, 1
    assert sel[:, 1].tolist() == [-1, -1] and st[1].tolist() == [0, 0, 0, 0]    # group 1: [2, 1) is empty
    assert sel[:, 2].tolist() == [1, 1]                                        # group 2: slots 1 .. 3
    # values past n_members are clamped
    sel, _, _ = run(rows, group_ptr=(0, 9, 99), members=(0, 1, 2, 3), vf=1)
    assert sel[:, 0].tolist() == [1, 1] and sel[:, 1].tolist() == [-1, -1]


def test_count_saturates():
    st0 = np.array([[0xFFFFFFFF, 1, 1, 0xFFFFFFFF]], np.uint32)
    _, st, _ = run([[W(1, 1), 0, 0, 0]], state=st0, words=np.array([W(1, 1), 0, 0, 0], np.uint32))
    assert st[0].tolist() == [0xFFFFFFFF, 1, 1, 0xFFFFFFFF]


def test_emit_is_a_one_member_conf_mix():
    from tests import conf_model as cm

    rng = np.random.default_rng(3)
    x = rng.integers(-32768, 32768, (2, 3, 16)).astype(np.int64)
    gain = np.array([128, 300, 0], np.uint16)
    length = np.array([[16, 5, 16], [0, 16, 16]], np.uint16)
    sel = np.array([[1, -1, 2], [0, 1, -1]], np.int32)
    out, st = bm.emit(sel, x, 16, gain, length)
    for f in range(2):
        for g in range(3):
            c = sel[f, g]
            if c < 0:
                assert st["flags"][f, g] == cm.FLAG_EMPTY and not out[f, g].any()
                continue
            o, s = cm.mix(x[f:f + 1], gain, np.array([0, 1]), np.array([c]), 1, 1, length[f:f + 1])
            np.testing.assert_array_equal(out[f, g], o[0, 0])
            for k in ("sumsq", "peak", "flags"):
                assert st[k][f, g] == s[k][0, 0], k


# ---------------------------------------------------------------- split invariance of the model
def _random_case(rng, F_, C_, G_):
    sizes = rng.integers(0, 7, G_)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    mem = rng.integers(0, C_ + 2, int(ptr[-1])).astype(np.uint32)
    info = np.zeros((F_, C_), capi.RTP_INFO)
    info["ed137"] = [[W(rng.random() < 0.6, int(rng.integers(0, 4))) for _ in range(C_)] for _ in range(F_)]
    info["pt"] = rng.choice([0, 8, 18, 96, 123], (F_, C_), p=[0.6, 0.2, 0.05, 0.05, 0.1])
    info["flags"] = np.where(rng.random((F_, C_)) < 0.1, bm.RTP_RUNT, 0)
    return ptr, mem, info


def test_model_split_invariance():
    rng = np.random.default_rng(11)
    F_, C_, G_ = 40, 12, 5
    ptr, mem, info = _random_case(rng, F_, C_, G_)
    st0 = np.zeros((G_, 4), np.uint32)
    wd0 = np.zeros(len(mem), np.uint32)
    sel, st, wd = bm.select(info, ptr, mem, len(mem), C_, G_, st0, wd0, 4)
    for cuts in ([1] * F_, [3, 7, 30], [F_ - 1, 1]):
        s, w = st0, wd0
        parts = []
        f0 = 0
        for k in cuts:
            p, s, w = bm.select(info[f0:f0 + k], ptr, mem, len(mem), C_, G_, s, w, 4)
            parts.append(p)
            f0 += k
        np.testing.assert_array_equal(np.concatenate(parts), sel)
        np.testing.assert_array_equal(s, st)
        np.testing.assert_array_equal(w, wd)


# ---------------------------------------------------------------- the C entry without a device
def test_null_context_is_einval(lib):
    args = [None] * 9 + [0, None, 4, 1, 1, 160, 0] + [None] * 6
    assert lib.igdsp_bss_select(*args) == EINVAL
    assert lib.igdsp_bss_select(None, *([None] * 8), 0, None, 0, 0, 0, 160, 0, *([None] * 6)) == EINVAL    # even an empty batch


def test_uniform_model_equals_the_general_model():
    rng = np.random.default_rng(5)
    F_, m, G_ = 60, 4, 6
    C_ = m * G_
    info = np.zeros((F_, C_), capi.RTP_INFO)
    info["ed137"] = [[W(rng.random() < 0.5, int(rng.integers(0, 3))) for _ in range(C_)] for _ in range(F_)]
    info["pt"] = rng.choice([0, 18, 96, 123], (F_, C_), p=[0.7, 0.1, 0.1, 0.1])
    info["flags"] = np.where(rng.random((F_, C_)) < 0.1, bm.RTP_RUNT, 0)
    st0 = np.array([[3, 2, 1, 7]] * G_, np.uint32)
    wd0 = rng.integers(0, 2**32, C_, dtype=np.uint64).astype(np.uint32)
    a = bm.select(info, np.arange(0, C_ + 1, m), np.arange(C_), C_, C_, G_, st0, wd0, 4)
    b = bm.select_uniform(info, m, st0, wd0, 4)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
