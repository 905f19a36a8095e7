"""-m gpu: igdsp_link_watch (include/igdsp.h, "R2S link supervision") bit for bit against tests/link_model.py — the state bytes, the
kind bytes, the event list and its two counts: shapes around the wave, the block and the part; every optional input given and NULL;
event_cap around the total with guard bytes behind the list; the masks; no list; no kind; launch-split equivalence on the device; d_up
toggled between launches; two streams; nothing to do; every argument rule; and the compute-free yardstick's promise."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import link_model as lm  # noqa: E402

GUARD = 256
PART = 128                                                            # kLinkPart
CHANNELS = (1, 63, 64, 65, 257, 4099)                                # a lane, a wave -1 / 0 / +1, a block + 1, many blocks and a ragged end
TICKS = (1, 2, PART + 1, 300)
SLOTS = (1, 2, 8)
EINVAL, ERANGE = -22, -34


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def _dev(a):
    a = np.ascontiguousarray(a)
    return gu.to_dev(a if a.size else np.zeros(4, np.uint8))


class Guarded:
    """a device buffer of nbytes between two guard zones"""

    def __init__(self, nbytes, fill, init=None):
        self.n, self.fill = int(nbytes), fill
        raw = np.full(self.n + 2 * GUARD, fill, np.uint8)
        if init is not None:
            raw[GUARD:GUARD + self.n] = np.ascontiguousarray(init).view(np.uint8).reshape(-1)
        self.t = gu.to_dev(raw)
        self.ptr = self.t.data_ptr() + GUARD

    def take(self, what):
        raw = self.t.cpu().numpy()
        assert np.all(raw[:GUARD] == self.fill) and np.all(raw[GUARD + self.n:] == self.fill), f"guard bytes around {what} written"
        return raw[GUARD:GUARD + self.n].copy()


def run_link(ctx, info, sizes, up, period, T, S, t0, tick_ms, miss, mask, state, cap=None, want_list=True, want_kind=True, stream=None, entry=None):
    """igdsp_link_watch through the C ABI with guard bytes around the state and every output; cap None: room for every (tick, channel).
    Returns (state, kind, events stored, (total, stored)); None where not asked for.  entry: another C entry with the same arguments."""
    torch = gu.torch_cuda()
    C = info.shape[1]
    cap = C * T if cap is None else cap
    b_state = Guarded(C * 16, 0x77, state)
    b_kind = Guarded(T * C, 0x4D) if want_kind else None
    b_ev = Guarded(cap * 16, 0x3C) if want_list and cap else None
    b_cnt = Guarded(8, 0x2B) if want_list else None
    work = gu.dev_zeros(capi.link_work_bytes(C, T), 0xCD) if want_list else None
    keep = [_dev(x) if x is not None else None for x in (info, sizes, up, period)]
    d_info, d_sizes, d_up, d_period = keep
    p = lambda b: b.ptr if b is not None else None                  # noqa: E731
    if entry is None:
        ctx.link_watch(d_info, b_state.ptr, C, T, S, t0_ms=t0, tick_ms=tick_ms, sizes=d_sizes, up=d_up, period_ms=d_period, miss_ticks=miss,
                       event_mask=mask, kind=p(b_kind), events=p(b_ev), event_cap=cap if want_list else 0, event_count=p(b_cnt), work=work,
                       stream=stream)
    else:
        q = lambda x: x.data_ptr() if x is not None else None       # noqa: E731
        rc = entry(ctx.h, q(d_info), q(d_sizes), q(d_up), q(d_period), C, T, S, t0, tick_ms, miss, mask, b_state.ptr, p(b_kind), p(b_ev),
                   cap if want_list else 0, p(b_cnt), q(work), stream)
        assert rc == 0, rc
    if stream is None:
        torch.cuda.synchronize()
    else:
        ctx.sync(stream)
    st = b_state.take("d_state").view(capi.LINK_STATE)
    kind = b_kind.take("d_kind").reshape(T, C) if want_kind else None
    cnt = tuple(int(x) for x in b_cnt.take("d_event_count").view("<u4")) if want_list else None
    ev = None
    if want_list:
        raw = b_ev.take("d_events") if b_ev is not None else np.zeros(0, np.uint8)
        stored = min(cnt[1], cap)
        assert np.all(raw[stored * 16:] == 0x3C), "d_events written past the stored events"
        ev = raw[:stored * 16].view(capi.LINK_EVENT)
    return st, kind, ev, cnt


def check(got, exp, cap=None):
    st, kind, ev, cnt = got
    est, ekind, eev, total = exp
    np.testing.assert_array_equal(st.view(np.uint8), est.view(np.uint8))
    if kind is not None:
        np.testing.assert_array_equal(kind, ekind)
    if cnt is not None:
        stored = total if cap is None else min(total, cap)
        assert cnt == (total, stored), (cnt, total, cap)
        np.testing.assert_array_equal(ev.view(np.uint8), eev[:stored].view(np.uint8))


def make_case(seed, C, T, S, sizes=True, up=True, period=True, garbage=True, t0=None):
    rng = np.random.default_rng(seed)
    t0 = int(rng.integers(0, 1 << 40)) if t0 is None else t0
    info, sz = lm.traffic(rng, C, T, S, with_sizes=sizes)
    u = (rng.random(C) < 0.85).astype(np.uint8) if up else None
    per = rng.choice([0, 20, 40, 200, 65535], C, p=[0.1, 0.3, 0.3, 0.2, 0.1]).astype(np.uint16) if period else None
    st = lm.garbage_state(rng, C, t0) if garbage else np.zeros(C, capi.LINK_STATE)
    return info, sz, u, per, st, t0


SHAPES = [(C, T, SLOTS[(i + j) % 3], i * 4 + j) for i, C in enumerate(CHANNELS) for j, T in enumerate(TICKS)]


@pytest.mark.parametrize("C,T,S,i", SHAPES, ids=[f"C{c}-T{t}-S{s}" for c, t, s, _ in SHAPES])
def test_shapes_and_inputs(ctx, C, T, S, i):
    """every channel count against every tick count, the slot counts in turn; the optional inputs given and NULL in turn (sizes with 0,
    runts and payloads of 1024 or more; periods with 0 and 65535), reset and garbage states, the three masks"""
    info, sz, up, per, st0, t0 = make_case(1000 + i, C, T, S, sizes=i % 2 == 0, up=i % 3 != 0, period=i % 4 < 2, garbage=i % 5 != 0)
    miss, mask = (0, 3, 6)[i % 3], (0, 0x3F, capi.LINK_MISSING)[(i // 2) % 3]
    exp = lm.watch_numpy(info, sz, up, per, T, S, t0, 20, miss, mask, st0)
    if C * T * S <= 4096:
        s2 = lm.watch_scalar(info, sz, up, per, T, S, t0, 20, miss, mask, st0)
        np.testing.assert_array_equal(s2[1], exp[1])
    check(run_link(ctx, info, sz, up, per, T, S, t0, 20, miss, mask, st0), exp)


def test_every_kind_reaches_the_device(ctx):
    info, sz, up, per, st0, t0 = make_case(7, 257, 80, 2, garbage=False)
    exp = lm.watch_numpy(info, sz, up, per, 80, 2, t0, 20, 3, 0x3F, st0)
    assert int(np.bitwise_or.reduce(exp[1].reshape(-1))) == 0x3F and np.any((exp[1] & 3) == 3) and exp[3] > 257
    check(run_link(ctx, info, sz, up, per, 80, 2, t0, 20, 3, 0x3F, st0), exp)


@pytest.mark.parametrize("mask", [0, 0x3F, capi.LINK_MISSING], ids=["default", "late-included", "missing-only"])
def test_event_cap_and_masks(ctx, mask):
    """the first event_cap events in tick-major, ascending-channel order are kept, both counts are exact and nothing is written past
    d_events[event_cap) (two parts, so the list offset carries across them)"""
    C, T, S = 257, PART + 12, 2
    info, sz, up, per, st0, t0 = make_case(21, C, T, S)
    exp = lm.watch_numpy(info, sz, up, per, T, S, t0, 20, 3, mask, st0)
    total = exp[3]
    assert total > 8 and np.any(exp[2]["tick"] >= PART)
    for cap in (0, 1, total - 1, total, total + 7):
        check(run_link(ctx, info, sz, up, per, T, S, t0, 20, 3, mask, st0, cap=cap), exp, cap)


def test_no_list_and_no_kind(ctx):
    C, T, S = 65, PART + 1, 2
    info, sz, up, per, st0, t0 = make_case(31, C, T, S)
    exp = lm.watch_numpy(info, sz, up, per, T, S, t0, 20, 0, 0, st0)
    check(run_link(ctx, info, sz, up, per, T, S, t0, 20, 0, 0, st0, want_list=False), exp)          # one pass: state and kind only
    check(run_link(ctx, info, sz, up, per, T, S, t0, 20, 0, 0, st0, want_kind=False), exp)
    check(run_link(ctx, info, sz, up, per, T, S, t0, 20, 0, 0, st0, want_list=False, want_kind=False), exp)


def test_launch_split_equivalence(ctx):
    """40 launches of one tick, t0 advanced each time, against one launch of 40 ticks: state bytes, kind and the concatenated list"""
    C, T, S, tick_ms = 65, 40, 2, 20
    info, sz, up, per, st0, t0 = make_case(41, C, T, S)
    whole = run_link(ctx, info, sz, up, per, T, S, t0, tick_ms, 3, 0x3F, st0)
    check(whole, lm.watch_numpy(info, sz, up, per, T, S, t0, tick_ms, 3, 0x3F, st0))
    st, kinds, evs = st0, [], []
    for t in range(T):
        st, k, e, cnt = run_link(ctx, info[t * S:(t + 1) * S], sz[t * S:(t + 1) * S], up, per, 1, S, t0 + t * tick_ms, tick_ms, 3, 0x3F, st)
        assert np.all(e["tick"] == 0) and cnt == (len(e), len(e))
        e = e.copy()
        e["tick"] += t
        kinds.append(k)
        evs.append(e)
    np.testing.assert_array_equal(st.view(np.uint8), whole[0].view(np.uint8))
    np.testing.assert_array_equal(np.concatenate(kinds), whole[1])
    np.testing.assert_array_equal(np.concatenate(evs).view(np.uint8), whole[2].view(np.uint8))


def test_up_toggled_between_launches(ctx):
    """calls that drop and come back between launches: a dropped call keeps its state but for UP, a returning one is stamped again"""
    C, T, S = 130, 20, 1
    rng = np.random.default_rng(51)
    st_dev = st_mod = np.zeros(C, capi.LINK_STATE)
    came = 0
    for launch in range(4):
        info, sz = lm.traffic(rng, C, T, S)
        up = None if launch == 0 else (rng.random(C) < 0.6).astype(np.uint8)
        t0 = 10_000 + launch * T * 20
        exp = lm.watch_numpy(info, sz, up, None, T, S, t0, 20, 3, 0, st_mod)
        got = run_link(ctx, info, sz, up, None, T, S, t0, 20, 3, 0, st_dev)
        check(got, exp)
        st_dev, st_mod = got[0], exp[0]
        came += int(np.count_nonzero(exp[1][0] & capi.LINK_CAME_UP))
    assert came > C                                                   # some calls came up more than once


def test_two_streams_from_two_threads(ctx):
    torch = gu.torch_cuda()
    C, T, S = 257, PART + 5, 2
    cases = [make_case(60 + i, C, T, S) for i in range(2)]
    results, errors = [None, None], []

    def worker(i):
        try:
            s = torch.cuda.Stream()
            info, sz, up, per, st0, t0 = cases[i]
            for _ in range(3):
                results[i] = run_link(ctx, info, sz, up, per, T, S, t0, 20, 3, 0x3F, st0, stream=s.cuda_stream)   # its own d_work
        except Exception as e:                                      # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for i in range(2):
        info, sz, up, per, st0, t0 = cases[i]
        check(results[i], lm.watch_numpy(info, sz, up, per, T, S, t0, 20, 3, 0x3F, st0))


def test_nothing_to_do_writes_zero_counts(ctx):
    torch = gu.torch_cuda()
    info = _dev(np.zeros(8, capi.RTP_INFO))
    state = Guarded(16, 0x77)
    work = gu.dev_zeros(capi.link_work_bytes(0, 0), 0xCD)
    for C, T in ((0, 4), (4, 0), (0, 0)):
        cnt = Guarded(8, 0x2B)
        ctx.link_watch(info, state.ptr, C, T, 1, event_count=cnt.ptr, work=work)
        torch.cuda.synchronize()
        assert cnt.take("d_event_count").view("<u4").tolist() == [0, 0]
        ctx.link_watch(None, None, C, T, 1)                          # no list either: nothing at all, and no buffer is needed
    torch.cuda.synchronize()
    assert np.all(state.take("d_state") == 0x77)


def test_argument_rules(ctx):
    C, T = 8, 2
    info, st = _dev(np.zeros((T * 8, C), capi.RTP_INFO)), gu.dev_zeros(C * 16 + 16)
    ev, cnt, work = gu.dev_zeros(64 * 16 + 16), gu.dev_zeros(16), gu.dev_zeros(capi.link_work_bytes(C, T) + 16)
    L = ctx.L

    def rc(info=info.data_ptr(), sizes=None, up=None, period=None, C=C, T=T, S=1, tick_ms=20, miss=0, mask=0, state=st.data_ptr(), kind=None,
           events=ev.data_ptr(), cap=64, count=cnt.data_ptr(), work=work.data_ptr(), h=ctx.h):
        return L.igdsp_link_watch(h, info, sizes, up, period, C, T, S, 0, tick_ms, miss, mask, state, kind, events, cap, count, work, None)

    assert rc() == 0
    assert rc(h=None) == EINVAL
    assert rc(S=0) == EINVAL and rc(S=capi.STAGE_DEPTH + 1) == EINVAL and rc(S=capi.STAGE_DEPTH) == 0
    assert rc(tick_ms=0) == EINVAL and rc(tick_ms=1) == 0
    assert rc(miss=65536) == EINVAL and rc(miss=65535) == 0 and rc(miss=1) == 0
    assert rc(events=None) == EINVAL and rc(events=None, cap=0) == 0               # d_events may be NULL iff event_cap == 0
    assert rc(work=None) == EINVAL and rc(work=work.data_ptr() + 8) == EINVAL      # required, 16-byte aligned, when a list is requested
    assert rc(work=None, count=None) == 0 and rc(work=None, count=None, events=None, cap=0) == 0
    assert rc(info=None) == EINVAL and rc(state=None) == EINVAL
    assert rc(info=info.data_ptr() + 2) == EINVAL and rc(state=st.data_ptr() + 4) == EINVAL and rc(events=ev.data_ptr() + 2) == EINVAL
    assert rc(count=cnt.data_ptr() + 2) == EINVAL and rc(sizes=info.data_ptr() + 1) == EINVAL and rc(period=info.data_ptr() + 1) == EINVAL
    assert rc(C=0, S=0) == EINVAL and rc(T=0, tick_ms=0) == EINVAL                # the rules hold with nothing to do, too
    assert rc(C=0, info=None, state=None) == 0 and rc(T=0, info=None, state=None) == 0
    assert rc(C=1 << 31, T=2) == ERANGE
    gu.torch_cuda().cuda.synchronize()


def test_yardstick_same_passes_no_state_machine(ctx):
    """igdsp_internal_link_copy (tools/link_bench.py's yardstick) walks the same passes and stores the state as it read it, kind bytes of
    0 and an empty list"""
    cp = capi.internal("igdsp_internal_link_copy")
    C, T, S = 257, PART + 3, 2
    info, sz, up, per, st0, t0 = make_case(71, C, T, S)
    for want_list in (True, False):
        st, kind, ev, cnt = run_link(ctx, info, sz, up, per, T, S, t0, 20, 0, 0x3F, st0, want_list=want_list, entry=cp)
        np.testing.assert_array_equal(st.view(np.uint8), st0.view(np.uint8))
        assert np.all(kind == 0)
        if want_list:
            assert cnt == (0, 0) and len(ev) == 0
