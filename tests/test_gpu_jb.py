"""-m gpu: igdsp_jb_receive (include/igdsp.h, "Jitter buffer") bit for bit against tests/jb_model.py — payload, len, info, tick flags,
packet status and the final state: a fuzz of simulated networks (loss, bursts, reorder, duplicates, SSRC changes, keep-alive-only
spans, runts, bad versions, other PTs, oversize, seq wraps) over channel counts, slots per tick and delays; split launches; the in-order
case against igdsp_depayload; the chains into igdsp_bss_select and igdsp_conf_mix; two streams at once; guard bytes and arguments;
and the full-size in-order shape against a torch statement."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import jb_model as jm  # noqa: E402

GUARD = 256


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def _guarded(nbytes, fill):
    return gu.dev_zeros(nbytes + GUARD, fill)


def _take(d, nbytes, fill, what):
    raw = d.cpu().numpy()
    assert np.all(raw[nbytes:] == fill), f"guard bytes after {what} written"
    return raw[:nbytes]


class Dev:
    """device state + ring of C channels (zero = reset; fill: every byte of both holds it), carried across run() calls"""

    def __init__(self, C_, n=160, fill=0):
        self.C, self.n = C_, n
        self.state = _guarded(C_ * capi.JB_STATE.itemsize, fill)
        self.ring = _guarded(capi.jb_ring_bytes(C_, n), fill)
        self.state[C_ * capi.JB_STATE.itemsize:] = 0x77
        self.ring[capi.jb_ring_bytes(C_, n):] = 0x66

    def host_state(self):
        return _take(self.state, self.C * capi.JB_STATE.itemsize, 0x77, "d_state").view(capi.JB_STATE)

    def ring_bytes(self):
        return _take(self.ring, capi.jb_ring_bytes(self.C, self.n), 0x66, "d_ring")


def run_jb(ctx, dev, packets, sizes, radio, S, delay, arrival=None, stream=None, status=True, flags=True, entry=None, fill=None, raw=None):
    """one igdsp_jb_receive launch over packets [T*S][C][stride]; returns (payload, len, info, flags, status) numpy.  entry: through
    that yardstick of capi.INTERNAL_TWIN instead; fill: the byte every output and its guard hold before the launch; raw: a dict that
    takes the whole output buffers' bytes after it."""
    torch = gu.torch_cuda()
    A, C_, stride = packets.shape
    T, n = A // S, dev.n
    fp, fn, fi, ff, fs = (0xA5, 0x5A, 0x3C, 0x11, 0x22) if fill is None else (fill,) * 5
    d_pay, d_len, d_inf = _guarded(T * C_ * n, fp), _guarded(T * C_ * 2, fn), _guarded(T * C_ * 8, fi)
    d_fl = _guarded(T * C_, ff) if flags else None
    d_st = _guarded(A * C_, fs) if status else None
    (ctx.via(entry) if entry else ctx).jb_receive(
        gu.to_dev(packets), gu.to_dev(np.asarray(radio, np.uint8)), dev.state, dev.ring, d_pay, d_len, d_inf, C_, T, S, stride, n, delay,
        sizes=None if sizes is None else gu.to_dev(np.asarray(sizes, "<u2")),
        arrival=None if arrival is None else gu.to_dev(np.asarray(arrival, "<u4")), tick_flags=d_fl, pkt_status=d_st, stream=stream)
    if stream is None:
        torch.cuda.synchronize()
    else:
        ctx.sync(stream)
    pay = _take(d_pay, T * C_ * n, fp, "payload").reshape(T, C_, n)
    ln = _take(d_len, T * C_ * 2, fn, "len").view("<u2").reshape(T, C_)
    inf = _take(d_inf, T * C_ * 8, fi, "info").view(capi.RTP_INFO).reshape(T, C_)
    fl = _take(d_fl, T * C_, ff, "tick flags").reshape(T, C_) if flags else None
    st = _take(d_st, A * C_, fs, "packet status").reshape(A, C_) if status else None
    if raw is not None:
        raw.update({k: t.cpu().numpy() for k, t in (("payload", d_pay), ("len", d_len), ("info", d_inf), ("tick_flags", d_fl), ("pkt_status", d_st))
                    if t is not None})
        raw.update(state=dev.host_state().view(np.uint8), ring=dev.ring_bytes())      # (their guards hold bytes of their own, checked there)
    return pay, ln, inf, fl, st


def info_tuples(inf):
    return np.stack([inf["ed137"].astype(np.int64), inf["payload_len"], inf["pt"], inf["flags"]], axis=-1)


def expect(orc, packets, sizes, radio, S, delay, n=160, arrival=None, chans=None):
    dep = orc.depayload(packets, sizes, radio, n)
    return jm.run(packets, sizes, radio, S, delay, n, arrival, chans, dep)


def check(got, exp, dev=None, chans=None):
    pay, ln, inf, fl, st = got
    epay, eln, einf, efl, est, _ = exp
    np.testing.assert_array_equal(fl, efl, err_msg="tick flags")
    np.testing.assert_array_equal(st, est, err_msg="packet status")
    np.testing.assert_array_equal(ln, eln, err_msg="len")
    np.testing.assert_array_equal(info_tuples(inf), einf, err_msg="info")
    np.testing.assert_array_equal(pay, epay, err_msg="payload")
    if dev is not None:
        hs = dev.host_state()
        for c, ch in enumerate(chans):
            er = ch.state_record(capi.JB_STATE)
            for k in capi.JB_STATE.names:
                assert hs[c][k] == er[k], (c, k, hs[c][k], er[k])


def simulate(rng, C_, T, S, stride=180, n=160, radio=None):
    """a simulated network: per channel one sender at 20 ms with squelch spans (keep-alives only), SSRC changes, seq starting anywhere
    (wraps), and a path with loss, bursts, reorder by 1-3 ticks, duplicates, junk (runts, V != 2), other PTs and oversize payloads"""
    radio = rng.integers(0, 2, C_).astype(np.uint8) if radio is None else radio
    arrivals = {}
    for c in range(C_):
        hdr = 20 if radio[c] else 12
        seq = int(rng.integers(0, 65536)) if rng.random() < 0.7 else 65536 - int(rng.integers(1, 40))
        ssrc = int(rng.integers(0, 1 << 32))
        ts = int(rng.integers(0, 1 << 32))
        p_loss, p_dup, p_re = rng.choice([0.0, 0.03, 0.15]), rng.choice([0.0, 0.02, 0.1]), rng.choice([0.0, 0.05, 0.2])
        squelch = True
        for t in range(T):
            if rng.random() < 0.01:
                ssrc = int(rng.integers(0, 1 << 32))
                seq = int(rng.integers(0, 65536))
            if rng.random() < 0.02:
                squelch = not squelch
            if rng.random() < 0.005:
                seq = (seq + int(rng.integers(100, 60000))) % 65536          # a large jump
            send = []
            word = (1 << 28) | (int(rng.integers(0, 32)) << 3) if squelch else 0
            if squelch:
                r = rng.random()
                pt = 8 if r < 0.9 else (18 if r < 0.95 else 0)
                ln = n if rng.random() < 0.9 else int(rng.integers(0, stride - hdr + 1))
                pl = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
                send.append(jm.rtp_header(pt, seq, ts, ssrc, bool(radio[c]), word, rng.random() < 0.05) + pl)
                seq = (seq + 1) % 65536
            else:
                send.append(jm.rtp_header(123, 0, 0, 0, bool(radio[c]), word))
            ts = (ts + n) & 0xFFFFFFFF
            if rng.random() < 0.01:
                send.append(bytes(rng.integers(0, 256, int(rng.integers(1, hdr)), dtype=np.uint8)))   # runt
            if rng.random() < 0.01:
                send.append(bytes([0x40]) + jm.rtp_header(8, seq, ts, ssrc, False)[1:] + bytes(n))      # V = 1
            burst = rng.random() < 0.01
            for p in send:
                if burst or rng.random() < p_loss:
                    continue
                for _ in range(2 if rng.random() < p_dup else 1):
                    ta = t + (int(rng.integers(1, 4)) if rng.random() < p_re else 0)
                    if ta < T:
                        arrivals.setdefault((ta, c), []).append(p)
    arrival = np.zeros((T * S, C_), np.uint32)
    for (t, c), lst in list(arrivals.items()):
        rng.shuffle(lst)
        arrivals[(t, c)] = lst[:S]                                           # the rest is lost: the tick holds S slots
        for k in range(len(arrivals[(t, c)])):
            arrival[t * S + k, c] = (t * n + int(rng.integers(-80, 81)) + 7 * k) & 0xFFFFFFFF
    packets, sizes = jm.pack(arrivals, C_, T, S, stride)
    return packets, sizes, radio, arrival


@pytest.mark.parametrize("C_,S,delay,n,stride", [(1, 1, 3, 160, 180), (5, 2, 0, 160, 180), (16, 1, 3, 160, 184), (37, 8, 7, 160, 180),
                                                 (23, 3, 15, 160, 184), (17, 4, 3, 37, 64), (3, 2, 1, 256, 280)])
def test_fuzz_vs_model(ctx, orc, C_, S, delay, n, stride):
    rng = np.random.default_rng(1000 * C_ + 10 * S + delay)
    T = 200                                                                 # two parts of the launch
    packets, sizes, radio, arrival = simulate(rng, C_, T, S, stride, n)
    use_arr = C_ % 2 == 1
    dev = Dev(C_, n)
    got = run_jb(ctx, dev, packets, sizes, radio, S, delay, arrival if use_arr else None)
    exp = expect(orc, packets, sizes, radio, S, delay, n, arrival if use_arr else None)
    check(got, exp, dev, exp[5])
    # every outcome of the semantics occurred somewhere in the fuzz
    if C_ >= 16:
        assert set(np.unique(exp[4])) >= {jm.P_INVALID, jm.P_KEEPALIVE, jm.P_PLACED, jm.P_RESTART}
        assert set(np.unique(exp[3])) == {jm.IDLE, jm.PLAYED, jm.LOST}


def test_split_launches_identical(ctx, orc):
    rng = np.random.default_rng(7)
    C_, T, S, delay = 19, 150, 2, 3
    packets, sizes, radio, arrival = simulate(rng, C_, T, S)
    whole = Dev(C_)
    g = run_jb(ctx, whole, packets, sizes, radio, S, delay, arrival)
    exp = expect(orc, packets, sizes, radio, S, delay, arrival=arrival)
    check(g, exp, whole, exp[5])
    for cuts in ([1] * T, [100, 50], [128, 1, 21], [3, 130, 17]):
        dev, parts, t0 = Dev(C_), [], 0
        for m in cuts:
            sl = slice(t0 * S, (t0 + m) * S)
            parts.append(run_jb(ctx, dev, packets[sl], sizes[sl], radio, S, delay, arrival[sl]))
            t0 += m
        for i in range(5):
            np.testing.assert_array_equal(np.concatenate([p[i] for p in parts]), g[i], err_msg=f"output {i}, cuts {cuts[:4]}")
        np.testing.assert_array_equal(dev.host_state(), whole.host_state())
        assert live_ring(dev) == live_ring(whole)


def live_ring(dev):
    """the ring's tags and the bytes of every occupied slot (a freed slot keeps stale bytes, which no launch reads)"""
    raw = dev.ring_bytes()
    tags = raw[:dev.C * 64].view("<u4").reshape(dev.C, 16)
    slot = 16 + (dev.n + 15) // 16 * 16
    slots = raw[dev.C * 64:].reshape(dev.C, 16, slot)
    return [(c, s, int(tags[c, s]), slots[c, s].tobytes()) for c in range(dev.C) for s in range(16) if tags[c, s]]


def in_order(C_, T, stride=180, n=160, seed=5):
    rng = np.random.default_rng(seed)
    radio = (np.arange(C_) % 3 != 0).astype(np.uint8)
    arrivals = {}
    for c in range(C_):
        s0, ssrc = int(rng.integers(0, 65536)), int(rng.integers(0, 1 << 32))
        for t in range(T):
            arrivals[(t, c)] = [jm.rtp_header(8, s0 + t, 160 * t, ssrc, bool(radio[c]), 1 << 28 | c << 3) +
                                rng.integers(0, 256, n, dtype=np.uint8).tobytes()]
    packets, sizes = jm.pack(arrivals, C_, T, 1, stride)
    return packets, sizes, radio


def test_in_order_delay0_equals_depayload(ctx, orc):
    C_, T = 64, 40
    packets, sizes, radio = in_order(C_, T)
    dev = Dev(C_)
    pay, ln, inf, fl, st = run_jb(ctx, dev, packets, sizes, radio, 1, 0)
    dpay, dln, dinf = orc.depayload(packets, sizes, radio)
    assert np.all(fl[0] == jm.IDLE) and np.all(st[0] == jm.P_INVALID)      # the probation packet
    assert np.all(fl[1:] == jm.PLAYED) and np.all(st[1] == jm.P_RESTART) and np.all(st[2:] == jm.P_PLACED)
    np.testing.assert_array_equal(pay[1:], dpay[1:])
    np.testing.assert_array_equal(ln[1:], dln[1:])
    np.testing.assert_array_equal(inf[1:].view(np.uint64), dinf[1:].view(np.uint64))
    hs = dev.host_state()
    assert np.all(hs["played"] == T - 1) and np.all(hs["lost"] == 0) and np.all(hs["invalid"] == 1) and np.all(hs["received"] == T - 1)


def test_chain_into_bss_select_and_conf_mix(ctx, orc):
    torch = gu.torch_cuda()
    rng = np.random.default_rng(11)
    C_, T, S = 16, 60, 2
    packets, sizes, radio, arrival = simulate(rng, C_, T, S, radio=np.ones(16, np.uint8))
    dev = Dev(C_)
    pay, ln, inf, fl, st = run_jb(ctx, dev, packets, sizes, radio, S, 3, arrival)
    epay, eln, einf, _, _, _ = expect(orc, packets, sizes, radio, S, 3, arrival=arrival)
    minf = np.zeros((T, C_), capi.RTP_INFO)
    for i, k in enumerate(("ed137", "payload_len", "pt", "flags")):
        minf[k] = einf[..., i]
    codec = np.full(C_, 8, np.uint8)
    ptr = np.arange(0, C_ + 1, 4, dtype=np.uint32)
    mem = np.arange(C_, dtype=np.uint32)
    s = torch.cuda.current_stream().cuda_stream

    def bss(p, l, i):
        G_ = len(ptr) - 1
        sel, out = gu.dev_zeros(T * G_ * 4), gu.dev_zeros(T * G_ * 160 * 2)
        state, words = gu.dev_zeros(G_ * 16), gu.dev_zeros(C_ * 4)
        ctx.bss_select(gu.to_dev(i), gu.to_dev(ptr), gu.to_dev(mem), C_, state, words, C_, G_, T, 160, payload=gu.to_dev(p),
                       codec=gu.to_dev(codec), length=gu.to_dev(l), vote_frames=3, sel=sel, out=out, stream=s)
        torch.cuda.synchronize()
        return sel.cpu().numpy(), out.cpu().numpy()

    def conf(p, l):
        out = gu.dev_zeros(T * 2 * 160 * 2)
        gain = np.full(C_, 128, np.uint16)
        cptr = np.array([0, 8, 16], np.uint32)
        ctx.conf_mix(gu.to_dev(gain), gu.to_dev(cptr), gu.to_dev(mem), C_, C_, 2, T, 160, out=out, payload=gu.to_dev(p), codec=gu.to_dev(codec),
                     length=gu.to_dev(l), stream=s)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    a, b = bss(pay, ln, inf), bss(epay, eln, minf)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert (a[0].view("<i4") >= 0).any(), "the vote never latched: the chain test saw no voted frame"
    np.testing.assert_array_equal(conf(pay, ln), conf(epay, eln))


def test_two_streams_concurrently(ctx, orc):
    torch = gu.torch_cuda()
    rng = np.random.default_rng(23)
    jobs = [simulate(rng, 21, 90, 2), simulate(rng, 13, 90, 2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = [None, None]
    devs = [Dev(21), Dev(13)]

    def go(i):
        p, sz, r, ar = jobs[i]
        res[i] = run_jb(ctx, devs[i], p, sz, r, 2, 3, ar, stream=streams[i].cuda_stream)

    th = [threading.Thread(target=go, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i in range(2):
        p, sz, r, ar = jobs[i]
        exp = expect(orc, p, sz, r, 2, 3, arrival=ar)
        check(res[i], exp, devs[i], exp[5])


def test_arguments(ctx):
    C_, T, S, n = 4, 2, 1, 160
    d = {k: gu.dev_zeros(1 << 16) for k in ("pk", "rad", "pay", "len", "inf", "ring", "st")}
    base = dict(packets=d["pk"], radio=d["rad"], state=d["st"], ring=d["ring"], payload=d["pay"], length=d["len"], info=d["inf"], C_=C_, T_=T,
                S_=S, stride=180, n=n, delay=3)
    ctx.jb_receive(**base)
    gu.torch_cuda().cuda.synchronize()
    bad = [dict(stride=182), dict(stride=16), dict(stride=2052), dict(S_=0), dict(S_=9), dict(delay=16), dict(n=0), dict(n=257),
           dict(packets=None), dict(radio=None), dict(state=None), dict(ring=None), dict(payload=None), dict(length=None), dict(info=None),
           dict(ring=d["ring"].data_ptr() + 4), dict(info=d["inf"].data_ptr() + 4), dict(length=d["len"].data_ptr() + 1)]
    for b in bad:
        with pytest.raises(capi.IgdspError) as e:
            ctx.jb_receive(**{**base, **b})
        assert e.value.code == -22, b
    ctx.jb_receive(**{**base, "C_": 0, "packets": None})                  # nothing to do: no argument is looked at
    ctx.jb_receive(**{**base, "T_": 0})


def test_full_size_in_order(ctx):
    """J1: 65 536 channels x 128 ticks, one slot per tick, in order without loss, delay 3 — against a torch statement: tick t plays
    arrival t - 3 from t = 4 on (arrival 0 is the probation packet, arrival 1 starts playout with three ticks of pre-roll)"""
    torch = gu.torch_cuda()
    C_, T, n, stride, delay = 65536, 128, 160, 180, 3
    g = torch.Generator(device="cuda").manual_seed(3)
    pk = torch.randint(0, 256, (T, C_, stride), dtype=torch.uint8, device="cuda", generator=g)
    seq0 = torch.randint(0, 65535, (C_,), device="cuda", generator=g)   # not 65535: A.1 keeps probation across that wrap
    seq = (seq0[None, :] + torch.arange(T, device="cuda")[:, None]) % 65536
    ts = torch.arange(T, device="cuda")[:, None] * 160 + torch.zeros(C_, dtype=torch.int64, device="cuda")[None, :]
    pk[:, :, 0] = 0x90
    pk[:, :, 1] = 8
    pk[:, :, 2], pk[:, :, 3] = (seq >> 8).to(torch.uint8), (seq & 0xFF).to(torch.uint8)
    for i in range(4):
        pk[:, :, 4 + i] = ((ts >> (24 - 8 * i)) & 0xFF).to(torch.uint8)
    pk[:, :, 8:12] = torch.tensor([0xCA, 0xFE, 0x00, 0x01], dtype=torch.uint8, device="cuda")
    pk[:, :, 12:16] = torch.tensor([0x01, 0x67, 0x00, 0x01], dtype=torch.uint8, device="cuda")
    radio = torch.ones(C_, dtype=torch.uint8, device="cuda")
    state = torch.zeros(C_ * capi.JB_STATE.itemsize, dtype=torch.uint8, device="cuda")
    ring = torch.zeros(capi.jb_ring_bytes(C_, n), dtype=torch.uint8, device="cuda")
    pay = torch.full((T, C_, n), 0xA5, dtype=torch.uint8, device="cuda")
    ln = torch.full((T, C_), 0x5A5A, dtype=torch.int16, device="cuda")
    inf = torch.full((T, C_, 8), 0x3C, dtype=torch.uint8, device="cuda")
    fl = torch.zeros((T, C_), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ctx.jb_receive(pk, radio, state, ring, pay, ln, inf, C_, T, 1, stride, n, delay, tick_flags=fl, stream=s)
    torch.cuda.synchronize()
    assert bool((fl[:4] == jm.IDLE).all()) and bool((fl[4:] == jm.PLAYED).all())
    assert bool((pay[4:] == pk[1:T - 3, :, 20:20 + n]).all())
    assert bool((pay[:4] == 0).all()) and bool((ln[:4] == 0).all()) and bool((ln[4:] == n).all())
    want = torch.tensor([0, 0, 0, 0, 160, 0, 8, 0x01 | 0x02 | 0x08 | 0x20], dtype=torch.uint8, device="cuda")
    want[0:4] = pk[1, 0, 16:20].flip(0)                                    # ntohl of the (random) ED-137 word
    got_w = inf[4:, :, :4].flip(-1)
    assert bool((got_w == pk[1:T - 3, :, 16:20]).all())
    assert bool((inf[4:, :, 4:] == want[4:]).all())
    assert bool((inf[:4, :, :7] == 0).all()) and bool((inf[:4, :, 7] == 0x40).all())
    st = state.cpu().numpy().view(capi.JB_STATE)
    assert np.all(st["played"] == T - 4) and np.all(st["lost"] == 0) and np.all(st["invalid"] == 1) and np.all(st["received"] == T - 1)
    # the ring holds the three packets of the pre-roll
    tags = ring[:C_ * 64].view(torch.int32).view(C_, 16).cpu().numpy()
    assert np.all((tags != 0).sum(axis=1) == 3)


# ---- the compute-free yardstick (igdsp_internal_jb_copy, tools/jb_bench.py) against its promise in csrc/igdsp_capi.hip: "the rows of
# an in-order lossless launch (arrival slot 0 of every tick copied as igdsp_depayload would), with no header walk, state machine or
# ring store; the state, the ring and d_pkt_status are not touched"

def slot0_traffic(C_, T, n, S=2, seed=5):
    """in order, lossless: the tick's packet in arrival slot 0 (payloads of n bytes, and some shorter), junk bytes of size 0 in the others"""
    rng = np.random.default_rng(seed)
    stride = (20 + n + 3) // 4 * 4
    radio = (np.arange(C_) % 3 != 0).astype(np.uint8)
    arrivals = {}
    for c in range(C_):
        s0, ssrc = int(rng.integers(0, 65536)), int(rng.integers(0, 1 << 32))
        for t in range(T):
            ln = n if rng.random() < 0.9 else int(rng.integers(0, n))
            arrivals[(t, c)] = [jm.rtp_header(8, s0 + t, n * t, ssrc, bool(radio[c]), 1 << 28 | (c & 31) << 3) + rng.integers(0, 256, ln, dtype=np.uint8).tobytes()]
    packets, sizes = jm.pack(arrivals, C_, T, S, stride)
    junk = rng.integers(0, 256, packets.shape, dtype=np.uint8)
    for k in range(1, S):
        packets[k::S] = junk[k::S]
    return packets, sizes, radio


@pytest.mark.parametrize("T", [3, 131])
@pytest.mark.parametrize("n", [160, 24, 13])
def test_yardstick_footprint_values_independence(ctx, orc, n, T):
    """igdsp_internal_jb_copy on an in-order lossless launch, two arrival slots per tick, channel counts around the wave's, one part and
    two: it stores the bytes igdsp_jb_receive stores in the rows, lengths, records and tick flags and not a byte of the state, the ring
    or d_pkt_status; the state and the ring may hold any garbage; rows, lengths and records are igdsp_depayload's of slot 0"""
    S = 2
    for C_ in (1, 15, 17, 65):
        packets, sizes, radio = slot0_traffic(C_, T, n, S, seed=C_ + T)
        got = {}

        def yard(fill):
            raw = {}
            got[fill] = run_jb(ctx, Dev(C_, n, fill), packets, sizes, radio, S, 0, entry="jb_copy", fill=fill, raw=raw)
            return raw

        def real(fill):
            raw = {}
            run_jb(ctx, Dev(C_, n), packets, sizes, radio, S, 0, fill=fill, raw=raw)
            return raw

        outs = ("payload", "len", "info", "tick_flags")
        ym, rmk = gu.written_mask(yard), gu.written_mask(real)
        assert all(rmk[k][:-GUARD].all() for k in outs)
        gu.assert_same_footprint(ym, rmk, not_written=("state", "ring", "pkt_status"))
        dpay, dln, dinf = orc.depayload(packets[0::S], sizes[0::S], radio, n)
        zero = run_jb(ctx, Dev(C_, n), packets, sizes, radio, S, 0, entry="jb_copy")
        for pay, ln, inf, fl, _ in (got[gu.FILL_A], got[gu.FILL_B], zero):
            np.testing.assert_array_equal(pay, dpay)
            np.testing.assert_array_equal(ln, dln)
            np.testing.assert_array_equal(inf.view(np.uint64), dinf.view(np.uint64))
            assert (fl == jm.PLAYED).all()
