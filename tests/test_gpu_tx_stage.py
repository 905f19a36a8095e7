"""-m gpu: the staged ED-137 send path (igdsp_tx_open / igdsp_tx_set_* / igdsp_on_tx_frame / igdsp_tx_flush) against
tests/tx_stage_model.py — a fuzz with setters, overflowing rings and mixed n; the same answer as one igdsp_tx_packetize launch; the
real-time shape; producer / setter / owner / RX threads on one context; the round trip through igdsp_depayload; the error paths."""
import threading

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import capi
from tests import tx_model as tm
from tests import tx_stage_model as sm
from tests.gpu_util import dev_zeros, to_dev, to_host, torch_cuda

pytestmark = pytest.mark.gpu
CALLTYPES = ["Tx", "Rx", "Rxonly", "TRx", "Idle", "RxTx", "Foo", "IdleTx"]
EBUSY, ENOENT, EINVAL = -16, -2, -22
CALL0 = 1000                                   # call_id of leg l = CALL0 + l


class Stream:
    """one leg's pjmedia stream: pt, ssrc, seq, ts"""

    def __init__(self, rng):
        self.pt = int(rng.choice([0, 8]))
        self.ssrc, self.seq, self.ts = int(rng.integers(1 << 32)), int(rng.integers(1 << 16)), int(rng.integers(1 << 32))

    def packet(self, payload, marker=0):
        p = sm.stream_packet(self.pt, self.seq, self.ts, self.ssrc, payload, marker)
        self.seq = (self.seq + 1) & 0xFFFF
        self.ts = (self.ts + len(payload)) & 0xFFFFFFFF
        return p


def open_legs(ctx, model, rng, L, now):
    for l in range(L):
        ctx.map_call(CALL0 + l, l)
        ct, ci, ka, t = CALLTYPES[rng.integers(len(CALLTYPES))], bool(rng.integers(2)), int(rng.choice([200, 60, 0, -1, 1000])), int(now + rng.integers(-100, 400))
        ctx.tx_open(CALL0 + l, ct, ci, ka, t)
        model.open(l, ct, ci, ka, t)


def random_setter(ctx, rng, call_id):
    """one adapter setter through the C ABI; returns its model assignment"""
    k = int(rng.integers(6))
    if k == 0:
        a = (bool(rng.integers(2)), int(rng.integers(0, 300)), int(rng.integers(2)))
        ctx.tx_set_ptt(call_id, *a)
        return sm.setter("ptt", *a)
    if k == 1:
        a = (bool(rng.integers(2)), int(rng.integers(8)), int(rng.choice([-1, int(rng.integers(0, 300))])))
        ctx.tx_set_sql(call_id, *a)
        return sm.setter("sql", *a)
    if k == 2:
        v = int(rng.integers(0, 300))
        ctx.tx_set_ptt_id(call_id, v)
        return sm.setter("ptt_id", v)
    if k == 3:
        a = (bool(rng.integers(2)), bool(rng.integers(2)))
        ctx.tx_set_slave(call_id, *a)
        return sm.setter("slave", *a)
    if k == 4:
        v = bool(rng.integers(2))
        ctx.tx_set_recorder(call_id, v)
        return sm.setter("recorder", v)
    ct = CALLTYPES[rng.integers(len(CALLTYPES))]
    ctx.tx_set_calltype(call_id, ct)
    return sm.setter("calltype", ct)


def check_flush(ctx, model, frames, n_expected=None):
    n = ctx.tx_flush()
    assert n == len(frames) if n_expected is None else n_expected
    ent, pk = ctx.tx_results()
    assert len(ent) == len(frames)
    exp = model.run(frames)
    for i, (leg, _, _, _) in enumerate(frames):
        b, inf = exp[i]
        e = ent[i]
        assert (e["call_id"], e["size"], e["ed137"], e["flags"], e["level"]) == (CALL0 + leg, inf["size"], inf["ed137"], inf["flags"], inf["level"]), (i, leg)
        assert pk[i, :e["size"]].tobytes() == b, (i, leg)
    return ent, pk


def compare_chans(ctx, model, L):
    for l in range(L):
        got = ctx.tx_get_chan(CALL0 + l)
        for f in capi.TX_CHAN.names:
            if f not in ("reserved", "reserved0"):
                assert got[f] == model.st[l][f], (l, f, got[f], model.st[l][f])


NS = [160, 80, 24, 236, 13, 49]


def test_fuzz_against_model():
    rng = np.random.default_rng(20261015)
    L, flushes = 4096, 40
    model = sm.Legs(L)
    refused = np.zeros(L, np.int64)
    keep = []
    with capi.Context(device=0, max_channels=L) as ctx:
        open_legs(ctx, model, rng, L, 1_000_000)
        streams = [Stream(rng) for _ in range(L)]
        pending = [None] * L
        t = 1_000_000
        for fl in range(flushes):
            frames = []
            for l in range(L):
                staged = 0
                for k in range(int(rng.integers(0, 11))):          # 0 .. 10 frames: rings of 8 overflow
                    while rng.random() < 0.15:                       # setters between frames, on the producer's thread
                        pending[l] = dict(pending[l] or {}, **random_setter(ctx, rng, CALL0 + l))
                    n = int(rng.choice(NS))
                    now = t + 20 * k + int(rng.choice([0, 0, 0, -25, 3, 400]))
                    pay = rng.integers(0, 256, n, dtype=np.uint8)
                    if rng.random() < 0.3 and n + 12 > 60:
                        pay[28] = pay[38] = pay[48] = 0xD5           # the silence probe's bytes
                    pkt = streams[l].packet(pay.tobytes(), int(rng.random() < 0.1))
                    rc = ctx.on_tx_frame(CALL0 + l, pkt, now)
                    if staged < capi.STAGE_DEPTH:
                        assert rc == 0
                        frames.append((l, pkt, now, pending[l]))
                        pending[l] = None
                        staged += 1
                    else:
                        assert rc == EBUSY
                        refused[l] += 1
                if rng.random() < 0.05:                               # a setter after the leg's last frame: carries over
                    pending[l] = dict(pending[l] or {}, **random_setter(ctx, rng, CALL0 + l))
            ent, pk = check_flush(ctx, model, frames)
            if fl < 4:
                keep.append((ent, pk))
            t += 160
        compare_chans(ctx, model, L)
        for l in range(L):
            assert ctx.tx_counts(CALL0 + l) == (refused[l], 0)
        assert refused.sum() > 0
        # the round trip: every sent packet of the first flushes through igdsp_depayload
        torch = torch_cuda()
        for ent, pk in keep:
            sent = ent["size"] > 0
            P = int(sent.sum())
            d_pk, d_sz = to_dev(pk[sent]), to_dev(ent["size"][sent].astype(np.uint16))
            pl, ln, inf = dev_zeros(P * 236), dev_zeros(P * 2), dev_zeros(P * 8)
            ctx.depayload(d_pk, d_sz, to_dev(np.ones(P, np.uint8)), P, 1, 256, 236, pl, ln, inf)
            torch.cuda.synchronize()
            rinfo = to_host(inf, capi.RTP_INFO, (P,))
            rpl = to_host(pl, np.uint8, (P, 236))
            e, p = ent[sent], pk[sent]
            assert np.array_equal(rinfo["ed137"], e["ed137"])
            assert np.array_equal((rinfo["flags"] & capi.RTP_KEEPALIVE) != 0, (p[:, 1] & 0x7F) == 123)
            assert np.array_equal((rinfo["flags"] & capi.RTP_MARKER) != 0, (p[:, 1] & 0x80) != 0)
            assert np.all(rinfo["flags"] & capi.RTP_ED137_OK)
            assert np.array_equal(rinfo["pt"], p[:, 1] & 0x7F)
            full = e["size"] > 20
            assert np.array_equal(rinfo["payload_len"][full], e["size"][full] - 20)
            met = full & ((p[:, 1] & 0x7F) != 123)              # an Rx leg's 20 + n packet may carry pt 123: never metered
            assert np.array_equal((rinfo["flags"] & capi.RTP_METERED) != 0, met)
            for i in np.nonzero(met)[0]:
                assert rpl[i, :e["size"][i] - 20].tobytes() == p[i, 20:e["size"][i]].tobytes()


def test_same_answer_as_batched_packetize():
    torch = torch_cuda()
    rng = np.random.default_rng(7)
    C_, F_, n, t0, fms = 512, 16, 160, 50_000, 20
    cts = [CALLTYPES[i] for i in rng.integers(len(CALLTYPES), size=C_)]
    cin = rng.integers(0, 2, C_).astype(bool)
    ka = rng.choice([200, 60, 0, 1000], C_)
    now0 = t0 + rng.integers(-100, 400, C_)
    pt = rng.choice([0, 8], C_)
    ssrc, seq0, ts0 = rng.integers(0, 1 << 32, C_), rng.integers(0, 1 << 16, C_), rng.integers(0, 1 << 32, C_)
    st = np.zeros(C_, capi.TX_CHAN)
    for c in range(C_):
        st[c] = tm.chan_init(cts[c], bool(cin[c]), int(pt[c]), int(ssrc[c]), int(seq0[c]), int(ts0[c]), int(ka[c]), int(now0[c]))
    g711 = rng.integers(0, 256, (F_, C_, n), dtype=np.uint8)
    ctl = ((rng.random((F_, C_)) < 0.2).astype(np.uint8) * capi.TX_CTL_SET) | rng.integers(0, 8, (F_, C_)).astype(np.uint8)
    with capi.Context(device=0, max_channels=C_) as ctx:
        # one batched launch
        d_st, d_last = to_dev(st), dev_zeros(C_ * n)
        d_pk, d_sz, d_inf = dev_zeros(F_ * C_ * 256), dev_zeros(F_ * C_ * 2), dev_zeros(F_ * C_ * 8)
        ctx.tx_packetize(d_st, d_last, d_pk, 256, d_sz, d_inf, C_, F_, n, t0, fms, g711=to_dev(g711), ctl=to_dev(ctl))
        torch.cuda.synchronize()
        bst, bpk, binf = to_host(d_st, capi.TX_CHAN), to_host(d_pk, np.uint8, (F_, C_, 256)), to_host(d_inf, capi.TX_INFO, (F_, C_))
        # the same frames staged, in two flushes of 8
        for c in range(C_):
            ctx.map_call(CALL0 + c, c)
            ctx.tx_open(CALL0 + c, cts[c], bool(cin[c]), int(ka[c]), int(now0[c]))
        for f0 in (0, 8):
            for c in range(C_):
                for f in range(f0, f0 + 8):
                    if ctl[f, c] & capi.TX_CTL_SET:            # IGDSP_TX_CTL_SET: setAdapterPtt / setAdapterQslOn before this frame
                        ctx.tx_set_ptt(CALL0 + c, bool(ctl[f, c] & 1), 0, 0)
                        ctx.tx_set_sql(CALL0 + c, bool(ctl[f, c] & 2), 0, -1)
                    pkt = sm.stream_packet(int(pt[c]), int(seq0[c] + f) & 0xFFFF, int(ts0[c] + f * n) & 0xFFFFFFFF, int(ssrc[c]), g711[f, c].tobytes(),
                                           int((ctl[f, c] >> 2) & 1))
                    assert ctx.on_tx_frame(CALL0 + c, pkt, t0 + f * fms) == 0
            assert ctx.tx_flush() == 8 * C_
            ent, pk = ctx.tx_results()
            ent, pk = ent.reshape(C_, 8), pk.reshape(C_, 8, 256)
            for k in range(8):
                f = f0 + k
                assert np.array_equal(ent["size"][:, k], binf["size"][f])
                assert np.array_equal(ent["ed137"][:, k], binf["ed137"][f])
                assert np.array_equal(ent["flags"][:, k], binf["flags"][f])
                assert np.array_equal(ent["level"][:, k], binf["level"][f])
                for c in range(C_):
                    s = int(binf["size"][f, c])
                    assert pk[c, k, :s].tobytes() == bpk[f, c, :s].tobytes(), (f, c)
        for c in range(C_):
            assert ctx.tx_get_chan(CALL0 + c).tobytes() == bst[c].tobytes(), c


def test_real_time_shape():
    rng = np.random.default_rng(11)
    L, n = 65536, 160
    model = sm.Legs(L)
    with capi.Context(device=0, max_channels=L) as ctx:
        open_legs(ctx, model, rng, L, 10_000)
        streams = [Stream(rng) for _ in range(L)]
        pays = rng.integers(0, 256, (64, n), dtype=np.uint8)
        t = 10_000
        for fl in range(20):
            frames = []
            for l in range(L):
                a = random_setter(ctx, rng, CALL0 + l) if rng.random() < 0.02 else None
                pkt = streams[l].packet(pays[(l + fl) % 64].tobytes())
                assert ctx.on_tx_frame(CALL0 + l, pkt, t) == 0
                frames.append((l, pkt, t, a))
            check_flush(ctx, model, frames)
            t += 20
        # full rings: 8 frames on every leg
        frames = []
        for l in range(L):
            for k in range(8):
                pkt = streams[l].packet(pays[(l + k) % 64].tobytes())
                assert ctx.on_tx_frame(CALL0 + l, pkt, t + 20 * k) == 0
                frames.append((l, pkt, t + 20 * k, None))
            assert ctx.on_tx_frame(CALL0 + l, streams[l].packet(pays[0].tobytes()), t + 160) == EBUSY
        check_flush(ctx, model, frames)
        compare_chans(ctx, model, L)


def test_threads_producers_setter_owner_and_rx(orc):
    L, P, rounds, n = 2048, 8, 30, 160
    rx0, n_rx, rx_call = L, 256, 100_000                       # RX calls rx_call + c on channels L + c
    rng = np.random.default_rng(3)
    with capi.Context(device=0, max_channels=L + n_rx) as ctx:
        for l in range(L):
            ctx.map_call(CALL0 + l, l)
            ctx.tx_open(CALL0 + l, "Tx", False, 200, 0)
            ctx.tx_set_ptt(CALL0 + l, True, 1, 0)              # gated: every frame 20 + n with its own payload
        for c in range(n_rx):
            ctx.map_call(rx_call + c, rx0 + c)
        pays = rng.integers(0, 256, (rounds, L, n), dtype=np.uint8)
        staged = [[] for _ in range(L)]                        # per leg: seq of each accepted frame
        busy = np.zeros(L, np.int64)
        last_id = np.zeros(L, np.int64)
        stop = threading.Event()
        errors = []

        def producer(p):
            try:
                for r in range(rounds):
                    for l in range(p, L, P):
                        pkt = sm.stream_packet(8, r, r * n, l, pays[r, l].tobytes())
                        rc = ctx.on_tx_frame(CALL0 + l, pkt, 20 * r)
                        if rc == 0:
                            staged[l].append(r)
                        else:
                            assert rc == EBUSY
                            busy[l] += 1
            except Exception as e:                             # noqa: BLE001
                errors.append(e)

        def setter():
            v = 1
            while not stop.is_set() and v < 64:               # pttid rises 1 .. 63 on every leg
                for l in range(L):
                    ctx.tx_set_ptt_id(CALL0 + l, v)
                last_id[:] = v
                v += 1

        results = []

        def owner():
            while not stop.is_set():
                ctx.tx_flush()
                results.append(ctx.tx_results())

        rx_bad = []

        def rx():
            codec = np.zeros(n_rx, np.uint8)
            for r in range(rounds):
                pl = rng.integers(0, 256, (1, n_rx, n), dtype=np.uint8)
                for c in range(n_rx):
                    ctx.on_rtp_frame(rx_call + c, 0, pl[0, c].tobytes())
                ctx.flush()
                est, _ = orc.decode_meter(pl, codec, want_pcm=True)
                for c in range(n_rx):
                    lv = ctx.poll(rx0 + c)
                    if (lv.byte_mean, lv.peak) != (est["byte_mean"][0, c], est["peak"][0, c]):
                        rx_bad.append((r, c))

        ths = [threading.Thread(target=producer, args=(p,)) for p in range(P)]
        aux = [threading.Thread(target=setter), threading.Thread(target=owner), threading.Thread(target=rx)]
        for th in ths + aux:
            th.start()
        for th in ths:
            th.join()
        aux[2].join()
        stop.set()
        aux[0].join()
        aux[1].join()
        assert not errors, errors
        assert not rx_bad, rx_bad[:5]
        ctx.tx_flush()
        results.append(ctx.tx_results())
        got = [[] for _ in range(L)]
        ids = [[] for _ in range(L)]
        for ent, pk in results:
            for i in range(len(ent)):
                l = int(ent["call_id"][i]) - CALL0
                r = int(pk[i, 2]) << 8 | int(pk[i, 3])
                got[l].append(r)
                ids[l].append((int(ent["ed137"][i]) >> 22) & 0x3F)
                assert ent["size"][i] == 20 + n and pk[i, 20:20 + n].tobytes() == pays[r, l].tobytes()
        for l in range(L):
            assert got[l] == staged[l], l                        # nothing lost or duplicated, staging order kept
            assert len(staged[l]) + busy[l] == rounds
            assert ids[l] == sorted(ids[l]), l                   # setters land in order
            assert ctx.tx_counts(CALL0 + l) == (busy[l], 0)
        # the setter's last values are applied by the next frame
        for l in range(L):
            ctx.on_tx_frame(CALL0 + l, sm.stream_packet(8, 999, 0, l, bytes(n)), 10_000)
        ctx.tx_flush()
        ent, _ = ctx.tx_results()
        assert np.all(((ent["ed137"] >> 22) & 0x3F) == last_id)


def test_error_paths():
    with capi.Context(device=0, max_channels=64) as ctx:
        good = sm.stream_packet(8, 1, 2, 3, bytes(160))
        assert ctx.tx_flush() == 0                              # no leg ever opened
        assert ctx.on_tx_frame(5, good, 0) == ENOENT            # not mapped
        ctx.map_call(5, 3)
        assert ctx.on_tx_frame(5, good, 0) == ENOENT            # mapped, no TX leg
        with pytest.raises(capi.IgdspError):
            ctx.tx_set_ptt(5, True)
        ctx.map_call(6, 4)
        ctx.tx_open(6, "Tx", False, 200, 0)
        assert ctx.on_tx_frame(5, good, 0) == ENOENT            # another channel's leg is open, not this one
        bad = [bytes([0x40]) + good[1:], bytes([0xC0]) + good[1:],             # V = 1, V = 3
               bytes([0x81]) + good[1:], bytes([0x90]) + good[1:], bytes([0xA0]) + good[1:],   # CC = 1, X, P
               good[:12], sm.stream_packet(8, 1, 2, 3, bytes(237))]           # n = 0, n = 237
        for b in bad:
            assert ctx.on_tx_frame(6, b, 0) == EINVAL
        assert ctx.on_tx_frame(6, sm.stream_packet(8, 1, 2, 3, bytes(236)), 0) == 0
        assert ctx.on_tx_frame(6, sm.stream_packet(8, 1, 2, 3, bytes(1)), 0) == 0
        ctx.tx_close(6)                                         # the two staged frames are dropped
        assert ctx.tx_counts(6) == (0, 2)
        assert ctx.on_tx_frame(6, good, 0) == ENOENT
        assert ctx.tx_flush() == 0
        ent, _ = ctx.tx_results()
        assert len(ent) == 0
        ctx.tx_open(6, "Rx", True, 100, 7)                      # starts over from the defaults
        assert ctx.tx_get_chan(6).tobytes() == sm.open_state("Rx", True, 100, 7).tobytes()
        assert ctx.on_tx_frame(6, good, 7) == 0
        assert ctx.tx_flush() == 1
        ent, _ = ctx.tx_results()
        assert len(ent) == 1 and ent["call_id"][0] == 6
