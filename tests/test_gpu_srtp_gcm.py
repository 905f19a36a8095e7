"""-m gpu: igdsp_srtp_gcm_protect / igdsp_srtp_gcm_unprotect (include/igdsp.h, "SRTP with AES-GCM") through the C ABI, byte for byte:
packets, sizes, records and states.  The reference is tests/srtp_gcm_model.py directly on one small scene and, everywhere else, the
library's host entries (igdsp_srtp_gcm_protect_packet / igdsp_srtp_gcm_unprotect_packet), which tests/test_srtp_gcm_cpu.py holds
against that model, the standards' known answers and OpenSSL.  Every output buffer is prefilled with 0xA5, so bytes behind size_out and
the slots of refused packets are seen untouched; guard bytes stand around every buffer.  Shapes around the kernel's ownership units (a
lane a leg, 64 legs a wave and block): 1 x 1, 65 x 3, 130 x 5 with the size list spread over (f, c) in 192-byte slots, 3 x 2 with
2032-byte packets in 2048-byte slots, 5 x 2 in 180-byte slots; both key sizes side by side; in place and out of place.  The size list
is tests/test_gpu_srtp.py's (its 180- and 181-byte packets do not leave room for 16 tag bytes in a 192-byte slot: MALFORMED by the rule,
beside healthy legs) and sizes that put a GHASH block's end on either side of a 64-byte piece boundary.  Then: one launch against the
same frames in two; a leg at another position and leg count; the chain igdsp_tx_packetize -> protect -> unprotect -> igdsp_depayload;
replay of a whole launch; tampered packets; the sequence wrap; BYPASS, RESET, a state of another suite or of random bytes and malformed
packets beside healthy legs; the yardstick's promise; argument clauses.  Every malformed input is one the rule refuses by its own
bounds, and every launch is valid by the argument rule."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import gpu_util as gu  # noqa: E402
from tests import srtp_gcm_model as gm  # noqa: E402

GUARD, FILL, TAG = 256, 0xA5, 16
SB = capi.SRTP_GCM_STATE.itemsize
# tests/test_gpu_srtp.py's list, then: with a 12-byte header ciphertext block k ends at 28 + 16 k, with a 20-byte header at 36 + 16 k, with
# an 80-byte one at 96 + 16 k: sizes whose last block ends just before, on and just behind the boundaries 64 and 128, and a last block
# whose slot lies in a piece of its own
SIZES = (12, 20, 33, 51, 52, 59, 60, 115, 116, 172, 180, 181) + (63, 64, 65, 76, 77, 124, 128, 129, 140, 141, 176)
FIT = tuple(s for s in SIZES if s + TAG <= 192)
KEY = bytes.fromhex("e1f97a0d3e018be0d64fa32c06de41390ec675ad498afeebb6960b3aabe6c173c317f2dabe357a7d5bb1c6a1c2")
EINVAL, ERANGE = -22, -34
MOVING = ("roc", "s_l", "have_s_l", "window", "n_ok", "n_auth_fail", "n_replay", "n_malformed")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


def leg_key(c):
    """a leg's own master key and salt: 32-byte keys on the even legs, 16-byte keys on the odd ones"""
    k = bytes((b + 31 * c) % 256 for b in KEY)
    return k[:28] if c % 2 else k[:44]


def fresh_states(C_, first=0):
    return np.array([capi.srtp_gcm_derive(leg_key(first + c)) for c in range(C_)], capi.SRTP_GCM_STATE)


def one_packet(size, seq, c, f):
    """a seeded packet of exactly `size` bytes: CSRCs and header extensions where they fit, the PT 123 keep-alive at 20 bytes"""
    rng = np.random.default_rng(1000 * c + f)
    if size == 20:
        return gm.rtp(seq, 0x5000 + c, b"", ext_len=1, pt=123)
    cc, ext = (3 if c % 3 == 1 else 0), (1 if c % 4 == 2 else None)
    if c % 7 == 3:
        cc, ext = 15, 1                                                    # the extension's length lies in the packet's second 64 bytes
    hdr = 12 + 4 * cc + (0 if ext is None else 4 + 4 * ext)
    if hdr > size:
        cc, ext, hdr = 0, None, 12
    return gm.rtp(seq, 0x5000 + c, rng.integers(0, 256, size - hdr, dtype=np.uint8).tobytes(), cc=cc, ext_len=ext, ts=160 * seq)


def scene(C_, F_, stride, sizes=SIZES, seq0=None, first=0):
    """packets [F][C][stride] (slack bytes 0x3C) and sizes [F][C]: the size list spread over (f, c), sequence numbers seq0[c] + f"""
    pk, sz = np.full((F_, C_, stride), 0x3C, np.uint8), np.zeros((F_, C_), np.uint16)
    for f in range(F_):
        for c in range(C_):
            g = first + c
            size = sizes[(f * 131 + g) % len(sizes)]
            p = one_packet(size, ((100 + 3 * g) if seq0 is None else seq0[c]) + f, g, f)
            pk[f, c, :size], sz[f, c] = np.frombuffer(p, np.uint8), size
    return pk, sz


def host_run(states, pk, sz, ostride, unprotect, ctl=None, base=None):
    """the host entries over [F][C]: (out [F][C][ostride] over `base` (default: all 0xA5), sizes_out, rec, the states after)"""
    F_, C_, stride = pk.shape
    out = np.full((F_, C_, ostride), FILL, np.uint8) if base is None else base.copy()
    szo, rec, st = np.zeros((F_, C_), np.uint16), np.zeros((F_, C_), capi.SRTP_REC), states.copy()
    for c in range(C_):
        s = np.array(st[c])                                                 # a record of its own, updated in place
        for f in range(F_):
            n_in = int(sz[f, c])
            if n_in > stride:                                              # the input slot is the packet's bound on the device
                assert ctl is None or ctl[f, c] != capi.SRTP_BYPASS
                got, n, r = capi.srtp_gcm_packet(s, bytes(2049), unprotect=unprotect, ctl=0 if ctl is None else int(ctl[f, c]), capacity=ostride)
            else:
                got, n, r = capi.srtp_gcm_packet(s, pk[f, c, :n_in].tobytes(), unprotect=unprotect, ctl=0 if ctl is None else int(ctl[f, c]), capacity=ostride)
            out[f, c, :n], szo[f, c], rec[f, c] = got[:n], n, r
        st[c] = s[()]
    return out, szo, rec, st


def guarded(a, fill=FILL):
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    g = np.full(GUARD, fill, np.uint8)
    return gu.to_dev(np.concatenate([g, b, g]))


def unguard(t, nbytes, what, fill=FILL):
    b = t.cpu().numpy()
    assert len(b) == nbytes + 2 * GUARD and np.all(b[:GUARD] == fill), f"bytes in front of {what} written"
    assert np.all(b[GUARD + nbytes:] == fill), f"bytes after {what} written"
    return b[GUARD:GUARD + nbytes]


def dev_run(ctx, states, pk, sz, ostride, unprotect, ctl=None, in_place=False, entry=None, with_rec=True):
    """one launch through the C ABI (entry: through that yardstick instead): (out, sizes_out, rec, the states after)"""
    torch = gu.torch_cuda()
    F_, C_, stride = pk.shape
    d_pk, d_sz, d_st = guarded(pk), guarded(sz.astype("<u2")), guarded(states)
    d_ctl = None if ctl is None else gu.to_dev(np.ascontiguousarray(ctl, np.uint8))
    d_out = d_pk if in_place else guarded(np.full((F_, C_, ostride), FILL, np.uint8))
    d_szo = d_sz if in_place else guarded(np.full((F_, C_), 0xA5A5, "<u2"))
    d_rec = guarded(np.full(F_ * C_ * 8, FILL, np.uint8)) if with_rec else None
    p = lambda t: None if t is None else t.data_ptr() + GUARD
    if entry:
        rc = capi.internal(entry)(ctx.h, None if d_ctl is None else d_ctl.data_ptr(), p(d_pk), p(d_sz), C_, F_, stride, p(d_st), p(d_out), ostride, p(d_szo), p(d_rec), None)
        assert rc == 0, rc
    else:
        ctx.srtp_gcm_protect(p(d_st), p(d_pk), p(d_sz), C_, F_, stride, p(d_out), ostride, p(d_szo), rec=p(d_rec), ctl=d_ctl, unprotect=unprotect)
    torch.cuda.synchronize()
    if not in_place:
        assert unguard(d_pk, pk.size, "d_packets").tobytes() == pk.tobytes() and unguard(d_sz, 2 * sz.size, "d_sizes").tobytes() == sz.astype("<u2").tobytes()
    out = unguard(d_out, F_ * C_ * ostride, "d_out").reshape(F_, C_, ostride).copy()
    szo = unguard(d_szo, 2 * F_ * C_, "d_sizes_out").view("<u2").reshape(F_, C_).copy()
    rec = unguard(d_rec, 8 * F_ * C_, "d_rec").view(capi.SRTP_REC).reshape(F_, C_).copy() if with_rec else None
    st = unguard(d_st, C_ * SB, "d_state").view(capi.SRTP_GCM_STATE).copy()
    return out, szo, rec, st


def same(dev, host, what=""):
    out, szo, rec, st = dev
    eout, eszo, erec, est = host
    assert np.array_equal(szo, eszo), (what, "sizes", np.argwhere(szo != eszo)[:6].tolist())
    if rec is not None:
        assert rec.tobytes() == erec.tobytes(), (what, "records", [(k, np.argwhere(rec[k] != erec[k])[:4].tolist()) for k in erec.dtype.names if not np.array_equal(rec[k], erec[k])])
    assert np.array_equal(out, eout), (what, "packets", np.argwhere(out != eout)[:6].tolist())
    assert st.tobytes() == est.tobytes(), (what, "states", [(k, np.argwhere(st[k] != est[k])[:4].tolist()) for k in est.dtype.names if not np.array_equal(st[k], est[k])])


def both_ways(ctx, C_, F_, stride, sizes=SIZES, in_place=False, seq0=None):
    """protect on the device against the host, then unprotect of that; returns the protected launch and the receiver's states"""
    pk, sz = scene(C_, F_, stride, sizes, seq0)
    fit = sz + TAG <= stride                                               # the others find no room for the tag in their slot: MALFORMED
    tx = fresh_states(C_)
    host = host_run(tx, pk, sz, stride, False, base=pk if in_place else None)
    same(dev_run(ctx, tx, pk, sz, stride, False, in_place=in_place), host, "protect")
    assert (host[2]["flags"][fit] & capi.SRTP_OK).all() and (host[2]["flags"][~fit] == capi.SRTP_MALFORMED).all() and fit.any()
    assert np.array_equal(host[1], np.where(fit, sz + TAG, 0))
    rx = fresh_states(C_)
    back = host_run(rx, host[0], host[1], stride, True, base=host[0] if in_place else None)
    same(dev_run(ctx, rx, host[0], host[1], stride, True, in_place=in_place), back, "unprotect")
    assert np.array_equal(back[1], np.where(fit, sz, 0)) and (back[2]["flags"][~fit] == capi.SRTP_EMPTY).all()
    assert all(back[0][f, c, :sz[f, c]].tobytes() == pk[f, c, :sz[f, c]].tobytes() for f in range(F_) for c in range(C_) if fit[f, c])
    return pk, sz, host, back


# ---- 1. shapes, both key sizes side by side, in place and out of place
@pytest.mark.parametrize("in_place", (False, True))
@pytest.mark.parametrize("C_,F_,stride,sizes", [(1, 1, 192, (176,)), (65, 3, 192, SIZES), (130, 5, 192, SIZES), (3, 2, 2048, (2032,)), (5, 2, 180, (115, 164, 12))])
def test_shapes(ctx, C_, F_, stride, sizes, in_place):
    both_ways(ctx, C_, F_, stride, sizes, in_place)


def test_device_against_the_model(ctx):
    """the model itself, not the host entries: bytes, sizes, records and the state's moving fields, both directions"""
    C_, F_, stride = 6, 3, 192
    pk, sz = scene(C_, F_, stride, (176, 20, 77, 12, 129, 65, 33))
    prot = dev_run(ctx, fresh_states(C_), pk, sz, stride, False)
    back = dev_run(ctx, fresh_states(C_), prot[0], prot[1], stride, True)
    for c in range(C_):
        mtx, mrx = gm.Leg(leg_key(c)), gm.Leg(leg_key(c))
        for f in range(F_):
            want, wrec = mtx.protect(pk[f, c, :sz[f, c]].tobytes(), in_cap=stride, out_cap=stride)
            n = int(prot[1][f, c])
            assert prot[0][f, c, :n].tobytes() == want and (prot[0][f, c, n:] == FILL).all(), (c, f)
            assert {k: int(prot[2][f, c][k]) for k in ("flags", "size_out", "roc_used")} == wrec, (c, f)
            clear, crec = mrx.unprotect(want, in_cap=stride, out_cap=stride)
            m = int(back[1][f, c])
            assert back[0][f, c, :m].tobytes() == clear == pk[f, c, :sz[f, c]].tobytes() and (back[0][f, c, m:] == FILL).all(), (c, f)
            assert {k: int(back[2][f, c][k]) for k in ("flags", "size_out", "roc_used")} == crec, (c, f)
        assert {k: int(prot[3][c][k]) for k in MOVING} == mtx.moving() and {k: int(back[3][c][k]) for k in MOVING} == mrx.moving(), c


def test_other_output_stride_and_no_records(ctx):
    pk, sz = scene(7, 2, 192)
    tx = fresh_states(7)
    host = host_run(tx, pk, sz, 256, False)                                # 256 holds every protected packet, the 181 + 16 bytes too
    assert (host[2]["flags"] & capi.SRTP_OK).all()
    same(dev_run(ctx, tx, pk, sz, 256, False, with_rec=False), host)
    rx = fresh_states(7)
    pk2 = np.full((2, 7, 200), 0x3C, np.uint8)
    pk2[:, :, :200] = host[0][:, :, :200]
    same(dev_run(ctx, rx, pk2, host[1], 184, True), host_run(rx, pk2, host[1], 184, True))   # 184 holds every clear packet, no slack for more


# ---- 2. one launch against the same frames in two
def test_split_over_launches(ctx):
    C_, stride = 67, 192
    pk, sz = scene(C_, 6, stride)
    for unprotect in (False, True):
        if unprotect:
            pk, sz = host_run(fresh_states(C_), pk, sz, stride, False)[:2]
        st0 = fresh_states(C_)
        whole = dev_run(ctx, st0, pk, sz, stride, unprotect)
        a = dev_run(ctx, st0, pk[:2], sz[:2], stride, unprotect)
        b = dev_run(ctx, a[3], pk[2:], sz[2:], stride, unprotect)
        assert np.array_equal(np.concatenate([a[0], b[0]]), whole[0]) and np.array_equal(np.concatenate([a[1], b[1]]), whole[1])
        assert np.concatenate([a[2], b[2]]).tobytes() == whole[2].tobytes() and b[3].tobytes() == whole[3].tobytes()
        same(whole, host_run(st0, pk, sz, stride, unprotect))


# ---- 3. a leg's bytes do not depend on its position or the leg count
def test_position_invariance(ctx):
    F_, stride = 4, 192
    pk, sz = scene(130, F_, stride)
    st = fresh_states(130)
    full = dev_run(ctx, st, pk, sz, stride, False)
    for c in (0, 63, 64, 129):
        alone = dev_run(ctx, st[c:c + 1], pk[:, c:c + 1], sz[:, c:c + 1], stride, False)
        assert np.array_equal(alone[0][:, 0], full[0][:, c]) and np.array_equal(alone[1][:, 0], full[1][:, c]), c
        assert alone[2][:, 0].tobytes() == full[2][:, c].tobytes() and alone[3][0].tobytes() == full[3][c].tobytes(), c
    # and the other way round: one leg's packets and state at lane 0, lane 63 and lane 64 of 130 legs
    for pos in (0, 63, 64):
        pk2, sz2, st2 = pk.copy(), sz.copy(), st.copy()
        pk2[:, pos], sz2[:, pos], st2[pos] = pk[:, 5], sz[:, 5], st[5]
        moved = dev_run(ctx, st2, pk2, sz2, stride, False)
        assert np.array_equal(moved[0][:, pos], full[0][:, 5]) and moved[3][pos].tobytes() == full[3][5].tobytes(), pos


# ---- 4. the chain: igdsp_tx_packetize -> protect -> unprotect -> igdsp_depayload
def test_chain_packetize_protect_unprotect_depayload(ctx):
    torch = gu.torch_cuda()
    C_, F_, n, stride, t0 = 70, 6, 160, 208, 1_700_000_000_000             # 180-byte ED-137 packets and their 16 tag bytes: 208-byte slots
    rng = np.random.default_rng(12)
    g711 = rng.integers(0, 256, (F_, C_, n), dtype=np.uint8)
    txst = np.zeros(C_, capi.TX_CHAN)
    for c in range(C_):
        txst[c] = capi.tx_chan_init("Tx", False, 8 if c % 2 else 0, 0x2000 + c, 65530 + c if c % 5 == 0 else 9 * c, 1000 * c, now_ms=t0)[()]
    ptt = np.where(rng.random((F_, C_)) < 0.7, 0x81, 0x80).astype(np.uint8)    # a PTT-type leg sends a payload on the frames with PTT alone,
    ptt[1:, ::3] = 0x80                                                    # every third leg falls silent after its first frame and, past its
    txst["first_r2s"][::3] = 0                                             # first R2S packets, sends nothing until a keep-alive is due
    d_pk, d_sz, d_inf = gu.dev_zeros(F_ * C_ * stride, FILL), gu.dev_zeros(F_ * C_ * 2), gu.dev_zeros(F_ * C_ * 8)
    ctx.tx_packetize(gu.to_dev(txst), gu.to_dev(np.zeros((C_, n), np.uint8)), d_pk, stride, d_sz, d_inf, C_, F_, n, t0, 20, g711=gu.to_dev(g711), ctl=gu.to_dev(ptt))
    torch.cuda.synchronize()
    pk, sz = gu.to_host(d_pk, np.uint8, (F_, C_, stride)).copy(), gu.to_host(d_sz, np.uint16, (F_, C_)).copy()
    assert (sz == 0).any() and (sz > n).any()                        # unsent frames and voice packets, side by side
    tx, rx = fresh_states(C_), fresh_states(C_)
    prot = dev_run(ctx, tx, pk, sz, stride, False)
    same(prot, host_run(tx, pk, sz, stride, False), "protect")
    assert np.array_equal(prot[2]["flags"][sz == 0], np.full(int((sz == 0).sum()), capi.SRTP_EMPTY)) and (prot[1][sz == 0] == 0).all()
    assert ((prot[2]["flags"][sz != 0] & capi.SRTP_OK) != 0).all() and np.array_equal(prot[1][sz != 0], sz[sz != 0] + TAG)
    back = dev_run(ctx, rx, prot[0], prot[1], stride, True)
    same(back, host_run(rx, prot[0], prot[1], stride, True), "unprotect")
    assert np.array_equal(back[1], sz)

    def depay(packets, sizes):
        d_pl, d_len, d_info = gu.dev_zeros(F_ * C_ * n, 0x11), gu.dev_zeros(F_ * C_ * 2, 0x11), gu.dev_zeros(F_ * C_ * 8, 0x11)
        ctx.depayload(gu.to_dev(packets), gu.to_dev(sizes.astype("<u2")), gu.to_dev(np.ones(C_, np.uint8)), C_, F_, stride, n, d_pl, d_len, d_info)
        torch.cuda.synchronize()
        return d_pl.cpu().numpy().tobytes(), d_len.cpu().numpy().tobytes(), d_info.cpu().numpy().tobytes()

    clear = np.full_like(pk, FILL)                                         # the bytes behind a packet's end are not the packet's
    for f in range(F_):
        for c in range(C_):
            clear[f, c, :sz[f, c]] = pk[f, c, :sz[f, c]]
    assert np.array_equal(back[0], clear)
    assert depay(back[0], back[1]) == depay(pk, sz)


# ---- 5. the same protected launch a second time: every packet a replay
def test_replay_of_a_launch(ctx):
    C_, F_, stride = 66, 4, 192
    pk, sz, prot, back = both_ways(ctx, C_, F_, stride, FIT)
    again = dev_run(ctx, back[3], prot[0], prot[1], stride, True)
    same(again, host_run(back[3], prot[0], prot[1], stride, True))
    assert (again[2]["flags"] == capi.SRTP_REPLAY).all() and (again[1] == 0).all() and (again[0] == FILL).all()
    assert (again[3]["n_replay"] == F_).all() and (again[3]["n_ok"] == F_).all()


# ---- 6. one bit flipped in one packet of each of three legs
@pytest.mark.parametrize("in_place", (False, True))
def test_tampered_packets(ctx, in_place):
    C_, F_, stride = 66, 3, 192
    pk, sz = scene(C_, F_, stride, FIT)
    prot = host_run(fresh_states(C_), pk, sz, stride, False)
    bad = prot[0].copy()
    for (f, c, where) in ((0, 0, 1), (1, 63, int(prot[1][1, 63]) - 1), (2, 64, 14)):     # a header byte (the AAD), the tag's last byte, a payload or header byte
        bad[f, c, where] ^= 0x04
    rx = fresh_states(C_)
    host = host_run(rx, bad, prot[1], stride, True, base=bad if in_place else None)
    dev = dev_run(ctx, rx, bad, prot[1], stride, True, in_place=in_place)
    same(dev, host)
    fl = dev[2]["flags"]
    assert fl[0, 0] == fl[1, 63] == fl[2, 64] == capi.SRTP_AUTH_FAIL and int((fl == capi.SRTP_AUTH_FAIL).sum()) == 3 and int(((fl & capi.SRTP_OK) != 0).sum()) == F_ * C_ - 3
    assert dev[3]["n_auth_fail"][[0, 63, 64]].tolist() == [1, 1, 1] and int(dev[3]["n_auth_fail"].sum()) == 3
    for (f, c) in ((0, 0), (1, 63), (2, 64)):                              # a refused slot keeps its bytes: the fill, in place the packet as it came
        assert dev[1][f, c] == 0 and (dev[0][f, c] == (bad[f, c] if in_place else FILL)).all(), (f, c)


# ---- 7. the sequence wrap on one leg, its neighbours far from it: the rollover counter enters the IV
def test_roc_wrap(ctx):
    C_, F_, stride = 5, 6, 192
    seq0 = [100, 100, 65534, 100, 65533]
    pk, sz, prot, back = both_ways(ctx, C_, F_, stride, FIT, seq0=seq0)
    assert prot[3]["roc"].tolist() == [0, 0, 1, 0, 1] == back[3]["roc"].tolist()
    rolled = (prot[2]["flags"] & capi.SRTP_ROLLED) != 0
    assert rolled.sum(axis=0).tolist() == [0, 0, 1, 0, 1] and rolled[2, 2] and rolled[3, 4]
    assert ((back[2]["flags"] & capi.SRTP_ROLLED) != 0).sum(axis=0).tolist() == [0, 0, 1, 0, 1]
    assert prot[2]["roc_used"][:, 2].tolist() == [0, 0, 1, 1, 1, 1]
    # the packets from behind the wrap fail under a receiver that starts there with roc 0
    late = dev_run(ctx, fresh_states(C_), prot[0][3:], prot[1][3:], stride, True)
    same(late, host_run(fresh_states(C_), prot[0][3:], prot[1][3:], stride, True))
    assert (late[2]["flags"][:, [2, 4]] == capi.SRTP_AUTH_FAIL).all() and ((late[2]["flags"][:, [0, 1, 3]] & capi.SRTP_OK) != 0).all()


# ---- 8. BYPASS and RESET per leg and frame, states that are not this suite's, malformed packets: the neighbours stay what they are
@pytest.mark.parametrize("unprotect", (False, True))
def test_control_bad_state_and_malformed(ctx, unprotect):
    C_, F_, stride = 70, 4, 192
    pk, sz = scene(C_, F_, stride, FIT)
    if unprotect:
        pk, sz = host_run(fresh_states(C_), pk, sz, stride, False)[:2]
    st = fresh_states(C_)
    st[3] = np.random.default_rng(4).integers(0, 256, SB, dtype=np.uint8).view(capi.SRTP_GCM_STATE)[0]      # no key
    st[64] = np.zeros((), capi.SRTP_GCM_STATE)
    other = np.zeros(SB, np.uint8)
    other[:288] = np.frombuffer(capi.srtp_derive(KEY[:30], 10).tobytes(), np.uint8)                       # an igdsp_srtp_state's bytes: another suite's tag word
    st[11] = other.view(capi.SRTP_GCM_STATE)[0]
    st["tag"][12] = capi.SRTP_GCM_TAG | 24                                                              # the constant with a key size that is none
    ctl = np.zeros((F_, C_), np.uint8)
    ctl[:, 1] = capi.SRTP_BYPASS
    ctl[2, 5] = capi.SRTP_BYPASS
    ctl[:, 64] = capi.SRTP_BYPASS                                          # BYPASS needs no key
    ctl[2, 6] = ctl[1, 65] = capi.SRTP_RESET
    ctl[:, 8] = 200                                                        # another value is RUN
    pk, sz = pk.copy(), sz.copy()
    pk[0, 7, 0] = (pk[0, 7, 0] & 0x3F) | 0x40                              # version 1
    sz[1, 7] = 11                                                          # shorter than a header
    pk[2, 7, :16] = np.frombuffer(gm.rtp(9, 1, b"", ext_len=0)[:14] + (200).to_bytes(2, "big"), np.uint8)   # the extension passes the packet's end
    pk[3, 7, 0] = 0x8F                                                     # 15 CSRCs in a packet that ends before them
    sz[3, 7] = 40
    pk[0, 66, 0], sz[0, 66] = 0x9F, 74                                     # X behind 15 CSRCs, the extension's header cut off
    sz[1, 66] = stride + 4                                                 # longer than its slot
    sz[2, 66] = 180 if not unprotect else 12                               # protect: no room for the tag; unprotect: no room for one in the packet
    sz[3, 9] = 0                                                           # an unsent frame
    host = host_run(st, pk, sz, stride, unprotect, ctl=ctl)
    dev = dev_run(ctx, st, pk, sz, stride, unprotect, ctl=ctl)
    same(dev, host)
    fl = dev[2]["flags"]
    for c in (3, 11, 12):
        assert (fl[:, c] == capi.SRTP_NO_KEY).all() and (dev[1][:, c] == 0).all() and (dev[0][:, c] == FILL).all() and dev[3][c].tobytes() == st[c].tobytes(), c
    assert (fl[:, [1, 64]] == capi.SRTP_BYPASSED).all() and np.array_equal(dev[0][:, 1, :12], pk[:, 1, :12]) and dev[3][1].tobytes() == st[1].tobytes()
    assert (fl[:, 7] == capi.SRTP_MALFORMED).all() and (fl[:3, 66] == capi.SRTP_MALFORMED).all() and int(dev[3]["n_malformed"][7]) == 4
    assert fl[3, 9] == capi.SRTP_EMPTY and ((fl[:, 13:63] & capi.SRTP_OK) != 0).all()
    if unprotect:
        assert fl[2, 6] & capi.SRTP_OK and int(dev[3]["window"][6]) == 3    # RESET, then two packets in order
    else:
        assert (fl[:, 6] & capi.SRTP_OK).all()


# ---- 9. the yardstick's written promise
def test_yardstick_moves_and_computes_nothing(ctx):
    C_, F_, stride = 66, 3, 192
    pk, sz = scene(C_, F_, stride, FIT)
    sz[1, 4] = 0
    sz[2, 7] = 11
    st = fresh_states(C_)
    st[9] = np.zeros((), capi.SRTP_GCM_STATE)
    out, szo, rec, after = dev_run(ctx, st, pk, sz, stride, False, entry="igdsp_internal_srtp_gcm_move")
    assert after.tobytes() == st.tobytes()                                 # the state's words are stored as read
    for f in range(F_):
        for c in range(C_):
            n = int(sz[f, c])
            if c == 9 or n < 12:
                assert szo[f, c] == 0 and (out[f, c] == FILL).all(), (f, c)
                continue
            assert szo[f, c] == n + TAG and rec[f, c]["flags"] == capi.SRTP_BYPASSED and rec[f, c]["size_out"] == n + TAG and rec[f, c]["roc_used"] == 0, (f, c)
            assert np.array_equal(out[f, c, :n], pk[f, c, :n]) and (out[f, c, n:n + TAG] == 0).all() and (out[f, c, n + TAG:] == FILL).all(), (f, c)


# ---- 10. the argument clauses through the C ABI
def test_argument_paths(ctx):
    L = capi.load()
    C_, F_, stride = 4, 2, 192
    d = dict(pk=gu.dev_zeros(F_ * C_ * stride + 64), sz=gu.dev_zeros(F_ * C_ * 2 + 64), st=gu.to_dev(fresh_states(C_)), out=gu.dev_zeros(F_ * C_ * stride + 64),
             szo=gu.dev_zeros(F_ * C_ * 2 + 64), rec=gu.dev_zeros(F_ * C_ * 8 + 64))
    p = {k: t.data_ptr() for k, t in d.items()}

    def call(fn=L.igdsp_srtp_gcm_protect, h=ctx.h, ctl=None, pk=p["pk"], sz=p["sz"], C=C_, F=F_, s=stride, st=p["st"], out=p["out"], os=stride, szo=p["szo"], rec=p["rec"]):
        return fn(h, ctl, pk, sz, C, F, s, st, out, os, szo, rec, None)

    for fn in (L.igdsp_srtp_gcm_protect, L.igdsp_srtp_gcm_unprotect, capi.internal("igdsp_internal_srtp_gcm_move")):
        assert call(fn) == 0 and call(fn, h=None) == EINVAL
        assert call(fn, s=190) == EINVAL and call(fn, os=2052) == EINVAL and call(fn, s=8, C=0) == EINVAL
        assert call(fn, C=0, st=None) == 0 and call(fn, F=0, sz=None) == 0
        assert call(fn, sz=None) == EINVAL and b"d_sizes is required" in L.igdsp_last_error(ctx.h)
        assert call(fn, st=None) == EINVAL and call(fn, out=None) == EINVAL and call(fn, szo=None) == EINVAL and call(fn, rec=None) == 0
        assert call(fn, C=1 << 28, F=16) == ERANGE
        assert call(fn, pk=p["pk"] + 2) == EINVAL and call(fn, st=p["st"] + 8) == EINVAL and call(fn, rec=p["rec"] + 4) == EINVAL and call(fn, szo=p["szo"] + 1) == EINVAL
        assert call(fn, out=p["pk"], szo=p["sz"]) == 0                     # in place
        assert call(fn, out=p["pk"], os=196) == EINVAL and b"overlap" in L.igdsp_last_error(ctx.h)
        assert call(fn, out=p["pk"] + stride) == EINVAL and call(fn, rec=p["st"]) == EINVAL and call(fn, szo=p["out"]) == EINVAL
    gu.torch_cuda().cuda.synchronize()
