"""Independent numpy restatement of igdsp_bss_select (include/igdsp.h, section "Best signal selection") for any group size: the word
rule, the squelch, the reference's vote (roip_ed137.cpp:5985-6119) with a frame as the tick, and the emit.  Decodes with the oracle's
G.711 tables and scales with conf_model.scale (the Q7 rule of igdsp_conf_mix)."""
import numpy as np

from tests import conf_model as cm
from tests import record_model

RTP_RUNT = 0x40
STORE_PTS = (0, 8, 18, 123)
U32 = 0xFFFFFFFF


def squ(w):
    return (int(w) >> 28) & 1


def bss(w):
    return (int(w) & 0xF8) >> 3


def stores(info_rec):
    """the record stores its word on the channel: not a runt, PT 0 / 8 / 18 / 123 (transport_rtp_cb)"""
    return not (int(info_rec["flags"]) & RTP_RUNT) and int(info_rec["pt"]) in STORE_PTS


def groups_of(group_ptr, n_members, n_groups):
    """[(b, e)] per group: values clamped to n_members, a descending range empty"""
    ptr = np.minimum(np.asarray(group_ptr, np.int64), n_members)
    out = []
    for g in range(n_groups):
        b, e = int(ptr[g]), int(ptr[g + 1])
        out.append((b, max(b, e)))
    return out


def select(info, group_ptr, members, n_members, n_channels, n_groups, state, words, vote_frames=0, mute=None):
    """info: RTP_INFO [F][C].  state: list of [count, voted, on, votes] per group (or a BSS_STATE array), words: uint32 [n_members];
    both are copied.  Returns (sel int32 [F][G], state uint32 [G][4], words uint32 [n_members])."""
    vf = vote_frames or 10
    F_ = info.shape[0]
    mem = [int(m) for m in np.asarray(members, np.int64)[:n_members]]
    words = [int(w) for w in np.asarray(words, np.int64)[:n_members]]
    st = np.array([[int(s[0]), int(s[1]), int(s[2]), int(s[3])] for s in np.asarray(state).tolist()], np.int64).reshape(-1, 4)
    rng = groups_of(group_ptr, n_members, n_groups)
    sel = np.full((F_, n_groups), -1, np.int32)
    for f in range(F_):
        for k, c in enumerate(mem):                                   # 1. the words, every slot
            if c < n_channels and stores(info[f, c]):
                words[k] = int(info[f, c]["ed137"])
        for g, (b, e) in enumerate(rng):
            muted = mute is not None and mute[g] != 0
            rx = [squ(words[k]) == 1 and mem[k] < n_channels and not muted for k in range(b, e)]    # 2.
            rssi = [bss(words[k]) if rx[k - b] else -1 for k in range(b, e)]
            count, voted, on, votes = (int(x) for x in st[g])
            on = 1 if on else 0
            if voted and (voted > e - b or not rx[voted - 1]):        # 3. the voted member closed (or names none)
                count, on, voted = 0, 0, 0
            if any(rx):
                count = min(count + 1, U32)
                if count >= vf and not on:
                    best = max(rssi)
                    pos = next(i for i in range(e - b) if rx[i] and rssi[i] == best)
                    on, voted, votes = 1, pos + 1, (votes + 1) & U32
            else:
                count, on, voted = 0, 0, 0
            st[g] = (count, voted, on, votes)
            sel[f, g] = mem[b + voted - 1] if voted else -1
    return sel, st.astype(np.uint32), np.array(words, np.uint32)


def emit(sel, x, n, gain=None, length=None):
    """out int16 [F][G][n] and stats [F][G] for the selection sel [F][G] over decoded samples x [F][C][n] (int64); gain [C] Q7 (None:
    256), length [F][C] (None: n).  A voted frame is igdsp_conf_mix of a one-member port."""
    F_, G_ = sel.shape
    out = np.zeros((F_, G_, n), np.int16)
    live, sat = np.zeros((F_, G_), bool), np.zeros((F_, G_), bool)
    s_idx = np.arange(n)
    for f in range(F_):
        for g in range(G_):
            c = int(sel[f, g])
            if c < 0:
                continue
            ln = n if length is None else min(int(length[f, c]), n)
            if ln == 0:
                continue
            gq = 256 if gain is None else int(gain[c])
            out[f, g], fired = cm.scale(np.where(s_idx < ln, x[f, c], 0), gq)
            live[f, g], sat[f, g] = True, fired.any()
    rec = record_model.records(out, live=live, extra=np.where(sat, cm.FLAG_SATURATED, 0))
    return out, {k: rec[k].astype(np.float32 if k == "rms" else rec.dtype[k]) for k in rec.dtype.names}


def word(squelch, bss_q, ptt_type=0):
    """an ED-137 word (host order) with SQU and the BSS index set"""
    return ((ptt_type & 7) << 29) | ((1 if squelch else 0) << 28) | ((bss_q & 31) << 3)


def select_uniform(info, m, state, words, vote_frames=0):
    """select() for n_groups = C / m groups of m consecutive channels (members = arange(C), no mute), vectorised over the groups for
    full-size shapes.  Same arguments and results as select()."""
    vf = vote_frames or 10
    F_, C_ = info.shape
    G_ = C_ // m
    w = np.asarray(words, np.int64).reshape(G_, m).copy()
    st = np.array(np.asarray(state).tolist(), np.int64).reshape(G_, 4)
    count, voted, on, votes = st[:, 0].copy(), st[:, 1].copy(), (st[:, 2] != 0).astype(np.int64), st[:, 3].copy()
    sel = np.full((F_, G_), -1, np.int32)
    gi = np.arange(G_)
    for f in range(F_):
        rec = info[f].reshape(G_, m)
        upd = ((rec["flags"].astype(np.int64) & RTP_RUNT) == 0) & np.isin(rec["pt"], STORE_PTS)
        w = np.where(upd, rec["ed137"].astype(np.int64), w)
        rx = ((w >> 28) & 1) == 1
        rssi = np.where(rx, (w & 0xF8) >> 3, -1)
        vrx = rx[gi, np.clip(voted - 1, 0, m - 1)] & (voted >= 1) & (voted <= m)
        drop = (voted != 0) & ~vrx
        count, on, voted = np.where(drop, 0, count), np.where(drop, 0, on), np.where(drop, 0, voted)
        anyrx = rx.any(axis=1)
        count = np.where(anyrx, np.minimum(count + 1, U32), 0)
        vote = anyrx & (count >= vf) & (on == 0)
        pos = np.argmax(rssi, axis=1)                                    # the first of the highest (closed: -1)
        voted = np.where(vote, pos + 1, np.where(anyrx, voted, 0))
        votes = np.where(vote, (votes + 1) & U32, votes)
        on = np.where(vote, 1, np.where(anyrx, on, 0))
        sel[f] = np.where(voted > 0, gi * m + voted - 1, -1)
    return sel, np.stack([count, voted, on, votes], axis=1).astype(np.uint32), w.reshape(-1).astype(np.uint32)
