"""Two independent restatements of igdsp_ptt_arbitrate (include/igdsp.h, section "PTT priority arbitration"), written from that
contract: arbitrate_literal — the reference's loop shape (roip_ed137.cpp:6124-6231) with a volume per leg, scalar, from the reset
state, for tables in which every slot belongs to one group; and arbitrate — the holder form the device keeps, any table and any start
state, vectorised over slots and groups (a numpy step per member position).  The emit is bss_model.emit (step 4 of the vote)."""
import numpy as np

from tests import bss_model as bm

RELEASE_FRAMES = 12
ON, PRESS, RELEASE, TAKEOVER = 1, 2, 4, 8
CTL_PTT, CTL_SET = 1, 0x80
STATE = np.dtype([("level", "<u4"), ("holder", "<u4"), ("takeovers", "<u4"), ("reserved", "<u4")])
SLOT = np.dtype([("word", "<u4"), ("last_tx", "u1"), ("release_cnt", "u1"), ("pressed", "u1"), ("reserved", "u1")])
TICK = np.dtype([("sel", "<i4"), ("level", "u1"), ("ptt_id", "u1"), ("flags", "u1"), ("ctl", "u1")])


def ptt_type(w):
    return (int(w) >> 29) & 7


def ptt_id(w):
    return (int(w) >> 22) & 0x3F


def word(ptype, pid=0, squelch=0):
    """an ED-137 word (host order) with the PTT type and id set"""
    return ((ptype & 7) << 29) | ((1 if squelch else 0) << 28) | ((pid & 0x3F) << 22)


def stored_words(info, members, n_channels, words0=None):
    """[F][n_members]: every slot's stored word after step 1 of each frame (a slot whose member is >= n_channels keeps words0)"""
    mem = [int(m) for m in members]
    w = [0] * len(mem) if words0 is None else [int(x) for x in words0]
    out = np.zeros((info.shape[0], len(mem)), np.uint32)
    for f in range(info.shape[0]):
        for k, c in enumerate(mem):
            if c < n_channels and bm.stores(info[f, c]):
                w[k] = int(info[f, c]["ed137"])
        out[f] = w
    return out


def arbitrate_literal(info, group_ptr, members, n_members, n_channels, n_groups, rxonly=None, release_frames=0):
    """The literal form from the reset state: per leg the stored word, lastTx, lastTxmsec, m_PttPressed and a volume (unmuted or not);
    per group ptt_level.  Returns (tick TICK [F][G], level [G], takeovers [G], slots SLOT [n_members], unmuted bool [n_members],
    counts): counts tallies what a fuzz must contain (takeover, steal, bridged, equal, held, ticks)."""
    rf = release_frames or RELEASE_FRAMES
    F_ = info.shape[0]
    mem = [int(m) for m in np.asarray(members, np.int64)[:n_members]]
    rng = bm.groups_of(group_ptr, n_members, n_groups)
    seen = np.zeros(n_members, np.int64)
    for b, e in rng:
        seen[b:e] += 1
    assert seen.max(initial=0) <= 1, "the literal form takes tables without shared slots"
    wordk, last_tx, cnt, pressed, unmuted = ([0] * n_members for _ in range(5))
    level, takeovers, stolen = [0] * n_groups, [0] * n_groups, [False] * n_groups
    counts = dict(takeover=0, steal=0, bridged=0, equal=0, held=0, ticks=0)
    tick = np.zeros((F_, n_groups), TICK)
    for f in range(F_):
        for k, c in enumerate(mem):                                   # transport_rtp_cb stores the word, whatever checkEvents does
            if c < n_channels and bm.stores(info[f, c]):
                wordk[k] = int(info[f, c]["ed137"])
        for g, (b, e) in enumerate(rng):
            flags = 0
            for k in range(b, e):
                c = mem[k]
                if c >= n_channels:                                   # :6131 no call
                    continue
                p = 0 if (rxonly is not None and rxonly[c]) else ptt_type(wordk[k])          # :6134
                if p != last_tx[k]:                                   # :6139-6154
                    if p == 0:
                        cnt[k] = min(cnt[k] + 1, 255)
                        if cnt[k] < rf:
                            p = 1
                            counts["bridged"] += 1
                else:
                    cnt[k] = 0
                last_tx[k] = p
                if p > level[g]:                                      # :6157-6177 the highest type takes the transmitter
                    if any(unmuted[j] for j in range(b, e) if j != k):
                        counts["steal"] += 1 if stolen[g] else 0
                    level[g] = p
                    for j in range(b, e):
                        unmuted[j] = 1 if j == k else 0               # MUTE every other leg, UNMUTE this one
                    takeovers[g] = (takeovers[g] + 1) & bm.U32
                    flags |= TAKEOVER
                    counts["takeover"] += 1
                    stolen[g] = False
                elif p > 0 and p == level[g] and not unmuted[k]:
                    counts["equal"] += 1
                if p > 0 and not pressed[k]:                          # :6191-6222
                    pressed[k] = 1
                    flags |= PRESS
                elif p == 0 and pressed[k]:
                    pressed[k] = 0
                    flags |= RELEASE
                    if unmuted[k]:
                        unmuted[k] = 0
                        stolen[g] = False
                    elif any(unmuted[j] for j in range(b, e)):
                        stolen[g] = True                              # a non-holder's release: the level drops under the holder
                    level[g] = 0
            if any(pressed[k] for k in range(b, e) if mem[k] < n_channels):
                flags |= ON
            who = [k for k in range(b, e) if unmuted[k]]
            assert len(who) <= 1
            t = tick[f, g]
            t["sel"] = mem[who[0]] if who and mem[who[0]] < n_channels else -1
            t["level"] = level[g]
            t["ptt_id"] = ptt_id(wordk[who[0]]) if who else 0
            t["flags"] = flags
            t["ctl"] = CTL_SET | (CTL_PTT if flags & ON else 0)
            counts["ticks"] += 1
            counts["held"] += 1 if who else 0
    slots = np.zeros(n_members, SLOT)
    slots["word"], slots["last_tx"], slots["release_cnt"], slots["pressed"] = wordk, last_tx, cnt, pressed
    return tick, np.array(level, np.uint32), np.array(takeovers, np.uint32), slots, np.array(unmuted, bool), counts


def arbitrate(info, group_ptr, members, n_members, n_channels, n_groups, state, slots, rxonly=None, release_frames=0):
    """The holder form.  info: RTP_INFO [F][C]; state: STATE-shaped [G] (any 16-byte records), slots: SLOT-shaped [n_members]; both are
    copied.  Returns (sel int32 [F][G], tick TICK [F][G], state STATE [G], slots SLOT [n_members])."""
    rf = release_frames or RELEASE_FRAMES
    F_ = info.shape[0]
    G_, nm = n_groups, n_members
    mem = np.asarray(members, np.int64)[:nm]
    st = np.ascontiguousarray(state).view(np.uint8).reshape(-1)[:16 * G_].copy().view(STATE)
    sl = np.ascontiguousarray(slots).view(np.uint8).reshape(-1)[:8 * nm].copy().view(SLOT)
    rng = np.array(bm.groups_of(group_ptr, nm, G_), np.int64).reshape(G_, 2)
    gb, gm = rng[:, 0], rng[:, 1] - rng[:, 0]
    live = mem < n_channels
    cc = np.where(live, mem, 0)
    rx = np.zeros(nm, bool) if rxonly is None else (np.asarray(rxonly)[cc] != 0)
    w = sl["word"].astype(np.int64)
    last_tx, cnt, pressed = (sl[k].astype(np.int64) for k in ("last_tx", "release_cnt", "pressed"))
    level = (st["level"] & 7).astype(np.int64)
    holder = np.where(st["holder"] <= gm, st["holder"], 0).astype(np.int64)
    takeovers = st["takeovers"].astype(np.int64)
    sel = np.full((F_, G_), -1, np.int32)
    tick = np.zeros((F_, G_), TICK)
    mmax = int(gm.max(initial=0))
    for f in range(F_):
        # per slot: steps 1-4 and the slot's half of step 6
        if nm:
            rec = info[f, cc]
            sto = live & ((rec["flags"].astype(np.int64) & bm.RTP_RUNT) == 0) & np.isin(rec["pt"], bm.STORE_PTS)
            w = np.where(sto, rec["ed137"].astype(np.int64), w)
        p = np.where(rx, 0, (w >> 29) & 7)
        ne = p != last_tx
        rel = live & ne & (p == 0)
        cnt = np.where(rel, np.minimum(cnt + 1, 255), np.where(live & ~ne, 0, cnt))
        p = np.where(rel & (cnt < rf), 1, p)
        p = np.where(live, p, 0)
        last_tx = np.where(live, p, last_tx)
        press = live & (p > 0) & (pressed == 0)
        release = live & (p == 0) & (pressed != 0)
        pressed = np.where(press, 1, np.where(release, 0, pressed))
        # per group, a member position at a time: steps 5 and 6
        flags = np.zeros(G_, np.int64)
        for pos in range(mmax):
            act = pos < gm
            k = np.where(act, gb + pos, 0)
            pp = np.where(act, p[k], 0) if nm else np.zeros(G_, np.int64)
            tk = pp > level
            level = np.where(tk, pp, level)
            holder = np.where(tk, pos + 1, holder)
            takeovers = np.where(tk, (takeovers + 1) & bm.U32, takeovers)
            rl = act & release[k] if nm else np.zeros(G_, bool)
            holder = np.where(rl & (holder == pos + 1), 0, holder)
            level = np.where(rl, 0, level)
            flags |= np.where(tk, TAKEOVER, 0) | np.where(pp > 0, ON, 0) | np.where(act & press[k], PRESS, 0) | np.where(rl, RELEASE, 0)
        hk = np.where(holder > 0, gb + holder - 1, 0)
        hc = mem[hk] if nm else np.zeros(G_, np.int64)
        sel[f] = np.where((holder > 0) & (hc < n_channels), hc, -1)
        tick["sel"][f] = sel[f]
        tick["level"][f] = level
        tick["ptt_id"][f] = np.where(holder > 0, (w[hk] >> 22) & 0x3F, 0) if nm else 0
        tick["flags"][f] = flags
        tick["ctl"][f] = CTL_SET | np.where(flags & ON, CTL_PTT, 0)
    st["level"], st["holder"], st["takeovers"] = level, holder, takeovers
    sl["word"], sl["last_tx"], sl["release_cnt"], sl["pressed"] = w, last_tx, cnt, pressed
    return sel, tick, st, sl
