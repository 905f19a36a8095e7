// igdsp_k_jb_body.h — the four phases of the jitter-buffer kernels (igdsp_k_jb.hip), included as the body of k_jb_receive<COPY> and of
// k_jb_adaptive.  In scope at the point of inclusion: `a` (JbArgs), `COPY` and `ADAPT` (constant bools) and, where ADAPT, `x`
// (JbAdaptArgs).  One text for both, included and not a __device__ function: as a function inlined into the kernels the same statements
// compile to a different schedule for k_jb_receive<COPY>, whose ISA igdsp_jb_receive_adaptive must leave as it is.
    __shared__ uint32_t desc[kJbWaves][kJbPart][kJbCh];
    __shared__ uint32_t rtag[kJbWaves][kJbCh][IGDSP_JB_DEPTH];
    __shared__ uint16_t rsrc[kJbWaves][kJbCh][IGDSP_JB_DEPTH];
    __shared__ uint32_t todo[kJbWaves][kJbCh * IGDSP_JB_DEPTH];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t c0l = ((uint64_t)blockIdx.x * kJbWaves + w) * kJbCh;
    if (c0l >= a.C) return;                                                // waves are independent: no block barrier below
    const uint32_t c0 = (uint32_t)c0l, nch = min(kJbCh, a.C - c0), pt = a.pt, ntag = nch * IGDSP_JB_DEPTH;
    uint32_t *tags = reinterpret_cast<uint32_t *>(a.ring) + (uint64_t)c0 * IGDSP_JB_DEPTH;   // the wave's tags: contiguous
    uint32_t *rt = &rtag[w][0][0];
    uint16_t *rs = &rsrc[w][0][0];
    for (uint32_t i = lane; i < ntag; i += 64u) { rt[i] = tags[i]; rs[i] = kJbOld; }
    wave_lds_fence();

    // A. decide
    if (lane < nch) {
        const uint32_t c = c0 + lane;
        const bool radio = a.radio[c] != 0u;
        if (COPY) {
            for (uint32_t t = 0; t < pt; ++t) desc[w][t][lane] = jb_desc(kJdArr, t * a.S, IGDSP_JB_PLAYED) | (radio ? 1u << 14 : 0u);
        } else {
            JbLane L;
            JbAdaptLane ad;
            if (ADAPT) {
                const uint32_t *aw = reinterpret_cast<const uint32_t *>(x.adapt + c);
                const uint32_t v[2] = {aw[0], aw[1]};      // d_adapt is 4-byte aligned: two dwords, not byte and short loads
                __builtin_memcpy(&ad.a, v, 8);
                ad.cfg = x.cfg;
                ad.n = a.n;
            }
            L.s = a.state[c];
            L.tag = rt + lane * IGDSP_JB_DEPTH;
            L.src = rs + lane * IGDSP_JB_DEPTH;
            const uint32_t hdr = radio ? 20u : 12u, na = pt * a.S;
            uint32_t ka = kJbOld, k = 0, t = 0;
            for (uint32_t a0 = 0; a0 < na; a0 += kJbU) {
                uint32_t sz[kJbU], w0[kJbU], w1[kJbU], w2[kJbU], ar[kJbU];
#pragma unroll
                for (uint32_t u = 0; u < kJbU; ++u) {                      // the headers of kJbU arrivals in flight
                    const uint32_t al = min(a0 + u, na - 1u);
                    const uint32_t *p = reinterpret_cast<const uint32_t *>(jb_pkt(a, al, c));
                    sz[u] = jb_size(a, al, c);
                    w0[u] = p[0]; w1[u] = p[1]; w2[u] = p[2];
                    ar[u] = a.arrival ? a.arrival[(uint64_t)(a.t0 * a.S + al) * a.C + c] : 0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < kJbU; ++u) {
                    const uint32_t al = a0 + u;
                    if (al >= na) break;
                    uint32_t st = IGDSP_JB_PKT_NONE;
                    if (sz[u] != 0u) {
                        if (sz[u] < hdr) { ++L.s.invalid; st = IGDSP_JB_PKT_INVALID; }
                        else st = L.template packet<ADAPT>(al, w0[u], w1[u], w2[u], ar[u], a.arrival != nullptr, a.delay, &ka, &ad);
                    }
                    if (a.pkt) a.pkt[(uint64_t)(a.t0 * a.S + al) * a.C + c] = (uint8_t)st;
                    if (++k == a.S) {                                      // the tick's last arrival: playout
                        desc[w][t][lane] = L.tick(ka) | (radio ? 1u << 14 : 0u) | (ADAPT ? (uint32_t)ad.a.delay << 28 : 0u);
                        k = 0; ++t; ka = kJbOld;
                    }
                }
            }
            a.state[c] = L.s;
            if (ADAPT) {
                uint32_t v[2];
                __builtin_memcpy(v, &ad.a, 8);
                uint32_t *aw = reinterpret_cast<uint32_t *>(x.adapt + c);
                aw[0] = v[0]; aw[1] = v[1];
            }
        }
    }
    wave_lds_fence();

    // B. records
    const uint32_t items = pt * nch;
    for (uint32_t j = lane; j < items; j += 64u) {
        const uint32_t t = j / nch, ch = j - t * nch, c = c0 + ch;
        const uint32_t d = desc[w][t][ch], kind = d & 3u, idx = (d >> 2) & 0x3FFu, flag = (d >> 12) & 3u;
        uint2 inf = make_uint2(0u, (uint32_t)IGDSP_RTP_RUNT << 24);
        uint32_t l = 0;
        if (kind == kJdRing) {
            const uint4 h = *reinterpret_cast<const uint4 *>(jb_slot(a, c, idx));
            inf = make_uint2(h.x, h.y); l = h.z;
        } else if (kind != kJdNone) {
            const FrameHdr h = jb_parse(a, idx, c, (d >> 14) & 1u);
            inf = make_uint2(h.info.ed137, (uint32_t)h.info.payload_len | (uint32_t)h.info.pt << 16 | (uint32_t)h.info.flags << 24);
            l = kind == kJdArr ? h.len : 0u;
        }
        const uint64_t o = (uint64_t)(a.t0 + t) * a.C + c;
        a.len[o] = (uint16_t)l;
        *reinterpret_cast<uint2 *>(a.info + o) = inf;
        if (a.tick) a.tick[o] = (uint8_t)flag;
        if (ADAPT && x.delay_out) x.delay_out[o] = (uint8_t)(d >> 28);
        desc[w][t][ch] = d | l << 16;
    }
    wave_lds_fence();

    // C. rows: piece q of frame (t, ch), kJbU pieces of a lane in flight
    const uint32_t P = a.pieces, n = a.n, total = items * P;
    for (uint32_t j0 = 0; j0 < total; j0 += 64u * kJbU) {
        uint4 v[kJbU];
        uint64_t dst[kJbU];
        uint32_t b0s[kJbU];
#pragma unroll
        for (uint32_t u = 0; u < kJbU; ++u) {
            const uint32_t j = j0 + u * 64u + lane;
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            dst[u] = ~0ull;
            if (j < total) {
                const uint32_t row = j / P, q = j - row * P, t = row / nch, ch = row - t * nch, c = c0 + ch;
                const uint32_t d = desc[w][t][ch], kind = d & 3u, idx = (d >> 2) & 0x3FFu, l = ADAPT ? (d >> 16) & 0xFFFu : d >> 16;
                if (kind == kJdArr) v[u] = jb_piece(a, idx, c, (d >> 14) & 1u ? 20u : 12u, l, 16u * q);
                else if (kind == kJdRing) v[u] = *reinterpret_cast<const uint4 *>(jb_slot(a, c, idx) + kJbSlotHead + 16u * q);
                dst[u] = ((uint64_t)(a.t0 + t) * a.C + c) * n;
                b0s[u] = 16u * q;
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kJbU; ++u) {
            if (dst[u] == ~0ull) continue;
            uint8_t *o = a.payload + dst[u] + b0s[u];
            if (a.vec) {
                *reinterpret_cast<uint4 *>(o) = v[u];
            } else {
                const uint32_t x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                for (uint32_t b = 0; b < 16u && b0s[u] + b < n; ++b) o[b] = (uint8_t)(x[b >> 2] >> (8u * (b & 3u)));
            }
        }
    }

    // D. ring: this part's unplayed packets into their slots, then the tags
    if (!COPY) {
        uint32_t cnt = 0;
        for (uint32_t i0 = 0; i0 < ntag; i0 += 64u) {
            const uint32_t i = i0 + lane;
            const bool st = i < ntag && rt[i] != 0u && rs[i] != kJbOld;
            const uint64_t m = __builtin_amdgcn_ballot_w64(st);
            if (st) todo[w][cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = i | (uint32_t)rs[i] << 16;
            cnt += (uint32_t)__builtin_popcountll(m);
        }
        wave_lds_fence();
        const uint32_t per = P + 1u;                                       // the record head, then P payload pieces
        for (uint32_t j = lane; j < cnt * per; j += 64u) {
            const uint32_t e = j / per, q = j - e * per, ent = todo[w][e];
            const uint32_t ch = (ent & 0xFFFFu) / IGDSP_JB_DEPTH, s = ent & (IGDSP_JB_DEPTH - 1u), al = ent >> 16, c = c0 + ch;
            const bool radio = a.radio[c] != 0u;
            const FrameHdr h = jb_parse(a, al, c, radio);
            uint8_t *slot = jb_slot(a, c, s);
            if (q == 0u)
                *reinterpret_cast<uint4 *>(slot) = make_uint4(h.info.ed137, (uint32_t)h.info.payload_len | (uint32_t)h.info.pt << 16 |
                                                                                (uint32_t)h.info.flags << 24, h.len, 0u);
            else
                *reinterpret_cast<uint4 *>(slot + kJbSlotHead + 16u * (q - 1u)) = jb_piece(a, al, c, radio ? 20u : 12u, h.len, 16u * (q - 1u));
        }
        for (uint32_t i = lane; i < ntag; i += 64u) tags[i] = rt[i];
    }
