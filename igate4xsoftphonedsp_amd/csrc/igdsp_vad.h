// igdsp_vad.h — the voice detector's rule (include/igdsp.h, "Voice activity"; independent restatement: tests/vad_model.py) in plain
// C++17, so that the host entry igdsp_vad_frame and the kernel k_vad run the same code: how a state is read, the decision, the floor
// and the hangover of a frame, the noise model's step of one lag, the DTX step, the level, the reflection coefficients and their
// bytes.  What the two sides do differently is only who walks: the host sums the eleven lags in loops, the kernel gives a lane a lag;
// the host finds a level by bisection, the kernel's sixteen lanes count the table's entries above it (igdsp_k_vad.hip: the same value,
// because the table never rises).  Every step is an exact integer operation, "/" is C division toward zero on both sides.
// The rule is the library's own; the payload's scale and sign are RFC 3389 section 3.2 as recalled.
// UNVERIFIED against RFC 3389 and G.711 Appendix II.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "igdsp.h"
#include "igdsp_vad_tab.h"

#if defined(__HIPCC__)
#define IGDSP_VAD_HD __host__ __device__ inline __attribute__((always_inline))   // (no HIP header need come first)
#define IGDSP_VAD_LOOP _Pragma("unroll 1")                                        // the rare path stays a loop on the device
#else
#define IGDSP_VAD_HD inline
#define IGDSP_VAD_LOOP
#endif

namespace igdsp {

static_assert(sizeof(igdsp_vad_cfg) == 32 && sizeof(igdsp_vad_state) == 128 && sizeof(igdsp_vad_rec) == 16 && sizeof(igdsp_vad_event) == 16,
              "capi.VAD_CFG, VAD_STATE, VAD_REC, VAD_EVENT");
static_assert(offsetof(igdsp_vad_state, A) == 8 && offsetof(igdsp_vad_state, since_sid) == 96 && offsetof(igdsp_vad_state, hang) == 100 &&
              offsetof(igdsp_vad_state, sid_sent) == 104 && offsetof(igdsp_vad_rec, run) == 8 && offsetof(igdsp_vad_rec, level) == 12 &&
              offsetof(igdsp_vad_event, ms) == 8 && offsetof(igdsp_vad_event, run) == 12, "the state goes as dwords, record and event as one 16-byte store");
static_assert(IGDSP_VAD_ORDER == 10 && IGDSP_VAD_KMAX == 126 * 258 && IGDSP_VAD_EVENT_DEFAULT == (IGDSP_VAD_F_ONSET | IGDSP_VAD_F_OFFSET), "the payload's scale");

constexpr uint32_t kVadLags = IGDSP_VAD_ORDER + 1;
constexpr int64_t kVadAMax = 1ll << 40;
constexpr uint64_t kVadT8[128] = {IGDSP_VAD_T8_VALUES};
// |v| <= 8192: eight products stay below 2^31 (the kernel's 32-bit partial sums), a row of 256 below 2^34 (r[0], the table's scale)
static_assert(8ll * 8192 * 8192 < (1ll << 31) && 256ll * 8192 * 8192 <= (1ll << 34) && kVadT8[0] == (1ull << 34) && kVadT8[127] == 0, "the sums' widths");

constexpr bool vad_n_ok(uint32_t n) { return n >= 16u && n <= IGDSP_MAX_PAYLOAD && (n & 7u) == 0u; }
constexpr igdsp_vad_cfg vad_cfg_default()
{
    return igdsp_vad_cfg{212, 8, 1u << 20, 0, 80, 40, 2, 5, 7, 2, 5, 10, 2, 10, 1, 2, 2, 0x81, 0x80, {0, 0, 0}};
}
constexpr bool vad_cfg_ok(const igdsp_vad_cfg *c)
{
    return !c || (c->nf_min >= 1u && c->nf_min <= c->nf_max && c->nf_max <= (1u << 24) && c->ratio_off_q4 >= 16u && c->ratio_off_q4 <= c->ratio_on_q4 &&
                  c->dn <= 15u && c->up <= 15u && c->up_v <= 15u && c->asm_shift <= 15u && c->order <= IGDSP_VAD_ORDER && c->hang_short <= c->hang_long);
}
constexpr igdsp_vad_cfg vad_cfg_or_default(const igdsp_vad_cfg *c) { return c ? *c : vad_cfg_default(); }
constexpr uint32_t vad_ctl(uint32_t v) { return v <= 3u ? v : (uint32_t)IGDSP_VAD_RUN; }

// the rule's numbers as the kernel carries them: 32-bit copies of the cfg
struct VadK {
    uint32_t thr_abs, nf_min, nf_max, sid_every, ratio_on, ratio_off, dn, up, up_v, asm_shift, burst, hang_long, hang_short, order, dtx, sid_delta,
        sid_gap, vox_on, vox_off;
};
constexpr VadK vad_k(const igdsp_vad_cfg &c)
{
    return VadK{c.thr_abs, c.nf_min, c.nf_max, c.sid_every, c.ratio_on_q4, c.ratio_off_q4, c.dn, c.up, c.up_v, c.asm_shift, c.burst, c.hang_long,
                c.hang_short, c.order, c.dtx, c.sid_delta, c.sid_gap, c.vox_on, c.vox_off};
}

// what runs through a channel's frames beside A[]
struct VadRun { uint32_t nf, since_sid, run, hang, voice, avalid, last_level, sid_sent; };
IGDSP_VAD_HD uint32_t vad_clamp(uint32_t v, uint32_t lo, uint32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
// a state as it is READ, from its dwords 0, 1, 24, 25, 26: another tag (or RESET) is the reset state; under the tag nf is clamped (0
// stays unset) and every other value stands
IGDSP_VAD_HD bool vad_is_reset(uint32_t tag, bool reset) { return reset || tag != (uint32_t)IGDSP_VAD_TAG; }
IGDSP_VAD_HD VadRun vad_read(uint32_t tag, uint32_t nf, uint32_t w24, uint32_t w25, uint32_t w26, bool reset, const VadK &k)
{
    if (vad_is_reset(tag, reset)) return VadRun{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    return VadRun{nf ? vad_clamp(nf, k.nf_min, k.nf_max) : 0u, w24 & 0xFFFFu, w24 >> 16, w25 & 0xFFu, (w25 >> 8) & 1u, (w25 >> 16) & 1u, w25 >> 24, w26 & 1u};
}
IGDSP_VAD_HD int64_t vad_read_a(int64_t a, bool is_reset) { return is_reset ? 0 : (a < -kVadAMax ? -kVadAMax : (a > kVadAMax ? kVadAMax : a)); }
IGDSP_VAD_HD uint32_t vad_w24(const VadRun &r) { return r.since_sid | r.run << 16; }
IGDSP_VAD_HD uint32_t vad_w25(const VadRun &r) { return r.hang | r.voice << 8 | r.avalid << 16 | r.last_level << 24; }
IGDSP_VAD_HD uint32_t vad_w26(const VadRun &r, uint32_t flags) { return r.sid_sent | flags << 8; }

// E / n for n a multiple of 8 and E < 2^34: one 32-bit division
IGDSP_VAD_HD uint32_t vad_ms(uint64_t E, uint32_t n) { return (uint32_t)(E >> 3) / (n >> 3); }

// steps 2, 3 and 4 of a frame: the flags RAW, VOICE, ONSET, OFFSET, QUIET, FROZEN; r.nf, run, hang, voice move
IGDSP_VAD_HD uint32_t vad_decide(VadRun &r, uint32_t ms, bool frozen, const VadK &k)
{
    if (r.nf == 0u) r.nf = vad_clamp(ms, k.nf_min, k.nf_max);
    const uint32_t ratio = r.voice ? k.ratio_off : k.ratio_on;
    const bool raw = ms >= k.thr_abs && (uint64_t)ms * 16u > (uint64_t)r.nf * ratio;
    const bool quiet = ms < k.nf_min;
    uint32_t flags = (raw ? (uint32_t)IGDSP_VAD_F_RAW : 0u) | (quiet ? (uint32_t)IGDSP_VAD_F_QUIET : 0u) | (frozen ? (uint32_t)IGDSP_VAD_F_FROZEN : 0u);
    if (!frozen && !quiet) {
        if (ms <= r.nf) {
            r.nf -= (r.nf - ms) >> k.dn;
        } else {
            const uint32_t s = r.nf >> (raw ? k.up_v : k.up), up = r.nf + (s > 1u ? s : 1u);
            r.nf = ms < up ? ms : up;
        }
        r.nf = vad_clamp(r.nf, k.nf_min, k.nf_max);
    }
    const uint32_t was = r.voice;
    if (raw) {
        r.run = r.run < 65535u ? r.run + 1u : 65535u;
        r.hang = r.run >= k.burst ? k.hang_long : (r.hang > k.hang_short ? r.hang : k.hang_short);
        r.voice = 1u;
    } else {
        r.run = 0u;
        if (r.hang > 0u) r.hang -= 1u;
        else r.voice = 0u;
    }
    if (r.voice) flags |= IGDSP_VAD_F_VOICE;
    if (r.voice && !was) flags |= IGDSP_VAD_F_ONSET;
    if (!r.voice && was) flags |= IGDSP_VAD_F_OFFSET;
    return flags;
}
// step 5 for one lag (the caller sets avalid afterwards)
IGDSP_VAD_HD int64_t vad_model(int64_t A, int64_t r, uint32_t avalid, uint32_t sh) { return avalid ? A + ((r - A) >> sh) : r; }

// level(e) over tab(d) = n * T8[d], d = 0..126: a bisection of seven steps (T8 never rises)
template <class Tab>
IGDSP_VAD_HD uint32_t vad_level(int64_t e, Tab tab)
{
    if (e <= 0) return 127u;
    const uint64_t lhs = (uint64_t)e << 8;                                 // e <= 2^40
    uint32_t lo = 0u, hi = 127u;
    IGDSP_VAD_LOOP
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;                               // <= 126
        if (lhs >= tab(mid)) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}
struct VadHostTab {
    uint32_t n;
    uint64_t operator()(uint32_t d) const { return kVadT8[d] * n; }
};

// step 6 of a frame that is not bypassed: the kind; since_sid, last_level, sid_sent move.  lvl is read on a non-VOICE frame with dtx only
IGDSP_VAD_HD uint32_t vad_dtx(VadRun &r, uint32_t flags, uint32_t lvl, const VadK &k)
{
    if (!k.dtx || (flags & IGDSP_VAD_F_VOICE)) return IGDSP_VAD_VOICE;
    const uint32_t d = lvl > r.last_level ? lvl - r.last_level : r.last_level - lvl;
    const bool due = (flags & IGDSP_VAD_F_OFFSET) || !r.sid_sent || (k.sid_every > 0u && r.since_sid >= k.sid_every) ||
                     (d >= k.sid_delta && r.since_sid >= k.sid_gap);
    if (due) {
        r.since_sid = 0u; r.last_level = lvl; r.sid_sent = 1u;
        return IGDSP_VAD_SID;
    }
    r.since_sid = r.since_sid < 65535u ? r.since_sid + 1u : 65535u;
    return IGDSP_VAD_NONE;
}

// N of a coefficient, |k| <= 32766; and back
IGDSP_VAD_HD uint32_t vad_quant(int32_t kq)
{
    const int32_t m = ((kq < 0 ? -kq : kq) + 129) / 258;
    return (uint32_t)(127 + (kq < 0 ? -m : m));
}
IGDSP_VAD_HD int32_t vad_dequant(uint32_t N) { return 258 * ((int32_t)(N > 254u ? 254u : N) - 127); }
IGDSP_VAD_HD uint32_t vad_bitlen(uint64_t v)
{
    uint32_t b = 0u;
    for (uint32_t s = 32u; s; s >>= 1) if (v >> s) { v >>= s; b += s; }
    return b + (v ? 1u : 0u);
}
IGDSP_VAD_HD int64_t vad_shift(int64_t v, int32_t sh) { return sh >= 0 ? v >> sh : (int64_t)((uint64_t)v << -sh); }

// clamp(num / err, -KMAX, KMAX), "/" toward zero, for 1 <= err < 2^31 and |num| < 2^62, without a 64-bit division (the kernel would run
// it in software): a quotient past the clamp is settled by one product; a smaller one, below 2^15 with |num| < 2^46, comes from a
// double division of two exactly represented numbers, which is within one of it, and one step either way makes it exact
IGDSP_VAD_HD int64_t vad_kdiv(int64_t num, int64_t err)
{
    const bool neg = num < 0;
    const uint64_t m = neg ? (uint64_t)-num : (uint64_t)num, e = (uint64_t)err;
    if (m >= (uint64_t)(IGDSP_VAD_KMAX + 1) * e) return neg ? -(int64_t)IGDSP_VAD_KMAX : (int64_t)IGDSP_VAD_KMAX;
    uint64_t q = (uint64_t)((double)m / (double)e);
    if (q * e > m) --q;
    else if ((q + 1u) * e <= m) ++q;
    return neg ? -(int64_t)q : (int64_t)q;
}

// step 7: the payload of 1 + order bytes into sid[16] (zeros behind it), from A[11]; R[11] and a[11] are the caller's work arrays (the
// kernel's lie in LDS: nothing here indexes a register array).  Returns the payload's length
IGDSP_VAD_HD uint32_t vad_sid(const int64_t *A, uint32_t lvl, uint32_t order, int64_t *R, int64_t *a, uint8_t *sid)
{
    for (uint32_t i = 0; i < 16u; ++i) sid[i] = i >= 1u && i <= order ? 127u : 0u;          // k = 0
    sid[0] = (uint8_t)lvl;
    const int64_t A0 = A[0];
    if (A0 <= 0 || order == 0u) return 1u + order;
    const int64_t R0 = A0 + (A0 >> 10) + 1;
    const int32_t sh = (int32_t)vad_bitlen((uint64_t)R0) - 30;
    R[0] = vad_shift(R0, sh);                                              // 2^29 <= R[0] < 2^30
    for (uint32_t i = 1; i <= order; ++i) {
        const int64_t v = A[i] < -A0 ? -A0 : (A[i] > A0 ? A0 : A[i]);      // |r[k]| <= r[0] holds for a sum of products; garbage is held to it
        R[i] = vad_shift(v, sh);
    }
    int64_t err = R[0];
    IGDSP_VAD_LOOP
    for (uint32_t i = 1; i <= order; ++i) {
        int64_t acc = (int64_t)((uint64_t)R[i] << 15);
    IGDSP_VAD_LOOP
        for (uint32_t j = 1; j < i; ++j) acc += a[j] * R[i - j];           // |a[j]| <= C(10, j) 2^15 < 2^23, |R| < 2^30, nine terms
        const int64_t kq = vad_kdiv(-acc, err);
    IGDSP_VAD_LOOP
        for (uint32_t j = 1; 2u * j <= i - 1u; ++j) {                      // a'[j] and a'[i - j] from the old pair
            const int64_t p = a[j], q = a[i - j];
            a[j] = p + ((kq * q + 16384) >> 15);
            a[i - j] = q + ((kq * p + 16384) >> 15);
        }
        if ((i & 1u) == 0u) { const int64_t p = a[i >> 1]; a[i >> 1] = p + ((kq * p + 16384) >> 15); }
        a[i] = kq;
        sid[i] = (uint8_t)vad_quant((int32_t)kq);
        err -= (((kq * kq) >> 15) * err) >> 15;
        if (err <= 0) break;
    }
    return 1u + order;
}

IGDSP_VAD_HD void vad_pack_rec(uint32_t ms, uint32_t nf, uint32_t run, uint32_t flags, uint32_t kind, uint32_t level, uint32_t hang, uint32_t sid_len,
                               uint32_t (&w)[4])
{
    w[0] = ms; w[1] = nf; w[2] = run | flags << 16 | kind << 24; w[3] = level | hang << 8 | sid_len << 16;
}

// ---- the host: one frame of one channel.  cfg, n checked by the caller; rec, sid may be nullptr.  Returns the kind
inline uint32_t vad_frame_run(const igdsp_vad_cfg &cfg, igdsp_vad_state &st, const int16_t *x, uint32_t n, uint32_t ctl_in, igdsp_vad_rec *rec, uint8_t *sid)
{
    const VadK k = vad_k(cfg);
    const uint32_t ctl = vad_ctl(ctl_in);
    uint32_t sw[32];
    std::memcpy(sw, &st, sizeof st);
    const bool is_reset = vad_is_reset(sw[0], ctl == IGDSP_VAD_RESET);
    VadRun r = vad_read(sw[0], sw[1], sw[24], sw[25], sw[26], ctl == IGDSP_VAD_RESET, k);
    int64_t A[kVadLags], rr[kVadLags];
    for (uint32_t i = 0; i < kVadLags; ++i) A[i] = vad_read_a(st.A[i], is_reset);
    for (uint32_t lag = 0; lag < kVadLags; ++lag) {
        int64_t s = 0;
        for (uint32_t j = lag; j < n; ++j) s += (int64_t)(x[j] >> 2) * (x[j - lag] >> 2);
        rr[lag] = s;
    }
    const uint32_t ms = vad_ms((uint64_t)rr[0], n), lvl_e = vad_level(rr[0], VadHostTab{n});
    uint8_t pay[16] = {0};
    uint32_t w[4], kind = IGDSP_VAD_VOICE, sid_len = 0u, flags = IGDSP_VAD_F_BYPASSED;
    if (ctl != IGDSP_VAD_BYPASS) {
        const bool frozen = ctl == IGDSP_VAD_FREEZE;
        flags = vad_decide(r, ms, frozen, k);
        if (!frozen && !(flags & IGDSP_VAD_F_RAW)) {
            for (uint32_t i = 0; i < kVadLags; ++i) A[i] = vad_model(A[i], rr[i], r.avalid, k.asm_shift);
            r.avalid = 1u;
        }
        const uint32_t lvl = (k.dtx && !(flags & IGDSP_VAD_F_VOICE)) ? vad_level(A[0], VadHostTab{n}) : 0u;
        kind = vad_dtx(r, flags, lvl, k);
        if (kind == IGDSP_VAD_SID) {
            int64_t R[kVadLags] = {0}, a[kVadLags] = {0};
            flags |= IGDSP_VAD_F_SID;
            sid_len = vad_sid(A, lvl, k.order, R, a, pay);
        }
        igdsp_vad_state o;
        std::memset(&o, 0, sizeof o);
        o.tag = IGDSP_VAD_TAG; o.nf = r.nf;
        for (uint32_t i = 0; i < kVadLags; ++i) o.A[i] = A[i];
        o.since_sid = (uint16_t)r.since_sid; o.run = (uint16_t)r.run; o.hang = (uint8_t)r.hang; o.voice = (uint8_t)r.voice; o.avalid = (uint8_t)r.avalid;
        o.last_level = (uint8_t)r.last_level; o.sid_sent = (uint8_t)r.sid_sent; o.flags = (uint8_t)flags;
        st = o;
    }
    vad_pack_rec(ms, r.nf, r.run, flags, kind, lvl_e, r.hang, sid_len, w);
    if (rec) std::memcpy(rec, w, 16);
    if (sid) std::memcpy(sid, pay, 16);
    return kind;
}

}  // namespace igdsp
