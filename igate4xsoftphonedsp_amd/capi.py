"""ctypes binding of ``include/igdsp.h`` (``libigdsp.so``).

This is plumbing: it declares the C prototypes and turns negative return codes
into ``IgdspError``.  Device buffers are passed as raw integer addresses
(``tensor.data_ptr()``), streams as ``torch.cuda.current_stream().cuda_stream``.
There is no fallback: if the HIP extension is missing or no gfx950 device is
present, importing works but every use raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libigdsp.so")

ABI_VERSION = 3
PT_PCMU, PT_PCMA, PT_R2S = 0, 8, 123
SAMPLES_PER_FRAME = 160
MAX_PAYLOAD = 256
STAGE_DEPTH = 8
ENC_SUN16, ENC_G191 = 0, 1
FLAG_SILENT, FLAG_PROBE_D5, FLAG_CLIPPED, FLAG_EMPTY = 1, 2, 4, 8
FLAG_SATURATED = 0x10        # igdsp_conf_mix
BSS_VOTE_FRAMES = 10         # IGDSP_BSS_VOTE_FRAMES
PTT_RELEASE_FRAMES = 12      # IGDSP_PTT_RELEASE_FRAMES
PTT_ON, PTT_PRESS, PTT_RELEASE, PTT_TAKEOVER = 1, 2, 4, 8   # IGDSP_PTT_*
# R2S link supervision (igdsp_link_watch): IGDSP_LINK_*
LINK_R2S_PERIOD_MS, LINK_MISS_TICKS = 200, 12
LINK_AUDIO_ON, LINK_AUDIO_OFF, LINK_MISSING, LINK_LATE, LINK_RECOVERED, LINK_CAME_UP = 1, 2, 4, 8, 0x10, 0x20   # kind bits
LINK_EVENT_DEFAULT = 0x37
LINK_UP, LINK_AUDIO, LINK_ALARMED = 1, 2, 4                  # state flags
JB_DEPTH, JB_DELAY = 16, 3   # IGDSP_JB_DEPTH, IGDSP_JB_DELAY
JB_IDLE, JB_PLAYED, JB_LOST = 1, 2, 3
JB_PKT_NONE, JB_PKT_INVALID, JB_PKT_KEEPALIVE, JB_PKT_PLACED, JB_PKT_LATE, JB_PKT_DUPLICATE, JB_PKT_RESTART = 0, 1, 2, 3, 4, 5, 6
JB_HEARD, JB_PLAYING, JB_TRANSIT = 1, 2, 4
JB_ADAPT_MIN, JB_ADAPT_MAX, JB_ADAPT_MULT, JB_ADAPT_LATE_RESTART, JB_ADAPT_SET = 1, 12, 4, 3, 1   # IGDSP_JB_ADAPT_*
PLC_PMIN, PLC_PMAX, PLC_SPAN, PLC_HIST, PLC_FLAT, PLC_STEP = 40, 120, 160, 280, 80, 82   # IGDSP_PLC_*
FLAG_CONCEALED = 0x20        # igdsp_plc_conceal
AGG_MAX_RANKS = 8
AGG_LINE_WORDS = 16
AGG_WORDS = 7 * AGG_LINE_WORDS

ERRORS = {
    0: "IGDSP_OK", -22: "IGDSP_EINVAL", -12: "IGDSP_ENOMEM", -19: "IGDSP_ENODEV", -2: "IGDSP_ENOENT",
    -34: "IGDSP_ERANGE", -16: "IGDSP_EBUSY", -5: "IGDSP_EDEVICE",
}

# numpy views of the ABI structs (layout asserted against the C side in tests)
FRAME_STATS = np.dtype(
    [("sumsq", "<u8"), ("rms", "<f4"), ("peak", "<u2"), ("byte_mean", "u1"), ("flags", "u1")], align=True
)
CHAN_HOLD = np.dtype(
    [("sumsq_acc", "<u8"), ("count", "<u4"), ("level_sum", "<u4"), ("samples", "<u4"), ("peak_hold", "<u2"),
     ("level_max", "u1"), ("level_min", "u1"), ("n_silent", "<u4"), ("n_clipped", "<u4")],
    align=True,
)
RTP_INFO = np.dtype([("ed137", "<u4"), ("payload_len", "<u2"), ("pt", "u1"), ("flags", "u1")], align=True)
BSS_STATE = np.dtype([("count", "<u4"), ("voted", "<u4"), ("on", "<u4"), ("votes", "<u4")], align=True)   # igdsp_bss_state
# PTT priority arbitration (igdsp_ptt_arbitrate)
PTT_STATE = np.dtype([("level", "<u4"), ("holder", "<u4"), ("takeovers", "<u4"), ("reserved", "<u4")], align=True)   # igdsp_ptt_state
PTT_SLOT = np.dtype([("word", "<u4"), ("last_tx", "u1"), ("release_cnt", "u1"), ("pressed", "u1"), ("reserved", "u1")], align=True)
PTT_TICK = np.dtype([("sel", "<i4"), ("level", "u1"), ("ptt_id", "u1"), ("flags", "u1"), ("ctl", "u1")], align=True)
# R2S link supervision (igdsp_link_watch)
LINK_STATE = np.dtype([("last_ms", "<u8"), ("alarms", "<u4"), ("count", "<u2"), ("flags", "u1"), ("reserved", "u1")], align=True)   # igdsp_link_state
LINK_EVENT = np.dtype([("channel", "<u4"), ("tick", "<u4"), ("word", "<u4"), ("count", "<u2"), ("kind", "u1"), ("reserved", "u1")], align=True)
# sound-card splitter / combiner (igdsp_snd_combine / igdsp_snd_split / igdsp_snd_vu)
SND_MAX_CHANNELS = 8
SND_DB_FLOOR = -100.0
SND_VU = np.dtype([("percent", "<i4"), ("reserved", "<u4"), ("db", "<f8")], align=True)   # igdsp_snd_vu_t
# the tone generator (igdsp_tone_plan_build / igdsp_tone_frame / igdsp_tone_generate)
TONE_MAX = 8
TONE_VOLUME = 12288
TONE_LOOP, TONE_NO_FADE = 1, 2
TONE_PLAYING = 1
TONE_CMD_REWIND, TONE_CMD_STOP, TONE_CMD_HOLD = 1, 2, 4
TONE_DESC = np.dtype([("freq1", "<u2"), ("freq2", "<u2"), ("on_msec", "<u2"), ("off_msec", "<u2"), ("volume", "<u2"), ("reserved", "<u2")], align=True)
TONE_SEG = np.dtype([("start", "<u4"), ("on", "<u4"), ("step1", "<u4"), ("step2", "<u4"), ("vol", "<u2"), ("fade_in", "<u2"), ("fade_out", "<u2"),
                     ("reserved", "<u2")], align=True)                                             # igdsp_tone_seg, 24 bytes
TONE_PLAN = np.dtype([("n_tones", "<u4"), ("options", "<u4"), ("cycle", "<u4"), ("clock_rate", "<u4"), ("seg", TONE_SEG, (TONE_MAX,))], align=True)   # 208 bytes
TONE_STATE = np.dtype([("pos", "<u4"), ("flags", "<u4")], align=True)                            # igdsp_tone_state
# the rate converter (igdsp_rs_taps / igdsp_rs_frame / igdsp_resample)
RS_UP, RS_DOWN = 0, 1
RS_ROWS, RS_SUBFRAMES = 0, 1
RS_TAPS, RS_HIST = 24, 144
RS_FACTORS = (2, 3, 4, 6)
RS_STATE = np.dtype([("hist", "<i2", (RS_HIST,)), ("flags", "<u4"), ("frames", "<u4")], align=True)   # igdsp_rs_state, 296 bytes
# the sound port's delay buffer (igdsp_dbuf_run / igdsp_dbuf_step)
DBUF_CAP, DBUF_WIN, DBUF_RECALC = 1024, 280, 200
DBUF_PUT, DBUF_GET = 1, 2
DBUF_STATE = np.dtype(
    [("ring", "<i2", (DBUF_CAP,)), ("head", "<u2"), ("len", "<u2"), ("eff", "<u2"), ("level", "<u2"), ("max_level", "<u2"), ("since", "<u2"),
     ("last_op", "<u2"), ("reserved0", "<u2"), ("underruns", "<u4"), ("shrinks", "<u4"), ("shrunk", "<u4"), ("dropped", "<u4"), ("puts", "<u4"),
     ("gets", "<u4"), ("reserved", "<u4", (6,))],
    align=True,
)                                                                                                # igdsp_dbuf_state, 2112 bytes
# the spectrum graph (igdsp_spectrum / igdsp_spec_frame)
SPEC_N, SPEC_BINS, SPEC_FLOOR_DB = 1024, 512, -70.0
SPEC_HOP, SPEC_LIVE = 1, 1
SPEC_STATE = np.dtype([("hist", "<i2", (SPEC_N,)), ("avg", "<f4", (SPEC_BINS,)), ("since", "<u4"), ("hops", "<u4"), ("flags", "<u4"),
                       ("reserved", "<u4")], align=True)                                          # igdsp_spec_state, 4112 bytes
SPEC_REC = np.dtype([("peak_bin", "<u2"), ("flags", "<u2"), ("peak_db", "<f4")], align=True)     # igdsp_spec_rec, 8 bytes
# the tone detector (igdsp_tone_detect / igdsp_tdet_frame)
TDET_MAX_FREQ, TDET_HIST = 16, 128
TDET_ON0, TDET_OFF0, TDET_ON1, TDET_OFF1, TDET_EVENT_DEFAULT = 1, 2, 4, 8, 15
TDET_THR = np.dtype([("min_amp", "<u2"), ("rel_q8", "<u2"), ("fwd_q8", "<u2"), ("rev_q8", "<u2"), ("frac_q8", "<u2"), ("min_on", "u1"),
                     ("min_off", "u1")], align=True)                                               # igdsp_tdet_thr, 12 bytes
TDET_PLAN = np.dtype([("clock_rate", "<u4"), ("n_lo", "u1"), ("n_hi", "u1"), ("reserved", "u1", (2,)), ("thr", TDET_THR),
                      ("step", "<u4", (TDET_MAX_FREQ,))], align=True)                              # igdsp_tdet_plan, 84 bytes
TDET_STATE = np.dtype([("hist", "<i2", (TDET_HIST,)), ("cur", "u1"), ("cand", "u1"), ("run", "u1"), ("off", "u1"), ("len", "<u2"),
                       ("reserved", "<u2")], align=True)                                           # igdsp_tdet_state, 264 bytes
TDET_REC = np.dtype([("hit", "u1", (2,)), ("cur", "u1"), ("flags", "u1"), ("len", "<u2"), ("code", "u1"), ("reserved", "u1")], align=True)
TDET_EVENT = np.dtype([("channel", "<u4"), ("frame", "<u4"), ("rec", TDET_REC)], align=True)     # igdsp_tdet_event, 16 bytes
# the echo canceller (igdsp_echo_cancel / igdsp_ec_frame)
EC_MAX_TAIL, EC_BLOCK, EC_TAG = 256, 8, 0xEC010000
EC_RUN, EC_FREEZE, EC_BYPASS, EC_RESET = 0, 1, 2, 3
EC_ADAPTED, EC_DOUBLETALK, EC_FAR_ACTIVE, EC_W_SATURATED, EC_BYPASSED = 1, 2, 4, 8, 16
EC_CFG = np.dtype([("tail", "<u2"), ("mu_shift", "u1"), ("reserved", "u1"), ("pmin", "<u4"), ("hang", "<u2"), ("dmin", "<u2")],
                  align=True)                                                                      # igdsp_ec_cfg, 12 bytes
EC_STATE = np.dtype([("w", "<i4", (EC_MAX_TAIL,)), ("hist", "<i2", (EC_MAX_TAIL,)), ("hang", "<u4"), ("flags", "<u4"), ("tag", "<u4"),
                     ("reserved", "<u4")], align=True)                                             # igdsp_ec_state, 1552 bytes
EC_REC = np.dtype([("near_e", "<u4"), ("out_e", "<u4"), ("flags", "u1"), ("n_adapt", "u1"), ("n_dt", "u1"), ("reserved", "u1"),
                   ("wmax", "<u2"), ("reserved2", "<u2")], align=True)                             # igdsp_ec_rec, 16 bytes
# the level control (igdsp_agc_run / igdsp_agc_frame)
AGC_BLOCK, AGC_UNITY, AGC_CAP, AGC_TAG = 8, 4096, 65535, 0xA6C10001
AGC_RUN, AGC_FREEZE, AGC_BYPASS, AGC_RESET = 0, 1, 2, 3
AGC_ACTIVE, AGC_LIMITED, AGC_AT_MAX, AGC_AT_MIN, AGC_ATTACKED, AGC_FROZEN, AGC_BYPASSED = 1, 2, 4, 8, 16, 32, 64
AGC_CFG = np.dtype([("target", "<u2"), ("ceil", "<u2"), ("gate", "<u2"), ("gmin", "<u2"), ("gmax", "<u2"), ("att", "u1"), ("rel", "u1"), ("up", "u1"),
                    ("down", "u1"), ("lrel", "u1"), ("reserved", "u1")], align=True)               # igdsp_agc_cfg, 16 bytes
AGC_STATE = np.dtype([("tag", "<u4"), ("env", "<u2"), ("gain", "<u2"), ("cap", "<u2"), ("flags", "<u2"), ("reserved", "<u4")],
                     align=True)                                                                   # igdsp_agc_state, 16 bytes
AGC_REC = np.dtype([("gain", "<u2"), ("tmin", "<u2"), ("in_peak", "<u2"), ("out_peak", "<u2"), ("env", "<u2"), ("flags", "u1"), ("n_limited", "u1"),
                    ("reserved", "<u4")], align=True)                                              # igdsp_agc_rec, 16 bytes
# voice activity, DTX and the comfort-noise payload (igdsp_vad_run / igdsp_vad_frame)
VAD_ORDER, VAD_KMAX, VAD_TAG = 10, 32508, 0x7AD10001
VAD_RUN, VAD_FREEZE, VAD_BYPASS, VAD_RESET = 0, 1, 2, 3
VAD_NONE, VAD_VOICE, VAD_SID = 0, 1, 2
VAD_F_RAW, VAD_F_VOICE, VAD_F_ONSET, VAD_F_OFFSET, VAD_F_SID, VAD_F_QUIET, VAD_F_FROZEN, VAD_F_BYPASSED = 1, 2, 4, 8, 16, 32, 64, 128
VAD_EVENT_DEFAULT = 0x0C
VAD_CFG = np.dtype([("thr_abs", "<u4"), ("nf_min", "<u4"), ("nf_max", "<u4"), ("sid_every", "<u2"), ("ratio_on_q4", "u1"), ("ratio_off_q4", "u1"),
                    ("dn", "u1"), ("up", "u1"), ("up_v", "u1"), ("asm_shift", "u1"), ("burst", "u1"), ("hang_long", "u1"), ("hang_short", "u1"),
                    ("order", "u1"), ("dtx", "u1"), ("sid_delta", "u1"), ("sid_gap", "u1"), ("vox_on", "u1"), ("vox_off", "u1"),
                    ("reserved", "u1", (3,))], align=True)                                         # igdsp_vad_cfg, 32 bytes
VAD_STATE = np.dtype([("tag", "<u4"), ("nf", "<u4"), ("A", "<i8", (11,)), ("since_sid", "<u2"), ("run", "<u2"), ("hang", "u1"), ("voice", "u1"),
                      ("avalid", "u1"), ("last_level", "u1"), ("sid_sent", "u1"), ("flags", "u1"), ("reserved", "u1", (22,))],
                     align=True)                                                                   # igdsp_vad_state, 128 bytes
VAD_REC = np.dtype([("ms", "<u4"), ("nf", "<u4"), ("run", "<u2"), ("flags", "u1"), ("kind", "u1"), ("level", "u1"), ("hang", "u1"), ("sid_len", "u1"),
                    ("reserved", "u1")], align=True)                                               # igdsp_vad_rec, 16 bytes
VAD_EVENT = np.dtype([("channel", "<u4"), ("frame", "<u4"), ("ms", "<u4"), ("run", "<u2"), ("flags", "u1"), ("level", "u1")],
                     align=True)                                                                   # igdsp_vad_event, 16 bytes
# comfort noise from RFC 3389 SIDs (igdsp_cng_run / igdsp_cng_frame)
CNG_TAG, CNG_GMAX = 0xC4610001, 3632640
CNG_RUN, CNG_FREEZE, CNG_BYPASS, CNG_RESET = 0, 1, 2, 3
CNG_F_GENERATED, CNG_F_SID, CNG_F_NO_MODEL, CNG_F_VOICE, CNG_F_CLIPPED, CNG_F_SID_EMPTY, CNG_F_FROZEN, CNG_F_BYPASSED = 1, 2, 4, 8, 16, 32, 64, 128
CNG_STATE = np.dtype([("tag", "<u4"), ("seed", "<u4"), ("ctr", "<u4"), ("g", "<u4"), ("g_tgt", "<u4"), ("b", "<i4", (10,)), ("kq", "<i2", (10,)),
                      ("since_sid", "<u2"), ("level", "u1"), ("order", "u1"), ("have", "u1"), ("flags", "u1"), ("reserved", "u1", (10,))],
                     align=True)                                                                   # igdsp_cng_state, 96 bytes
CNG_REC = np.dtype([("g", "<u4"), ("g_tgt", "<u4"), ("since_sid", "<u2"), ("flags", "u1"), ("level", "u1"), ("order", "u1"), ("reserved", "u1", (3,))],
                   align=True)                                                                     # igdsp_cng_rec, 16 bytes
# the filter: per channel a chain of second-order sections (igdsp_filt_run / igdsp_filt_frame)
FILT_TAG, FILT_MAX_SECTIONS, FILT_UNITY = 0xF1170001, 4, 8192
FILT_RUN, FILT_BYPASS, FILT_RESET = 0, 1, 2
FILT_CLIPPED, FILT_NO_PLAN, FILT_BAD_PLAN, FILT_BYPASSED, FILT_WAS_RESET = 1, 2, 4, 8, 16
FILT_LOWPASS, FILT_HIGHPASS, FILT_BANDPASS, FILT_NOTCH, FILT_PEAK, FILT_LOWSHELF, FILT_HIGHSHELF, FILT_LP1, FILT_HP1 = range(9)
FILT_VOICE_BAND, FILT_CTCSS_HP, FILT_DEEMPH, FILT_PREEMPH, FILT_DC_BLOCK = range(5)
FILT_SECTION = np.dtype([("b0", "<i2"), ("b1", "<i2"), ("b2", "<i2"), ("a1", "<i2"), ("a2", "<i2")])      # igdsp_filt_section, 10 bytes
FILT_PLAN = np.dtype([("n_sections", "<u2"), ("reserved", "<u2"), ("clock_rate", "<u4"), ("s", FILT_SECTION, (4,))])   # igdsp_filt_plan, 48 bytes
FILT_HIST = np.dtype([("x1", "<i2"), ("x2", "<i2"), ("y1", "<i2"), ("y2", "<i2"), ("e", "<u2")])         # igdsp_filt_hist, 10 bytes
FILT_STATE = np.dtype([("tag", "<u4"), ("s", FILT_HIST, (4,)), ("flags", "<u2"), ("reserved", "<u2")])    # igdsp_filt_state, 48 bytes
FILT_REC = np.dtype([("in_peak", "<u2"), ("out_peak", "<u2"), ("n_clipped", "<u2"), ("plan", "<u2"), ("flags", "u1"), ("n_sections", "u1"),
                     ("reserved", "u1", (6,))])                                                    # igdsp_filt_rec, 16 bytes
assert FILT_PLAN.itemsize == 48 and FILT_STATE.itemsize == 48 and FILT_REC.itemsize == 16
# noise suppression: per channel a spectral gain under and between speech (igdsp_ns_run / igdsp_ns_frame)
NS_TAG, NS_HOP, NS_BANDS, NS_UNITY = 0x4E530001, 80, 32, 32768
NS_RUN, NS_FREEZE, NS_BYPASS, NS_RESET = 0, 1, 2, 3
NS_LEARNING, NS_SUPPRESSING, NS_CLIPPED, NS_FROZEN, NS_BYPASSED, NS_WAS_RESET = 1, 2, 4, 8, 16, 32
NS_CFG = np.dtype([("floor_q15", "<u4"), ("over_q4", "<u2"), ("init_hops", "<u2"), ("track_shift", "<u2"), ("rise_shift", "<u2"), ("reserved", "<u4")],
                  align=True)                                                                      # igdsp_ns_cfg, 16 bytes
NS_STATE = np.dtype([("tag", "<u4"), ("hops", "<u2"), ("flags", "<u2"), ("reserved", "<u4", (2,)), ("prev", "<i2", (80,)), ("ola", "<i4", (80,)),
                     ("S", "<u8", (32,)), ("N", "<u8", (32,)), ("Gt", "<u2", (32,))], align=True)  # igdsp_ns_state, 1 072 bytes
NS_REC = np.dtype([("in_energy", "<u4"), ("out_energy", "<u4"), ("min_gain_q15", "<u2"), ("n_clipped", "<u2"), ("noise_idx", "u1"), ("flags", "u1"),
                   ("reserved", "u1", (2,))], align=True)                                          # igdsp_ns_rec, 16 bytes
assert NS_CFG.itemsize == 16 and NS_STATE.itemsize == 1072 and NS_REC.itemsize == 16
# SRTP (RFC 3711, AES_CM_128_HMAC_SHA1_80 / _32): per leg and direction (igdsp_srtp_protect / igdsp_srtp_unprotect / igdsp_srtp_*_packet)
SRTP_TAG, SRTP_MAX_PACKET = 0x53525000, 2048
SRTP_RUN, SRTP_BYPASS, SRTP_RESET = 0, 1, 2
SRTP_NO_KEY, SRTP_OK, SRTP_AUTH_FAIL, SRTP_REPLAY, SRTP_OLD, SRTP_MALFORMED, SRTP_EMPTY, SRTP_ROLLED, SRTP_BYPASSED = 0, 1, 2, 4, 8, 16, 32, 64, 128
SRTP_STATE = np.dtype([("tag", "<u4"), ("roc", "<u4"), ("s_l", "<u2"), ("have_s_l", "<u2"), ("reserved", "<u4"), ("window", "<u8"), ("n_ok", "<u4"),
                       ("n_auth_fail", "<u4"), ("n_replay", "<u4"), ("n_malformed", "<u4"), ("rk", "<u4", (44,)), ("ks", "u1", (16,)), ("mid_i", "<u4", (5,)),
                       ("mid_o", "<u4", (5,)), ("reserved2", "<u4", (4,))], align=True)            # igdsp_srtp_state, 288 bytes
SRTP_REC = np.dtype([("roc_used", "<u4"), ("size_out", "<u2"), ("flags", "u1"), ("reserved", "u1")], align=True)   # igdsp_srtp_rec, 8 bytes
assert SRTP_STATE.itemsize == 288 and SRTP_REC.itemsize == 8
# SRTP with AES-GCM (RFC 7714, AEAD_AES_128_GCM / AEAD_AES_256_GCM): igdsp_srtp_gcm_protect / igdsp_srtp_gcm_unprotect / igdsp_srtp_gcm_*_packet;
# the controls, the record and its flags are SRTP's
SRTP_GCM_TAG, SRTP_GCM_TAG_LEN = 0x53524700, 16
SRTP_GCM_STATE = np.dtype([("tag", "<u4"), ("roc", "<u4"), ("s_l", "<u2"), ("have_s_l", "<u2"), ("reserved", "<u4"), ("window", "<u8"), ("n_ok", "<u4"),
                           ("n_auth_fail", "<u4"), ("n_replay", "<u4"), ("n_malformed", "<u4"), ("rk", "<u4", (60,)), ("salt", "u1", (12,)), ("pad", "<u4"),
                           ("h", "u1", (16,)), ("reserved2", "<u4", (2,))], align=True)            # igdsp_srtp_gcm_state, 320 bytes
assert SRTP_GCM_STATE.itemsize == 320 and SRTP_GCM_STATE.fields["rk"][1] == 40 and SRTP_GCM_STATE.fields["salt"][1] == 280 and SRTP_GCM_STATE.fields["h"][1] == 296
assert all(SRTP_GCM_STATE.fields[k][1] == SRTP_STATE.fields[k][1] for k in SRTP_STATE.names[:10])   # the ten words that move are SRTP's
CHAN_PROBE = np.dtype([("run", "<u4"), ("alarms", "<u4")], align=True)
# the jitter buffer (igdsp_jb_receive / igdsp_jb_report)
JB_STATE = np.dtype(
    [("ssrc", "<u4"), ("cycles", "<u4"), ("base_seq", "<u4"), ("bad_seq", "<u4"), ("probation", "<u4"), ("received", "<u4"),
     ("transit", "<u4"), ("jitter", "<u4"), ("epoch", "<u4"), ("max_seq", "<u2"), ("head", "<u2"), ("wait", "u1"), ("lost_run", "u1"),
     ("flags", "u1"), ("reserved0", "u1"), ("played", "<u4"), ("lost", "<u4"), ("late", "<u4"), ("duplicate", "<u4"), ("invalid", "<u4"),
     ("keepalives", "<u4"), ("discarded", "<u4"), ("restarts", "<u4"), ("reserved1", "<u4")],
    align=True,
)
# packet loss concealment (igdsp_plc_conceal)
PLC_STATE = np.dtype(
    [("hist", "<i2", (PLC_HIST,)), ("cycle", "<i2", (PLC_PMAX,)), ("head", "<u2"), ("pitch", "<u2"), ("pos", "<u2"), ("missing", "<u2"),
     ("runs", "<u4"), ("concealed", "<u4"), ("reserved", "<u4", (4,))],
    align=True,
)
JB_PRIOR = np.dtype([("expected_prior", "<u4"), ("received_prior", "<u4"), ("epoch", "<u4"), ("reserved", "<u4")], align=True)
JB_RR = np.dtype([("ssrc", "<u4"), ("ext_max_seq", "<u4"), ("cum_lost", "<i4"), ("jitter", "<u4"), ("fraction_lost", "u1"), ("valid", "u1"),
                  ("reserved", "<u2")], align=True)
# RTCP / SRTCP (igdsp_rtcp_build / igdsp_rtcp_parse / igdsp_srtcp_protect / igdsp_srtcp_unprotect and their host entries)
RTCP_MAX_BUILT, RTCP_CNAME_MAX = 136, 64
RTCP_NONE, RTCP_REPORT, RTCP_BYE = 0, 1, 2
RTCP_SR, RTCP_RR, RTCP_HAS_BLOCK, RTCP_BYE_SENT = 1, 2, 4, 8                         # RTCP_BUILT.flags
RTCP_HAVE_SR, RTCP_PEER_VALID, RTCP_RTT_VALID, RTCP_BYE_SEEN = 1, 2, 4, 8            # RTCP_STATE.flags
RTCP_PARSED, RTCP_MALFORMED, RTCP_EMPTY, RTCP_GOT_SR, RTCP_GOT_BLOCK, RTCP_GOT_RTT, RTCP_RTT_NEGATIVE, RTCP_GOT_BYE = 1, 2, 4, 8, 16, 32, 64, 128   # RTCP_SEEN.flags
SRTCP_TAG, SRTCP_TRAILER, SRTCP_CLEAR = 0x53524300, 14, 0x40
RTCP_SRC = np.dtype([("ssrc", "<u4"), ("rtp_ts", "<u4"), ("packets", "<u4"), ("octets", "<u4")], align=True)   # igdsp_rtcp_src, 16 bytes
RTCP_STATE = np.dtype([("prior", JB_PRIOR), ("sent_prior", "<u4"), ("n_built", "<u4"), ("lsr", "<u4"), ("lsr_arrival", "<u4"), ("flags", "<u4"),
                       ("n_parsed", "<u4"), ("n_malformed", "<u4"), ("rtt_last", "<u4"), ("rtt_count", "<u4"), ("peer_fraction_lost", "<u4"),
                       ("peer_cum_lost", "<i4"), ("peer_ext_seq", "<u4"), ("peer_jitter", "<u4"), ("reserved", "<u4", (3,))], align=True)   # igdsp_rtcp_state, 80 bytes
RTCP_BUILT = np.dtype([("size", "<u2"), ("flags", "u1"), ("reserved", "u1"), ("reserved2", "<u4")], align=True)   # igdsp_rtcp_built, 8 bytes
RTCP_SEEN = np.dtype([("flags", "u1"), ("n_sub", "u1"), ("peer_fraction_lost", "u1"), ("reserved", "u1"), ("sender_ssrc", "<u4"), ("rtt", "<u4"),
                      ("peer_cum_lost", "<i4"), ("peer_ext_seq", "<u4"), ("peer_jitter", "<u4"), ("sr_packets", "<u4"), ("sr_octets", "<u4")],
                     align=True)                                                    # igdsp_rtcp_seen, 32 bytes
assert RTCP_SRC.itemsize == 16 and RTCP_STATE.itemsize == 80 and RTCP_BUILT.itemsize == 8 and RTCP_SEEN.itemsize == 32
# the adaptive playout delay (igdsp_jb_receive_adaptive / igdsp_jb_adapt_next)
JB_ADAPT_CFG = np.dtype([("min_frames", "u1"), ("max_frames", "u1"), ("init_frames", "u1"), ("jitter_mult", "u1"), ("late_restart", "u1"),
                         ("reserved", "u1", (3,))], align=True)   # igdsp_jb_adapt_cfg
JB_ADAPT = np.dtype([("delay", "u1"), ("flags", "u1"), ("need", "u1"), ("late_run", "u1"), ("grows", "<u2"), ("shrinks", "<u2")],
                    align=True)   # igdsp_jb_adapt
GATE_ALWAYS, GATE_SQU, GATE_PTT, GATE_SQU_OR_PTT = 0, 1, 2, 3
PKT_SLOTS, PKT_PACKED, PKT_MIXED = 0, 1, 2
PROBE_ALARM = 500
RTP_V2, RTP_X, RTP_MARKER, RTP_ED137_OK, RTP_KEEPALIVE, RTP_METERED, RTP_RUNT, RTP_OVERSIZE = 1, 2, 4, 8, 16, 32, 64, 128
# ED-137 TX packetizer (igdsp_tx_packetize)
TX_CHAN = np.dtype(
    [("r2s_send_ms", "<u8"), ("ts", "<u4"), ("ssrc", "<u4"), ("keepalive_ms", "<i4"), ("packet_cnt", "<i4"), ("seq", "<u2"), ("pt", "u1"),
     ("first_r2s", "u1"), ("tx_slave", "u1"), ("rx_slave", "u1"), ("tx_slave_changed", "u1"), ("rx_slave_changed", "u1"),
     ("slave_count", "<i4"), ("ptt", "u1"), ("sql", "u1"), ("call_in", "u1"), ("call_recorder", "u1"), ("pttid", "u1"),
     ("pttpriority", "u1"), ("bssi", "u1"), ("calltype", "u1"), ("tx_run", "<i2"), ("level", "u1"), ("reserved0", "u1"),
     ("reserved", "<u4", (4,))],
    align=True,
)
TX_INFO = np.dtype([("ed137", "<u4"), ("size", "<u2"), ("flags", "u1"), ("level", "u1")], align=True)
TX_CT_IDLE, TX_CT_RX, TX_CT_TX = 1, 2, 4
TX_SENT, TX_KEEPALIVE_PT, TX_MARKER, TX_STALE_PAYLOAD, TX_LEVEL_VALID = 1, 2, 4, 8, 16
TX_CTL_PTT, TX_CTL_SQL, TX_CTL_MARK, TX_CTL_SET = 1, 2, 4, 0x80
# the staged send path (igdsp_on_tx_frame / igdsp_tx_flush): one igdsp_tx_packet per processed frame, packets in 256-byte slots
TX_PACKET = np.dtype([("pkt", "<u8"), ("call_id", "<i4"), ("ed137", "<u4"), ("size", "<u2"), ("flags", "u1"), ("level", "u1")], align=True)
TX_MAX_N = 236
TX_SLOT = 256
AGGREGATE = np.dtype({      # one 128-byte line per counter (include/igdsp.h); the padding is not exposed as fields
    "names": ["sumsq", "samples", "frames", "n_silent", "n_clipped", "byte_mean_sum", "peak_slot"],
    "formats": ["<u8", "<u8", "<u8", "<u8", "<u8", "<u8", ("<u8", (AGG_MAX_RANKS,))],
    "offsets": [128 * i for i in range(7)],
    "itemsize": 8 * AGG_WORDS,
})


class Level(C.Structure):
    _fields_ = [("byte_mean", C.c_uint8), ("flags", C.c_uint8), ("peak", C.c_uint16), ("rms", C.c_float),
                ("percent", C.c_int32), ("peak_hold", C.c_uint16), ("dropped", C.c_uint16), ("frames", C.c_uint32)]


class Window(C.Structure):
    """igdsp_window: the ED-137 gated window of igdsp_window_update / igdsp_decode_meter_window."""
    _fields_ = [("gate_mode", C.c_uint32), ("probe_alarm", C.c_uint32), ("d_hold", C.c_void_p), ("d_gate", C.c_void_p),
                ("d_probe", C.c_void_p), ("d_work", C.c_void_p)]


class SpecCfg(C.Structure):
    """igdsp_spec_cfg: a spectrum every hop_frames frames, the average's gain alpha"""
    _fields_ = [("hop_frames", C.c_uint32), ("alpha", C.c_float)]


class ChanProbe(C.Structure):
    _fields_ = [("run", C.c_uint32), ("alarms", C.c_uint32)]


IO_INPUT, IO_RECORD, IO_BULK = 0, 1, 2


class IoBuf(C.Structure):
    _fields_ = [("bytes", C.c_size_t), ("role", C.c_uint32), ("reserved", C.c_uint32), ("ptr", C.c_void_p)]


class IoReport(C.Structure):
    _fields_ = [("placed", C.c_uint32), ("bulk_spread", C.c_uint32), ("classes_found", C.c_uint32), ("chunks_explored", C.c_uint32),
                ("probes", C.c_uint32), ("reseeds", C.c_uint32), ("chunk_bytes", C.c_uint64), ("explored_bytes", C.c_uint64),
                ("probe_ms_same", C.c_float), ("probe_ms_other", C.c_float), ("setup_ms", C.c_float), ("settle_ms", C.c_float)]

    def as_dict(self):
        return {k: (round(getattr(self, k), 4) if isinstance(getattr(self, k), float) else getattr(self, k))
                for k, _ in self._fields_ if not k.startswith("reserved")}


class IgdspError(RuntimeError):
    def __init__(self, code: int, where: str, detail: str = ""):
        self.code = code
        super().__init__(f"{where} failed: {ERRORS.get(code, code)}" + (f" ({detail})" if detail else ""))


# every symbol include/igdsp.h declares: (name, restype, argtypes)
_vp, _u32, _u64, _i32, _int = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32, C.c_int
PROTOTYPES = [
    ("igdsp_abi_version", _int, []),
    ("igdsp_create", _int, [C.POINTER(_vp), _int, _u32]),
    ("igdsp_destroy", _int, [_vp]),
    ("igdsp_last_error", C.c_char_p, [_vp]),
    ("igdsp_device_info", _int, [_vp, C.POINTER(_int), C.POINTER(_int), C.c_char_p, C.c_size_t]),
    ("igdsp_map_call", _int, [_vp, _i32, _u32]),
    ("igdsp_unmap_call", _int, [_vp, _i32]),
    ("igdsp_on_rtp_frame", _int, [_vp, _i32, C.c_uint8, _vp, _u32]),
    ("igdsp_flush", _int, [_vp, C.POINTER(_u32)]),
    ("igdsp_flush_begin", _int, [_vp, C.POINTER(_u32)]),
    ("igdsp_flush_end", _int, [_vp, _int]),
    ("igdsp_set_ed137", _int, [_vp, _i32, _u32]),
    ("igdsp_set_gate_mode", _int, [_vp, _u32]),
    ("igdsp_get_probe", _int, [_vp, _u32, C.POINTER(ChanProbe)]),
    ("igdsp_poll", _int, [_vp, _u32, C.POINTER(Level)]),
    ("igdsp_poll_call", _int, [_vp, _i32, C.POINTER(Level)]),
    ("igdsp_reset_hold", _int, [_vp, _u32]),
    ("igdsp_get_hold", _int, [_vp, _u32, _vp]),
    ("igdsp_decode_meter", _int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _u32, _vp]),
    ("igdsp_encode", _int, [_vp, _vp, _vp, _u32, _u32, _u32, _vp, _int, _vp]),
    ("igdsp_roundtrip_peakhold", _int, [_vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _int, _vp]),
    ("igdsp_hold_update", _int, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    ("igdsp_hold_reset", _int, [_vp, _vp, _u32, _vp, _vp]),
    ("igdsp_agg_reset", _int, [_vp, _vp, _vp]),
    ("igdsp_depayload", _int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    ("igdsp_decode_meter_rtp", _int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _u32, _vp]),
    ("igdsp_decode_meter_packets", _int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _u32, _vp]),
    ("igdsp_decode_meter_packets_mixed", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _u32, _vp]),
    ("igdsp_window_work_bytes", C.c_size_t, [_u32]),
    ("igdsp_window_update", _int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, C.POINTER(Window), _vp]),
    ("igdsp_decode_meter_window", _int, [_vp, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _u32, C.POINTER(Window), _vp]),
    ("igdsp_wav_expand", _int, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _u64, _vp]),
    ("igdsp_tx_chan_init", _int, [_vp, C.c_char_p, _int, C.c_uint8, _u32, C.c_uint16, _u32, _i32, _u64]),
    ("igdsp_tx_calltype_bits", _int, [C.c_char_p]),
    ("igdsp_tx_packetize", _int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u64, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _int, _vp]),
    ("igdsp_tx_open", _int, [_vp, _i32, C.c_char_p, _int, _i32, _u64]),
    ("igdsp_tx_close", _int, [_vp, _i32]),
    ("igdsp_tx_set_ptt", _int, [_vp, _i32, _int, _int, _int]),
    ("igdsp_tx_set_sql", _int, [_vp, _i32, _int, _int, _i32]),
    ("igdsp_tx_set_ptt_id", _int, [_vp, _i32, _int]),
    ("igdsp_tx_set_slave", _int, [_vp, _i32, _int, _int]),
    ("igdsp_tx_set_recorder", _int, [_vp, _i32, _int]),
    ("igdsp_tx_set_calltype", _int, [_vp, _i32, C.c_char_p]),
    ("igdsp_on_tx_frame", _int, [_vp, _i32, _vp, _u32, _u64]),
    ("igdsp_tx_flush", _int, [_vp, C.POINTER(_u32)]),
    ("igdsp_tx_results", _int, [_vp, C.POINTER(_vp), C.POINTER(_u32)]),
    ("igdsp_tx_get_chan", _int, [_vp, _i32, _vp]),
    ("igdsp_tx_counts", _int, [_vp, _i32, C.POINTER(_u32), C.POINTER(_u32)]),
    ("igdsp_conf_level_q7", _int, [C.c_float]),
    ("igdsp_conf_build", _int, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, C.POINTER(_u32)]),
    ("igdsp_conf_mix", _int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    ("igdsp_bss_select", _int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp,
                                _vp]),
    ("igdsp_ptt_arbitrate", _int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp]),
    ("igdsp_link_work_bytes", C.c_size_t, [_u32, _u32]),
    ("igdsp_link_watch", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u64, _u32, _u32, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _vp]),
    ("igdsp_jb_ring_bytes", C.c_size_t, [_u32, _u32]),
    ("igdsp_jb_report", _int, [_vp, _vp, _vp]),
    ("igdsp_jb_receive", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("igdsp_jb_adapt_cfg_default", None, [_vp]),
    ("igdsp_jb_adapt_next", _int, [_vp, _u32, _u32, _vp]),
    ("igdsp_jb_receive_adaptive", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _vp]),
    ("igdsp_plc_conceal", _int, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    ("igdsp_snd_combine", _int, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    ("igdsp_snd_split", _int, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    ("igdsp_snd_vu", _int, [_vp, _vp]),
    ("igdsp_tone_plan_build", _int, [_vp, _u32, _u32, _u32, _vp]),
    ("igdsp_tone_frame", _int, [_vp, _vp, _u32, _u32, _vp, _vp]),
    ("igdsp_tone_generate", _int, [_vp, _vp, _u32, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    ("igdsp_rs_taps", _int, [_u32, _u32, C.POINTER(_vp), C.POINTER(_u32)]),
    ("igdsp_rs_frame", _int, [_vp, _u32, _u32, _vp, _u32, _vp]),
    ("igdsp_resample", _int, [_vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    ("igdsp_dbuf_run", _int, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("igdsp_dbuf_step", _int, [_vp, _u32, _vp, _u32, _u32, _vp, C.POINTER(_u32)]),
    ("igdsp_spectrum", _int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("igdsp_spec_frame", _int, [_vp, _vp, _u32, _vp, _vp, _vp]),
    ("igdsp_spec_tables", _int, [C.POINTER(_vp), C.POINTER(_vp)]),
    ("igdsp_tdet_plan_build", _int, [_u32, _vp, _u32, _u32, _vp, _vp]),
    ("igdsp_tdet_plan_dtmf", _int, [_u32, _vp]),
    ("igdsp_tdet_digit", _int, [_u32]),
    ("igdsp_tdet_table", _int, [_vp, _u32, _vp]),
    ("igdsp_tdet_frame", _int, [_vp, _vp, _vp, _u32, _vp]),
    ("igdsp_tdet_work_bytes", C.c_size_t, [_u32, _u32, _int]),
    ("igdsp_tone_detect", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _vp]),
    ("igdsp_ec_cfg_default", None, [_u32, _vp]),
    ("igdsp_ec_frame", _int, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp]),
    ("igdsp_echo_cancel", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    ("igdsp_agc_cfg_default", None, [_vp]),
    ("igdsp_agc_frame", _int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp]),
    ("igdsp_agc_run", _int, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    ("igdsp_vad_cfg_default", None, [_vp]),
    ("igdsp_vad_table", _int, [_vp]),
    ("igdsp_vad_frame", _int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp]),
    ("igdsp_sid_decode", _int, [_vp, _u32, _vp, _vp]),
    ("igdsp_vad_work_bytes", C.c_size_t, [_u32, _u32, _int]),
    ("igdsp_vad_run", _int, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp]),
    ("igdsp_cng_table", _int, [_vp]),
    ("igdsp_cng_gain", _int, [_vp, _u32, _vp]),
    ("igdsp_cng_frame", _int, [_vp, _u32, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _vp]),
    ("igdsp_cng_run", _int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("igdsp_filt_frame", _int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp]),
    ("igdsp_filt_plan_check", _int, [_vp]),
    ("igdsp_filt_design", _int, [_u32, _u32, C.c_double, C.c_double, C.c_double, _vp]),
    ("igdsp_filt_plan_preset", _int, [_u32, _u32, _vp]),
    ("igdsp_filt_run", _int, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    ("igdsp_ns_cfg_default", None, [_vp]),
    ("igdsp_ns_tables", _int, [C.POINTER(_vp), C.POINTER(_vp)]),
    ("igdsp_ns_frame", _int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp]),
    ("igdsp_ns_run", _int, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    ("igdsp_srtp_derive", _int, [_vp, _u32, _u32, _vp]),
    ("igdsp_srtp_protect_packet", _int, [_vp, _u32, _vp, _u32, _vp, _u32, C.POINTER(_u32), _vp]),
    ("igdsp_srtp_unprotect_packet", _int, [_vp, _u32, _vp, _u32, _vp, _u32, C.POINTER(_u32), _vp]),
    ("igdsp_srtp_protect", _int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _u32, _vp, _vp, _vp]),
    ("igdsp_srtp_unprotect", _int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _u32, _vp, _vp, _vp]),
    ("igdsp_rtcp_build_packet", _int, [_vp, _u32, _vp, _vp, _u64, _vp, _u32, _vp, _u32, C.POINTER(_u32), _vp]),
    ("igdsp_rtcp_parse_packet", _int, [_vp, _vp, _u32, _u32, _u32, _vp]),
    ("igdsp_srtcp_derive", _int, [_vp, _u32, _vp]),
    ("igdsp_srtcp_protect_packet", _int, [_vp, _u32, _vp, _u32, _vp, _u32, C.POINTER(_u32), _vp]),
    ("igdsp_srtcp_unprotect_packet", _int, [_vp, _u32, _vp, _u32, _vp, _u32, C.POINTER(_u32), _vp]),
    ("igdsp_rtcp_build", _int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _u32, _vp, _vp, _vp]),
    ("igdsp_rtcp_parse", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    ("igdsp_srtcp_protect", _int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _u32, _vp, _vp, _vp]),
    ("igdsp_srtcp_unprotect", _int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _u32, _vp, _vp, _vp]),
    ("igdsp_srtp_gcm_derive", _int, [_vp, _u32, _u32, _vp]),
    ("igdsp_srtp_gcm_protect_packet", _int, [_vp, _u32, _vp, _u32, _vp, _u32, C.POINTER(_u32), _vp]),
    ("igdsp_srtp_gcm_unprotect_packet", _int, [_vp, _u32, _vp, _u32, _vp, _u32, C.POINTER(_u32), _vp]),
    ("igdsp_srtp_gcm_protect", _int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _u32, _vp, _vp, _vp]),
    ("igdsp_srtp_gcm_unprotect", _int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _u32, _vp, _vp, _vp]),
    ("igdsp_g726_reorder", _int, [_vp, _vp, _vp, _u64, _int, _vp]),
    ("igdsp_gen_uniform", _int, [_vp, _vp, _u64, _u64, _u64, _vp]),
    ("igdsp_dev_alloc", _int, [_vp, C.POINTER(_vp), C.c_size_t]),
    ("igdsp_dev_free", _int, [_vp, _vp]),
    ("igdsp_dev_alloc_far", _int, [_vp, C.POINTER(_vp), C.c_size_t, _vp, C.c_size_t, _u32, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("igdsp_io_alloc", _int, [_vp, C.POINTER(IoBuf), _u32, C.c_size_t, C.POINTER(_vp), C.POINTER(IoReport)]),
    ("igdsp_io_free", _int, [_vp, _vp]),
    ("igdsp_copy_h2d", _int, [_vp, _vp, _vp, C.c_size_t]),
    ("igdsp_copy_d2h", _int, [_vp, _vp, _vp, C.c_size_t]),
    ("igdsp_dev_memset", _int, [_vp, _vp, _int, C.c_size_t]),
    ("igdsp_sync", _int, [_vp, _vp]),
    ("igdsp_timer_create", _int, [_vp, C.POINTER(_vp)]),
    ("igdsp_timer_destroy", _int, [_vp, _vp]),
    ("igdsp_timer_start", _int, [_vp, _vp, _vp]),
    ("igdsp_timer_stop", _int, [_vp, _vp, _vp]),
    ("igdsp_timer_elapsed_ms", _int, [_vp, _vp, C.POINTER(C.c_float)]),
    ("igdsp_stream_read", _int, [_vp, _vp, C.c_size_t, _vp, _vp]),
    ("igdsp_probe_placement", _int, [_vp, _vp, C.c_size_t, _vp, _u32, C.POINTER(C.c_float), _vp]),
    ("igdsp_set_variant", _int, [_vp, _int]),
]

# The compute-free yardsticks (igdsp_internal_*, not in include/igdsp.h; tools/*_bench.py and the tests call them).  Nine take the
# arguments of a public entry and are derived from that entry's row above; igdsp_internal_tx_copy has no twin.
INTERNAL_TWIN = {
    "igdsp_internal_conf_copy": "igdsp_conf_mix",
    "igdsp_internal_bss_copy": "igdsp_bss_select",
    "igdsp_internal_ptt_copy": "igdsp_ptt_arbitrate",
    "igdsp_internal_link_copy": "igdsp_link_watch",
    "igdsp_internal_jb_copy": "igdsp_jb_receive",
    "igdsp_internal_plc_copy": "igdsp_plc_conceal",
    "igdsp_internal_snd_copy": "igdsp_snd_combine",
    "igdsp_internal_tone_fill": "igdsp_tone_generate",
    "igdsp_internal_rs_copy": "igdsp_resample",
}
_PUBLIC = {name: (res, args) for name, res, args in PROTOTYPES}
INTERNAL = {name: _PUBLIC[twin] for name, twin in INTERNAL_TWIN.items()}
INTERNAL["igdsp_internal_tx_copy"] = (_int, [_vp, _vp, _vp, _u32, _u32, _u32, _vp, _u32, _vp])

# A yardstick whose name is not of the *_copy / *_fill form: the same derivation, a table of its own; internal() consults both
INTERNAL_MORE_TWIN = {"igdsp_internal_dbuf_move": "igdsp_dbuf_run", "igdsp_internal_spec_move": "igdsp_spectrum",
                      "igdsp_internal_tdet_move": "igdsp_tone_detect", "igdsp_internal_ec_move": "igdsp_echo_cancel",
                      "igdsp_internal_agc_move": "igdsp_agc_run", "igdsp_internal_vad_move": "igdsp_vad_run",
                      "igdsp_internal_cng_move": "igdsp_cng_run", "igdsp_internal_filt_move": "igdsp_filt_run",
                      "igdsp_internal_ns_move": "igdsp_ns_run", "igdsp_internal_srtp_move": "igdsp_srtp_protect",
                      "igdsp_internal_srtcp_move": "igdsp_srtcp_protect", "igdsp_internal_srtp_gcm_move": "igdsp_srtp_gcm_protect",
                      "igdsp_internal_rtcp_build_move": "igdsp_rtcp_build", "igdsp_internal_rtcp_parse_move": "igdsp_rtcp_parse"}
INTERNAL_MORE = {name: _PUBLIC[twin] for name, twin in INTERNAL_MORE_TWIN.items()}

_lib = None


def internal(name: str):
    """The bound function of a yardstick entry of INTERNAL or INTERNAL_MORE ("igdsp_internal_rs_copy", or short "rs_copy"); it returns
    the raw code."""
    name = name if name.startswith("igdsp_internal_") else "igdsp_internal_" + name
    res, args = INTERNAL[name] if name in INTERNAL else INTERNAL_MORE[name]   # KeyError == not a yardstick entry
    fn = getattr(load(), name)
    fn.restype, fn.argtypes = res, list(args)
    return fn


def load() -> C.CDLL:
    """dlopen libigdsp.so and bind every prototype.  Raises if the extension is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -m igate4xsoftphonedsp_amd.build` "
                "(there is no CPU fallback for the igdsp kernels)"
            )
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7.  Import torch first so
        # libigdsp.so's DT_NEEDED resolves to the runtime that also owns the tensors whose device pointers
        # we are handed (loading ours first leaves torch without a usable device).  Plumbing only.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, res, args in PROTOTYPES:
            fn = getattr(L, name)          # AttributeError here == ABI symbol missing
            fn.restype = res
            fn.argtypes = args
        if L.igdsp_abi_version() != ABI_VERSION:
            raise ImportError(f"libigdsp ABI {L.igdsp_abi_version()} != binding {ABI_VERSION}")
        _lib = L
    return _lib


def tx_calltype_bits(calltype: str) -> int:
    """IGDSP_TX_CT_* bits of a calltype (host only, no GPU)."""
    return load().igdsp_tx_calltype_bits(calltype.encode())


def tx_chan_init(calltype: str, call_in: bool, pt: int, ssrc: int, seq0: int, ts0: int, keepalive_ms: int = 200, now_ms: int = 0) -> np.ndarray:
    """One igdsp_tx_chan with transport_adapter_create's defaults (host only, no GPU); a TX_CHAN record."""
    out = np.zeros((), dtype=TX_CHAN)
    rc = load().igdsp_tx_chan_init(out.ctypes.data_as(_vp), calltype.encode(), 1 if call_in else 0, pt, ssrc & 0xFFFFFFFF, seq0 & 0xFFFF,
                                   ts0 & 0xFFFFFFFF, keepalive_ms, now_ms)
    if rc != 0:
        raise IgdspError(rc, "igdsp_tx_chan_init")
    return out


def conf_level_q7(level: float) -> int:
    """igdsp_conf_level_q7: the Q7 receive level of a float slot volume (host only, no GPU); raises on IGDSP_EINVAL."""
    q = load().igdsp_conf_level_q7(level)
    if q < 0:
        raise IgdspError(q, "igdsp_conf_level_q7")
    return q


def conf_build(channel, port, n_channels: int, n_ports: int):
    """igdsp_conf_build: (channel, port) connection lists -> (port_ptr uint32 [n_ports + 1], members uint32 [n_members]) (host only)."""
    ch = np.ascontiguousarray(channel, dtype=np.uint32).reshape(-1)
    pt = np.ascontiguousarray(port, dtype=np.uint32).reshape(-1)
    if ch.shape != pt.shape:
        raise ValueError("channel and port lists differ in length")
    ptr = np.zeros(n_ports + 1, np.uint32)
    mem = np.zeros(max(1, ch.size), np.uint32)
    nm = _u32()
    rc = load().igdsp_conf_build(ch.ctypes.data_as(_vp), pt.ctypes.data_as(_vp), ch.size, n_channels, n_ports, ptr.ctypes.data_as(_vp),
                                 mem.ctypes.data_as(_vp), C.byref(nm))
    if rc != 0:
        raise IgdspError(rc, "igdsp_conf_build")
    return ptr, mem[: nm.value].copy()

def jb_ring_bytes(n_channels: int, n: int = SAMPLES_PER_FRAME) -> int:
    """igdsp_jb_ring_bytes (host only, no GPU): bytes of the jitter-buffer ring of n_channels at n samples per frame."""
    return int(load().igdsp_jb_ring_bytes(n_channels, n))


def link_work_bytes(n_channels: int, n_ticks: int) -> int:
    """igdsp_link_work_bytes (host only, no GPU): bytes of igdsp_link_watch's d_work for a launch of this shape."""
    return int(load().igdsp_link_work_bytes(n_channels, n_ticks))


def snd_vu(stats) -> dict:
    """igdsp_snd_vu (host only, no GPU): the broadcastVUMeter numbers of one FRAME_STATS record: {"percent": int, "db": float}."""
    st = np.ascontiguousarray(np.asarray(stats, dtype=FRAME_STATS).reshape(()))
    out = np.zeros((), dtype=SND_VU)
    rc = load().igdsp_snd_vu(st.ctypes.data_as(_vp), out.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_snd_vu")
    return {"percent": int(out["percent"]), "db": float(out["db"])}


def tone_plan_build(tones, clock_rate: int = 8000, options: int = TONE_LOOP) -> np.ndarray:
    """igdsp_tone_plan_build (host only, no GPU): tones = a TONE_DESC array or a list of (freq1, freq2, on_msec, off_msec[, volume]);
    returns one TONE_PLAN record."""
    if not (isinstance(tones, np.ndarray) and tones.dtype == TONE_DESC):
        d = np.zeros(len(tones), TONE_DESC)
        for i, t in enumerate(tones):
            d[i] = tuple(t) + (0,) * (6 - len(t))
        tones = d
    tones = np.ascontiguousarray(tones)
    out = np.zeros((), TONE_PLAN)
    rc = load().igdsp_tone_plan_build(tones.ctypes.data_as(_vp), len(tones), clock_rate, options, out.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_tone_plan_build")
    return out


def tone_frame(plan, state, n: int = SAMPLES_PER_FRAME, cmd: int = 0):
    """igdsp_tone_frame (host only, no GPU): one frame of one port.  plan a TONE_PLAN record, state a TONE_STATE record updated in
    place.  Returns (samples [n] int16, len)."""
    assert plan.dtype == TONE_PLAN and state.dtype == TONE_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    plan = np.ascontiguousarray(plan)
    out = np.zeros(max(int(n), 0), np.int16)
    ln = np.zeros((), np.uint16)
    rc = load().igdsp_tone_frame(plan.ctypes.data_as(_vp), state.ctypes.data_as(_vp), cmd, n, out.ctypes.data_as(_vp), ln.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_tone_frame")
    return out, int(ln)


def rs_taps(direction: int, factor: int) -> np.ndarray:
    """igdsp_rs_taps (host only, no GPU): a copy of the Q14 table of a direction and factor: U_R as [R][24] for RS_UP, D_R as [24 R] for
    RS_DOWN."""
    p, n = _vp(), _u32()
    rc = load().igdsp_rs_taps(direction, factor, C.byref(p), C.byref(n))
    if rc != 0:
        raise IgdspError(rc, "igdsp_rs_taps")
    t = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int16)), (n.value,)).copy()
    return t.reshape(factor, RS_TAPS) if direction == RS_UP else t


def dbuf_step(state, op: int, n: int, max_samples: int, x=None):
    """igdsp_dbuf_step (host only, no GPU): one step of one channel.  state a DBUF_STATE record updated in place, op DBUF_PUT / DBUF_GET /
    both / 0, x the frame a PUT appends (int16 [n]).  Returns (the row a GET took or None, the step's flag: JB_PLAYED / JB_LOST / JB_IDLE)."""
    assert state.dtype == DBUF_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    x = None if x is None else np.ascontiguousarray(x, dtype=np.int16)
    assert x is None or len(x) == n
    out = np.zeros(n, np.int16) if op & DBUF_GET else None
    flag = _u32(0)
    rc = load().igdsp_dbuf_step(state.ctypes.data_as(_vp), op, None if x is None else x.ctypes.data_as(_vp), n, max_samples,
                                None if out is None else out.ctypes.data_as(_vp), C.byref(flag))
    if rc != 0:
        raise IgdspError(rc, "igdsp_dbuf_step")
    return out, int(flag.value)


def _spec_cfg(cfg):
    """a SpecCfg from one, a (hop_frames, alpha) pair or None (the defaults: 1, 0.25)"""
    if cfg is None or isinstance(cfg, SpecCfg):
        return cfg
    return SpecCfg(int(cfg[0]), float(cfg[1]))


def spec_frame(state, row, cfg=None, want_raw=True):
    """igdsp_spec_frame (host only, no GPU): one frame of one channel.  state a SPEC_STATE record updated in place, row the frame's PCM
    (int16 [n]), cfg a SpecCfg, a (hop_frames, alpha) pair or None.  Returns (the frame's SPEC_REC record, the raw spectrum float32 [512]
    or None when the frame did not hop or want_raw is off)."""
    assert state.dtype == SPEC_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    row = np.ascontiguousarray(row, dtype=np.int16)
    c = _spec_cfg(cfg)
    rec = np.zeros((), SPEC_REC)
    raw = np.zeros(SPEC_BINS, np.float32) if want_raw else None
    rc = load().igdsp_spec_frame(state.ctypes.data_as(_vp), row.ctypes.data_as(_vp), len(row), None if c is None else C.cast(C.pointer(c), _vp),
                                 rec.ctypes.data_as(_vp), None if raw is None else raw.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_spec_frame")
    return rec, (raw if want_raw and rec["flags"] & SPEC_HOP else None)


def tdet_plan_build(freq_lo, freq_hi=(), clock_rate: int = 8000, thr=None) -> np.ndarray:
    """igdsp_tdet_plan_build (host only, no GPU): the low group's and the high group's frequencies in Hz, thr a TDET_THR record or None
    (the defaults); returns one TDET_PLAN record."""
    f = np.asarray(list(freq_lo) + list(freq_hi), "<u2")
    out = np.zeros((), TDET_PLAN)
    t = None if thr is None else np.asarray(thr, TDET_THR)
    rc = load().igdsp_tdet_plan_build(clock_rate, f.ctypes.data_as(_vp), len(freq_lo), len(freq_hi), None if t is None else t.ctypes.data_as(_vp),
                                      out.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_tdet_plan_build")
    return out


def tdet_plan_dtmf(clock_rate: int = 8000) -> np.ndarray:
    """igdsp_tdet_plan_dtmf (host only, no GPU): the 4 + 4 DTMF plan with the default thresholds."""
    out = np.zeros((), TDET_PLAN)
    rc = load().igdsp_tdet_plan_dtmf(clock_rate, out.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_tdet_plan_dtmf")
    return out


def tdet_digit(code: int) -> str:
    """igdsp_tdet_digit: the DTMF plan's character of a code, "" for any other code."""
    v = int(load().igdsp_tdet_digit(int(code)))
    return chr(v) if v else ""


def tdet_table(plan, n: int) -> np.ndarray:
    """igdsp_tdet_table (host only, no GPU): int16 [n_lo + n_hi][2][n], the cosine then the sine column of every frequency."""
    assert plan.dtype == TDET_PLAN
    nf = min(int(plan["n_lo"]), 8) + min(int(plan["n_hi"]), 8)
    out = np.zeros((nf, 2, n), "<i2")
    rc = load().igdsp_tdet_table(plan.ctypes.data_as(_vp), n, out.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_tdet_table")
    return out


def tdet_frame(plan, state, row):
    """igdsp_tdet_frame (host only, no GPU): one frame of one channel.  plan a TDET_PLAN record, state a TDET_STATE record updated in
    place, row the frame's PCM (int16 [n]).  Returns the frame's TDET_REC record."""
    assert plan.dtype == TDET_PLAN and state.dtype == TDET_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    row = np.ascontiguousarray(row, dtype=np.int16)
    rec = np.zeros((), TDET_REC)
    rc = load().igdsp_tdet_frame(plan.ctypes.data_as(_vp), state.ctypes.data_as(_vp), row.ctypes.data_as(_vp), len(row), rec.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_tdet_frame")
    return rec


def ec_cfg_default(tail: int = 128) -> np.ndarray:
    """igdsp_ec_cfg_default (host only, no GPU): one EC_CFG record, the defaults at this tail."""
    out = np.zeros((), EC_CFG)
    load().igdsp_ec_cfg_default(int(tail), out.ctypes.data_as(_vp))
    return out


def ec_frame(cfg, state, near, far=None, ctl: int = EC_RUN):
    """igdsp_ec_frame (host only, no GPU): one frame of one channel.  cfg an EC_CFG record or None (the defaults at tail 128), state an
    EC_STATE record updated in place, near and far the frame's PCM (int16 [n]; far None: no far end).  Returns (out int16 [n], the
    frame's EC_REC record)."""
    assert state.dtype == EC_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    near = np.ascontiguousarray(near, np.int16)
    far = None if far is None else np.ascontiguousarray(far, np.int16)
    assert far is None or len(far) == len(near)
    c = None if cfg is None else np.ascontiguousarray(cfg, EC_CFG)
    out = np.zeros(len(near), np.int16)
    rec = np.zeros((), EC_REC)
    rc = load().igdsp_ec_frame(None if c is None else c.ctypes.data_as(_vp), state.ctypes.data_as(_vp), near.ctypes.data_as(_vp),
                               None if far is None else far.ctypes.data_as(_vp), len(near), int(ctl), out.ctypes.data_as(_vp), rec.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_ec_frame")
    return out, rec


def agc_cfg_default() -> np.ndarray:
    """igdsp_agc_cfg_default (host only, no GPU): one AGC_CFG record, the defaults."""
    out = np.zeros((), AGC_CFG)
    load().igdsp_agc_cfg_default(out.ctypes.data_as(_vp))
    return out


def agc_frame(cfg, state, pcm, ctl: int = AGC_RUN):
    """igdsp_agc_frame (host only, no GPU): one frame of one channel.  cfg an AGC_CFG record or None (the defaults), state an AGC_STATE
    record updated in place, pcm the frame (int16 [n]).  Returns (out int16 [n], the frame's AGC_REC record)."""
    assert state.dtype == AGC_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    pcm = np.ascontiguousarray(pcm, np.int16)
    c = None if cfg is None else np.ascontiguousarray(cfg, AGC_CFG)
    out = np.zeros(len(pcm), np.int16)
    rec = np.zeros((), AGC_REC)
    rc = load().igdsp_agc_frame(None if c is None else c.ctypes.data_as(_vp), state.ctypes.data_as(_vp), pcm.ctypes.data_as(_vp), len(pcm), int(ctl),
                                out.ctypes.data_as(_vp), rec.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_agc_frame")
    return out, rec


def vad_cfg_default() -> np.ndarray:
    """igdsp_vad_cfg_default (host only, no GPU): one VAD_CFG record, the defaults."""
    out = np.zeros((), VAD_CFG)
    load().igdsp_vad_cfg_default(out.ctypes.data_as(_vp))
    return out


def vad_table() -> np.ndarray:
    """igdsp_vad_table (host only, no GPU): the 128 values of T8 as uint64."""
    out = np.zeros(128, "<u8")
    rc = load().igdsp_vad_table(out.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_vad_table")
    return out


def vad_frame(cfg, state, pcm, ctl: int = VAD_RUN):
    """igdsp_vad_frame (host only, no GPU): one frame of one channel.  cfg a VAD_CFG record or None (the defaults), state a VAD_STATE
    record updated in place, pcm the frame (int16 [n]).  Returns (kind, the frame's VAD_REC record, the payload's 16 bytes)."""
    assert state.dtype == VAD_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    pcm = np.ascontiguousarray(pcm, np.int16)
    c = None if cfg is None else np.ascontiguousarray(cfg, VAD_CFG)
    rec, sid = np.zeros((), VAD_REC), np.zeros(16, np.uint8)
    rc = load().igdsp_vad_frame(None if c is None else c.ctypes.data_as(_vp), state.ctypes.data_as(_vp), pcm.ctypes.data_as(_vp), len(pcm), int(ctl),
                                rec.ctypes.data_as(_vp), sid.ctypes.data_as(_vp))
    if rc < 0:
        raise IgdspError(rc, "igdsp_vad_frame")
    return rc, rec, sid


def sid_decode(payload):
    """igdsp_sid_decode (host only, no GPU): (level in -dBov, the ten Q15 reflection coefficients) of an RFC 3389 payload."""
    p = np.ascontiguousarray(payload, np.uint8)
    lvl, k = np.zeros(1, np.uint8), np.zeros(10, np.int16)
    rc = load().igdsp_sid_decode(p.ctypes.data_as(_vp), len(p), lvl.ctypes.data_as(_vp), k.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_sid_decode")
    return int(lvl[0]), k


def cng_table() -> np.ndarray:
    """igdsp_cng_table (host only, no GPU): the 128 values of G as uint32."""
    out = np.zeros(128, np.uint32)
    rc = load().igdsp_cng_table(out.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_cng_table")
    return out


def cng_gain(payload) -> int:
    """igdsp_cng_gain (host only, no GPU): g_tgt of an RFC 3389 payload of 1..16 bytes."""
    p = np.ascontiguousarray(payload, np.uint8)
    out = C.c_uint32(0)
    rc = load().igdsp_cng_gain(p.ctypes.data_as(_vp), len(p), C.byref(out))
    if rc != 0:
        raise IgdspError(rc, "igdsp_cng_gain")
    return int(out.value)


def cng_frame(state, kind: int, n: int, sid=None, sid_len: int = 11, voice=None, ctl: int = CNG_RUN, seed: int = 0):
    """igdsp_cng_frame (host only, no GPU): one frame of one channel.  state a CNG_STATE record updated in place, sid the payload
    (uint8, up to 16 bytes) or None, voice the leg's row (int16 [n]) or None.  Returns (out int16 [n], len_out, the frame's CNG_REC)."""
    assert state.dtype == CNG_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    p = None if sid is None else np.ascontiguousarray(sid, np.uint8)
    v = None if voice is None else np.ascontiguousarray(voice, np.int16)
    assert v is None or len(v) == n
    out, rec = np.zeros(n, np.int16), np.zeros((), CNG_REC)
    rc = load().igdsp_cng_frame(state.ctypes.data_as(_vp), int(kind), None if p is None else p.ctypes.data_as(_vp), int(sid_len),
                                None if v is None else v.ctypes.data_as(_vp), n, int(ctl), int(seed), out.ctypes.data_as(_vp), rec.ctypes.data_as(_vp))
    if rc < 0:
        raise IgdspError(rc, "igdsp_cng_frame")
    return out, rc, rec


def filt_frame(plan, state, pcm, ctl: int = FILT_RUN):
    """igdsp_filt_frame (host only, no GPU): one frame of one channel.  plan a FILT_PLAN record or None (a channel without a plan),
    state a FILT_STATE record updated in place, pcm the frame (int16 [n]).  Returns (out int16 [n], the frame's FILT_REC)."""
    assert state.dtype == FILT_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    pcm = np.ascontiguousarray(pcm, np.int16)
    p = None if plan is None else np.ascontiguousarray(plan, FILT_PLAN)
    out, rec = np.zeros(len(pcm), np.int16), np.zeros((), FILT_REC)
    rc = load().igdsp_filt_frame(None if p is None else p.ctypes.data_as(_vp), state.ctypes.data_as(_vp), pcm.ctypes.data_as(_vp), len(pcm), int(ctl),
                                 out.ctypes.data_as(_vp), rec.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_filt_frame")
    return out, rec


def filt_plan_check(plan) -> int:
    """igdsp_filt_plan_check (host only, no GPU): 0, or IGDSP_EINVAL for a plan the kernel would flag.  Returns the raw code."""
    p = np.ascontiguousarray(plan, FILT_PLAN)
    return int(load().igdsp_filt_plan_check(p.ctypes.data_as(_vp)))


def filt_design(kind: int, clock_rate: int, f0_hz: float, q: float = 0.7071067811865476, gain_db: float = 0.0) -> np.ndarray:
    """igdsp_filt_design (host only, no GPU): the section {b0, b1, b2, a1, a2} in Q13 as int16 [5]."""
    out = np.zeros(5, np.int16)
    rc = load().igdsp_filt_design(int(kind), int(clock_rate), float(f0_hz), float(q), float(gain_db), out.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_filt_design")
    return out


def filt_plan_preset(preset: int, clock_rate: int) -> np.ndarray:
    """igdsp_filt_plan_preset (host only, no GPU): the preset's FILT_PLAN record."""
    plan = np.zeros((), FILT_PLAN)
    rc = load().igdsp_filt_plan_preset(int(preset), int(clock_rate), plan.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_filt_plan_preset")
    return plan


def srtp_derive(key_salt, tag_len: int = 10, roc0: int = 0, raw: bool = False):
    """igdsp_srtp_derive (host only, no GPU): the 30 bytes of master key and salt -> one SRTP_STATE record (RFC 3711 4.3.1, labels 0, 1, 2;
    the key schedule of k_e, k_s, the two HMAC-SHA1 midstates of k_a); tag_len 4 or 10.  raw: the return code alone."""
    ks = np.frombuffer(bytes(key_salt), np.uint8).copy()
    assert ks.size == 30
    out = np.zeros((), SRTP_STATE)
    rc = load().igdsp_srtp_derive(ks.ctypes.data_as(_vp), int(tag_len), int(roc0) & 0xFFFFFFFF, out.ctypes.data_as(_vp))
    if raw:
        return int(rc)
    if rc != 0:
        raise IgdspError(rc, "igdsp_srtp_derive")
    return out


def srtp_packet(state, packet, unprotect: bool = False, ctl: int = SRTP_RUN, capacity: int = SRTP_MAX_PACKET, in_place: bool = False, fill: int = 0xA5):
    """igdsp_srtp_protect_packet / igdsp_srtp_unprotect_packet (host only, no GPU): one packet of one leg.  state an SRTP_STATE record
    updated in place, packet bytes.  Returns (the output buffer of `capacity` bytes, prefilled with `fill`, as a uint8 array, size_out,
    the packet's SRTP_REC record); in_place: the packet sits in that buffer and in == out."""
    assert state.dtype == SRTP_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    pkt = np.frombuffer(bytes(packet), np.uint8).copy()
    out = np.full(max(int(capacity), 1), fill, np.uint8)
    if in_place:
        assert pkt.size <= capacity
        out[:pkt.size] = pkt
    src = out if in_place else (pkt if pkt.size else np.zeros(1, np.uint8))
    size_out, rec = _u32(0), np.zeros((), SRTP_REC)
    fn = load().igdsp_srtp_unprotect_packet if unprotect else load().igdsp_srtp_protect_packet
    rc = fn(state.ctypes.data_as(_vp), int(ctl), src.ctypes.data_as(_vp), pkt.size, out.ctypes.data_as(_vp), int(capacity), C.byref(size_out),
            rec.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_srtp_unprotect_packet" if unprotect else "igdsp_srtp_protect_packet")
    return out, int(size_out.value), rec


def srtp_gcm_derive(key_salt, key_bytes: int = None, roc0: int = 0, raw: bool = False):
    """igdsp_srtp_gcm_derive (host only, no GPU): key_bytes (16 or 32; default: what the length says) of master key and 12 of master salt
    -> one SRTP_GCM_STATE record (RFC 3711 4.3.1 with AES of the key's size, labels 0 and 2; the key schedule of k_e, k_s, H).  raw: the
    return code alone."""
    ks = np.frombuffer(bytes(key_salt), np.uint8).copy()
    key_bytes = ks.size - 12 if key_bytes is None else int(key_bytes)
    assert ks.size == key_bytes + 12 or key_bytes not in (16, 32)          # (a key size that is none is refused before a byte is read)
    out = np.zeros((), SRTP_GCM_STATE)
    rc = load().igdsp_srtp_gcm_derive(ks.ctypes.data_as(_vp), key_bytes, int(roc0) & 0xFFFFFFFF, out.ctypes.data_as(_vp))
    if raw:
        return int(rc)
    if rc != 0:
        raise IgdspError(rc, "igdsp_srtp_gcm_derive")
    return out


def srtp_gcm_packet(state, packet, unprotect: bool = False, ctl: int = SRTP_RUN, capacity: int = SRTP_MAX_PACKET, in_place: bool = False, fill: int = 0xA5):
    """igdsp_srtp_gcm_protect_packet / igdsp_srtp_gcm_unprotect_packet (host only, no GPU): one packet of one leg; state an SRTP_GCM_STATE
    record updated in place; arguments and return as srtp_packet."""
    assert state.dtype == SRTP_GCM_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    pkt = np.frombuffer(bytes(packet), np.uint8).copy()
    out = np.full(max(int(capacity), 1), fill, np.uint8)
    if in_place:
        assert pkt.size <= capacity
        out[:pkt.size] = pkt
    src = out if in_place else (pkt if pkt.size else np.zeros(1, np.uint8))
    size_out, rec = _u32(0), np.zeros((), SRTP_REC)
    fn = load().igdsp_srtp_gcm_unprotect_packet if unprotect else load().igdsp_srtp_gcm_protect_packet
    rc = fn(state.ctypes.data_as(_vp), int(ctl), src.ctypes.data_as(_vp), pkt.size, out.ctypes.data_as(_vp), int(capacity), C.byref(size_out),
            rec.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_srtp_gcm_unprotect_packet" if unprotect else "igdsp_srtp_gcm_protect_packet")
    return out, int(size_out.value), rec


def srtcp_derive(key_salt, index0: int = 0):
    """igdsp_srtcp_derive (host only, no GPU): the 30 bytes of master key and salt -> one SRTP_STATE record for SRTCP (RFC 3711 4.3.1, labels
    3, 4, 5; the tag word SRTCP_TAG | 10); roc holds the 31-bit index, index0 the first a protecting leg sends."""
    ks = np.frombuffer(bytes(key_salt), np.uint8).copy()
    assert ks.size == 30
    out = np.zeros((), SRTP_STATE)
    rc = load().igdsp_srtcp_derive(ks.ctypes.data_as(_vp), int(index0) & 0xFFFFFFFF, out.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_srtcp_derive")
    return out


def srtcp_packet(state, packet, unprotect: bool = False, ctl: int = SRTP_RUN, capacity: int = SRTP_MAX_PACKET, in_place: bool = False, fill: int = 0xA5):
    """igdsp_srtcp_protect_packet / igdsp_srtcp_unprotect_packet (host only, no GPU): one packet of one leg; arguments and return as
    srtp_packet."""
    assert state.dtype == SRTP_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    pkt = np.frombuffer(bytes(packet), np.uint8).copy()
    out = np.full(max(int(capacity), 1), fill, np.uint8)
    if in_place:
        assert pkt.size <= capacity
        out[:pkt.size] = pkt
    src = out if in_place else (pkt if pkt.size else np.zeros(1, np.uint8))
    size_out, rec = _u32(0), np.zeros((), SRTP_REC)
    fn = load().igdsp_srtcp_unprotect_packet if unprotect else load().igdsp_srtcp_protect_packet
    rc = fn(state.ctypes.data_as(_vp), int(ctl), src.ctypes.data_as(_vp), pkt.size, out.ctypes.data_as(_vp), int(capacity), C.byref(size_out),
            rec.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_srtcp_unprotect_packet" if unprotect else "igdsp_srtcp_protect_packet")
    return out, int(size_out.value), rec


def rtcp_build_packet(state, ctl: int, src, now: int, jb=None, cname=None, capacity: int = RTCP_MAX_BUILT, fill: int = 0xA5, raw: bool = False):
    """igdsp_rtcp_build_packet (host only, no GPU): one report of one leg.  state an RTCP_STATE record updated in place, src an RTCP_SRC
    record, now the 64-bit NTP time, jb a JB_STATE record or None, cname bytes or None.  Returns (the output buffer of `capacity` bytes
    prefilled with `fill`, the size, the RTCP_BUILT record); raw: the return code alone."""
    assert state.dtype == RTCP_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    s = np.ascontiguousarray(np.asarray(src, dtype=RTCP_SRC).reshape(()))
    j = None if jb is None else np.ascontiguousarray(np.asarray(jb, dtype=JB_STATE).reshape(()))
    cn = None if cname is None else np.frombuffer(bytes(cname) + b"\0", np.uint8).copy()
    out = np.full(max(int(capacity), 1), fill, np.uint8)
    size_out, rec = _u32(0), np.zeros((), RTCP_BUILT)
    rc = load().igdsp_rtcp_build_packet(state.ctypes.data_as(_vp), int(ctl), None if j is None else j.ctypes.data_as(_vp), s.ctypes.data_as(_vp), int(now),
                                        None if cn is None else cn.ctypes.data_as(_vp), 0 if cname is None else len(cname), out.ctypes.data_as(_vp),
                                        int(capacity), C.byref(size_out), rec.ctypes.data_as(_vp))
    if raw:
        return int(rc)
    if rc != 0:
        raise IgdspError(rc, "igdsp_rtcp_build_packet")
    return out, int(size_out.value), rec


def rtcp_parse_packet(state, packet, arrival: int, local_ssrc: int):
    """igdsp_rtcp_parse_packet (host only, no GPU): one received compound packet of one leg.  state an RTCP_STATE record updated in place;
    arrival the arrival time's middle 32 NTP bits.  Returns the RTCP_SEEN record."""
    assert state.dtype == RTCP_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    pkt = np.frombuffer(bytes(packet), np.uint8).copy()
    rec = np.zeros((), RTCP_SEEN)
    rc = load().igdsp_rtcp_parse_packet(state.ctypes.data_as(_vp), pkt.ctypes.data_as(_vp) if pkt.size else None, pkt.size, int(arrival) & 0xFFFFFFFF,
                                        int(local_ssrc) & 0xFFFFFFFF, rec.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_rtcp_parse_packet")
    return rec


def ns_cfg_default() -> np.ndarray:
    """igdsp_ns_cfg_default (host only, no GPU): one NS_CFG record, the defaults."""
    out = np.zeros((), NS_CFG)
    load().igdsp_ns_cfg_default(out.ctypes.data_as(_vp))
    return out


def ns_tables():
    """igdsp_ns_tables (host only, no GPU): the committed window (int16 [160]) and twiddle factors (int32 [128][2]: cos, sin in Q30)."""
    w, t = _vp(), _vp()
    rc = load().igdsp_ns_tables(C.byref(w), C.byref(t))
    if rc != 0:
        raise IgdspError(rc, "igdsp_ns_tables")
    win = np.ctypeslib.as_array(C.cast(w, C.POINTER(C.c_int16)), (2 * NS_HOP,)).copy()
    tw = np.ctypeslib.as_array(C.cast(t, C.POINTER(C.c_int32)), (256,)).copy()
    return win, tw.reshape(128, 2)


def ns_frame(cfg, state, pcm, ctl: int = NS_RUN, raw: bool = False):
    """igdsp_ns_frame (host only, no GPU): one frame of one channel.  cfg an NS_CFG record, state an NS_STATE record updated in place,
    pcm the frame (int16 [80, 160, 240 or 320]).  Returns (out int16 [n], the frame's NS_REC record); raw: the return code alone."""
    assert state.dtype == NS_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    pcm = np.ascontiguousarray(pcm, np.int16)
    c = np.ascontiguousarray(cfg, NS_CFG)
    out, rec = np.zeros(len(pcm), np.int16), np.zeros((), NS_REC)
    rc = load().igdsp_ns_frame(c.ctypes.data_as(_vp), state.ctypes.data_as(_vp), pcm.ctypes.data_as(_vp), len(pcm), int(ctl), out.ctypes.data_as(_vp),
                               rec.ctypes.data_as(_vp))
    if raw:
        return int(rc)
    if rc != 0:
        raise IgdspError(rc, "igdsp_ns_frame")
    return out, rec


def vad_work_bytes(n_channels: int, n_frames: int, with_rec: bool) -> int:
    """igdsp_vad_work_bytes (host only, no GPU): bytes of igdsp_vad_run's d_work for a launch of this shape."""
    return int(load().igdsp_vad_work_bytes(n_channels, n_frames, 1 if with_rec else 0))


def tdet_work_bytes(n_channels: int, n_frames: int, with_rec: bool) -> int:
    """igdsp_tdet_work_bytes (host only, no GPU): bytes of igdsp_tone_detect's d_work for a launch of this shape."""
    return int(load().igdsp_tdet_work_bytes(n_channels, n_frames, 1 if with_rec else 0))


def spec_tables():
    """igdsp_spec_tables (host only, no GPU): the committed window (float32 [1024]) and twiddle factors (float32 [1024][2]: cos, -sin)."""
    w, t = _vp(), _vp()
    rc = load().igdsp_spec_tables(C.byref(w), C.byref(t))
    if rc != 0:
        raise IgdspError(rc, "igdsp_spec_tables")
    win = np.ctypeslib.as_array(C.cast(w, C.POINTER(C.c_float)), (SPEC_N,)).copy()
    tw = np.ctypeslib.as_array(C.cast(t, C.POINTER(C.c_float)), (2 * SPEC_N,)).copy()
    return win, tw.reshape(SPEC_N, 2)


def rs_frame(state, direction: int, factor: int, x) -> np.ndarray:
    """igdsp_rs_frame (host only, no GPU): one frame of one channel.  state an RS_STATE record updated in place, x the frame's input
    (int16: n for RS_UP, n * factor for RS_DOWN).  Returns the output samples (n * factor / n)."""
    assert state.dtype == RS_STATE and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]
    x = np.ascontiguousarray(x, np.int16)
    out = np.zeros(len(x) * factor if direction == RS_UP else len(x) // max(factor, 1), np.int16)
    rc = load().igdsp_rs_frame(state.ctypes.data_as(_vp), direction, factor, x.ctypes.data_as(_vp), len(x), out.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_rs_frame")
    return out


def jb_report(state, prior) -> np.ndarray:
    """igdsp_jb_report (host only, no GPU): the RFC 3550 receiver-report fields of one JB_STATE record; advances prior (a JB_PRIOR
    record, updated in place) and returns a JB_RR record."""
    st = np.ascontiguousarray(np.asarray(state, dtype=JB_STATE).reshape(()))
    assert prior.dtype == JB_PRIOR and prior.flags["C_CONTIGUOUS"]
    out = np.zeros((), dtype=JB_RR)
    rc = load().igdsp_jb_report(st.ctypes.data_as(_vp), prior.ctypes.data_as(_vp), out.ctypes.data_as(_vp))
    if rc != 0:
        raise IgdspError(rc, "igdsp_jb_report")
    return out


def jb_adapt_cfg_default() -> np.ndarray:
    """igdsp_jb_adapt_cfg_default (host only, no GPU): the default JB_ADAPT_CFG record."""
    cfg = np.zeros((), dtype=JB_ADAPT_CFG)
    load().igdsp_jb_adapt_cfg_default(cfg.ctypes.data_as(_vp))
    return cfg


def _jb_cfg(cfg) -> np.ndarray | None:
    """a JB_ADAPT_CFG record from a record, a (min, max, init, mult, late_restart) sequence or None"""
    if cfg is None:
        return None
    if isinstance(cfg, np.ndarray) and cfg.dtype == JB_ADAPT_CFG:
        return np.ascontiguousarray(cfg.reshape(()))
    out = np.zeros((), dtype=JB_ADAPT_CFG)
    out["min_frames"], out["max_frames"], out["init_frames"], out["jitter_mult"], out["late_restart"] = cfg
    return out


def jb_adapt_next(cfg, jitter_q4: int, n: int, adapt) -> int:
    """igdsp_jb_adapt_next (host only, no GPU): the Start rule of igdsp_jb_receive_adaptive for one channel: cfg (a JB_ADAPT_CFG record,
    a (min, max, init, mult, late_restart) sequence or None for the defaults), the state's jitter (scaled by 16), n samples per frame;
    adapt (a JB_ADAPT record) is updated in place.  Returns the new delay."""
    c = _jb_cfg(cfg)
    assert adapt.dtype == JB_ADAPT and adapt.flags["C_CONTIGUOUS"]
    rc = load().igdsp_jb_adapt_next(None if c is None else c.ctypes.data_as(_vp), jitter_q4, n, adapt.ctypes.data_as(_vp))
    if rc < 0:
        raise IgdspError(rc, "igdsp_jb_adapt_next")
    return rc


def _ptr(x) -> int | None:
    """device pointer of a torch tensor / raw int / None."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    return x.data_ptr()


class Context:
    """RAII wrapper over ``igdsp_ctx``.  ``stream`` arguments are raw ``hipStream_t`` integers."""

    def __init__(self, device: int = 0, max_channels: int = 4096):
        self.L = load()
        h = _vp()
        rc = self.L.igdsp_create(C.byref(h), device, max_channels)
        if rc != 0:
            raise IgdspError(rc, "igdsp_create", "no usable gfx950 device" if rc == -19 else "")
        self.h = h
        self.max_channels = max_channels

    # -- helpers
    def _ck(self, rc: int, where: str):
        if rc != 0:
            raise IgdspError(rc, where, (self.L.igdsp_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.igdsp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def device_info(self):
        dev, cus = _int(), _int()
        name = C.create_string_buffer(128)
        self._ck(self.L.igdsp_device_info(self.h, C.byref(dev), C.byref(cus), name, 128), "igdsp_device_info")
        return {"device": dev.value, "compute_units": cus.value, "name": name.value.decode()}

    def set_variant(self, v: int):
        self._ck(self.L.igdsp_set_variant(self.h, v), "igdsp_set_variant")

    # -- single-frame path (mirrors setIncomingRTP / setOutgoingRTP inputs)
    def map_call(self, call_id: int, channel: int):
        self._ck(self.L.igdsp_map_call(self.h, call_id, channel), "igdsp_map_call")

    def unmap_call(self, call_id: int):
        self._ck(self.L.igdsp_unmap_call(self.h, call_id), "igdsp_unmap_call")

    def on_rtp_frame(self, call_id: int, pt: int, payload: bytes) -> int:
        buf = (C.c_uint8 * len(payload)).from_buffer_copy(payload) if payload else None
        return self.L.igdsp_on_rtp_frame(self.h, call_id, pt, C.cast(buf, _vp) if buf is not None else None, len(payload))

    def flush(self) -> int:
        n = _u32()
        self._ck(self.L.igdsp_flush(self.h, C.byref(n)), "igdsp_flush")
        return n.value

    def flush_begin(self) -> int:
        n = _u32()
        self._ck(self.L.igdsp_flush_begin(self.h, C.byref(n)), "igdsp_flush_begin")
        return n.value

    def flush_end(self, wait: bool = True) -> int:
        """0 when the flush has been published, IGDSP_EBUSY (-16) when wait is False and the device has not finished."""
        rc = self.L.igdsp_flush_end(self.h, 1 if wait else 0)
        if rc not in (0, -16):
            self._ck(rc, "igdsp_flush_end")
        return rc

    def set_ed137(self, call_id: int, value: int):
        self._ck(self.L.igdsp_set_ed137(self.h, call_id, value & 0xFFFFFFFF), "igdsp_set_ed137")

    def set_gate_mode(self, mode: int):
        self._ck(self.L.igdsp_set_gate_mode(self.h, mode), "igdsp_set_gate_mode")

    def get_probe(self, channel: int) -> ChanProbe:
        p = ChanProbe()
        self._ck(self.L.igdsp_get_probe(self.h, channel, C.byref(p)), "igdsp_get_probe")
        return p

    def poll(self, channel: int) -> Level:
        lv = Level()
        self._ck(self.L.igdsp_poll(self.h, channel, C.byref(lv)), "igdsp_poll")
        return lv

    def poll_call(self, call_id: int) -> Level:
        lv = Level()
        self._ck(self.L.igdsp_poll_call(self.h, call_id, C.byref(lv)), "igdsp_poll_call")
        return lv

    def reset_hold(self, channel: int = 0xFFFFFFFF):
        self._ck(self.L.igdsp_reset_hold(self.h, channel), "igdsp_reset_hold")

    def get_hold(self, channel: int) -> np.ndarray:
        out = np.zeros((), dtype=CHAN_HOLD)
        self._ck(self.L.igdsp_get_hold(self.h, channel, out.ctypes.data_as(_vp)), "igdsp_get_hold")
        return out

    # -- batched device entries
    def decode_meter(self, payload, codec, C_, F_, n, stats, pcm=None, length=None, agg=None, rank=0, stream=None):
        self._ck(self.L.igdsp_decode_meter(self.h, _ptr(payload), _ptr(codec), _ptr(length), C_, F_, n, _ptr(stats),
                                           _ptr(pcm), _ptr(agg), rank, stream), "igdsp_decode_meter")

    def encode(self, pcm, codec, C_, F_, n, out, variant=ENC_G191, stream=None):
        self._ck(self.L.igdsp_encode(self.h, _ptr(pcm), _ptr(codec), C_, F_, n, _ptr(out), variant, stream), "igdsp_encode")

    def roundtrip_peakhold(self, payload, codec, C_, F_, n, out, stats, hold, gate=None, variant=ENC_G191, stream=None):
        self._ck(self.L.igdsp_roundtrip_peakhold(self.h, _ptr(payload), _ptr(codec), C_, F_, n, _ptr(out), _ptr(stats),
                                                 _ptr(hold), _ptr(gate), variant, stream), "igdsp_roundtrip_peakhold")

    def hold_update(self, stats, C_, F_, n, hold, gate=None, stream=None):
        self._ck(self.L.igdsp_hold_update(self.h, _ptr(stats), C_, F_, n, _ptr(hold), _ptr(gate), stream), "igdsp_hold_update")

    def hold_reset(self, hold, C_, mask=None, stream=None):
        self._ck(self.L.igdsp_hold_reset(self.h, _ptr(hold), C_, _ptr(mask), stream), "igdsp_hold_reset")

    def agg_reset(self, agg, stream=None):
        self._ck(self.L.igdsp_agg_reset(self.h, _ptr(agg), stream), "igdsp_agg_reset")

    def depayload(self, packets, sizes, radio, C_, F_, stride, n, payload_out, len_out, info_out, stream=None):
        self._ck(self.L.igdsp_depayload(self.h, _ptr(packets), _ptr(sizes), _ptr(radio), C_, F_, stride, n, _ptr(payload_out),
                                        _ptr(len_out), _ptr(info_out), stream), "igdsp_depayload")

    def decode_meter_rtp(self, slots, codec, C_, F_, stats, info=None, agg=None, rank=0, stream=None):
        self._ck(self.L.igdsp_decode_meter_rtp(self.h, _ptr(slots), _ptr(codec), C_, F_, _ptr(stats), _ptr(info), _ptr(agg), rank, stream),
                 "igdsp_decode_meter_rtp")

    def decode_meter_packets(self, packets, sizes, codec, C_, F_, stride, hdr, stats, info=None, agg=None, rank=0, stream=None):
        self._ck(self.L.igdsp_decode_meter_packets(self.h, _ptr(packets), _ptr(sizes), _ptr(codec), C_, F_, stride, hdr, _ptr(stats),
                                                   _ptr(info), _ptr(agg), rank, stream), "igdsp_decode_meter_packets")

    def decode_meter_packets_mixed(self, packets, sizes, codec, radio, C_, F_, stride, stats, info=None, agg=None, rank=0, stream=None):
        self._ck(self.L.igdsp_decode_meter_packets_mixed(self.h, _ptr(packets), _ptr(sizes), _ptr(codec), _ptr(radio), C_, F_, stride,
                                                         _ptr(stats), _ptr(info), _ptr(agg), rank, stream), "igdsp_decode_meter_packets_mixed")

    def tx_packetize(self, state, last_payload, packets, stride, sizes, info, C_, F_, n, t0_ms, frame_ms=20, pcm=None, g711=None,
                     ctl=None, variant=ENC_G191, stream=None):
        """igdsp_tx_packetize: exactly one of pcm [F][C][n] int16 / g711 [F][C][n] u8 (device)."""
        self._ck(self.L.igdsp_tx_packetize(self.h, _ptr(pcm), _ptr(g711), _ptr(ctl), C_, F_, n, t0_ms, frame_ms, _ptr(state),
                                           _ptr(last_payload), _ptr(packets), stride, _ptr(sizes), _ptr(info), variant, stream),
                 "igdsp_tx_packetize")

    def conf_mix(self, gain, port_ptr, members, n_members, C_, P_, F_, n, out=None, stats=None, payload=None, codec=None, pcm=None,
                 length=None, stream=None):
        """igdsp_conf_mix: exactly one of payload [F][C][n] u8 (+ codec [C]) / pcm [F][C][n] int16; out [F][P][n] int16 and / or
        stats [F][P] (device buffers)."""
        self._ck(self.L.igdsp_conf_mix(self.h, _ptr(payload), _ptr(codec), _ptr(pcm), _ptr(length), _ptr(gain), _ptr(port_ptr), _ptr(members),
                                       n_members, C_, P_, F_, n, _ptr(out), _ptr(stats), stream), "igdsp_conf_mix")

    def snd_combine(self, pcm, D_, K_, F_, n=SAMPLES_PER_FRAME, frames=None, stats=None, stream=None):
        """igdsp_snd_combine: pcm [F][D * K][n] int16 -> frames [F][D][n][K] int16 and / or stats [F][D * K] FRAME_STATS (the out VU)."""
        self._ck(self.L.igdsp_snd_combine(self.h, _ptr(pcm), D_, K_, F_, n, _ptr(frames), _ptr(stats), stream), "igdsp_snd_combine")

    def snd_split(self, frames, D_, K_, F_, n=SAMPLES_PER_FRAME, pcm=None, stats=None, stream=None):
        """igdsp_snd_split: frames [F][D][n][K] int16 -> pcm [F][D * K][n] int16 and / or stats [F][D * K] FRAME_STATS (the in VU)."""
        self._ck(self.L.igdsp_snd_split(self.h, _ptr(frames), D_, K_, F_, n, _ptr(pcm), _ptr(stats), stream), "igdsp_snd_split")

    def tone_generate(self, plans, n_plans, state, P_, F_, n=SAMPLES_PER_FRAME, plan_of=None, cmd=None, rows_per_frame=0, pcm=None, length=None,
                      stats=None, stream=None):
        """igdsp_tone_generate: plans [n_plans] TONE_PLAN, state [P] TONE_STATE (in and out), plan_of [P] u16 / None (plan 0), cmd [P] u8 /
        None -> pcm [F][rows_per_frame or P][n] int16 rows [0, P) of each frame, length likewise u16, stats [F][P] FRAME_STATS."""
        self._ck(self.L.igdsp_tone_generate(self.h, _ptr(plans), n_plans, _ptr(plan_of), _ptr(cmd), _ptr(state), P_, F_, n, rows_per_frame,
                                            _ptr(pcm), _ptr(length), _ptr(stats), stream), "igdsp_tone_generate")

    def resample(self, direction, factor, state, C_, F_, n=SAMPLES_PER_FRAME, layout=RS_ROWS, payload=None, codec=None, pcm=None, length=None,
                 rows_narrow=0, rows_wide=0, out=None, stats=None, stream=None):
        """igdsp_resample: RS_UP takes payload [F][C][n] u8 (+ codec [C]) or pcm [F][rows_narrow or C][n] int16 to the wide side, RS_DOWN takes
        pcm from the wide side to [F][rows_narrow or C][n]; the wide side is [F][rows_wide or C][n * factor] (RS_ROWS) or
        [F * factor][rows_wide or C][n] (RS_SUBFRAMES); state [C] RS_STATE (in and out); stats dense, one per output row."""
        self._ck(self.L.igdsp_resample(self.h, direction, factor, layout, _ptr(payload), _ptr(codec), _ptr(pcm), _ptr(length), _ptr(state), C_, F_, n,
                                       rows_narrow, rows_wide, _ptr(out), _ptr(stats), stream), "igdsp_resample")

    def dbuf_run(self, ops, pcm, state, C_, T_, n, max_samples, out, flags=None, length=None, fill=None, stats=None, stream=None):
        """igdsp_dbuf_run: ops [T][C] u8 (DBUF_PUT | DBUF_GET), pcm [T][C][n] int16 (rows of PUT steps), state [C] DBUF_STATE (in and out)
        -> out [T][C][n] int16 (rows of GET steps), flags [T][C] u8, length [T][C] u16, fill [T][C] u16, stats [T][C] FRAME_STATS."""
        self._ck(self.L.igdsp_dbuf_run(self.h, _ptr(ops), _ptr(pcm), C_, T_, n, max_samples, _ptr(state), _ptr(out), _ptr(flags), _ptr(length),
                                       _ptr(fill), _ptr(stats), stream), "igdsp_dbuf_run")

    def spectrum(self, state, C_, F_, n, g711=None, codec=None, pcm=None, cfg=None, rec=None, avg=None, raw=None, stream=None):
        """igdsp_spectrum: exactly one of g711 [F][C][n] u8 (+ codec [C]) / pcm [F][C][n] int16; state [C] SPEC_STATE (in and out); cfg a
        SpecCfg, a (hop_frames, alpha) pair or None (1, 0.25) -> rec [F][C] SPEC_REC, avg [C][512] f32, raw [C][512] f32 (each optional)."""
        c = _spec_cfg(cfg)
        self._ck(self.L.igdsp_spectrum(self.h, _ptr(g711), _ptr(codec), _ptr(pcm), C_, F_, n, None if c is None else C.cast(C.pointer(c), _vp),
                                       _ptr(state), _ptr(rec), _ptr(avg), _ptr(raw), stream), "igdsp_spectrum")

    def tone_detect(self, plans, state, C_, F_, n, g711=None, codec=None, pcm=None, n_plans=1, plan_of=None, event_mask=0, rec=None, events=None,
                    event_cap=0, event_count=None, work=None, stream=None):
        """igdsp_tone_detect: exactly one of g711 [F][C][n] u8 (+ codec [C]) / pcm [F][C][n] int16; plans [n_plans] TDET_PLAN, plan_of [C]
        u16 or None (plan 0); state [C] TDET_STATE (in and out) -> rec [F][C] TDET_REC, events [event_cap] TDET_EVENT with event_count [2]
        u32 and work (tdet_work_bytes), each optional."""
        self._ck(self.L.igdsp_tone_detect(self.h, _ptr(g711), _ptr(codec), _ptr(pcm), _ptr(plans), n_plans, _ptr(plan_of), C_, F_, n, event_mask,
                                          _ptr(state), _ptr(rec), _ptr(events), event_cap, _ptr(event_count), _ptr(work), stream), "igdsp_tone_detect")

    def echo_cancel(self, far, n_far_rows, state, C_, F_, n, g711=None, codec=None, pcm=None, far_of=None, ctl=None, cfg=None, out=None, rec=None,
                    stats=None, stream=None):
        """igdsp_echo_cancel: exactly one of g711 [F][C][n] u8 (+ codec [C]) / pcm [F][C][n] int16 (the near end); far [F][n_far_rows][n]
        int16, far_of [C] u32 or None (row c), ctl [C] u8 or None (EC_RUN); cfg an EC_CFG record (host memory) or None (the defaults at
        tail 128); state [C] EC_STATE (in and out) -> out [F][C][n] int16, rec [F][C] EC_REC, stats [F][C] FRAME_STATS, each optional."""
        c = None if cfg is None else np.ascontiguousarray(cfg, EC_CFG)
        self._ck(self.L.igdsp_echo_cancel(self.h, _ptr(g711), _ptr(codec), _ptr(pcm), _ptr(far), n_far_rows, _ptr(far_of), _ptr(ctl),
                                          None if c is None else c.ctypes.data_as(_vp), C_, F_, n, _ptr(state), _ptr(out), _ptr(rec), _ptr(stats),
                                          stream), "igdsp_echo_cancel")

    def agc_run(self, state, C_, F_, n, g711=None, codec=None, pcm=None, ctl=None, cfg=None, out=None, rec=None, stats=None, stream=None):
        """igdsp_agc_run: exactly one of g711 [F][C][n] u8 (+ codec [C]) / pcm [F][C][n] int16; ctl [C] u8 or None (AGC_RUN); cfg an
        AGC_CFG record (host memory) or None (the defaults); state [C] AGC_STATE (in and out) -> out [F][C][n] int16, rec [F][C] AGC_REC,
        stats [F][C] FRAME_STATS, each optional, at least one."""
        c = None if cfg is None else np.ascontiguousarray(cfg, AGC_CFG)
        self._ck(self.L.igdsp_agc_run(self.h, _ptr(g711), _ptr(codec), _ptr(pcm), _ptr(ctl), None if c is None else c.ctypes.data_as(_vp), C_, F_, n,
                                      _ptr(state), _ptr(out), _ptr(rec), _ptr(stats), stream), "igdsp_agc_run")

    def vad_run(self, state, C_, F_, n, g711=None, codec=None, pcm=None, ctl=None, cfg=None, event_mask=0, kind=None, rec=None, sid=None, txctl=None,
                events=None, event_cap=0, event_count=None, work=None, stream=None):
        """igdsp_vad_run: exactly one of g711 [F][C][n] u8 (+ codec [C]) / pcm [F][C][n] int16; ctl [C] u8 or None (VAD_RUN); cfg a VAD_CFG
        record (host memory) or None (the defaults); state [C] VAD_STATE (in and out) -> kind [F][C] u8, rec [F][C] VAD_REC, sid [F][C][16]
        u8, txctl [F][C] u8, events [event_cap] VAD_EVENT with event_count [2] u32 and work (vad_work_bytes), each optional, at least one."""
        c = None if cfg is None else np.ascontiguousarray(cfg, VAD_CFG)
        self._ck(self.L.igdsp_vad_run(self.h, _ptr(g711), _ptr(codec), _ptr(pcm), _ptr(ctl), None if c is None else c.ctypes.data_as(_vp), C_, F_, n,
                                      event_mask, _ptr(state), _ptr(kind), _ptr(rec), _ptr(sid), _ptr(txctl), _ptr(events), event_cap,
                                      _ptr(event_count), _ptr(work), stream), "igdsp_vad_run")

    def cng_run(self, kind, sid, state, out, C_, F_, n, sid_len=None, g711=None, codec=None, pcm=None, ctl=None, seed=None, len_out=None, rec=None,
                stats=None, stream=None):
        """igdsp_cng_run: kind [F][C] u8 and sid [F][C][16] u8 as igdsp_vad_run writes them, sid_len [F][C] u8 or None (11); at most one of
        g711 [F][C][n] u8 (+ codec [C]) / pcm [F][C][n] int16; ctl [C] u8 or None (CNG_RUN); seed [C] u32 or None; state [C] CNG_STATE (in and
        out) -> out [F][C][n] int16, len_out [F][C] u16, rec [F][C] CNG_REC, stats [F][C] FRAME_STATS (the last three optional)."""
        self._ck(self.L.igdsp_cng_run(self.h, _ptr(kind), _ptr(sid), _ptr(sid_len), _ptr(g711), _ptr(codec), _ptr(pcm), _ptr(ctl), _ptr(seed), C_, F_, n,
                                      _ptr(state), _ptr(out), _ptr(len_out), _ptr(rec), _ptr(stats), stream), "igdsp_cng_run")

    def filt_run(self, plans, n_plans, state, C_, F_, n, g711=None, codec=None, pcm=None, ctl=None, plan_of=None, max_sections=0, out=None, rec=None,
                 stats=None, stream=None):
        """igdsp_filt_run: exactly one of g711 [F][C][n] u8 (+ codec [C]) / pcm [F][C][n] int16; plans [n_plans] FILT_PLAN (device memory),
        plan_of [C] u16 or None (plan 0), ctl [C] u8 or None (FILT_RUN); max_sections the largest n_sections among the plans (0: 4); state
        [C] FILT_STATE (in and out) -> out [F][C][n] int16, rec [F][C] FILT_REC, stats [F][C] FRAME_STATS, each optional, at least one."""
        self._ck(self.L.igdsp_filt_run(self.h, _ptr(g711), _ptr(codec), _ptr(pcm), _ptr(ctl), _ptr(plans), n_plans, _ptr(plan_of), max_sections, C_, F_, n,
                                       _ptr(state), _ptr(out), _ptr(rec), _ptr(stats), stream), "igdsp_filt_run")

    def ns_run(self, state, C_, F_, n, g711=None, codec=None, pcm=None, ctl=None, cfg=None, out=None, rec=None, stats=None, stream=None):
        """igdsp_ns_run: exactly one of g711 [F][C][n] u8 (+ codec [C]) / pcm [F][C][n] int16 at 8 kHz, n 80, 160, 240 or 320; ctl [C] u8 or
        None (NS_RUN); cfg an NS_CFG record (host memory) or None (ns_cfg_default()); state [C] NS_STATE (in and out) -> out [F][C][n] int16
        (the input delayed by 80 samples), rec [F][C] NS_REC, stats [F][C] FRAME_STATS, each optional, at least one."""
        c = np.ascontiguousarray(ns_cfg_default() if cfg is None else cfg, NS_CFG)
        self._ck(self.L.igdsp_ns_run(self.h, _ptr(g711), _ptr(codec), _ptr(pcm), _ptr(ctl), c.ctypes.data_as(_vp), C_, F_, n, _ptr(state), _ptr(out),
                                     _ptr(rec), _ptr(stats), stream), "igdsp_ns_run")

    def srtp_protect(self, state, packets, sizes, C_, F_, pkt_stride, out, out_stride, sizes_out, rec=None, ctl=None, unprotect=False, stream=None):
        """igdsp_srtp_protect (unprotect: igdsp_srtp_unprotect): packets [F][C][pkt_stride] u8 + sizes [F][C] u16 (what tx_packetize writes,
        depayload / jb_receive read); ctl [F][C] u8 or None (SRTP_RUN); state [C] SRTP_STATE (in and out) -> out [F][C][out_stride] u8,
        sizes_out [F][C] u16, rec [F][C] SRTP_REC (optional).  In place: out is packets with equal strides, sizes_out is sizes."""
        fn, name = (self.L.igdsp_srtp_unprotect, "igdsp_srtp_unprotect") if unprotect else (self.L.igdsp_srtp_protect, "igdsp_srtp_protect")
        self._ck(fn(self.h, _ptr(ctl), _ptr(packets), _ptr(sizes), C_, F_, pkt_stride, _ptr(state), _ptr(out), out_stride, _ptr(sizes_out), _ptr(rec), stream), name)

    def srtp_unprotect(self, state, packets, sizes, C_, F_, pkt_stride, out, out_stride, sizes_out, rec=None, ctl=None, stream=None):
        """igdsp_srtp_unprotect: sizes include the tag; a refused packet gets size 0 and its output slot is not written."""
        self.srtp_protect(state, packets, sizes, C_, F_, pkt_stride, out, out_stride, sizes_out, rec=rec, ctl=ctl, unprotect=True, stream=stream)

    def srtp_gcm_protect(self, state, packets, sizes, C_, F_, pkt_stride, out, out_stride, sizes_out, rec=None, ctl=None, unprotect=False, stream=None):
        """igdsp_srtp_gcm_protect (unprotect: igdsp_srtp_gcm_unprotect): srtp_protect's arguments; state [C] SRTP_GCM_STATE from
        srtp_gcm_derive, key sizes side by side allowed; a protected packet is 16 bytes longer."""
        fn, name = (self.L.igdsp_srtp_gcm_unprotect, "igdsp_srtp_gcm_unprotect") if unprotect else (self.L.igdsp_srtp_gcm_protect, "igdsp_srtp_gcm_protect")
        self._ck(fn(self.h, _ptr(ctl), _ptr(packets), _ptr(sizes), C_, F_, pkt_stride, _ptr(state), _ptr(out), out_stride, _ptr(sizes_out), _ptr(rec), stream), name)

    def srtp_gcm_unprotect(self, state, packets, sizes, C_, F_, pkt_stride, out, out_stride, sizes_out, rec=None, ctl=None, stream=None):
        """igdsp_srtp_gcm_unprotect: sizes include the tag; a refused packet gets size 0 and its output slot is not written."""
        self.srtp_gcm_protect(state, packets, sizes, C_, F_, pkt_stride, out, out_stride, sizes_out, rec=rec, ctl=ctl, unprotect=True, stream=stream)

    def srtcp_protect(self, state, packets, sizes, C_, F_, pkt_stride, out, out_stride, sizes_out, rec=None, ctl=None, unprotect=False, stream=None):
        """igdsp_srtcp_protect (unprotect: igdsp_srtcp_unprotect): srtp_protect's arguments on RTCP packets; state [C] SRTP_STATE from
        srtcp_derive; a protected packet is 14 bytes longer."""
        fn, name = (self.L.igdsp_srtcp_unprotect, "igdsp_srtcp_unprotect") if unprotect else (self.L.igdsp_srtcp_protect, "igdsp_srtcp_protect")
        self._ck(fn(self.h, _ptr(ctl), _ptr(packets), _ptr(sizes), C_, F_, pkt_stride, _ptr(state), _ptr(out), out_stride, _ptr(sizes_out), _ptr(rec), stream), name)

    def srtcp_unprotect(self, state, packets, sizes, C_, F_, pkt_stride, out, out_stride, sizes_out, rec=None, ctl=None, stream=None):
        """igdsp_srtcp_unprotect: sizes include the index word and the tag; a refused packet gets size 0 and its output slot is not written."""
        self.srtcp_protect(state, packets, sizes, C_, F_, pkt_stride, out, out_stride, sizes_out, rec=rec, ctl=ctl, unprotect=True, stream=stream)

    def rtcp_build(self, ctl, src, now, C_, F_, state, packets, pkt_stride, sizes, jb=None, cname=None, cname_len=None, rec=None, stream=None):
        """igdsp_rtcp_build: ctl [F][C] u8 (RTCP_NONE / REPORT / BYE), src [F][C] RTCP_SRC, now [F] u64 NTP, jb [C] JB_STATE or None, cname
        [C][64] u8 + cname_len [C] u8 or both None; state [C] RTCP_STATE (in and out) -> packets [F][C][pkt_stride] u8, sizes [F][C] u16, rec
        [F][C] RTCP_BUILT (optional)."""
        self._ck(self.L.igdsp_rtcp_build(self.h, _ptr(ctl), _ptr(jb), _ptr(src), _ptr(now), _ptr(cname), _ptr(cname_len), C_, F_, _ptr(state), _ptr(packets),
                                         pkt_stride, _ptr(sizes), _ptr(rec), stream), "igdsp_rtcp_build")

    def rtcp_parse(self, packets, sizes, arrival, local_ssrc, C_, F_, pkt_stride, state, rec=None, stream=None):
        """igdsp_rtcp_parse: packets [F][C][pkt_stride] u8 + sizes [F][C] u16, arrival [F][C] u32 (middle 32 NTP bits), local_ssrc [C] u32;
        state [C] RTCP_STATE (in and out) -> rec [F][C] RTCP_SEEN (optional)."""
        self._ck(self.L.igdsp_rtcp_parse(self.h, _ptr(packets), _ptr(sizes), _ptr(arrival), _ptr(local_ssrc), C_, F_, pkt_stride, _ptr(state), _ptr(rec), stream),
                 "igdsp_rtcp_parse")

    def bss_select(self, info, group_ptr, members, n_members, state, words, C_, G_, F_, n=160, payload=None, codec=None, pcm=None,
                   length=None, gain=None, mute=None, vote_frames=0, sel=None, out=None, stats=None, stream=None):
        """igdsp_bss_select: info [F][C] RTP_INFO; at most one of payload [F][C][n] u8 (+ codec [C]) / pcm [F][C][n] int16; state [G]
        BSS_STATE and words [n_members] u32 carried across calls; sel [F][G] int32, out [F][G][n] int16, stats [F][G] (device buffers)."""
        self._ck(self.L.igdsp_bss_select(self.h, _ptr(info), _ptr(payload), _ptr(codec), _ptr(pcm), _ptr(length), _ptr(gain), _ptr(group_ptr),
                                         _ptr(members), n_members, _ptr(mute), C_, G_, F_, n, vote_frames, _ptr(state), _ptr(words), _ptr(sel),
                                         _ptr(out), _ptr(stats), stream), "igdsp_bss_select")

    def ptt_arbitrate(self, info, group_ptr, members, n_members, state, slots, C_, G_, F_, n=160, payload=None, codec=None, pcm=None,
                      length=None, gain=None, rxonly=None, release_frames=0, sel=None, tick=None, ctl_out=None, out=None, stats=None,
                      stream=None):
        """igdsp_ptt_arbitrate: info [F][C] RTP_INFO; at most one of payload [F][C][n] u8 (+ codec [C]) / pcm [F][C][n] int16; state [G]
        PTT_STATE and slots [n_members] PTT_SLOT carried across calls; sel [F][G] int32, tick [F][G] PTT_TICK, ctl_out [F][G] u8, out
        [F][G][n] int16, stats [F][G] (device buffers)."""
        self._ck(self.L.igdsp_ptt_arbitrate(self.h, _ptr(info), _ptr(payload), _ptr(codec), _ptr(pcm), _ptr(length), _ptr(gain),
                                            _ptr(group_ptr), _ptr(members), n_members, _ptr(rxonly), C_, G_, F_, n, release_frames,
                                            _ptr(state), _ptr(slots), _ptr(sel), _ptr(tick), _ptr(ctl_out), _ptr(out), _ptr(stats), stream),
                 "igdsp_ptt_arbitrate")

    def link_watch(self, info, state, C_, T_, S_=1, t0_ms=0, tick_ms=20, sizes=None, up=None, period_ms=None, miss_ticks=0, event_mask=0,
                   kind=None, events=None, event_cap=0, event_count=None, work=None, stream=None):
        """igdsp_link_watch: info [T * S][C] RTP_INFO (arrival slots as jb_receive's), sizes [T * S][C] u16 (0 = no packet), up [C] u8,
        period_ms [C] u16; state [C] LINK_STATE carried across calls; kind [T][C] u8, events [event_cap] LINK_EVENT, event_count [2] u32
        {events of the launch, events stored}; work: link_work_bytes(C, T) bytes, 16-byte aligned, one per stream (device buffers)."""
        self._ck(self.L.igdsp_link_watch(self.h, _ptr(info), _ptr(sizes), _ptr(up), _ptr(period_ms), C_, T_, S_, t0_ms & 0xFFFFFFFFFFFFFFFF, tick_ms,
                                         miss_ticks, event_mask, _ptr(state), _ptr(kind), _ptr(events), event_cap, _ptr(event_count), _ptr(work),
                                         stream), "igdsp_link_watch")

    def jb_receive(self, packets, radio, state, ring, payload, length, info, C_, T_, S_=1, stride=180, n=160, delay=JB_DELAY, sizes=None,
                   arrival=None, tick_flags=None, pkt_status=None, stream=None):
        """igdsp_jb_receive: packets [T*S][C][stride] in arrival order, sizes [T*S][C] u16, radio [C], arrival [T*S][C] u32 (optional);
        state [C] JB_STATE and ring (jb_ring_bytes(C, n) bytes) carried across calls; payload [T][C][n], len [T][C], info [T][C],
        tick_flags [T][C] u8, pkt_status [T*S][C] u8 out (device buffers)."""
        self._ck(self.L.igdsp_jb_receive(self.h, _ptr(packets), _ptr(sizes), _ptr(radio), _ptr(arrival), C_, T_, S_, stride, n, delay,
                                         _ptr(state), _ptr(ring), _ptr(payload), _ptr(length), _ptr(info), _ptr(tick_flags),
                                         _ptr(pkt_status), stream), "igdsp_jb_receive")

    def jb_receive_adaptive(self, packets, radio, state, ring, adapt, payload, length, info, C_, T_, S_=1, stride=180, n=160, cfg=None,
                            sizes=None, arrival=None, tick_flags=None, pkt_status=None, delay_out=None, stream=None):
        """igdsp_jb_receive_adaptive: as jb_receive, with the playout delay of each channel adapted at every playout start: adapt [C]
        JB_ADAPT carried across calls beside state and ring, cfg a JB_ADAPT_CFG record / (min, max, init, mult, late_restart) / None for
        the defaults (host memory), delay_out [T][C] u8 out (optional)."""
        c = _jb_cfg(cfg)
        self._ck(self.L.igdsp_jb_receive_adaptive(self.h, _ptr(packets), _ptr(sizes), _ptr(radio), _ptr(arrival), C_, T_, S_, stride, n,
                                                  None if c is None else c.ctypes.data_as(_vp), _ptr(state), _ptr(ring), _ptr(adapt),
                                                  _ptr(payload), _ptr(length), _ptr(info), _ptr(tick_flags), _ptr(pkt_status), _ptr(delay_out),
                                                  stream), "igdsp_jb_receive_adaptive")

    def plc_conceal(self, tick_flags, state, out, C_, T_, n=160, payload=None, codec=None, pcm=None, length=None, len_out=None, stats=None,
                    stream=None):
        """igdsp_plc_conceal: tick_flags [T][C] u8 (IGDSP_JB_*); exactly one of payload [T][C][n] u8 (+ codec [C]) / pcm [T][C][n] int16;
        length [T][C] u16 (optional); state [C] PLC_STATE carried across calls; out [T][C][n] int16, len_out [T][C] u16 and stats [T][C]
        (the last two optional) (device buffers)."""
        self._ck(self.L.igdsp_plc_conceal(self.h, _ptr(tick_flags), _ptr(payload), _ptr(codec), _ptr(pcm), _ptr(length), C_, T_, n, _ptr(state),
                                          _ptr(out), _ptr(len_out), _ptr(stats), stream), "igdsp_plc_conceal")

    # -- staged ED-137 send path (transport_send_rtp as pjmedia calls it)
    def tx_open(self, call_id: int, calltype: str, call_in: bool, keepalive_ms: int = 200, now_ms: int = 0):
        self._ck(self.L.igdsp_tx_open(self.h, call_id, calltype.encode(), 1 if call_in else 0, keepalive_ms, now_ms), "igdsp_tx_open")

    def tx_close(self, call_id: int):
        self._ck(self.L.igdsp_tx_close(self.h, call_id), "igdsp_tx_close")

    def tx_set_ptt(self, call_id: int, ptt: bool, priority: int = 0, user_rec: int = 0):
        self._ck(self.L.igdsp_tx_set_ptt(self.h, call_id, 1 if ptt else 0, priority, user_rec), "igdsp_tx_set_ptt")

    def tx_set_sql(self, call_id: int, sql: bool, priority: int = 0, bssi: int = -1):
        """bssi < 0: the 3-argument setAdapterQslOn (bssi unchanged)"""
        self._ck(self.L.igdsp_tx_set_sql(self.h, call_id, 1 if sql else 0, priority, bssi), "igdsp_tx_set_sql")

    def tx_set_ptt_id(self, call_id: int, pttid: int):
        self._ck(self.L.igdsp_tx_set_ptt_id(self.h, call_id, pttid), "igdsp_tx_set_ptt_id")

    def tx_set_slave(self, call_id: int, rx: bool, tx: bool):
        self._ck(self.L.igdsp_tx_set_slave(self.h, call_id, 1 if rx else 0, 1 if tx else 0), "igdsp_tx_set_slave")

    def tx_set_recorder(self, call_id: int, on: bool):
        self._ck(self.L.igdsp_tx_set_recorder(self.h, call_id, 1 if on else 0), "igdsp_tx_set_recorder")

    def tx_set_calltype(self, call_id: int, calltype: str):
        self._ck(self.L.igdsp_tx_set_calltype(self.h, call_id, calltype.encode()), "igdsp_tx_set_calltype")

    def on_tx_frame(self, call_id: int, pkt: bytes, now_ms: int) -> int:
        """0, or the negative code (IGDSP_EBUSY: the leg's ring was full and this frame was refused)"""
        return self.L.igdsp_on_tx_frame(self.h, call_id, pkt, len(pkt), now_ms)

    def tx_flush(self) -> int:
        n = _u32()
        self._ck(self.L.igdsp_tx_flush(self.h, C.byref(n)), "igdsp_tx_flush")
        return n.value

    def tx_results(self):
        """(entries: TX_PACKET [N], packets: uint8 [N][TX_SLOT]) — copies of the last flush's results"""
        p, n = _vp(), _u32()
        self._ck(self.L.igdsp_tx_results(self.h, C.byref(p), C.byref(n)), "igdsp_tx_results")
        if n.value == 0:
            return np.zeros(0, TX_PACKET), np.zeros((0, TX_SLOT), np.uint8)
        ent = np.frombuffer((C.c_uint8 * (n.value * TX_PACKET.itemsize)).from_address(p.value), TX_PACKET).copy()
        # the flush writes the slots contiguously, frame i at entries[0].pkt + i * TX_SLOT
        pk = np.frombuffer((C.c_uint8 * (n.value * TX_SLOT)).from_address(int(ent["pkt"][0])), np.uint8).reshape(n.value, TX_SLOT).copy()
        return ent, pk

    def tx_get_chan(self, call_id: int) -> np.ndarray:
        out = np.zeros((), TX_CHAN)
        self._ck(self.L.igdsp_tx_get_chan(self.h, call_id, out.ctypes.data_as(_vp)), "igdsp_tx_get_chan")
        return out

    def tx_counts(self, call_id: int):
        """(refused, dropped) of the call's leg since its igdsp_tx_open"""
        r, d = _u32(), _u32()
        self._ck(self.L.igdsp_tx_counts(self.h, call_id, C.byref(r), C.byref(d)), "igdsp_tx_counts")
        return r.value, d.value

    # -- ED-137 gated window
    @staticmethod
    def window(hold, gate_mode=GATE_ALWAYS, gate=None, probe=None, work=None, probe_alarm=0) -> Window:
        w = Window(gate_mode, probe_alarm, _ptr(hold), _ptr(gate), _ptr(probe), _ptr(work))
        w._keep = (hold, gate, probe, work)          # the struct holds raw pointers: keep the tensors alive as long as it lives
        return w

    def window_work_bytes(self, C_: int) -> int:
        return int(self.L.igdsp_window_work_bytes(C_))

    def window_update(self, stats, C_, F_, n, win: Window, info=None, length=None, stream=None):
        self._ck(self.L.igdsp_window_update(self.h, _ptr(stats), _ptr(info), _ptr(length), C_, F_, n, C.byref(win), stream), "igdsp_window_update")

    def decode_meter_window(self, layout, packets, sizes, codec, radio, C_, F_, stride, hdr, stats, win: Window, info=None, agg=None, rank=0, stream=None):
        self._ck(self.L.igdsp_decode_meter_window(self.h, layout, _ptr(packets), _ptr(sizes), _ptr(codec), _ptr(radio), C_, F_, stride, hdr,
                                                  _ptr(stats), _ptr(info), _ptr(agg), rank, C.byref(win), stream), "igdsp_decode_meter_window")

    def wav_expand(self, payload, C_, F_, n, files, file_stride, rate=8000, stream=None):
        self._ck(self.L.igdsp_wav_expand(self.h, _ptr(payload), C_, F_, n, rate, _ptr(files), file_stride, stream), "igdsp_wav_expand")

    def g726_reorder(self, d_in, d_out, n_bytes, mode, stream=None):
        self._ck(self.L.igdsp_g726_reorder(self.h, _ptr(d_in), _ptr(d_out), n_bytes, mode, stream), "igdsp_g726_reorder")

    def gen_uniform(self, out, n_bytes, seed=0x20241218, first_byte=0, stream=None):
        self._ck(self.L.igdsp_gen_uniform(self.h, _ptr(out), n_bytes, seed, first_byte, stream), "igdsp_gen_uniform")

    def stream_read(self, src, n_bytes, sink, stream=None):
        self._ck(self.L.igdsp_stream_read(self.h, _ptr(src), n_bytes, _ptr(sink), stream), "igdsp_stream_read")

    # -- device memory
    def dev_alloc(self, nbytes: int) -> int:
        p = _vp()
        self._ck(self.L.igdsp_dev_alloc(self.h, C.byref(p), nbytes), "igdsp_dev_alloc")
        return p.value

    def dev_free(self, ptr: int):
        self._ck(self.L.igdsp_dev_free(self.h, ptr), "igdsp_dev_free")

    def dev_memset(self, ptr, value: int, nbytes: int):
        self._ck(self.L.igdsp_dev_memset(self.h, _ptr(ptr), value, nbytes), "igdsp_dev_memset")

    def io_alloc(self, bufs, explore_limit_bytes: int = 0):
        """bufs = [(nbytes, role), ...] -> (IoSet, [device pointers], report dict): igdsp_io_alloc."""
        arr = (IoBuf * len(bufs))()
        for a, (nb, role) in zip(arr, bufs):
            a.bytes, a.role = int(nb), int(role)
        st, rep = _vp(), IoReport()
        self._ck(self.L.igdsp_io_alloc(self.h, arr, len(bufs), explore_limit_bytes, C.byref(st), C.byref(rep)), "igdsp_io_alloc")
        return IoSet(self, st), [a.ptr for a in arr], rep.as_dict()

    def sync(self, stream=None):
        self._ck(self.L.igdsp_sync(self.h, stream), "igdsp_sync")

    def via(self, entry: str) -> "Context":
        """A view of this context whose stage method (conf_mix, resample, ...) calls the yardstick `entry` of INTERNAL_TWIN in place of
        the public twin whose arguments it takes (igdsp_internal_snd_copy: both directions); everything else is this context's.  The
        view owns nothing; a failing call raises IgdspError under the twin's name."""
        return _Via(self, entry)

    # -- timers
    def probe_placement(self, buf, n_bytes, out=None, reps=10, stream=None) -> float:
        ms = C.c_float(0)
        self._ck(self.L.igdsp_probe_placement(self.h, _ptr(buf), n_bytes, _ptr(out), reps, C.byref(ms), stream), "igdsp_probe_placement")
        return float(ms.value)

    def timer(self):
        return Timer(self)


class IoSet:
    """Owner of one igdsp_io_alloc buffer set (freed by close() / igdsp_io_free)."""

    def __init__(self, ctx: Context, handle):
        self.ctx, self.h = ctx, handle

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.L.igdsp_io_free(self.ctx.h, self.h)
        self.h = None


class DevView:
    """A raw device range as something torch can wrap without copying: torch.as_tensor(DevView(ptr, n), device="cuda")
    gives a uint8 tensor over it (plumbing for tests / bench; the memory stays owned by whoever allocated it)."""

    def __init__(self, ptr: int, nbytes: int):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 3, "strides": None}


def as_tensor(ptr: int, nbytes: int, dtype=None, shape=None):
    import torch

    t = torch.as_tensor(DevView(ptr, nbytes), device="cuda")
    if dtype is not None:
        t = t.view(dtype)
    return t.view(shape) if shape is not None else t


class Timer:
    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.t = _vp()
        ctx._ck(ctx.L.igdsp_timer_create(ctx.h, C.byref(self.t)), "igdsp_timer_create")

    def start(self, stream=None):
        self.ctx._ck(self.ctx.L.igdsp_timer_start(self.ctx.h, self.t, stream), "igdsp_timer_start")

    def stop(self, stream=None):
        self.ctx._ck(self.ctx.L.igdsp_timer_stop(self.ctx.h, self.t, stream), "igdsp_timer_stop")

    def elapsed_ms(self) -> float:
        ms = C.c_float()
        self.ctx._ck(self.ctx.L.igdsp_timer_elapsed_ms(self.ctx.h, self.t, C.byref(ms)), "igdsp_timer_elapsed_ms")
        return ms.value

    def close(self):
        if self.t:
            self.ctx.L.igdsp_timer_destroy(self.ctx.h, self.t)
            self.t = None


class _ViaLib:
    def __init__(self, lib, entry):
        name = entry if entry.startswith("igdsp_internal_") else "igdsp_internal_" + entry
        twin = INTERNAL_TWIN[name] if name in INTERNAL_TWIN else INTERNAL_MORE_TWIN[name]
        self._lib, self._fn = lib, internal(name)
        self._twins = {twin, "igdsp_snd_split"} if twin == "igdsp_snd_combine" else {twin}

    def __getattr__(self, name):
        return self._fn if name in self._twins else getattr(self._lib, name)


class _Via(Context):
    def __init__(self, ctx: Context, entry: str):
        self.L, self.h, self.max_channels = _ViaLib(ctx.L, entry), ctx.h, ctx.max_channels

    def close(self):
        self.h = None                               # the handle is the context's
