"""The kernel instantiations behind igdsp_decode_meter and igdsp_roundtrip_peakhold, one row each, with a recipe that reaches it.

Plain data (no pytest here).  csrc/igdsp_route.h picks one of a fixed set of template instantiations for every shape; each row
below names one of them (the fast form, its key and store flag, and the rest kernel that takes what the fast form leaves) and
gives the inputs that route to it: the frame size n, the byte offsets of the buffers past a 256-byte aligned base, PCM output
yes / no, a length array yes / no, the context variant (igdsp_set_variant) and the IGDSP_* knobs read at launch.

tests/test_kernel_matrix_cpu.py checks, through the route driver, that every row lands where it says at its small and its full
shape, and that the rows cover exactly the instantiations a sweep of all inputs reaches.  tests/test_gpu_kernel_matrix.py runs
every row on the device against the C oracle: meter rows once without and once with the launch aggregate (AGG), round-trip rows
with both encoder lineages.
"""
from dataclasses import dataclass

CUS = 256                       # MI355X compute units: the routes (grid sizes) are checked at this count

SMALL_C, SMALL_F = 150, 7       # 1050 frames = 16 whole super-chunks + a tail of 26; 150 channels: not a multiple of 64
FULL_C = 65536                  # the README's reference scale
FULL_C_ODD = 65519              # super-chunks straddle channels, and the tail goes to the rest kernel
RT_FULL_F = 24                  # round trip: the register form needs 3 segments of >= 8 frames to give every CU a block
BASE = 0x10000                  # driver addresses: a 256-byte aligned base plus the row's offset


def meter_full_f(n):
    """Frames of a full-size meter case: 4 slots of kTinySlot super-chunks per resident wave for n <= 32, >= 4 super-chunks otherwise."""
    return 64 if n <= 32 else 16


@dataclass(frozen=True)
class MeterRow:
    fast: str                   # chunk / fat / tiny / strided / none
    key: int                    # tiny: n / 4; strided: qt_key(Q, TAIL) = 2 Q + TAIL; else 0
    store: bool                 # the PCM-storing instantiation (chunk, strided)
    rest: str                   # what the small shape's tail goes to: image / image_ragged / wave_per_frame
    n: int
    payload_off: int = 0
    pcm_off: int = None         # None: no PCM output
    stats_off: int = 0
    has_len: bool = False
    variant: int = 0
    knobs: tuple = ()           # (("IGDSP_NO_TINY", "1"),)
    full: bool = True           # has a full-chip case

    @property
    def id(self):
        s = f"{self.fast}" + (f"-k{self.key}" if self.fast in ("tiny", "strided") else "") + ("-store" if self.store else "")
        s += f"-n{self.n}" + (f"-pl{self.payload_off}" if self.payload_off else "")
        s += (f"-pcm{self.pcm_off}" if self.pcm_off is not None else "") + ("-len" if self.has_len else "")
        s += (f"-v{self.variant}" if self.variant else "") + "".join("-" + k.replace("IGDSP_", "").lower() for k, _ in self.knobs)
        return s

    def fast_inst(self):
        return meter_fast_inst(self.fast, self.key, self.store)

    def rest_inst(self):
        return meter_rest_inst(self.rest)

    def driver_line(self, C, F):
        """A case line for tests/route/route_driver.cpp."""
        s = f"meter C={C} F={F} n={self.n} variant={self.variant} len={int(self.has_len)} payload={BASE + self.payload_off:#x}"
        s += f" pcm={BASE * 2 + self.pcm_off:#x}" if self.pcm_off is not None else ""
        s += f" stats={BASE * 3 + self.stats_off:#x}"
        return s + "".join(f" {k}={v}" for k, v in self.knobs)


def meter_fast_inst(fast, key, store):
    if fast == "chunk":
        return f"k_meter_chunk64<STORE={int(store)}>"
    if fast == "fat":
        return "k_meter_fat"
    if fast == "tiny":
        return f"k_meter_tiny<N4={key}>"
    if fast == "strided":
        return f"k_meter_strided<Q={key // 2},TAIL={key & 1},STORE={int(store)}>"
    return None


def meter_rest_inst(rest):
    return {"image": "k_meter_image<RAGGED=0>", "image_ragged": "k_meter_image<RAGGED=1>",
            "wave_per_frame": "k_meter_wave_per_frame", "none": None}[rest]


NO_TINY = (("IGDSP_NO_TINY", "1"),)
M = MeterRow
METER_ROWS = [
    # k_meter_chunk64 / k_meter_fat: dense 160-byte frames in 16-byte aligned buffers
    M("chunk", 0, False, "image", 160),
    M("chunk", 0, True, "wave_per_frame", 160, pcm_off=0),
    M("fat", 0, False, "image", 160, variant=3),
    # k_meter_tiny: 16 .. 32-byte frames, records only
    M("tiny", 4, False, "image", 16),
    M("tiny", 5, False, "image", 20, payload_off=4),
    M("tiny", 6, False, "image", 24),
    M("tiny", 7, False, "image", 28),
    M("tiny", 8, False, "image", 32, payload_off=4),
    # k_meter_strided, records only (MeterStridedKeys); 16 / 20 / 24-byte frames only without k_meter_tiny
    M("strided", 2, False, "image", 16, knobs=NO_TINY),
    M("strided", 3, False, "image", 24, knobs=NO_TINY),
    M("strided", 8, False, "image", 64),
    M("strided", 9, False, "image", 72),
    M("strided", 10, False, "image", 80, payload_off=4),
    M("strided", 11, False, "image", 88),
    M("strided", 12, False, "image", 96),
    M("strided", 13, False, "image", 104, payload_off=4),
    M("strided", 16, False, "image", 128),
    M("strided", 17, False, "image", 136),
    M("strided", 20, False, "image", 160, payload_off=4),           # 160-byte frames in a buffer that is only dword aligned
    M("strided", 21, False, "image", 164),
    M("strided", 24, False, "image", 192),
    M("strided", 25, False, "image", 200, payload_off=4),
    M("strided", 30, False, "image", 240),
    # k_meter_strided with PCM output (ReferenceSizeKeys)
    M("strided", 3, True, "wave_per_frame", 24, pcm_off=4),
    M("strided", 10, True, "wave_per_frame", 80, pcm_off=0),
    M("strided", 20, True, "wave_per_frame", 160, pcm_off=4),        # 160-byte frames, PCM not 16-byte aligned
    M("strided", 21, True, "wave_per_frame", 168, pcm_off=4, payload_off=4),
    M("strided", 30, True, "wave_per_frame", 240, pcm_off=0),
    # only the general kernels
    M("none", 0, False, "image", 244, full=False),
    M("none", 0, False, "image_ragged", 164, has_len=True, full=False),
    M("none", 0, False, "wave_per_frame", 159, full=False),
]


@dataclass(frozen=True)
class RtRow:
    form: str                   # lut64 / chunk64 / blk64 / strided / strided_blk / none
    key: int                    # strided forms: qt_key(Q, TAIL)
    rest: str                   # general (the small shape's C % 64 channels) / none
    n: int
    variant: int = 0            # kernel variant (igdsp_set_variant): 4 = k_roundtrip_chunk64
    rt_blk: int = None          # IGDSP_RT_BLK, None: unset
    payload_off: int = 0
    out_off: int = 0
    full: bool = True

    @property
    def id(self):
        s = self.form + (f"-k{self.key}" if self.form.startswith("strided") else "") + f"-n{self.n}"
        s += (f"-v{self.variant}" if self.variant else "") + (f"-blk{self.rt_blk}" if self.rt_blk is not None else "")
        return s + (f"-out{self.out_off}" if self.out_off else "")

    @property
    def knobs(self):
        return () if self.rt_blk is None else (("IGDSP_RT_BLK", str(self.rt_blk)),)

    def form_inst(self):
        return rt_form_inst(self.form, self.key)

    def rest_inst(self):
        return rt_rest_inst(self.rest)

    def driver_line(self, C, F):
        s = f"roundtrip C={C} F={F} n={self.n} variant={self.variant} payload={BASE + self.payload_off:#x} out={BASE * 2 + self.out_off:#x}"
        s += f" stats={BASE * 3:#x}"
        return s + "".join(f" {k}={v}" for k, v in self.knobs)


def rt_form_inst(form, key):
    if form in ("lut64", "chunk64", "blk64"):
        return f"k_roundtrip_{form}"
    if form in ("strided", "strided_blk"):
        return f"k_roundtrip_strided<Q={key // 2},TAIL={key & 1},BLK={int(form == 'strided_blk')}>"
    return None


def rt_rest_inst(rest):
    return "k_roundtrip_general" if rest == "general" else None


R = RtRow
RT_ROWS = [
    R("lut64", 0, "general", 160, rt_blk=0),
    R("blk64", 0, "general", 160, rt_blk=1),
    R("chunk64", 0, "general", 160, variant=4),
    R("strided", 3, "general", 24, rt_blk=0),
    R("strided_blk", 3, "general", 24, rt_blk=1),
    R("strided", 10, "general", 80, rt_blk=0),
    R("strided_blk", 10, "general", 80, rt_blk=1),
    R("strided", 21, "general", 164, rt_blk=0),
    R("strided_blk", 21, "general", 164, rt_blk=1),
    R("strided", 30, "general", 240, rt_blk=0),
    R("strided_blk", 30, "general", 240, rt_blk=1),
    R("none", 0, "general", 160, out_off=4, full=False),
]
