"""-m "not gpu": which kernel serves a shape, and with what geometry — the routes of csrc/igdsp_route.h at 256 CUs, compiled with
g++ through tests/route/route_driver.cpp.  The parity tests check outputs, not which kernel produced them; this table pins the
routing itself (kernel form, instantiation key, grid, block size, dynamic LDS, the split between the fast and the general
kernel), so a retune or a refactor shows here what it changed.  Unset fields of a case are not checked; "key" is the strided
kernels' qt_key(Q, TAIL) = 2 Q + TAIL (tiny: n / 4).  IGDSP_* entries are set in the environment of the route driver."""
import shutil

import pytest

from tests import route_util

# (case, expected fields).  Addresses default to 0x1000 (every alignment); pcm / g711 absent unless given.
CASES = [
    # the headline shape 65 536 x 128 x 160
    ("meter C=65536 F=128", "fast=chunk store=0 grid=256 threads=1024 done=8388608 rest=none"),
    ("meter C=65536 F=128 pcm=0x2000", "fast=chunk store=1 grid=256 threads=256 done=8388608 rest=none"),
    ("meter C=65536 F=128 variant=3", "fast=fat grid=256 threads=512 done=8388608 rest=none"),
    ("meter C=65536 F=128 variant=1", "fast=none done=0 rest=wave_per_frame rest_grid=2048 rest_threads=256"),
    ("roundtrip C=65536 F=128", "form=blk64 grid=256 threads=384 n_groups=1024 gpb=4 gsh=2 mid_start=0 c_first=65536 gen_grid=0"),
    ("roundtrip C=65536 F=128 spread=1", "form=blk64 grid=256 threads=384 gpb=4 gsh=2 mid_start=1"),
    ("roundtrip C=65536 F=128 variant=4", "form=chunk64 grid=256 threads=768 n_groups=1024 n_seg=3"),
    ("window C=65536 F=128", "fits=1 blk=1 n_groups=1024 n_seg=4 gpb=4 gsh=2 parts=1 grid=256 threads=768"),
    ("encode C=65536 F=128", "form=lut16 grid=256 threads=640 groups=167772160 table=1"),
    # the reference's other frame sizes: 164, 80, 24, 240 bytes
    ("meter C=65536 F=128 n=164", "fast=strided store=0 key=21 grid=256 threads=1024 done=8388608"),
    ("meter C=65536 F=128 n=164 pcm=0x2000", "fast=strided store=1 key=21 grid=256 threads=384"),
    ("meter C=65536 F=128 n=80", "fast=strided key=10 threads=1024"),
    ("meter C=65536 F=128 n=24", "fast=tiny key=6 grid=256 threads=1024 done=8388608"),
    ("meter C=65536 F=128 n=240", "fast=strided key=30 threads=768"),
    ("meter C=65536 F=128 n=244", "fast=none done=0 rest=image rest_grid=256 rest_threads=384 rest_lds=93696"),
    ("meter C=65536 F=128 n=164 len=1", "fast=none rest=image rest_threads=576 rest_lds=94464"),
    ("roundtrip C=65536 F=128 n=164", "form=strided_blk key=21 grid=256 threads=512 gpb=4 gsh=2 c_first=65536"),
    ("roundtrip C=65536 F=128 n=80", "form=strided_blk key=10 threads=640"),
    ("roundtrip C=65536 F=128 n=24", "form=strided_blk key=3 threads=1024"),
    ("roundtrip C=65536 F=128 n=240", "form=strided_blk key=30 threads=256"),
    # a C % 64 tail, and the < 64-frame tail of the meter
    ("roundtrip C=65568 F=128", "form=blk64 c_first=65536 gen_grid=8"),
    ("meter C=100 F=1", "fast=chunk grid=1 done=64 rest=image rest_grid=1 rest_threads=576 rest_lds=92160"),
    # unaligned buffers: a 160-byte frame off 16 bytes takes the strided meter; off 4 bytes, the general kernels
    ("meter C=65536 F=128 payload=0x1004", "fast=strided key=20 threads=1024 done=8388608"),
    ("meter C=65536 F=128 payload=0x1002", "fast=none rest=wave_per_frame rest_grid=2048"),
    ("roundtrip C=65536 F=128 out=0x1004", "form=none c_first=0 gen_grid=2048"),
    ("roundtrip C=65536 F=128 n=164 out=0x1002", "form=none c_first=0 gen_grid=2048"),
    ("encode C=65536 F=128 out=0x1004", "form=scalar grid=2048 threads=256 table=0"),
    # either side of the block-owned fill rules: round trip 0.6 to 1 round of blocks, window one round or whole rounds >= 85 %
    ("roundtrip C=10240 F=128", "form=blk64 grid=160 threads=384 gpb=1 gsh=0"),
    ("roundtrip C=8192 F=128", "form=lut64 grid=171 threads=768 n_groups=128 n_seg=16"),
    ("roundtrip C=24576 F=128", "form=lut64 grid=256 n_groups=384 n_seg=8"),
    ("window C=8192 F=128", "blk=1 gpb=1 gsh=0 grid=128 n_seg=8"),
    ("window C=24576 F=128", "blk=0 n_seg=8 grid=256 threads=768"),
    ("window C=131072 F=128", "blk=1 gpb=4 grid=512 n_seg=2"),
    # a window launch of more than 255 frames goes out in parts; more than 8 x 65 535 frames do not fit
    ("window C=65536 F=600", "fits=1 blk=1 parts=3"),
    ("window C=262144 F=70000", "fits=0 n_seg=1"),
    # the encoder-table thresholds: k_encode_lut16 from 2^25 samples, the TX table form from 2^22
    ("encode C=4096 F=128", "form=lut16 table=1"),
    ("encode C=1024 F=128", "form=v8_table grid=512 threads=1024 table=0"),
    ("encode C=256 F=8", "form=v8 grid=160 threads=256 table=0"),
    ("encode C=256 F=8 n=164", "form=scalar grid=1312 table=0"),
    ("tx C=65536 F=128 pcm=0x1000", "form=pcm_tab vec=1 n_groups=4096 grid=256 threads=512 lds=131072 table=1"),
    ("tx C=65536 F=128 pcm=0x1000 tab_lds=0", "form=pcm grid=512 lds=0 table=1"),
    ("tx C=65536 F=128 g711=0x1000", "form=g711 vec=1 grid=512 lds=0 table=0"),
    ("tx C=4096 F=1 pcm=0x1004", "form=pcm vec=0 n_groups=256 grid=32 table=0"),
    ("tx C=100 F=8 n=164 g711=0x1001", "form=g711 vec=0 n_groups=7 grid=1"),
    # every env override
    ("meter C=65536 F=128 n=24 IGDSP_NO_TINY=1", "fast=strided key=3 threads=1024"),
    ("meter C=65536 F=128 n=164 IGDSP_NO_STRIDED=1", "fast=none rest=image rest_threads=576"),
    ("meter C=65536 F=128 n=164 IGDSP_NO_STRIDED=1 IGDSP_IMG_WAVES=4", "rest=image rest_threads=256 rest_lds=41984"),
    ("roundtrip C=65536 F=128 IGDSP_RT_BLK=0", "form=lut64 grid=256 threads=768 n_seg=3 order=0"),
    ("roundtrip C=8192 F=128 IGDSP_RT_BLK=1 IGDSP_RT_GPB=2", "form=blk64 grid=64 threads=384 gpb=2 gsh=1"),
    ("roundtrip C=65536 F=128 IGDSP_RT_BLK=0 IGDSP_RT_ORDER=1 IGDSP_RT_NSEG=3", "form=lut64 n_seg=3 order=1"),
    ("roundtrip C=65536 F=128 IGDSP_RT_MID=1 IGDSP_RTB_WAVES=8", "form=blk64 threads=512 mid_start=1"),
    ("window C=65536 F=128 IGDSP_WIN_BLK=0 IGDSP_WIN_NSEG=2 IGDSP_WIN_WAVES=8", "blk=0 n_seg=2 grid=256 threads=512"),
    ("window C=65536 F=128 IGDSP_WIN_GPB=1", "blk=1 gpb=1 gsh=0 grid=1024"),
    ("window C=65536 F=128 IGDSP_WIN_GPB=2 IGDSP_WIN_WAVES=1", "blk=1 gpb=2 gsh=1 grid=512 threads=128"),
]


@pytest.fixture(scope="module")
def routes():
    return dict(zip((case for case, _ in CASES), route_util.run([case for case, _ in CASES])))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("case,expected", CASES, ids=[c for c, _ in CASES])
def test_route(routes, case, expected):
    got = routes[case]
    want = dict(kv.split("=") for kv in expected.split())
    assert {k: got[k] for k in want} == want, f"{case}: {got}"


TX_YARDSTICK = ["C=131072 F=1 n=16 pcm=0x1000",             # PCM below 2^22 samples: the enc_uni form, two blocks per CU
                "C=131072 F=1 n=32 pcm=0x1000",          # 2^22 samples exactly: the table form, one block per CU
                "C=65536 F=128 pcm=0x1000",
                "C=65536 F=128 pcm=0x1000 tab_lds=0",   # the raised LDS limit refused: the enc_uni form at any size
                "C=65536 F=128 g711=0x1000", "C=4096 F=1 pcm=0x1000", "C=100 F=8 n=164 g711=0x1000"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_tx_yardstick_grid_is_the_entry_grid():
    """igdsp_internal_tx_copy runs the groups, blocks and threads of the igdsp_tx_packetize launch of the same arguments at 256 CUs: a
    PCM launch below 2^22 samples takes cus * 2 blocks, the table form cus"""
    got = route_util.run([f"{e} {c} cus=256" for c in TX_YARDSTICK for e in ("tx", "tx_copy")])
    for i, c in enumerate(TX_YARDSTICK):
        entry, yard = got[2 * i], got[2 * i + 1]
        assert {k: yard[k] for k in ("n_groups", "grid", "threads", "form")} == {k: entry[k] for k in ("n_groups", "grid", "threads", "form")}, c
    assert (got[0]["form"], got[0]["grid"], got[0]["table"]) == ("pcm", "512", "0")
    assert (got[2]["form"], got[2]["grid"], got[2]["table"]) == ("pcm_tab", "256", "1")
