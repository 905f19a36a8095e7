"""-m gpu: the edges of one headline launch (k_meter_chunk64) — its prologue (the first item's loads ahead of the LUT fill, the two
static batches), its end, and what the write-through record store must still give a consumer.

  a. 65 536 channels x 128 frames (the benchmark's launch), x 1 and x 2 frames (64 and 128 batches on 256 blocks: most blocks have no
     second batch, many no first — the prologue's dropped loads are the whole block) against the oracle, records and aggregate exact;
  b. a super-chunk count that is not a multiple of the batch size, past the two static batches of every block;
  c. records consumed without a host synchronisation: a second stream waits on an event behind the launch and copies the records
     to pinned host memory;
  d. 20 back-to-back launches into one record buffer with alternating payloads: the last writer wins.

One process; every GPU step runs under a watchdog of its own that ends the process if the step does not return."""
import contextlib
import faulthandler

import numpy as np
import pytest

from igate4xsoftphonedsp_amd import capi

from tests import gpu_util as gu

pytestmark = pytest.mark.gpu

N = 160
AGG_FIELDS = ("sumsq", "samples", "frames", "n_silent", "n_clipped", "byte_mean_sum")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=4096)
    yield c
    c.close()


@contextlib.contextmanager
def gpu_step(seconds):
    """Time limit of one GPU step: the process is ended (with every thread's traceback) if the block does not finish in time."""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _codec(C_):
    return np.where((np.arange(C_) * 7 + 3) % 5 < 2, 8, 0).astype(np.uint8)


def _check(st, agg, est, eagg):
    gu.assert_stats_equal(st, est, n=N)
    if agg is not None:
        for f in AGG_FIELDS:
            assert int(agg[f]) == int(eagg[f]), (f, int(agg[f]), int(eagg[f]))
        assert agg["peak_slot"].tolist() == eagg["peak_slot"].tolist()


def _launch_and_check(ctx, orc, C_, F_, seed):
    torch = gu.torch_cuda()
    nb = F_ * C_ * N
    codec = _codec(C_)
    est, eagg = orc.decode_meter(orc.gen_uniform(nb, seed=seed).reshape(F_, C_, N), codec, want_agg=True)
    s = torch.cuda.current_stream().cuda_stream
    with gpu_step(120):
        d_pl = gu.dev_zeros(nb)
        ctx.gen_uniform(d_pl, nb, seed=seed, stream=s)
        d_st = gu.dev_zeros(F_ * C_ * 16, 0xEE)
        d_agg = gu.dev_zeros(capi.AGGREGATE.itemsize)
        ctx.agg_reset(d_agg, stream=s)
        ctx.decode_meter(d_pl, gu.to_dev(codec), C_, F_, N, d_st, agg=d_agg, stream=s)
        torch.cuda.synchronize()
        st, agg = gu.to_host(d_st, capi.FRAME_STATS, (F_, C_)), gu.to_host(d_agg, capi.AGGREGATE)[0]
    _check(st, agg, est, eagg)
    assert int(agg["frames"]) == C_ * F_


@pytest.mark.parametrize("F_", [128, 1, 2])
def test_headline_launch_against_oracle(ctx, orc, F_):
    _launch_and_check(ctx, orc, 65536, F_, seed=4100 + F_)


@pytest.mark.parametrize("C_,F_", [(65472, 24), (4160, 9)])
def test_partial_last_batch(ctx, orc, C_, F_):
    """24 552 super-chunks = 1 534 batches and a half (three times the 512 static ones); 585 super-chunks = 36 batches and 9 items."""
    assert (C_ * F_ // 64) % 16 != 0 and C_ * F_ % 64 == 0
    _launch_and_check(ctx, orc, C_, F_, seed=4300 + F_)


def test_records_visible_to_a_second_stream_without_host_sync(ctx, orc):
    torch = gu.torch_cuda()
    C_, F_ = 65536, 16
    nb = F_ * C_ * N
    codec = _codec(C_)
    est = orc.decode_meter(orc.gen_uniform(nb, seed=4400).reshape(F_, C_, N), codec)
    est = est[0] if isinstance(est, tuple) else est
    with gpu_step(120):
        producer, consumer = torch.cuda.Stream(), torch.cuda.Stream()
        d_pl, d_cd = gu.dev_zeros(nb), gu.to_dev(codec)
        d_st = gu.dev_zeros(F_ * C_ * 16, 0xEE)
        host = torch.empty((F_ * C_ * 16,), dtype=torch.uint8).pin_memory()
        host.fill_(0x77)
        torch.cuda.synchronize()                       # inputs and the 0xEE fill are in place; nothing below waits on the host
        done = torch.cuda.Event()
        with torch.cuda.stream(producer):
            ctx.gen_uniform(d_pl, nb, seed=4400, stream=producer.cuda_stream)
            ctx.decode_meter(d_pl, d_cd, C_, F_, N, d_st, stream=producer.cuda_stream)
            done.record(producer)
        with torch.cuda.stream(consumer):
            consumer.wait_event(done)
            host.copy_(d_st, non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(consumer)
        copied.synchronize()
        st = host.numpy().view(capi.FRAME_STATS).reshape(F_, C_).copy()
        torch.cuda.synchronize()
    _check(st, None, est, None)


def test_back_to_back_launches_last_writer_wins(ctx, orc):
    torch = gu.torch_cuda()
    C_, F_, launches = 65536, 16, 20
    nb = F_ * C_ * N
    codec = _codec(C_)
    exp = []
    for seed in (4500, 4501):
        e = orc.decode_meter(orc.gen_uniform(nb, seed=seed).reshape(F_, C_, N), codec)
        exp.append(e[0] if isinstance(e, tuple) else e)
    assert not np.array_equal(exp[0]["sumsq"], exp[1]["sumsq"])
    s = torch.cuda.current_stream().cuda_stream
    with gpu_step(120):
        d_pls = [gu.dev_zeros(nb), gu.dev_zeros(nb)]
        for d, seed in zip(d_pls, (4500, 4501)):
            ctx.gen_uniform(d, nb, seed=seed, stream=s)
        d_cd = gu.to_dev(codec)
        d_st = gu.dev_zeros(F_ * C_ * 16, 0xEE)
        for i in range(launches):
            ctx.decode_meter(d_pls[i & 1], d_cd, C_, F_, N, d_st, stream=s)
        torch.cuda.synchronize()
        st = gu.to_host(d_st, capi.FRAME_STATS, (F_, C_))
    _check(st, None, exp[(launches - 1) & 1], None)
