"""-m "not gpu": bench.py's command line (no GPU needed): --help lists the contract's flags, and the two refusals
(no GPU; --gpus N without a distributed launch) are loud and specific.  --dump-outputs' capture and writer run on host tensors."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_help_lists_contract_flags():
    r = _bench("--help")
    assert r.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--channels", "--frames", "--total-channels", "--placement", "--force-collective", "--prewarm-ms", "--dump-outputs"):
        assert flag in r.stdout, flag


def test_refuses_multi_gpu_without_launcher_and_cpu_only():
    r = _bench("--gpus", "2")
    assert r.returncode != 0 and "torch.distributed.run" in (r.stderr + r.stdout)
    import torch
    if not torch.cuda.is_available():
        r = _bench("--steps", "1")
        assert r.returncode != 0 and "no CPU fallback" in (r.stderr + r.stdout)


def test_dump_outputs_capture_on_host_tensors(orc, tmp_path):
    """capture_outputs / write_outputs on host copies of what the meter and store paths leave in their buffers (the oracle's
    records, PCM and aggregate): every field comes back exactly, as float32 / float64, and a larger output is cut to the same
    seeded positions every time."""
    import numpy as np
    import torch

    import bench

    C_, F_, n = 128, 4, 160
    payload = orc.gen_uniform(F_ * C_ * n).reshape(F_, C_, n)
    codec = np.where(np.arange(C_) & 1, 8, 0).astype(np.uint8)
    st, pcm, agg = orc.decode_meter(payload, codec, want_pcm=True, want_agg=True)
    t = {"st": torch.from_numpy(st.view(np.int64).reshape(-1).copy()), "pcm": torch.from_numpy(pcm.reshape(-1).copy())}
    res = bench.capture_outputs(t, torch.from_numpy(agg.reshape(1).view(np.int64).copy()))
    for f in ("sumsq", "rms", "peak", "byte_mean", "flags"):
        assert np.array_equal(res[f"stats_{f}"], st[f].reshape(-1)), f
    assert res["stats_sumsq"].dtype == np.float64 and res["stats_peak"].dtype == np.float32
    assert np.array_equal(res["stats_index"], np.arange(F_ * C_)) and np.array_equal(res["pcm"], pcm.reshape(-1))
    names = ("sumsq", "samples", "frames", "n_silent", "n_clipped", "byte_mean_sum")
    assert res["aggregate"].tolist() == [int(agg[f]) for f in names] + [int(x) for x in agg["peak_slot"]]
    hi, lo = res["aggregate_sumsq_words"]
    assert int(hi) << 32 | int(lo) == int(agg["sumsq"])

    big = torch.arange(bench.DUMP_BULK + 1000, dtype=torch.int16)
    a, b = bench.capture_outputs({"out": big}), bench.capture_outputs({"out": big})
    assert a["codes"].size == bench.DUMP_BULK and np.array_equal(a["codes_index"], b["codes_index"])
    assert np.all(np.diff(a["codes_index"]) > 0)
    assert np.array_equal(a["codes"], big.numpy()[a["codes_index"].astype(np.int64)])

    rep = bench.write_outputs(str(tmp_path / "dump"), res)
    assert rep["bytes"] <= 64 << 20
    for name, arr in res.items():
        back = np.load(tmp_path / "dump" / f"{name}.npy")
        assert back.dtype in (np.float32, np.float64) and np.array_equal(back, arr)
