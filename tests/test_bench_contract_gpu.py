"""GPU: `bench.py` prints exactly ONE JSON line on stdout that carries the driver contract; under --full also the roofline object and the CPU
baseline; with --dump-outputs it writes what the last timed step computed (tiny workload so the whole check takes seconds; the headline run
is the same code with the default workload)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", "cfg1_tiny_mlm_bs2", *extra], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _check_contract(d):
    for k, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                   ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict)):
        assert isinstance(d[k], typ), (k, d[k])
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic" and d["config"]["workload"] == "cfg1_tiny_mlm_bs2"
    assert abs(d["value"] - d["config"]["global_pairs"] / (d["ms_per_step"] / 1000.0)) < 1e-2 * d["value"]


def test_bench_json_contract(dev, lib):
    d = _bench("--full")
    _check_contract(d)
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] in ("GB/s", "TFLOP/s") and rf["peak"] > 0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and "traffic" in rf
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("reference", "port") and isinstance(cb["sample"], str) and cb["unit"] == d["unit"]


def test_bench_plain_run_and_dumped_outputs(dev, lib, tmp_path):
    """A plain run carries the contract and none of the --full measurements; two plain runs with the same arguments dump the same outputs
    (same inputs, same weights, same dropout stream), float32, within 64 MB, the loss equal to the line's final_loss."""
    dumps = []
    for i in range(2):
        d = _bench("--dump-outputs", str(tmp_path / f"run{i}"))
        _check_contract(d)
        for k in ("roofline", "cpu_baseline", "variants", "host_probe"):
            assert k not in d, k
        assert d["power"] is None
        files = sorted(os.listdir(tmp_path / f"run{i}"))
        assert {"loss.npy", "params_sample.npy", "adamw_exp_avg_sample.npy", "adamw_exp_avg_sq_sample.npy"} <= set(files), files
        arrs = {f[:-4]: np.load(tmp_path / f"run{i}" / f) for f in files}
        assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in arrs.values())
        assert sum(v.nbytes for v in arrs.values()) <= 64 << 20
        assert abs(float(arrs["loss"]) - d["final_loss"]) < 1e-3
        dumps.append(arrs)
    for k, v in dumps[0].items():
        assert v.shape == dumps[1][k].shape, k
        np.testing.assert_allclose(v, dumps[1][k], rtol=1e-4, atol=1e-6, err_msg=k)
