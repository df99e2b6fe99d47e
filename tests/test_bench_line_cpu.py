"""bench.py's final line: compact, parseable, contract keys (the 25 KB line of round 5 was lost by the
driver's parser).  The round-5 record (profiles/r05_bench_v8.json) is the input: the heaviest line the bench ever produced."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("record", ["r05_bench_v8.json", "r05_bench_v1.json", "r04_bench_v9.json"])
def test_compact_line_of_a_full_record_stays_small_and_keeps_the_contract(record):
    import bench
    path = os.path.join(ROOT, "profiles", record)
    full = json.loads(open(path).read().strip().splitlines()[-1])
    full["config"].setdefault("math", None)
    c = bench.compact_line(full, os.path.join(ROOT, "gpurun_out", "bench_detail.json"))
    line = json.dumps(c, separators=(",", ":"))
    assert len(line) < bench.COMPACT_LINE_MAX <= 6144 and "\n" not in line
    for k in ("metric", "value", "unit", "n_gpus", "n_ranks_seen", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "parity"):
        assert k in c, k
    assert c["value"] == full["value"] and c["ms_per_step"] == full["ms_per_step"]
    assert len(c["config"]["workload"]) <= 200 and set(c["config"]) == {"workload", "global_batch", "parallelism", "syncbn", "math"}
    r = c["roofline"]
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert "per_kernel" not in r and "note" not in r and "math" not in r
    assert c["cpu_baseline"]["kind"] == "port" and c["cpu_baseline"]["cores"] >= 1
    assert c["parity"]["pass"] is True
    assert all("per_kernel" not in e for e in c.get("encoder_forward", []))
    for o in c.get("other_configs", []):
        assert len(o["config"]) <= 40 and 0 < o["roofline"]["mfma"]["frac"] < 1
    assert c["detail"] == "gpurun_out/bench_detail.json"


def test_dump_outputs_stays_within_64_mb_and_samples_the_same_elements_every_time(tmp_path):
    """bench.py --dump-outputs: float32 files, at most 64 MB in all, small arrays whole, large ones as the same seeded sample
    in every run (so that two builds can be compared output for output)"""
    from types import SimpleNamespace

    import numpy as np
    import torch

    import bench
    g = torch.Generator().manual_seed(1)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 1), torch.nn.BatchNorm2d(4))
    optim = SimpleNamespace(flat_p=torch.randn(3 << 20, generator=g), flat_g=torch.randn(5, generator=g))
    preds = [torch.randn(2, 5, 1024, 1024, generator=g), torch.randn(2, 5, 512, 512, generator=g)]
    dumps = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.tensor(0.5), preds, model, optim)
        dumps.append({f.name: np.load(str(f)) for f in (tmp_path / d).iterdir()})
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= 64 << 20
    a, b = dumps
    assert set(a) == {"loss.npy", "logits.npy", "logits_aux1.npy", "params_sample.npy", "grads_sample.npy",
                      "bn_running_stats.npy"}
    assert all(v.dtype == np.float32 for v in a.values()) and all(np.array_equal(a[k], b[k]) for k in a)
    assert a["loss.npy"].tolist() == [0.5] and a["grads_sample.npy"].tolist() == optim.flat_g.tolist()
    assert a["logits_aux1.npy"].tolist() == preds[1].reshape(-1).tolist()
    assert a["params_sample.npy"].size == bench.DUMP_SAMPLE and 0 < a["logits.npy"].size < preds[0].numel()
    assert a["bn_running_stats.npy"].tolist() == [0.0] * 4 + [1.0] * 4
