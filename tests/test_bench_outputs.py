"""bench.py's plain run and --dump-outputs: exactly --steps timed steps, the headline keys, the last step's outputs as .npy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float_arrays_with_a_fixed_table_sample(tmp_path):
    """CPU: the writer itself, on the cfg2 model -- every parameter whole except the word table (a seeded row sample), float32,
    under the 64 MB cap, the same rows on every call."""
    import bench
    import synth
    cfg = synth.DEEPCONN_CFGS["cfg2"]
    model = bench.build_model(cfg, "cpu")
    last = (torch.tensor(1.25), torch.tensor(7.5), torch.arange(cfg["B"], dtype=torch.float32))
    total = bench.dump_outputs(str(tmp_path / "a"), model, last)
    bench.dump_outputs(str(tmp_path / "b"), model, last)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"loss.npy", "grad_norm.npy", "pred.npy"} <= set(names)
    assert total <= bench.DUMP_MAX_BYTES
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64), n
        assert np.array_equal(a, b), n
    table = model.word_embeddings.embedding.weight
    sample = np.load(tmp_path / "a" / "param.word_embeddings.embedding.weight.rows_sample.npy")
    assert sample.shape == (bench.DUMP_TABLE_ROWS, table.shape[1])
    rows = np.sort(np.random.default_rng(0).choice(table.shape[0], bench.DUMP_TABLE_ROWS, replace=False))
    assert np.array_equal(sample, table.detach().numpy()[rows])
    assert float(np.load(tmp_path / "a" / "loss.npy")) == 1.25
    assert np.array_equal(np.load(tmp_path / "a" / "pred.npy"), np.arange(cfg["B"], dtype=np.float32))
    for n, p in model.named_parameters():
        if p is not table:
            assert np.array_equal(np.load(tmp_path / "a" / f"param.{n}.npy"), p.detach().numpy()), n


@pytest.mark.gpu
def test_plain_bench_times_the_given_steps_and_dumps_the_last_one(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "pairs/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and abs(line["timed_region_s"] - 3 * line["ms_per_step"] / 1e3) < 1e-3
    assert "configs" not in line and "cpu_baseline" not in line and "roofline" not in line     # --full only
    pred = np.load(out / "pred.npy")
    assert pred.shape == (256,) and np.isfinite(pred).all()
    assert np.isfinite(np.load(out / "loss.npy")) and float(np.load(out / "grad_norm.npy")) > 0
    assert sum(os.path.getsize(out / n) for n in os.listdir(out)) <= 64 << 20


@pytest.mark.gpu
def test_two_runs_with_the_same_arguments_dump_the_same_outputs(tmp_path):
    """The dumped step starts from the seeded initial state, so two runs agree to rounding -- also after enough timed steps
    (60) for the trained state itself to have drifted apart between runs."""
    outs = []
    for k in range(2):
        out = tmp_path / f"dump{k}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "10",
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(out)
    names = sorted(os.listdir(outs[0]))
    assert names == sorted(os.listdir(outs[1])) and "pred.npy" in names
    for n in names:
        a = np.load(outs[0] / n).astype(np.float64)
        b = np.load(outs[1] / n).astype(np.float64)
        assert a.shape == b.shape, n
        assert float(np.abs(a - b).max()) <= 1e-5 * max(1.0, float(np.abs(a).max())), n
