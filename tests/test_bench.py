"""bench.py's own options: `--dump-outputs DIR` (what the last timed step computed, as .npy) and the lean plain run
(everything beyond the headline figure only with `--full`)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def _tiny_step():
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, attn_implementation="eager")
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg)
    ids = torch.randint(0, 512, (2, 64), generator=torch.Generator().manual_seed(1))
    out = model(input_ids=ids, labels=ids)
    out.loss.backward()
    return model, out


def test_sample_positions_are_fixed_by_name():
    t = torch.randn(6, 50, 40)[:, :, :30]  # a strided view: sampled without a flattened copy
    a, b = bench._sample("w", t, 100), bench._sample("w", t.contiguous(), 100)
    assert a.dtype == np.float32 and a.shape == (100,) and np.array_equal(a, b)
    assert not np.array_equal(a, bench._sample("other", t, 100))
    small = torch.randn(3, 4)
    assert np.array_equal(bench._sample("s", small, 100), small.numpy())  # small tensors whole, in their shape


def test_dump_outputs_writes_the_step_within_budget(tmp_path):
    model, out = _tiny_step()
    kept = {"out": out, "grads": [(n, p.grad) for n, p in model.named_parameters()], "optimizer_step": False}
    info = bench.dump_outputs(tmp_path / "a", kept, model)
    bench.dump_outputs(tmp_path / "b", kept, model)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(p.name for p in (tmp_path / "b").iterdir())
    assert "loss.npy" in files and "logits.npy" in files
    assert sum(f.startswith("grad.") for f in files) == len(list(model.parameters())) == info["arrays"] - 2
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.array_equal(a, b), f
        total += (tmp_path / "a" / f).stat().st_size
    assert total <= bench.DUMP_BUDGET_BYTES
    assert np.load(tmp_path / "a" / "loss.npy")[0] == np.float32(out.loss.item())
    g = model.model.layers[0].mlp.down_proj.weight.grad
    assert np.array_equal(np.load(tmp_path / "a" / "grad.model.layers.0.mlp.down_proj.weight.npy"), g.numpy())


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_bench_run_is_lean_and_dumps_its_last_step(tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--config", "llama-tiny", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["fallback_calls"] == 0
    assert line["unit"] == "tokens/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    for key in ("layer_forward", "cpu_baseline", "secondary"):
        assert key not in line, key
    assert line["roofline"] is None
    d = tmp_path / "out"
    files = sorted(p.name for p in d.iterdir())
    assert sum(f.startswith("grad.") for f in files) > 0 and "logits.npy" in files
    assert sum((d / f).stat().st_size for f in files) <= bench.DUMP_BUDGET_BYTES
    assert all(np.load(d / f).dtype == np.float32 for f in files)
    assert abs(float(np.load(d / "loss.npy")[0]) - line["loss"]) <= 1e-6 * abs(line["loss"])
