"""N>1 path on CPU: world_size-2 `gloo` DDP over the accelerated model (kernels on the CPU execution model).

Checks what the 8-GPU RCCL run relies on: (1) every parameter of the swapped modules (incl. the fused-QKV /
gate|up views and the custom autograd nodes) takes part in DDP's bucketed all-reduce, (2) the reduced gradient
equals the mean of the per-rank gradients computed without DDP, (3) replicas stay bit-identical after an SGD step."""
import os
import socket
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _build_model(kind="llama"):
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    if kind == "llama-tiles":  # q / k / v / gate / up of 256 rows each: the segmented dW GEMM stores whole tiles (tamd_gemm_seg)
        cfg = LlamaConfig(vocab_size=256, hidden_size=256, intermediate_size=256, num_hidden_layers=2,
                          num_attention_heads=4, num_key_value_heads=4, head_dim=64, max_position_embeddings=128,
                          rms_norm_eps=1e-5, attn_implementation="eager")
        return LlamaForCausalLM(cfg).bfloat16().train(), cfg
    if kind == "bert":  # the fused BertLayer op, the padded-vocabulary MLM head and loss (dropout off: the check below
        from transformers import BertConfig, BertForMaskedLM  # recomputes the per-rank gradients in this process)

        cfg = BertConfig(vocab_size=250, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                         max_position_embeddings=64, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                         attn_implementation="eager")
        return BertForMaskedLM(cfg).bfloat16().train(), cfg
    cfg = LlamaConfig(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                      num_attention_heads=2, num_key_value_heads=1, head_dim=64, max_position_embeddings=128,
                      rms_norm_eps=1e-5, attn_implementation="eager")
    return LlamaForCausalLM(cfg).bfloat16().train(), cfg


def _batch(cfg, rank, kind):
    g = torch.Generator().manual_seed(100 + rank)
    ids = torch.randint(0, cfg.vocab_size, (2, 64 if kind == "llama-tiles" else 48), generator=g)
    if kind != "bert":
        return dict(input_ids=ids, labels=ids, use_cache=False)
    labels = ids.clone()
    labels[torch.rand(ids.shape, generator=g) > 0.3] = -100  # MLM: most positions carry no label
    return dict(input_ids=ids, labels=labels)


def _worker_zero_copy(rank, world, port, out_dir, kind):
    """Three steps of a Llama model under DDP with transformers_amd.ddp.enable_zero_copy: step 1 fills the registry (and DDP
    rebuilds its buckets after it), step 2 still copies (stale views), step 3 writes the dW GEMMs into the buckets."""
    for p in (ROOT, ROOT / "tests", ROOT / "tests" / "hipemu"):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HIPEMU_THREADS="2")
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import transformers_amd
    from emu_backend import emu_backend
    from torch.nn.parallel import DistributedDataParallel as DDP
    from transformers_amd import ddp as tddp

    with emu_backend():
        model, cfg = _build_model(kind)
        transformers_amd.accelerate(model)
        net = DDP(model, bucket_cap_mb=1, gradient_as_bucket_view=True, broadcast_buffers=False,
                  find_unused_parameters=False, static_graph=True)
        tddp.reset()
        tddp.enable_zero_copy(net)
        per_step = []
        for step in range(3):
            model.zero_grad(set_to_none=True)  # (the Trainer's default between steps)
            out = net(**_batch(cfg, rank, kind))
            out.loss.backward()
            per_step.append(dict(tddp.STATS))
        grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters()}
        aliased = all(tddp._VIEWS[id(p)][1].data_ptr() == p.grad.data_ptr() for p in model.parameters() if id(p) in tddp._VIEWS)
        # what `bench.py --gpus N` runs around its timed region (the same functions, on every rank): BEFORE it, the reduced
        # gradients of a zero-copy step against a step with torch's copies (and the fall-back if they differ); after it, the
        # no_sync() steps that price the all-reduce
        import argparse

        import bench

        a = argparse.Namespace(verify_ddp=True, no_ddp_breakdown=False, no_ddp_zero_copy=False, steps=3, warmup=0)
        fwd = lambda n: n(**_batch(cfg, rank, kind))  # noqa: E731
        verify = bench.ddp_verify_or_fall_back(a, net, model, fwd, torch.device("cpu"), world)
        assert a.no_ddp_zero_copy is False and tddp._ENABLED
        report = bench.ddp_report(a, net, model, fwd, torch.device("cpu"), world, 1e9)
        report["verify"] = verify
    torch.save({"grads": grads, "stats": per_step, "aliased": aliased, "loss": out.loss.item(), "report": report},
               f"{out_dir}/rank{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


def _worker(rank, world, port, out_dir, kind="llama"):
    for p in (ROOT, ROOT / "tests", ROOT / "tests" / "hipemu"):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HIPEMU_THREADS="2")
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import transformers_amd
    from emu_backend import emu_backend
    from torch.nn.parallel import DistributedDataParallel as DDP

    with emu_backend():
        model, cfg = _build_model(kind)
        transformers_amd.accelerate(model)
        ddp = DDP(model, bucket_cap_mb=1, gradient_as_bucket_view=True, broadcast_buffers=False,
                  find_unused_parameters=False, static_graph=True)
        out = ddp(**_batch(cfg, rank, kind))
        out.loss.backward()
        grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters()}
        assert all(p.grad is not None for p in model.parameters())
        with torch.no_grad():
            for p in model.parameters():
                p.add_(p.grad, alpha=-0.1)
        weights = {n: p.detach().float().clone() for n, p in model.named_parameters()}
    torch.save({"grads": grads, "weights": weights, "loss": out.loss.item()}, f"{out_dir}/rank{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["llama", "bert"])
def test_ddp_world2_gloo(tmp_path, kind):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), kind), nprocs=world, join=True)
    r = [torch.load(tmp_path / f"rank{i}.pt") for i in range(world)]
    # (3) replicas identical
    for n in r[0]["weights"]:
        assert torch.equal(r[0]["weights"][n], r[1]["weights"][n]), n
        assert torch.equal(r[0]["grads"][n], r[1]["grads"][n]), n
    # (2) reduced gradient == mean of single-process gradients on the two data shards
    for p in (ROOT, ROOT / "tests", ROOT / "tests" / "hipemu"):
        sys.path.insert(0, str(p))
    import transformers_amd
    from emu_backend import emu_backend

    per_rank = []
    with emu_backend():
        for rank in range(world):
            model, cfg = _build_model(kind)
            transformers_amd.accelerate(model)
            model(**_batch(cfg, rank, kind)).loss.backward()
            per_rank.append({n: p.grad.detach().float() for n, p in model.named_parameters()})
    for n, gd in r[0]["grads"].items():
        want = (per_rank[0][n] + per_rank[1][n]) / 2
        err = (gd - want).norm() / want.norm().clamp_min(1e-12)
        assert err < 1e-2, (n, err.item())  # bf16 bucket arithmetic


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["llama-tiles", "llama"])  # whole-tile segments (tamd_gemm_seg); ragged ones (one product + slices)
def test_ddp_zero_copy_gradients_world2_gloo(tmp_path, kind):
    """transformers_amd/ddp.py (trainer.py:712-737): with the communication hook registered, the layer op's
    backward writes its weight gradients straight into DDP's bucket views from the third step on (tamd_gemm_seg for the fused
    q|k|v and gate|up products) and hands DDP aliases of them -- the reduced gradients are still the mean of the per-rank
    gradients, identical on both ranks, and `.grad` IS the bucket view."""
    world = 2
    mp.spawn(_worker_zero_copy, args=(world, _free_port(), str(tmp_path), kind), nprocs=world, join=True)
    r = [torch.load(tmp_path / f"rank{i}.pt") for i in range(world)]
    for n in r[0]["grads"]:
        assert torch.equal(r[0]["grads"][n], r[1]["grads"][n]), n
    assert r[0]["aliased"] and r[1]["aliased"]
    st = r[0]["stats"]
    assert st[0]["zero_copy_layers"] == 0                      # step 1: nothing registered yet
    assert st[2]["zero_copy_layers"] - st[1]["zero_copy_layers"] == 2, st  # step 3: both decoder layers wrote into the buckets
    for i in range(world):  # bench.ddp_report: the two hand-overs reduce to the same gradients; the breakdown legs ran
        rep = r[i]["report"]
        assert "error" not in rep["verify"] and "breakdown_error" not in rep, rep
        assert rep["verify"]["zero_copy_layers_in_checked_step"] == 2 and rep["verify"]["ranks"] == world
        assert rep["verify"]["bit_identical"] and rep["verify"]["max_rel_err"] == 0.0, rep["verify"]
        assert rep["verify"]["verified"] and "disabled_zero_copy" not in rep["verify"]
        assert rep["compute_only_ms"] > 0 and rep["busbw_GBps"] is not None and rep["buckets_per_step"] >= 1
    assert r[0]["report"]["verify"] == r[1]["report"]["verify"]
    for p in (ROOT, ROOT / "tests", ROOT / "tests" / "hipemu"):
        sys.path.insert(0, str(p))
    import transformers_amd
    from emu_backend import emu_backend

    per_rank = []
    with emu_backend():
        for rank in range(world):
            model, cfg = _build_model(kind)
            transformers_amd.accelerate(model)
            model(**_batch(cfg, rank, kind)).loss.backward()
            per_rank.append({n: p.grad.detach().float() for n, p in model.named_parameters()})
    for n, gd in r[0]["grads"].items():
        want = (per_rank[0][n] + per_rank[1][n]) / 2
        err = (gd - want).norm() / want.norm().clamp_min(1e-12)
        assert err < 1e-2, (n, err.item())  # bf16 bucket arithmetic


def _worker_corrupted_view(rank, world, port, out_dir):
    """A deliberately wrong registry on ONE rank: the noted bucket views of the two decoder layers' down_proj weights are
    swapped, so layer 1 writes its dW into layer 0's slot and layer 0 into layer 1's (DDP then copies what it finds: layer 1's
    gradient ends up being layer 0's).  `bench.ddp_verify_or_fall_back` must see it on BOTH ranks, switch the hand-over off,
    and the next steps must reduce to the right gradients again."""
    for p in (ROOT, ROOT / "tests", ROOT / "tests" / "hipemu"):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HIPEMU_THREADS="2")
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import argparse

    import bench
    import transformers_amd
    from emu_backend import emu_backend
    from torch.nn.parallel import DistributedDataParallel as DDP
    from transformers_amd import ddp as tddp

    kind = "llama-tiles"
    with emu_backend():
        model, cfg = _build_model(kind)
        transformers_amd.accelerate(model)
        net = DDP(model, bucket_cap_mb=1, gradient_as_bucket_view=True, broadcast_buffers=False,
                  find_unused_parameters=False, static_graph=True)
        tddp.reset()
        tddp.enable_zero_copy(net)
        fwd = lambda n: n(**_batch(cfg, rank, kind))  # noqa: E731
        for _ in range(3):  # registry filled, buckets rebuilt, zero-copy running
            model.zero_grad(set_to_none=True)
            fwd(net).loss.backward()
        assert tddp.STATS["zero_copy_layers"] > 0
        note = tddp._note_views
        if rank == 1:
            p0, p1 = (model.model.layers[i].mlp.down_proj.weight for i in (0, 1))

            def corrupt(bucket):  # (the hook re-notes the views at every reduction: keep them swapped)
                note(bucket)
                if id(p0) in tddp._VIEWS and id(p1) in tddp._VIEWS:
                    (r0, v0), (r1, v1) = tddp._VIEWS[id(p0)], tddp._VIEWS[id(p1)]
                    if v0.data_ptr() < v1.data_ptr():
                        tddp._VIEWS[id(p0)], tddp._VIEWS[id(p1)] = (r0, v1), (r1, v0)

            tddp._note_views = corrupt
            (r0, v0), (r1, v1) = tddp._VIEWS[id(p0)], tddp._VIEWS[id(p1)]
            tddp._VIEWS[id(p0)], tddp._VIEWS[id(p1)] = (r0, v1), (r1, v0)
        a = argparse.Namespace(verify_ddp=True, no_ddp_breakdown=True, no_ddp_zero_copy=False, steps=1, warmup=0)
        verify = bench.ddp_verify_or_fall_back(a, net, model, fwd, torch.device("cpu"), world)
        state = dict(no_zero_copy=a.no_ddp_zero_copy, enabled=tddp._ENABLED)
        before = tddp.STATS["zero_copy_layers"]
        for _ in range(2):  # what bench.py then times: torch's copies (gradients zeroed in place: `--ddp-grads zero`)
            model.zero_grad(set_to_none=False)
            fwd(net).loss.backward()
        grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters()}
        state["zero_copy_layers_after_fallback"] = tddp.STATS["zero_copy_layers"] - before
        tddp._note_views = note
        tddp.set_enabled(True)
    torch.save({"verify": verify, "state": state, "grads": grads}, f"{out_dir}/rank{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_ddp_corrupted_view_falls_back_world2_gloo(tmp_path):
    """the first multi-rank run must not report a throughput measured on wrong gradients."""
    world = 2
    mp.spawn(_worker_corrupted_view, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(tmp_path / f"rank{i}.pt") for i in range(world)]
    for i in range(world):  # both ranks reached the same verdict, although only rank 1's registry was wrong
        v = r[i]["verify"]
        assert v["verified"] is False and v["bit_identical"] is False and v["disabled_zero_copy"] is True, v
        assert v["max_rel_err"] > 0.1, v
        assert r[i]["state"] == dict(no_zero_copy=True, enabled=False, zero_copy_layers_after_fallback=0), r[i]["state"]
    for n in r[0]["grads"]:
        assert torch.equal(r[0]["grads"][n], r[1]["grads"][n]), n
    for p in (ROOT, ROOT / "tests", ROOT / "tests" / "hipemu"):
        sys.path.insert(0, str(p))
    import transformers_amd
    from emu_backend import emu_backend

    per_rank = []
    with emu_backend():
        for rank in range(world):
            model, cfg = _build_model("llama-tiles")
            transformers_amd.accelerate(model)
            model(**_batch(cfg, rank, "llama-tiles")).loss.backward()
            per_rank.append({n: p.grad.detach().float() for n, p in model.named_parameters()})
    for n, gd in r[0]["grads"].items():
        want = (per_rank[0][n] + per_rank[1][n]) / 2
        err = (gd - want).norm() / want.norm().clamp_min(1e-12)
        assert err < 1e-2, (n, err.item())


def _run(cmd, timeout=900):
    import subprocess

    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    import json

    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_bench_ddp_path_over_rccl_world1():
    """the RCCL path had never executed.  `bench.py --force-ddp` at world size 1: process-group init over
    RCCL ("nccl" on ROCm), DDP wrap of the accelerated model (fused-weight views, bucket views of the gradients),
    bucketed all-reduce overlapped with the backward of the custom ops, destroy -- and the same loss as without DDP."""
    base = [sys.executable, "bench.py", "--config", "llama-tiny", "--steps", "3", "--warmup", "2", "--no-cpu-baseline", "--full"]
    plain = _run(base)
    ddp = _run(base + ["--force-ddp", "--verify-ddp"])
    assert "DDP over RCCL" in ddp["config"]["parallelism"] and ddp["n_gpus"] == 1
    assert abs(ddp["loss"] - plain["loss"]) < 1e-6
    assert ddp["value"] > 0.5 * plain["value"]
    # the zero-copy hand-over engaged (from the third step on) and nothing went wrong registering it
    zc = ddp["ddp_zero_copy"]
    assert zc["enabled"] and "error" not in zc and zc["zero_copy_layers"] > 0, zc
    assert ddp["ddp_verify"].get("bit_identical") is True and ddp["ddp_verify"]["zero_copy_layers_in_checked_step"] > 0, ddp["ddp_verify"]
    assert "breakdown_error" not in ddp["ddp"] and ddp["ddp"]["compute_only_ms"] > 0 and ddp["ddp"]["buckets_per_step"] >= 1
    assert plain["layer_forward"]["ms"] > 0 and plain["layer_forward"]["fallback_calls"] == 0


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_bench_ddp_collective_branch_over_rccl_world1():
    """transformers_amd/ddp.py's RCCL branch (`ReduceOp.AVG` in place, async, on the bucket the dW GEMMs wrote into) never ran
    on hardware: gloo takes the div + SUM branch and one rank takes the early return.  TAMD_DDP_WORLD1_COLLECTIVE=1 forces the
    collective at world size 1 (AVG over one rank = identity), so the branch the first 8-GPU run depends on executes here:
    same loss as without DDP, the zero-copy hand-over engaged, reduced gradients bit-identical to torch's copies."""
    import subprocess

    base = [sys.executable, "bench.py", "--config", "llama-tiny", "--steps", "3", "--warmup", "2", "--no-cpu-baseline"]
    plain = _run(base)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", TAMD_DDP_WORLD1_COLLECTIVE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(base + ["--force-ddp", "--verify-ddp"], capture_output=True, text=True, timeout=900, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    import json

    ddp = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    zc = ddp["ddp_zero_copy"]
    assert zc["collective"] == "all_reduce AVG in place (RCCL)", zc
    assert zc["enabled"] and "error" not in zc and zc["zero_copy_layers"] > 0, zc
    assert abs(ddp["loss"] - plain["loss"]) < 1e-6
    assert ddp["ddp_verify"].get("bit_identical") is True, ddp["ddp_verify"]


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_bench_self_launches_under_torchrun():
    """`python bench.py --gpus N` must launch itself (the driver may call it without torchrun).  One GPU is visible
    here, so N = 1 through the launcher: `torch.distributed.run --nproc-per-node 1 bench.py --gpus 1` is the same code
    path the 8-GPU run takes (RANK / WORLD_SIZE / MASTER_* from the environment)."""
    import socket as _s

    with _s.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
                "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "1", "--config", "llama-tiny", "--steps",
                "2", "--warmup", "1", "--no-cpu-baseline", "--force-ddp"])
    assert out["n_gpus"] == 1 and out["value"] > 0


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_trainer_ddp_script_world1(tmp_path):
    """tools/train_ddp.py: torchrun + the reference's unchanged Trainer (DDP kwargs from TrainingArguments,
    trainer.py:720-737) + TamdAdamW, world size 1 on the one visible GPU."""
    out = _run([sys.executable, "tools/train_ddp.py", "--nproc", "1", "--max_steps", "3", "--output_dir", str(tmp_path)])
    assert out["steps"] == 3 and out["replicas_identical"] and out["attn_implementation"] == "tamd"
    assert out["ddp"] in ("DistributedDataParallel", "LlamaForCausalLM") and out["optimizer"].endswith("TamdAdamW")
    assert all(l == l and l < 20 for l in out["losses"])


def test_bench_self_launch_command_line(monkeypatch):
    """Host logic of the self-launcher (no GPU): `--gpus 4` without RANK/WORLD_SIZE re-executes under
    torch.distributed.run with one rank per GPU on 127.0.0.1."""
    sys.path.insert(0, str(ROOT))
    import bench

    seen = {}
    monkeypatch.setattr(bench.subprocess, "call", lambda cmd, env=None: seen.update(cmd=cmd, env=env) or 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    for k in ("RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-4:] == ["--gpus", "4", "--steps", "3"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


@pytest.mark.timeout(900)
def test_trainer_ddp_script_world2_gloo(tmp_path):
    """tools/train_ddp.py end to end on CPU: torch.distributed.run with 2 ranks, gloo, the reference's unchanged Trainer
    wrapping the accelerated model in DDP, TamdAdamW; replicas end bit-identical."""
    out = _run([sys.executable, "tools/train_ddp.py", "--nproc", "2", "--emu", "--max_steps", "4", "--seq", "32",
                "--per_device_train_batch_size", "2", "--output_dir", str(tmp_path)])
    assert out["world_size"] == 2 and out["steps"] == 4 and out["replicas_identical"]
    assert out["ddp"] == "DistributedDataParallel" and out["optimizer"] == "TamdAdamW"
    assert out["attn_implementation"] == "tamd" and out["losses"][1] < out["losses"][0]
    # the drop-in path gets the zero-copy hand-over too (VERDICT r4 missing 4): the Trainer passed no gradient_as_bucket_view and
    # registered no hook -- accelerate() arranged both; from the third step on (views noted, buckets rebuilt once) the layer
    # backwards write their weight gradients into the all-reduce buckets
    assert out["gradient_as_bucket_view"] is True
    assert out["ddp_zero_copy"]["buckets_reduced"] > 0 and out["ddp_zero_copy"]["zero_copy_layers"] > 0, out["ddp_zero_copy"]


def _worker_ctor_dropin(out_path, port):
    """one process, gloo: what ddp.install_trainer_dropin does to DistributedDataParallel's constructor -- and what it leaves alone"""
    import json
    import os

    import torch
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=0, world_size=1)
    import transformers_amd
    from transformers_amd import ddp as tddp

    res = {}
    plain = torch.nn.Linear(8, 8)
    tddp.install_trainer_dropin()
    res["plain_views"] = bool(DDP(plain).gradient_as_bucket_view)                      # not ours: the constructor it always saw
    marked = torch.nn.Linear(8, 8)
    marked._tamd_swapped = 1                                                           # what accelerate() leaves on a model
    d = DDP(marked)
    res["marked_views"] = bool(d.gradient_as_bucket_view)
    res["explicit_false"] = bool(DDP(marked, gradient_as_bucket_view=False).gradient_as_bucket_view)  # the caller's choice wins
    d(torch.randn(2, 8)).sum().backward()                                              # first forward registers the hook
    res["hook_registered"] = getattr(d, "_tamd_hook_state", None) is not None
    res["buckets_reduced"] = tddp.STATS["buckets_reduced"]
    theirs = DDP(marked)
    from torch.distributed.algorithms.ddp_comm_hooks import default_hooks

    theirs.register_comm_hook(None, default_hooks.allreduce_hook)                      # the user's hook (accelerate does this)
    theirs(torch.randn(2, 8)).sum().backward()
    res["their_hook_kept"] = getattr(theirs, "_tamd_hook_state", "unset") is None
    os.environ["TAMD_DDP_ZERO_COPY"] = "0"
    res["env_off"] = bool(DDP(marked).gradient_as_bucket_view)
    dist.destroy_process_group()
    with open(out_path, "w") as f:
        json.dump(res, f)


@pytest.mark.timeout(300)
def test_trainer_dropin_only_touches_accelerated_models(tmp_path):
    """`accelerate()` wraps DistributedDataParallel.__init__ once (ddp.install_trainer_dropin): bucket views + the zero-copy hook for
    models it marked, nothing for other modules, an explicit `gradient_as_bucket_view`, a user's own communication hook or
    TAMD_DDP_ZERO_COPY=0."""
    import json

    import torch.multiprocessing as mp

    out = tmp_path / "ctor.json"
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_worker_ctor_dropin, args=(str(out), _free_port()))
    p.start()
    p.join(240)
    assert p.exitcode == 0
    res = json.loads(out.read_text())
    assert res == {"plain_views": False, "marked_views": True, "explicit_false": False, "hook_registered": True,
                   "buckets_reduced": res["buckets_reduced"], "their_hook_kept": True, "env_off": False}, res
    assert res["buckets_reduced"] >= 1


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_train_step_and_secondary_legs_on_the_gpu():
    """`bench.py --train-step` (forward, backward, gradient-norm clip and AdamW on the kernels) prints the
    optimizer's share, and the `secondary` legs of the headline run are child processes whose failure cannot touch the parent:
    a leg that works, one that crashes and one that times out, through the same function the headline run calls."""
    sys.path.insert(0, str(ROOT))
    import bench

    tiny = ["--config", "llama-tiny", "--steps", "2", "--warmup", "1"]
    out = bench.secondary_legs(timeout_s=600, legs={"train_step": tiny + ["--train-step"], "crash": ["--config", "no-such-config"]})
    ts = out["train_step"]
    assert "error" not in ts and ts["fallback_calls"] == 0, ts
    assert ts["optimizer_ms"] > 0 and ts["grad_norm"] > 0 and ts["ms_per_step"] > ts["optimizer_ms"], ts
    assert "TamdAdamW" in ts["optimizer"] and ts["metric"].startswith("training-step")
    assert "error" in out["crash"] and out["crash"]["leg_wall_s"] >= 0
    slow = bench.secondary_legs(timeout_s=1, legs={"hang": tiny})
    assert "timeout" in slow["hang"]["error"]
    # the A/B arm: torch's clip + fused AdamW through the same step
    ref = _run([sys.executable, "bench.py", *tiny, "--train-step", "--optimizer", "torch", "--no-cpu-baseline", "--no-secondary"])
    assert ref["train_step"]["optimizer"].startswith("torch.nn.utils.clip_grad_norm_") and ref["train_step"]["optimizer_ms"] > 0
