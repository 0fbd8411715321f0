"""The sigmoid, group-limited router: the reference module (A: DeepseekV3TopkRouter.forward -- two casts to fp32, an fp32
`F.linear` and close to twenty small ATen launches) against the replacement of transformers_amd/models/moe.py (B:
ops.moe_gate_logits + ONE launch of ops.moe_router_grouped), bf16, at
    deepseek-v3   E 256, H 7168, 8 groups / 4 chosen, top-8, scale 2.5
    glm-4.5-air   E 128, H 4096, one group, top-8
T in {1, 16, 512, 8192} tokens, forward (no grad) and forward + backward.  One process; per point the arms run A B A B, each run
the median of `--windows` (3; 7 for forward + backward) windows of `--iters` calls between HIP events behind a warm-up; every line
carries the clock probe's readings taken right before and right after its point.  `new_not_slower`: the SLOWER of the two B
runs against the FASTER of the two A runs, widened by the spread of the A runs.  Next to them, per point, the two parts alone:
the gate product (A: the two casts + fp32 F.linear; B: ops.moe_gate_logits) and the selection on logits that exist already (A:
the reference's lines behind its product; B: ops.moe_router_grouped); for T <= 16 the share of the weight-bytes floor
(E H 2 bytes at `--hbm-tbs`, 8 TB/s) the gate kernel reaches.
    python tools/moe_router_group_bench.py [--iters 50] [--out profiles/moe_router_group_ab.jsonl]   (appends JSON lines)"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from moe_router_bench import median3  # noqa: E402

GEOMETRIES = {"deepseek-v3": dict(e=256, h=7168, n_group=8, topk_group=4, k=8, scale=2.5),
              "glm-4.5-air": dict(e=128, h=4096, n_group=1, topk_group=1, k=8, scale=1.0)}
TOKENS = (1, 16, 512, 8192)


def routers(torch, g, dev):
    """-> (reference module, replacement module) sharing one weight and one bias"""
    from transformers import DeepseekV3Config
    from transformers.models.deepseek_v3.modeling_deepseek_v3 import DeepseekV3TopkRouter as Ref

    from transformers_amd.models import moe

    cfg = DeepseekV3Config(hidden_size=g["h"], n_routed_experts=g["e"], num_experts_per_tok=g["k"], n_group=g["n_group"],
                           topk_group=g["topk_group"], routed_scaling_factor=g["scale"], norm_topk_prob=True)
    ref = Ref(cfg)
    torch.nn.init.normal_(ref.weight, std=0.02)
    ref.e_score_correction_bias = (torch.rand(g["e"]) - 0.5) * 0.1
    ref = ref.to(dev)
    ref.weight.data = ref.weight.data.bfloat16()  # (the bias stays fp32: what from_pretrained keeps)
    new = moe.REPLACEMENTS[Ref](cfg).to(dev)
    new.weight = ref.weight
    new.e_score_correction_bias = ref.e_score_correction_bias
    return ref, new


def reference_selection(torch, self, router_logits):
    """DeepseekV3TopkRouter.forward behind its gate product (modeling_deepseek_v3.py:148-169)"""
    scores = router_logits.sigmoid()
    scores_for_choice = scores + self.e_score_correction_bias
    group_scores = scores_for_choice.view(-1, self.num_group, self.num_experts // self.num_group).topk(2, dim=-1)[0].sum(dim=-1)
    group_idx = torch.topk(group_scores, k=self.topk_group, dim=-1, sorted=False)[1]
    group_mask = torch.zeros_like(group_scores)
    group_mask.scatter_(1, group_idx, 1)
    score_mask = group_mask.unsqueeze(-1).expand(-1, self.num_group, self.num_experts // self.num_group).reshape(-1, self.num_experts)
    scores_for_choice = scores_for_choice.masked_fill(~score_mask.bool(), float("-inf"))
    topk_indices = torch.topk(scores_for_choice, k=self.top_k, dim=-1, sorted=False)[1]
    topk_weights = scores.gather(1, topk_indices)
    if self.norm_topk_prob:
        topk_weights /= topk_weights.sum(dim=-1, keepdim=True) + 1e-20
    return topk_weights * self.routed_scaling_factor, topk_indices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--train-windows", type=int, default=7)
    ap.add_argument("--modes", nargs="+", default=["fwd", "fwd+bwd"])
    ap.add_argument("--geometries", nargs="+", default=list(GEOMETRIES))
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "moe_router_group_ab.jsonl"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F

    import bench
    import transformers_amd
    from transformers_amd import experts, ops

    dev = torch.device("cuda:0")
    out = open(args.out, "a")

    def probe():
        c = bench.clock_probe(dev)
        return dict(clock_GHz=round(c["clock_GHz"], 4), TFLOPs=round(c["TFLOPs"], 1))

    def emit(rec):
        line = json.dumps(rec)
        out.write(line + "\n")
        out.flush()
        print(line, flush=True)

    for name in args.geometries:
        g = GEOMETRIES[name]
        ref, new = routers(torch, g, dev)
        for mode in args.modes:
            train = mode != "fwd"
            for t in TOKENS:
                clock_before = probe()
                x = torch.randn(t, g["h"], generator=torch.Generator().manual_seed(t)).bfloat16().to(dev)
                x.requires_grad_(train)
                ref.weight.requires_grad_(train)
                iters = max(5, args.iters // (1 + t // 2048))

                def call(mod):
                    if not train:
                        with torch.no_grad():
                            return mod(x)
                    _logits, weights, _idx = mod(x)
                    (weights.sum() * 0.5).backward()  # (a gradient for every weight: dX and dW of the gate product too)
                    x.grad = None
                    ref.weight.grad = None

                transformers_amd.fallback_calls(reset=True)
                experts.router_call_count(reset=True)
                runs = {}
                for label in ("A1", "B1", "A2", "B2"):
                    mod = ref if label.startswith("A") else new
                    runs[label] = median3(torch, lambda: call(mod), iters, args.train_windows if train else args.windows)
                assert transformers_amd.fallback_calls() == {} and experts.router_call_count() > 0
                a, b = (runs["A1"][0], runs["A2"][0]), (runs["B1"][0], runs["B2"][0])
                spread = abs(a[0] - a[1]) / min(a)
                rec = dict(kind="router_group", geometry=name, mode=mode, tokens=t, e=g["e"], h=g["h"], n_group=g["n_group"],
                           topk_group=g["topk_group"], top_k=g["k"], iters=iters, reference_us=list(a), new_us=list(b),
                           windows={k_: v[1] for k_, v in runs.items()}, reference_spread=round(spread, 4),
                           reference_over_new=round(sum(a) / sum(b), 3), new_not_slower=bool(max(b) <= min(a) * (1 + spread)))
                if not train:
                    with torch.no_grad():
                        w = ref.weight
                        logits = ops.moe_gate_logits(x, w)
                        bias = ref.e_score_correction_bias
                        rec["gate_product_us"] = dict(
                            reference=median3(torch, lambda: F.linear(x.type(torch.float32), w.type(torch.float32)), iters)[0],
                            new=median3(torch, lambda: ops.moe_gate_logits(x, w), iters)[0])
                        rec["selection_us"] = dict(
                            reference=median3(torch, lambda: reference_selection(torch, ref, logits), iters)[0],
                            new=median3(torch, lambda: ops.moe_router_grouped(logits, bias, g["k"], g["n_group"], g["topk_group"],
                                                                              True, g["scale"]), iters)[0])
                        if t <= 16:
                            floor_us = g["e"] * g["h"] * 2 / (args.hbm_tbs * 1e12) * 1e6
                            rec["gate_weight_bytes_floor_us"] = round(floor_us, 3)
                            rec["gate_share_of_floor"] = round(floor_us / rec["gate_product_us"]["new"], 4)
                rec["clock_probe"] = dict(before=clock_before, after=probe())
                emit(rec)
    out.close()


if __name__ == "__main__":
    main()
