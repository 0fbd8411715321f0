"""The router of a sparse-MoE block: the reference module (A: `F.linear`, softmax, topk, sum, div, .to() through ATen) against the
replacement of transformers_amd/models/moe.py (B: the gate product on ops.linear + ONE launch of ops.moe_router), bf16, at
    mixtral-8x7b    E 8,   top-2, H 4096   (MixtralTopKRouter: fp32 scores, renormalised)
    qwen3-moe-like  E 128, top-8, H 2048   (Qwen3MoeTopKRouter: scores in bf16, norm_topk_prob)
T in {1, 4, 16, 512, 8192} tokens forward (no grad), forward + backward at 512 and 8192.  One process; per point the arms run
A B A B, each run the median of `--windows` (3; 7 for forward + backward, whose windows scatter more) windows of `--iters` calls
between HIP events behind a warm-up; every line carries the clock probe's readings taken right before and right after its point.
`new_not_slower`: the SLOWER of the two B runs against the FASTER of the two A runs, widened by the spread of the A runs.  Next to them, per point: the router kernel alone (`ops.moe_router` on logits that
exist already) and the experts call of the same shape (`ops.moe_experts`, forward, I = 14336 / 768), to show what share of the
block the router is.
    python tools/moe_router_bench.py [--iters 50] [--out profiles/moe_router_ab.jsonl]   (appends JSON lines)"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

GEOMETRIES = {"mixtral-8x7b": dict(e=8, k=2, h=4096, inter=14336, family="mixtral"),
              "qwen3-moe-like": dict(e=128, k=8, h=2048, inter=768, family="qwen3")}
TOKENS = (1, 4, 16, 512, 8192)
TRAIN_TOKENS = (512, 8192)


def window(torch, fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def median3(torch, fn, iters, windows=3):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    w = sorted(window(torch, fn, iters) for _ in range(windows))
    return round(w[len(w) // 2], 2), [round(v, 2) for v in w]


def routers(torch, g, dev):
    """-> (reference module, replacement module) sharing one weight"""
    from transformers_amd.models import moe

    if g["family"] == "mixtral":
        from transformers import MixtralConfig
        from transformers.models.mixtral.modeling_mixtral import MixtralTopKRouter as Ref

        cfg = MixtralConfig(hidden_size=g["h"], num_local_experts=g["e"], num_experts_per_tok=g["k"])
    else:
        from transformers import Qwen3MoeConfig
        from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeTopKRouter as Ref

        cfg = Qwen3MoeConfig(hidden_size=g["h"], num_experts=g["e"], num_experts_per_tok=g["k"], norm_topk_prob=True)
    ref = Ref(cfg)
    torch.nn.init.normal_(ref.weight, std=0.02)
    ref = ref.to(dev).bfloat16()
    new = moe.REPLACEMENTS[Ref](cfg).to(dev).bfloat16()
    new.weight = ref.weight
    return ref, new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--train-windows", type=int, default=7)
    ap.add_argument("--modes", nargs="+", default=["fwd", "fwd+bwd"])
    ap.add_argument("--geometries", nargs="+", default=list(GEOMETRIES))
    ap.add_argument("--no-experts", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "moe_router_ab.jsonl"))
    args = ap.parse_args()
    import torch

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
        wgu = wd = None
        if not args.no_experts:
            wgu = torch.randn(g["e"], 2 * g["inter"], g["h"], device=dev, dtype=torch.bfloat16) * 0.02
            wd = torch.randn(g["e"], g["h"], g["inter"], device=dev, dtype=torch.bfloat16) * 0.02
        for mode, tokens in (("fwd", TOKENS), ("fwd+bwd", TRAIN_TOKENS)):
            if mode not in args.modes:
                continue
            for t in tokens:
                clock_before = probe()
                x = torch.randn(t, g["h"], generator=torch.Generator().manual_seed(t)).bfloat16().to(dev)
                train = mode != "fwd"
                x.requires_grad_(train)
                ref.weight.requires_grad_(train)

                def call(mod):
                    if not train:
                        with torch.no_grad():
                            return mod(x)
                    logits, scores, _idx = mod(x)
                    (scores.float().sum() * 0.5).backward()  # (a gradient for every score: dX and dW of the gate product too)
                    x.grad = None
                    ref.weight.grad = None

                transformers_amd.fallback_calls(reset=True)
                experts.router_call_count(reset=True)
                runs = {}
                for label in ("A1", "B1", "A2", "B2"):
                    mod = ref if label.startswith("A") else new
                    runs[label] = median3(torch, lambda: call(mod), args.iters, args.train_windows if train else args.windows)
                assert transformers_amd.fallback_calls() == {} and experts.router_call_count() > 0
                a, b = (runs["A1"][0], runs["A2"][0]), (runs["B1"][0], runs["B2"][0])
                spread = abs(a[0] - a[1]) / min(a)
                rec = dict(kind="router", geometry=name, mode=mode, tokens=t, e=g["e"], top_k=g["k"], h=g["h"], iters=args.iters,
                           reference_us=list(a), new_us=list(b), windows={k_: v[1] for k_, v in runs.items()},
                           reference_spread=round(spread, 4), reference_over_new=round(sum(a) / sum(b), 3),
                           new_not_slower=bool(max(b) <= min(a) * (1 + spread)))
                if not train:
                    with torch.no_grad():
                        logits = ops.linear(x, ref.weight)
                        fp32 = g["family"] == "mixtral"
                        rec["router_kernel_us"] = median3(torch, lambda: ops.moe_router(logits, g["k"], True, fp32), args.iters)[0]
                        rec["gate_product_us"] = median3(torch, lambda: ops.linear(x, ref.weight), args.iters)[0]
                        if wgu is not None:
                            _l, s, idx = new(x)
                            it = max(3, args.iters // (1 + t // 512))
                            rec["experts_us"] = median3(torch, lambda: ops.moe_experts(x, idx, s, wgu, wd), it)[0]
                            rec["router_share_of_block"] = dict(
                                reference=round(sum(a) / 2 / (sum(a) / 2 + rec["experts_us"]), 4),
                                new=round(sum(b) / 2 / (sum(b) / 2 + rec["experts_us"]), 4))
                rec["clock_probe"] = dict(before=clock_before, after=probe())
                emit(rec)
        del wgu, wd
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
