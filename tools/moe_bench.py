"""The experts module of a sparse mixture-of-experts block under experts_implementation "tamd" (torch.ops.tamd.moe_experts),
under the reference's "grouped_mm" and under its "eager" per-expert loop: forward and forward + backward, interleaved in one
process behind a warm-up, min of 3 rounds -- at the Mixtral-8x7B layer shape (H 4096, I 14336, 8 experts, top-2) and at a
many-small-experts shape (H 2048, I 768, 128 experts, top-8), 8192 tokens each.  Also, per shape:
  * routing + gather + combine alone (the kernels of csrc/moe_route.inc),
  * the routed gate|up product with the SiLU*up way out and the routed down product in TFLOP/s beside the dense
    tamd_gemm_swiglu / tamd_gemm over the same number of rows (one expert's weight): the ceiling routing can approach, not pass,
  * which path the reference's "grouped_mm" took on this build (it falls back to a loop where torch's grouped_mm is missing).
   python tools/moe_bench.py [--quick] > profiles/moe_experts_ab.jsonl"""
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import transformers_amd  # noqa: E402,F401
from transformers import MixtralConfig  # noqa: E402
from transformers.integrations import moe as ref_moe  # noqa: E402
from transformers.models.mixtral.modeling_mixtral import MixtralExperts  # noqa: E402
from transformers_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
QUICK = "--quick" in sys.argv


def timeit(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


SHAPES = {"mixtral-8x7b layer": dict(h=4096, inter=14336, e=8, k=2, t=8192),
          "128 small experts": dict(h=2048, inter=768, e=128, k=8, t=8192)}
for name, sh in SHAPES.items():
    h, inter, e, k, t = sh["h"], sh["inter"], sh["e"], sh["k"], sh["t"]
    torch.manual_seed(0)
    cfg = MixtralConfig(hidden_size=h, intermediate_size=inter, num_local_experts=e, num_experts_per_tok=k, num_hidden_layers=1,
                        num_attention_heads=2, num_key_value_heads=1, vocab_size=64)
    with torch.device(dev):
        mod = MixtralExperts(cfg).bfloat16()
    with torch.no_grad():
        mod.gate_up_proj.normal_(std=0.02)
        mod.down_proj.normal_(std=0.02)
    x = torch.randn(t, h, device=dev).bfloat16().requires_grad_(True)
    probs = torch.softmax(torch.randn(t, e, device=dev), -1)
    w, idx = torch.topk(probs, k, -1)
    w = (w / w.sum(-1, keepdim=True)).requires_grad_(True)
    dout = torch.randn(t, h, device=dev).bfloat16()

    def arm(key):
        cfg._experts_implementation = key

        def fwd():
            with torch.no_grad():
                return mod(x, idx, w)

        def both():
            out = mod(x, idx, w)
            out.backward(dout)
            x.grad = w.grad = mod.gate_up_proj.grad = mod.down_proj.grad = None

        return fwd, both

    arms = {key: arm(key) for key in ("tamd", "grouped_mm", "eager")}
    iters = 3 if QUICK else 10
    times = {f"{key}_{what}": [] for key in arms for what in ("fwd", "fwd_bwd")}
    for _ in range(3):
        for key in arms:
            cfg._experts_implementation = key
            fwd, both = arm(key)
            times[f"{key}_fwd"].append(timeit(fwd, iters))
            times[f"{key}_fwd_bwd"].append(timeit(both, iters))
    rec = {"case": name, **sh}
    for kk, v in times.items():
        rec[kk + "_us"] = round(min(v), 1)
    # agreement of the three paths (relative to eager)
    outs = {}
    for key in arms:
        cfg._experts_implementation = key
        with torch.no_grad():
            outs[key] = mod(x, idx, w).float()
    rec["tamd_vs_eager_rel"] = float((outs["tamd"] - outs["eager"]).norm() / outs["eager"].norm())
    rec["grouped_vs_eager_rel"] = float((outs["grouped_mm"] - outs["eager"]).norm() / outs["eager"].norm())
    probe_w = torch.zeros(2, 16, 16, device=dev).bfloat16()
    rec["reference_grouped_mm_path"] = ("torch grouped_mm" if ref_moe._can_use_grouped_mm(torch.zeros(32, 16, device=dev).bfloat16(), probe_w,
                                                                                         torch.tensor([16, 32], device=dev, dtype=torch.int32))
                                        else "the reference's own fallback loop (_grouped_mm_fallback)")
    # routing + gather + combine alone
    xd = x.detach()
    count, offset, pos, tiles = ops.raw_moe_route(idx, e)
    xs = ops.raw_moe_gather(xd, pos, count, offset)

    def plumbing():
        c, o, p, _ = ops.raw_moe_route(idx, e)
        s = ops.raw_moe_gather(xd, p, c, o)
        ops.raw_moe_combine(s, p, w.detach())

    rec["route_gather_combine_us"] = round(min(timeit(plumbing, iters) for _ in range(3)), 1)
    # routed products against dense ones over the same rows
    pairs = t * k
    wgu, wd = mod.gate_up_proj.detach(), mod.down_proj.detach()
    act = torch.empty(xs.shape[0], inter, device=dev, dtype=torch.bfloat16)
    dense_x = xs[:pairs]
    dense_act = act[:pairs]
    f_gu, f_dn = 2.0 * pairs * 2 * inter * h, 2.0 * pairs * h * inter
    r_gu = min(timeit(lambda: ops.raw_gemm_routed(xs, wgu, offset, tiles, ops.ROUTED_SWIGLU, out2=act, need_gu=False), iters) for _ in range(3))
    d_gu = min(timeit(lambda: ops.raw_gemm_swiglu(dense_x, wgu[0], need_gu=False), iters) for _ in range(3))
    r_dn = min(timeit(lambda: ops.raw_gemm_routed(act, wd, offset, tiles, ops.ROUTED_NT), iters) for _ in range(3))
    d_dn = min(timeit(lambda: ops.raw_gemm(dense_act, wd[0]), iters) for _ in range(3))
    rec.update(routed_swiglu_us=round(r_gu, 1), routed_swiglu_TF=round(f_gu / r_gu / 1e6, 1), dense_swiglu_us=round(d_gu, 1),
               dense_swiglu_TF=round(f_gu / d_gu / 1e6, 1), routed_down_us=round(r_dn, 1), routed_down_TF=round(f_dn / r_dn / 1e6, 1),
               dense_down_us=round(d_dn, 1), dense_down_TF=round(f_dn / d_dn / 1e6, 1), rows_pad=int(xs.shape[0]),
               rows_in_segments=int(offset[-1]))
    print(json.dumps(rec), flush=True)
    del mod, x, xs, act
    torch.cuda.empty_cache()
