"""Attention at head_dim 256 (Gemma, bf16): the head_dim-256 kernel (ops.raw_attn_fwd -> tamd_attn_fwd / tamd_attn_decode)
against torch's scaled_dot_product_attention on the same operands, and -- a second yardstick -- the product forward at head_dim
128 with twice the heads: the same FLOPs and the same bytes in the same run.  Points: a 4096-token causal prefill at Gemma-7B
heads (16 / 16); at Gemma-3-12B heads (16 / 8) 8 rows over 4096 keys, one row per sequence at batch 8 over 4096 and over 32768
keys.  The arms alternate inside one process; one JSON line per point, appended to --out when given.

    python tools/attn_d256_bench.py [--out profiles/attn_d256_ab.jsonl]
"""
import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from transformers_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
D = 256
scale = D ** -0.5


def timed(fn, iters):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(iters):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / iters


POINTS = [("prefill", 1, 4096, 4096, 16, 16, 500), ("rows8", 1, 8, 4096, 16, 8, 2000), ("row1", 8, 1, 4096, 16, 8, 2000),
          ("row1_32k", 8, 1, 32768, 16, 8, 300)]  # (iterations: a timed window of at least ~50 ms)
torch.manual_seed(0)
for name, b, sq, sk, hq, hkv, iters in POINTS:
    q = torch.randn(b, sq, hq, D, device=dev).bfloat16()
    k = torch.randn(b, sk, hkv, D, device=dev).bfloat16()
    v = torch.randn(b, sk, hkv, D, device=dev).bfloat16()
    # the yardstick: every head cut into two heads of 128 -- another function, the same work
    q2, k2, v2 = q.view(b, sq, 2 * hq, 128), k.view(b, sk, 2 * hkv, 128), v.view(b, sk, 2 * hkv, 128)
    causal = sq > 1
    qt, kt, vt = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    mask = torch.ones(sq, sk, dtype=torch.bool, device=dev).tril(sk - sq) if causal and sq != sk else None  # (bottom-right)
    arms = {"tamd": lambda: ops.raw_attn_fwd(q, k, v, scale, causal, need_lse=False),
            "sdpa": lambda: F.scaled_dot_product_attention(qt, kt, vt, attn_mask=mask, is_causal=causal and mask is None,
                                                           scale=scale, enable_gqa=hq != hkv),
            "tamd_d128_2x_heads": lambda: ops.raw_attn_fwd(q2, k2, v2, 128 ** -0.5, causal, need_lse=False)}
    o = arms["tamd"]()[0].float()
    r = arms["sdpa"]().transpose(1, 2).float()
    err = float((o - r).norm() / r.norm())
    for fn in arms.values():  # warm-up of every arm
        timed(fn, 3)
    ms = {a: [] for a in arms}
    for _ in range(args.rounds):  # alternating
        for a, fn in arms.items():
            ms[a].append(timed(fn, iters))
    pairs = sq * (2 * sk - sq + 1) / 2 if causal else sq * sk
    med = {a: sorted(x)[len(x) // 2] for a, x in ms.items()}
    rec = {"point": name, "batch": b, "seq_q": sq, "seq_k": sk, "heads_q": hq, "heads_kv": hkv, "dtype": "bf16",
           "rel_diff_vs_sdpa": round(err, 5), **{f"{a}_ms": [round(x, 4) for x in ms[a]] for a in arms},
           **{f"{a}_median_ms": round(med[a], 4) for a in arms},
           "tamd_TFLOPs": round(4.0 * b * hq * pairs * D / (med["tamd"] * 1e-3) / 1e12, 1),
           "d128_2x_heads_TFLOPs": round(4.0 * b * hq * pairs * D / (med["tamd_d128_2x_heads"] * 1e-3) / 1e12, 1),
           "kv_TBps_tamd": round(b * sk * hkv * 2 * D * 2 / (med["tamd"] * 1e-3) / 1e12, 3),
           "kv_TBps_d128_2x_heads": round(b * sk * hkv * 2 * D * 2 / (med["tamd_d128_2x_heads"] * 1e-3) / 1e12, 3),
           "sdpa_over_tamd": round(med["sdpa"] / med["tamd"], 3), "clock_probe": "not measured"}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
