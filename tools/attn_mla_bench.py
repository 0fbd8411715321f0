"""MLA attention at the DeepSeek-V3 head shape (128 heads, q / k rows of 192, v rows of 128, bf16): the MLA kernel
(ops.raw_attn_fwd -> tamd_attn_fwd_mla / tamd_attn_decode_mla) against torch's scaled_dot_product_attention on the same
operands (the reference's sdpa path).  Points: a 4096-token prefill; 8 rows over 4096 keys; one row over 4096 and over 32768
keys.  The two arms alternate inside one process; one JSON line per point, appended to --out when given.

    python tools/attn_mla_bench.py [--out profiles/attn_mla_ab.jsonl]
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
ap.add_argument("--heads", type=int, default=128)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
H, DQK, DV = args.heads, 192, 128
scale = DQK ** -0.5


def timed(fn, iters):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(iters):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / iters


POINTS = [("prefill", 1, 4096, 4096, 10), ("rows8", 1, 8, 4096, 200), ("row1", 8, 1, 4096, 200), ("row1_32k", 8, 1, 32768, 100)]
torch.manual_seed(0)
for name, b, sq, sk, iters in POINTS:
    q = torch.randn(b, sq, H, DQK, device=dev).bfloat16()
    k = torch.randn(b, sk, H, DQK, device=dev).bfloat16()
    v = torch.randn(b, sk, H, 2 * DV, device=dev).bfloat16()[..., DV:]  # the right half of kv_b_proj's output, as the reference slices it
    causal = sq > 1
    qt, kt, vt = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    if causal and sq != sk:  # (torch's is_causal is top-left aligned: the bottom-right mask as a tensor)
        bias = torch.ones(sq, sk, dtype=torch.bool, device=dev).tril(sk - sq)
        arms = {"tamd": lambda: ops.raw_attn_fwd(q, k, v, scale, True, need_lse=False),
                "sdpa": lambda: F.scaled_dot_product_attention(qt, kt, vt, attn_mask=bias, scale=scale)}
    else:
        arms = {"tamd": lambda: ops.raw_attn_fwd(q, k, v, scale, causal, need_lse=False),
                "sdpa": lambda: F.scaled_dot_product_attention(qt, kt, vt, is_causal=causal, scale=scale)}
    o = arms["tamd"]()[0].float()
    r = arms["sdpa"]().transpose(1, 2).float()
    err = float((o - r).norm() / r.norm())
    for fn in arms.values():  # warm-up of both arms
        timed(fn, 3)
    ms = {a: [] for a in arms}
    for _ in range(args.rounds):  # alternating
        for a, fn in arms.items():
            ms[a].append(timed(fn, iters))
    pairs = sq * (2 * sk - sq + 1) / 2 if causal else sq * sk
    best = {a: min(x) for a, x in ms.items()}
    rec = {"point": name, "batch": b, "seq_q": sq, "seq_k": sk, "heads": H, "dtype": "bf16", "rel_diff_vs_sdpa": round(err, 5),
           "tamd_ms": [round(x, 4) for x in ms["tamd"]], "sdpa_ms": [round(x, 4) for x in ms["sdpa"]],
           "tamd_TFLOPs": round(2.0 * b * H * pairs * (DQK + DV) / (best["tamd"] * 1e-3) / 1e12, 1),
           "kv_GBps_tamd": round(b * sk * H * (DQK + DV) * 2 / (best["tamd"] * 1e-3) / 1e9, 1),
           "sdpa_over_tamd": round(best["sdpa"] / best["tamd"], 3), "clock_probe": "not measured"}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
