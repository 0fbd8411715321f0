"""FP8 block-scaled linear (torch.ops.tamd.linear_fp8w: csrc/gemv_fp8.inc, csrc/gemm_fp8w.inc) against this project's bf16 product on
the same N, K (ops.linear: csrc/gemv.hip at M <= 16, the GEMM kernels above) -- the yardstick: the streaming form reads half the
bytes -- and, with --reference where its Triton path runs on the box, the reference's FP8Linear.forward.  DeepSeek-V3 dense shapes
at M = 1 .. 4096 (--rows).  The ops run through libtamd_diag.so, whose switches (read at every call) give the arms:
  fp8w          the product's rule
  fp8w_before   the code as it ran before the kernel that now serves this M: up to 16 rows TAMD_FP8W_MFMA=0 (the streaming kernel);
                above, TAMD_FP8W_TILE=0: the parent's paths (gemv_fp8w_mfma_kernel up to 64 rows, dequantise + GEMM above)
  fp8w_mfma     2 and 4 rows, where the rule chooses per shape: TAMD_FP8W_MFMA=2 forces gemv_fp8w_mfma_kernel
  fp8w_tile     above 16 rows: TAMD_FP8W_TILE=2 forces gemm_fp8w_kernel; fp8w_tile64 / fp8w_tile128 (from 128 rows on) also fix its
                rows of X per workgroup (TAMD_FP8W_TILE_BM)

Every arm walks a ring of weight copies larger than the 256 MB of last-level cache, so each launch streams its weights from HBM;
the arms alternate inside one process; one JSON line per point, appended to --out when given.  Times are per call (device events
around a window of calls, launch overhead included), and the TB/s fields are the algorithmic bytes over that per-call time: not
kernel time.  `<arm>_spread` is (max - min) / median over the rounds of that arm.

    python tools/fp8_linear_bench.py [--rows 32,48,64,128,512,4096] [--out profiles/fp8_linear_ab.jsonl]
"""
import argparse
import json
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import _diag  # noqa: E402
from transformers_amd import ops  # noqa: E402

_diag.use_diag()

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--rows", default="1,2,4,8,16,32,48,64,128,512,4096", help="comma-separated M values")
ap.add_argument("--ring-bytes", type=int, default=640 << 20)
ap.add_argument("--reference", action="store_true",
                help="also time FP8Linear.forward (its Triton kernel comes from the `kernels` hub package: needs that package and its cache)")
args = ap.parse_args()
dev = torch.device("cuda:0")
SHAPES = [(7168, 1536), (7168, 576), (1536, 24576), (16384, 7168), (7168, 18432), (18432, 7168)]  # K -> N
ROWS = [int(v) for v in args.rows.split(",")]
KNOBS = ("TAMD_FP8W_MFMA", "TAMD_FP8W_TILE", "TAMD_FP8W_TILE_BM")
SWITCH = {"fp8w_mfma": {"TAMD_FP8W_MFMA": "2"}, "fp8w_tile": {"TAMD_FP8W_TILE": "2"},  # (any other arm: unset, the product's rule)
          "fp8w_tile64": {"TAMD_FP8W_TILE": "2", "TAMD_FP8W_TILE_BM": "64"}, "fp8w_tile128": {"TAMD_FP8W_TILE": "2", "TAMD_FP8W_TILE_BM": "128"}}


def switch(arm, m):
    for knob in KNOBS:
        os.environ.pop(knob, None)
    if arm == "fp8w_before":
        os.environ.update({"TAMD_FP8W_MFMA": "0"} if m <= 16 else {"TAMD_FP8W_TILE": "0"})
    os.environ.update(SWITCH.get(arm, {}))


def timed(arm, fn, iters, m):
    switch(arm, m)
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for i in range(iters):
        fn(i)
    en.record()
    torch.cuda.synchronize()
    switch(None, m)
    return st.elapsed_time(en) / iters


def reference_module(w8, s):
    from transformers.integrations.finegrained_fp8 import FP8Linear

    m = FP8Linear(w8.shape[1], w8.shape[0], block_size=(128, 128)).to(dev)
    m.weight, m.weight_scale_inv = torch.nn.Parameter(w8, requires_grad=False), torch.nn.Parameter(s, requires_grad=False)
    return m


torch.manual_seed(0)
# None: not tried yet; a string: why it is not timed; True: runs
reference_state = None if args.reference else "not requested: its Triton kernel is loaded through the `kernels` hub package"
for k, n in SHAPES:
    ring = max(2, min(64, -(-args.ring_bytes // (n * k))))  # the same number of copies for both arms: the bf16 ring is twice the bytes
    wb = [(torch.randn(n, k, device=dev) * 0.05).bfloat16() for _ in range(ring)]
    # per-block scales that keep every quotient inside e4m3's range (|w| <= 448 s): the tensor's maximum over 448, times 1 .. 2
    sc = [(w.abs().max().float() / 448.0) * (1 + torch.rand(-(-n // 128), -(-k // 128), device=dev)) for w in wb]
    w8 = [(w.float() / s.repeat_interleave(128, 0)[:n].repeat_interleave(128, 1)[:, :k]).to(torch.float8_e4m3fn)
          for w, s in zip(wb, sc)]
    for m in ROWS:
        x = torch.randn(m, k, device=dev).bfloat16()
        fp8w = lambda i: ops.linear_fp8w(x, w8[i % ring], sc[i % ring])  # noqa: E731
        arms = {"fp8w": fp8w, "fp8w_before": fp8w, "bf16": lambda i: ops.linear(x, wb[i % ring])}
        if m in (2, 4):
            arms["fp8w_mfma"] = fp8w
        if m > 16:
            arms["fp8w_tile"] = fp8w
        if m >= 128:
            arms["fp8w_tile64"] = arms["fp8w_tile128"] = fp8w
        if reference_state in (None, True):
            mods = [reference_module(w, s) for w, s in zip(w8, sc)]
            try:
                with torch.no_grad():
                    mods[0](x)
                torch.cuda.synchronize()
                reference_state = True
                arms["reference_fp8linear"] = lambda i: mods[i % ring](x)
            except Exception as e:  # (no Triton kernel for this box: reported, not timed)
                reference_state = f"{type(e).__name__}: {str(e)[:160]}"
        with torch.no_grad():
            y, yb = arms["fp8w"](0).float(), arms["bf16"](0).float()
            switch("fp8w_before", m)
            yo = fp8w(0).float()  # (the same operands through the code as it was: fp32 summation order apart, the same values)
            slowest = max(timed(a, fn, 5, m) for a, fn in arms.items())
            iters = max(10, min(20000, int(250.0 / max(slowest, 1e-3))))  # a timed window of ~250 ms of the slowest arm
            for a, fn in arms.items():
                timed(a, fn, 3, m)
            ms = {a: [] for a in arms}
            for _ in range(args.rounds):  # alternating
                for a, fn in arms.items():
                    ms[a].append(timed(a, fn, iters, m))
        med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
        nbytes = {a: n * k + 4 * sc[0].numel() + m * (k + n) * 2 for a in arms if a.startswith("fp8w")}
        nbytes["bf16"] = 2 * n * k + m * (k + n) * 2
        rec = {"K": k, "N": n, "M": m, "ring": ring, "iters": iters, "rel_diff_fp8w_vs_bf16_product": round(float((y - yb).norm() / yb.norm()), 4),
               "rel_diff_fp8w_vs_before": float(f"{float((y - yo).norm() / yo.norm()):.3g}"),
               **{f"{a}_ms": [round(v, 4) for v in ms[a]] for a in arms}, **{f"{a}_median_ms": round(med[a], 4) for a in arms},
               **{f"{a}_spread": round((max(ms[a]) - min(ms[a])) / med[a], 3) for a in arms},
               **{f"{a}_TBps": round(nbytes[a] / (med[a] * 1e-3) / 1e12, 3) for a in nbytes},
               "fp8w_over_bf16": round(med["fp8w"] / med["bf16"], 3), "fp8w_over_before": round(med["fp8w"] / med["fp8w_before"], 3),
               "reference_fp8linear": "timed" if reference_state is True else f"not run ({reference_state})", "clock_probe": "not run"}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    del wb, w8, sc
    torch.cuda.empty_cache()
