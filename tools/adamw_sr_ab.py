"""The multi-tensor AdamW launch with stochastic rounding of the bf16 parameters (tamd_mt_adamw_step_sr) against the
round-to-nearest launch (tamd_mt_adamw_step) on the same table: 2^30 bf16 elements in 16 tensors, bf16 moments and fp32
moments, the two arms alternated A B A B in one process, HIP events, warm-up first.  Is the hash (three 32-bit multiplies per
element pair) hidden behind the HBM traffic?  JSON lines to stdout:
    python tools/adamw_sr_ab.py > profiles/adamw_sr_ab.jsonl          (--elements N for a smaller set)"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from transformers_amd import _cabi, ops  # noqa: E402
from transformers_amd.optim import MtTable  # noqa: E402

dev = torch.device("cuda:0")
HYP = (2e-5, 0.9, 0.999, 1e-8, 0.01)  # lr, beta1, beta2, eps, weight decay


def timeit(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=1 << 30)
    ap.add_argument("--tensors", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    per = args.elements // args.tensors
    for mdt in (torch.bfloat16, torch.float32):
        torch.manual_seed(0)
        ps = [(torch.randn(per, device=dev) * 0.02).bfloat16() for _ in range(args.tensors)]
        gs = [(torch.randn(per, device=dev) * 1e-3).bfloat16() for _ in range(args.tensors)]
        ms = [torch.zeros(per, device=dev, dtype=mdt) for _ in range(args.tensors)]
        vs = [torch.zeros(per, device=dev, dtype=mdt) for _ in range(args.tensors)]
        tab = MtTable().update(ps, gs, ms, vs, [ops.sr_key(1234, k) for k in range(args.tensors)])
        step = [0]
        code = _cabi.TAMD_BF16 if mdt == torch.bfloat16 else _cabi.TAMD_F32

        def nearest():  # (the plain launch reads the first 6n + 1 words of the same table)
            step[0] += 1
            torch.ops.tamd.mt_adamw_step_(tab.table, tab.n, tab.chunks, *HYP, step[0], 1.0, None, _cabi.TAMD_BF16, code)

        def stochastic():
            step[0] += 1
            torch.ops.tamd.mt_adamw_step_sr_(tab.table, tab.n, tab.chunks, *HYP, step[0], 1.0, None, code)

        n = per * args.tensors
        nbytes = n * (2 + 2 + 2 * ms[0].element_size()) + n * (2 + 2 * ms[0].element_size())  # reads p g m v, writes p m v
        rec = {"elements": n, "tensors": args.tensors, "moments": str(mdt).replace("torch.", ""), "bytes_per_element": nbytes // n,
               "nearest_ms": [], "stochastic_ms": []}
        for _ in range(args.rounds):  # A B A B: the clock drifts with the temperature
            rec["nearest_ms"].append(timeit(nearest, args.iters, 3))
            rec["stochastic_ms"].append(timeit(stochastic, args.iters, 3))
        for arm in ("nearest", "stochastic"):
            t = rec[arm + "_ms"]
            rec[arm + "_GBps"] = [nbytes / x / 1e6 for x in t]
            rec[arm + "_ms_median"] = sorted(t)[len(t) // 2]
        rec["nearest_spread"] = max(rec["nearest_ms"]) / min(rec["nearest_ms"]) - 1.0  # what two A arms differ by
        rec["stochastic_over_nearest"] = rec["stochastic_ms_median"] / rec["nearest_ms_median"]
        print(json.dumps(rec), flush=True)
        del ps, gs, ms, vs, tab
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
