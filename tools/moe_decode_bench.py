"""One experts call of a decode step under experts_implementation "tamd": the weight-streaming kernels
(torch.ops.tamd.moe_experts_decode, csrc/gemv_moe.inc) against the routed GEMM (TAMD_MOE_GEMV=0), T in {1, 2, 4, 8, 16} tokens,
bf16, at two geometries:
    mixtral-8x7b   E 8,   top-2, H 4096, I 14336
    qwen3-moe-like E 128, top-8, H 2048, I 768
Every arm runs in a process of its own (this one starts them and never opens the GPU), ordered A B A B with A = the routed GEMM
and B = the decode kernels, between two runs of bench.py's clock probe.  A decode step of a model visits another layer's
weights with every call, so a call here cycles through several weight sets (more bytes than the 256 MB of last-level cache)
and through 8 routings drawn with a fixed seed; times are HIP events around a window of such calls behind a warm-up, the
median of three windows.  Per T the record holds the weight-bytes floor: (distinct chosen experts, averaged over the routings)
x 3 H I x 2 B at 4.9 and at 6.8 TB/s, the range the project's HBM-bound kernels reach.
--parent-tree DIR adds one run of the routed GEMM from a built checkout of the parent commit (arm P): TAMD_MOE_GEMV=0 must
reproduce it.  --arms picks the runs of a call (a later call can add arm P to the file); the summary lines are made from the
latest record of every arm in the file.
    python tools/moe_decode_bench.py [--parent-tree DIR] [--arms ...] [--out profiles/moe_decode_ab.jsonl]   (appends JSON lines)"""
import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
GEOMETRIES = {"mixtral-8x7b": dict(e=8, k=2, h=4096, inter=14336, layers=2),
              "qwen3-moe-like": dict(e=128, k=8, h=2048, inter=768, layers=4)}
TOKENS = (1, 2, 4, 8, 16)
ROUTINGS = 8


def timeit(torch, fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(iters):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def arm(args):
    """one arm, in this process: JSON lines to stdout"""
    sys.path.insert(0, args.tree)
    import torch

    from transformers_amd import ops

    assert Path(ops.__file__).resolve().is_relative_to(Path(args.tree).resolve()), ops.__file__
    dev = torch.device("cuda:0")
    counter = getattr(ops, "moe_decode_call_count", None)
    for name in args.geometries:
        g = GEOMETRIES[name]
        e, k, h, inter, layers = g["e"], g["k"], g["h"], g["inter"], g["layers"]
        torch.manual_seed(0)
        wgu = [torch.randn(e, 2 * inter, h, device=dev, dtype=torch.bfloat16) * 0.02 for _ in range(layers)]
        wd = [torch.randn(e, h, inter, device=dev, dtype=torch.bfloat16) * 0.02 for _ in range(layers)]
        for t in TOKENS:
            gen = torch.Generator().manual_seed(1000 * t + e)
            x = torch.randn(t, h, generator=gen).bfloat16().to(dev)
            ws, idxs, distinct = [], [], []
            for _ in range(ROUTINGS):
                w, idx = torch.topk(torch.softmax(torch.randn(t, e, generator=gen), -1), k, -1)
                ws.append((w / w.sum(-1, keepdim=True)).to(dev))
                idxs.append(idx.to(dev))
                distinct.append(idx.unique().numel())

            def call(i):
                with torch.no_grad():
                    return ops.moe_experts(x, idxs[i % ROUTINGS], ws[i % ROUTINGS], wgu[i % layers], wd[i % layers])

            if counter:
                counter(reset=True)
            for i in range(ROUTINGS):
                call(i)
            torch.cuda.synchronize()
            windows = sorted(timeit(torch, call, args.iters) for _ in range(3))
            weight_bytes = sum(distinct) / ROUTINGS * 3 * h * inter * 2
            rec = dict(kind="arm", arm=args.arm, geometry=name, tokens=t, e=e, top_k=k, h=h, inter=inter, us=round(windows[1], 2),
                       us_windows=[round(v, 2) for v in windows], iters=args.iters, distinct_experts=sum(distinct) / ROUTINGS,
                       weight_bytes=weight_bytes, floor_us_at_6p8=round(weight_bytes / 6.8e6, 2),
                       floor_us_at_4p9=round(weight_bytes / 4.9e6, 2), TBps=round(weight_bytes / windows[1] / 1e6, 3),
                       decode_calls=counter() if counter else None, TAMD_MOE_GEMV=os.environ.get("TAMD_MOE_GEMV"))
            if counter and t == TOKENS[-1]:  # both paths on the same inputs: they differ in fp32 summation order only
                outs = {}
                for flag in ("1", "0"):
                    os.environ["TAMD_MOE_GEMV"] = flag
                    outs[flag] = call(0).float()
                os.environ.pop("TAMD_MOE_GEMV")
                if args.env is not None:
                    os.environ["TAMD_MOE_GEMV"] = args.env
                rec["decode_vs_routed_rel"] = float((outs["1"] - outs["0"]).norm() / outs["0"].norm())
            print(json.dumps(rec), flush=True)
        del wgu, wd
        torch.cuda.empty_cache()


def clock(args):
    sys.path.insert(0, str(ROOT))
    import torch

    import bench

    print(json.dumps(dict(kind="clock_probe", **bench.clock_probe(torch.device("cuda:0")))), flush=True)


def child(out, *argv, env=None):
    e = dict(os.environ)
    e.pop("TAMD_MOE_GEMV", None)
    if env is not None:
        e["TAMD_MOE_GEMV"] = env
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), *argv] + (["--env", env] if env is not None else []),
                       env=e, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{argv}: exit {r.returncode}\n{r.stderr[-4000:]}")
    recs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    with open(out, "a") as f:
        for rec in recs:
            f.write(json.dumps(rec) + "\n")
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="parent", choices=["parent", "arm", "clock"])
    ap.add_argument("--arm", default="B")
    ap.add_argument("--env", default=None)
    ap.add_argument("--tree", default=str(ROOT))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--geometries", nargs="+", default=list(GEOMETRIES))
    ap.add_argument("--no-clock", action="store_true")
    ap.add_argument("--arms", nargs="+", default=None, help="default: A1 B1 A2 B2 (+ P with --parent-tree)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "moe_decode_ab.jsonl"))
    args = ap.parse_args()
    if args.mode == "arm":
        return arm(args)
    if args.mode == "clock":
        return clock(args)
    if args.arms is None:
        args.arms = ["A1", "B1", "A2", "B2"] + (["P"] if args.parent_tree else [])
    common = ["--iters", str(args.iters), "--geometries", *args.geometries]
    if not args.no_clock:
        child(args.out, "--mode", "clock")
    for label in args.arms:
        if label == "P":
            child(args.out, "--mode", "arm", "--arm", "P", "--tree", args.parent_tree, *common)
        else:
            child(args.out, "--mode", "arm", "--arm", label, *common, env="0" if label.startswith("A") else None)
    if not args.no_clock:
        child(args.out, "--mode", "clock")
    summarise(args.out)


def summarise(out):
    """one summary line per (geometry, T) from the arm records the file holds (the latest of each arm)"""
    runs = {}
    for line in open(out):
        r = json.loads(line)
        if r.get("kind") == "arm":
            runs[(r["arm"], r["geometry"], r["tokens"])] = r
    with open(out, "a") as f:
        for (label, geometry, t), a1 in sorted(runs.items()):
            rest = [runs.get((x, geometry, t)) for x in ("B1", "A2", "B2")]
            if label != "A1" or None in rest:
                continue
            b1, a2, b2 = rest
            assert a1["decode_calls"] == 0 and a2["decode_calls"] == 0 and b1["decode_calls"] > 0 and b2["decode_calls"] > 0
            routed, decode = (a1["us"] + a2["us"]) / 2, (b1["us"] + b2["us"]) / 2
            spread = abs(a1["us"] - a2["us"]) / min(a1["us"], a2["us"])
            rec = dict(kind="summary", geometry=geometry, tokens=t, routed_us=[a1["us"], a2["us"]], decode_us=[b1["us"], b2["us"]],
                       routed_spread=round(spread, 4), routed_over_decode=round(routed / decode, 3),
                       decode_faster=bool(max(b1["us"], b2["us"]) * (1 + spread) < min(a1["us"], a2["us"])),
                       floor_us=[a1["floor_us_at_6p8"], a1["floor_us_at_4p9"]], decode_TBps=round(a1["weight_bytes"] / decode / 1e6, 3))
            if ("P", geometry, t) in runs:
                rec["parent_routed_us"] = runs[("P", geometry, t)]["us"]
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
