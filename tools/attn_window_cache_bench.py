"""Attention under a sliding window over a KV cache (tamd_attn_fwd_window / tamd_attn_decode_window) on one MI355X; rows as
tools/decode_bench.py takes its kernel rows: device events, warmed up, the forms of a row interleaved in one process, several
rounds, every round's figure reported.
  ab PARENT.so COPY.so   calls WITHOUT a window through a build of the parent commit, the current library and a second copy
                         of the parent's build (the control: what two loads of the same code differ by): the Llama-3-8B decode
                         rows of tools/decode_bench.py and the Llama-3-8B forward shape; same bits asserted per row
  window                 Mistral-7B heads (32 / 8, head_dim 128), W = 4096: 8 query rows over the cropped cache of W - 1 + 8 keys
                         (every tile visited) against tamd_attn_decode on the same call; 8 and 512 rows over 32768 un-cropped
                         keys against the plain causal call; torch's sdpa with the dense boolean mask on the same calls
    python tools/attn_window_cache_bench.py ab tools/ab/libtamd_base.so tools/ab/libtamd_base_copy.so > attn_window_ab.jsonl
    python tools/attn_window_cache_bench.py window >> attn_window_ab.jsonl"""
import ctypes
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from transformers_amd import _cabi  # noqa: E402

dev = torch.device("cuda:0")
ROUNDS = 5


def timeit(fn, iters, warm=10):
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


def params(q, k, v, o, causal=True):
    ap = _cabi.AttnParams()
    ap.q, ap.k, ap.v, ap.o, ap.lse, ap.key_valid, ap.q_start = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), None, None, None
    ap.batch, ap.seq_q, ap.heads_q, ap.head_dim = q.shape
    ap.seq_k, ap.heads_kv = k.shape[1], k.shape[2]
    for nm, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        setattr(ap, f"{nm}_stride_b", t.stride(0))
        setattr(ap, f"{nm}_stride_s", t.stride(1))
        setattr(ap, f"{nm}_stride_h", t.stride(2))
    ap.scale, ap.causal, ap.dtype, ap.dropout_p, ap.dropout_seed, ap.q_prescaled = q.shape[3] ** -0.5, int(causal), _cabi.TAMD_BF16, 0.0, 0, 0
    return ap


def operands(b, sq, sk, hq, hkv, d):
    torch.manual_seed(0)
    return (torch.randn(b, sq, hq, d, device=dev).bfloat16(), torch.randn(b, sk, hkv, d, device=dev).bfloat16(),
            torch.randn(b, sk, hkv, d, device=dev).bfloat16())


def call(lib, entry, q, k, v, window=None):
    """-> (a function that makes the call, its output tensor)."""
    o = torch.empty_like(q)
    ap = params(q, k, v, o)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if entry == "fwd":
        if window is None:
            fn = lambda: lib.check(lib.tamd_attn_fwd(ctypes.byref(ap), stream), "fwd")  # noqa: E731
        else:
            fn = lambda: lib.check(lib.tamd_attn_fwd_window(ctypes.byref(ap), window, stream), "fwd_window")  # noqa: E731
    else:
        nbytes = lib.tamd_attn_decode_workspace_bytes(ctypes.byref(ap))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        if window is None:
            fn = lambda: lib.check(lib.tamd_attn_decode(ctypes.byref(ap), ws.data_ptr(), nbytes, stream), "decode")  # noqa: E731
        else:
            fn = lambda: lib.check(lib.tamd_attn_decode_window(ctypes.byref(ap), window, ws.data_ptr(), nbytes, stream),  # noqa: E731
                                   "decode_window")
    fn()
    torch.cuda.synchronize()
    return fn, o


def interleaved(forms, iters):
    """{tag: fn} -> {tag: [us per call of every round]}, the forms taking turns inside every round, the order rotating."""
    tags = list(forms)
    times = {t: [] for t in tags}
    for r in range(ROUNDS):
        for t in tags[r % len(tags):] + tags[:r % len(tags)]:
            times[t].append(round(timeit(forms[t], iters), 2))
    return times


def ab(parent_path, copy_path):
    libs = {"parent": _cabi.TamdLib(parent_path, accept_abi=(13,)), "new": _cabi.TamdLib(_cabi.default_library_path()),
            "parent_copy": _cabi.TamdLib(copy_path, accept_abi=(13,))}
    rows = [("decode", "llama3-8b b1 4k", 1, 1, 4096, 32, 8, 128), ("decode", "llama3-8b b1 16k", 1, 1, 16384, 32, 8, 128),
            ("decode", "llama3-8b b1 64k", 1, 1, 65536, 32, 8, 128), ("decode", "llama3-8b b8 8k", 8, 1, 8192, 32, 8, 128),
            ("decode", "llama3-8b b64 4k", 64, 1, 4096, 32, 8, 128), ("decode", "llama3-8b b1 4k, 8 rows", 1, 8, 4096, 32, 8, 128),
            ("fwd", "llama3-8b fwd 8 x 4096", 8, 4096, 4096, 32, 8, 128)]
    for entry, name, b, sq, sk, hq, hkv, d in rows:
        q, k, v = operands(b, sq, sk, hq, hkv, d)
        forms, outs = {}, {}
        for tag, lib in libs.items():
            forms[tag], outs[tag] = call(lib, entry, q, k, v)
        times = interleaved(forms, 2000 if entry == "decode" else 20)
        print(json.dumps({"bench": f"{entry} parent vs new (no window)", "shape": name,
                          **{f"{t}_us": ts for t, ts in times.items()},
                          "same_bits": bool(torch.equal(outs["new"], outs["parent"]) and torch.equal(outs["parent_copy"], outs["parent"]))}),
              flush=True)


def window_rows():
    lib = _cabi.TamdLib(_cabi.default_library_path())
    hq, hkv, d, w = 32, 8, 128, 4096
    for name, entry, sq, sk in (("8 rows over the cropped cache (W - 1 + 8 keys)", "decode", 8, w - 1 + 8),
                                ("8 rows over 32768 un-cropped keys", "decode", 8, 32768),
                                ("512 rows over 32768 un-cropped keys", "fwd", 512, 32768)):
        q, k, v = operands(1, sq, sk, hq, hkv, d)
        f_win, o_win = call(lib, entry, q, k, v, w)
        f_plain, o_plain = call(lib, entry, q, k, v)
        qs, ks, vs = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
        qi, ki = torch.arange(sq, device=dev)[:, None] + (sk - sq), torch.arange(sk, device=dev)[None, :]
        dense = ((ki <= qi) & (ki > qi - w))[None, None]
        sdpa = lambda: torch.nn.functional.scaled_dot_product_attention(qs, ks, vs, attn_mask=dense, enable_gqa=True)  # noqa: E731
        ref = torch.nn.functional.scaled_dot_product_attention(qs.float(), ks.float(), vs.float(), attn_mask=dense,
                                                               enable_gqa=True).transpose(1, 2)
        times = interleaved({"window": f_win, "plain_causal": f_plain, "sdpa_dense_mask": sdpa}, 500 if entry == "decode" else 50)
        print(json.dumps({"bench": "window entries, Mistral-7B heads, W = 4096", "shape": name, "entry": entry, "sq": sq, "sk": sk,
                          **{f"{t}_us": ts for t, ts in times.items()},
                          "window_err_vs_fp32": round(((o_win.float() - ref).norm() / ref.norm()).item(), 5),
                          "window_same_bits_as_plain": bool(torch.equal(o_win, o_plain))}), flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["ab"]:
        ab(sys.argv[2], sys.argv[3])
    elif sys.argv[1:2] == ["window"]:
        window_rows()
    else:
        sys.exit(__doc__)
