"""Host logic of sliding-window KV caches (CPU only, no backend): what `tamd_mask` returns for every forward of a generation over
a DynamicSlidingWindowLayer / StaticSlidingWindowLayer (cache_utils.py:203-277, :504-628), driven through the reference's own
`create_sliding_window_causal_mask` (masking_utils.py:1102) with real cache objects, expanded into a dense mask and compared
with the reference's `sdpa_mask(..., allow_is_causal_skip=False)` for the same arguments."""
import pytest
import torch
from hypothesis import given, settings
from hypothesis import strategies as st

import transformers_amd  # noqa: F401  (registers the attention function and the mask factory)
from transformers_amd import ops
from transformers_amd.attention import TamdMask, _mask_kv_len, split_mask, tamd_mask

HEAD_DIM, BATCH = 8, 2


def _config(window):
    from transformers import MistralConfig

    cfg = MistralConfig(vocab_size=32, hidden_size=16, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2,
                        num_key_value_heads=1, head_dim=HEAD_DIM, max_position_embeddings=256, sliding_window=window)
    cfg._attn_implementation = "tamd"
    return cfg


def _cache(kind, cfg, total):
    from transformers import DynamicCache, StaticCache

    return DynamicCache(config=cfg) if kind == "dynamic" else StaticCache(config=cfg, max_cache_len=total + 3)


def _dense(m, n, length, window):
    """What the attention function and the kernels compute from `tamd_mask`'s answer, as [B, n, length] bool over the keys the
    cache returns: padding AND the bottom-right causal diagonal AND the window term -- or the slots in use for the count form."""
    i, j = torch.arange(n)[:, None], torch.arange(length)[None, :]
    if isinstance(m, TamdMask) and m.kv_len is not None:       # one query over a pre-allocated cache: keys below the count
        assert n == 1 and m.q_start is None and m.window is None
        used = j[None] < m.kv_len[:, None, None]
        return used if m.key_valid is None else used & m.key_valid[:, None, :].bool()
    kv = m.key_valid if isinstance(m, TamdMask) else m
    sk = length if kv is None else kv.shape[-1]                 # (shorter than the allocation: K / V are sliced to it)
    assert sk <= length
    off = sk - n
    allow = (j <= i + off) & (j < sk)
    if isinstance(m, TamdMask) and m.window is not None:
        assert m.q_start is None and sk == length and n >= 2
        allow = allow & (j > i + off - m.window)
    if isinstance(m, TamdMask) and m.q_start is not None:       # the square call without a cache: the bound planes
        assert sk == n == length
        return (allow[None] & (m.q_start[0][:, :, None] <= j[None])) & (True if kv is None else kv[:, None, :].bool())
    allow = allow[None].expand(BATCH, -1, -1)
    if kv is not None:
        allow = allow & torch.nn.functional.pad(kv.bool(), (0, length - sk))[:, None, :]
    return allow


def _run(kind, window, steps, left_pad):
    """Every forward of a teacher-forced run -> [(n, P, L, o, binds, what tamd_mask returned)]; each compared with the
    reference's dense mask on the way."""
    from transformers import masking_utils as mu

    cfg = _config(window)
    total = sum(steps)
    cache = _cache(kind, cfg, total)
    am = None
    if left_pad:
        am = torch.ones(BATCH, total, dtype=torch.long)
        am[1, :left_pad] = 0
    seen, pos = [], 0
    for n in steps:
        emb = torch.empty(BATCH, n, 0)
        am_n = None if am is None else am[:, :pos + n]
        p = cache.get_query_offset(0)
        length, o = cache.get_mask_sizes(n, 0)
        assert p == pos and not torch.is_tensor(p)
        got = mu.create_sliding_window_causal_mask(cfg, emb, am_n, cache)
        want = mu.sdpa_mask(BATCH, n, length, p, o, mask_function=mu.sliding_window_causal_mask_function(window),
                            attention_mask=None if am_n is None else am_n.bool(), allow_is_causal_skip=False)[:, 0]
        k, _ = cache.update(torch.zeros(BATCH, 1, n, HEAD_DIM), torch.zeros(BATCH, 1, n, HEAD_DIM), 0)
        assert k.shape[2] == length, (kind, window, steps, n)  # the keys the attention function is handed
        dense = _dense(got, n, length, window)
        assert torch.equal(dense.expand(BATCH, n, length), want.expand(BATCH, n, length)), (kind, window, steps, pos, n, left_pad)
        # a mask prepared before the forward (generate with a pre-allocated cache) comes back from the factory as it is
        if got is not None:
            again = tamd_mask(BATCH, n, length, q_offset=p, kv_offset=o, mask_function=mu.sliding_window_causal_mask_function(window),
                              attention_mask=got.to(device="cpu", dtype=torch.bool), local_size=window, device="cpu")
            assert torch.equal(_dense(again, n, length, window).expand(BATCH, n, length), want.expand(BATCH, n, length))
        seen.append((n, pos, length, o, o <= pos + n - 1 - window, got))
        pos += n
    return seen


@pytest.mark.parametrize("kind", ["dynamic", "static"])
@pytest.mark.parametrize("left_pad", [0, 3])
def test_every_row_of_the_table(kind, left_pad):
    """W = 8 and step lengths 5, 1, 1, 6, 1, 3, 1: prefill below the window, decode steps, a step that crosses the window, a
    decode step and a multi-token step over the cropped cache."""
    seen = _run(kind, 8, [5, 1, 1, 6, 1, 3, 1], left_pad)
    geometry = [(n, p, length, o) for n, p, length, o, _, _ in seen]
    first = (5, 0, 5, 0) if kind == "dynamic" else (5, 0, 8, 0)
    second = [(1, 5, 6, 0), (1, 6, 7, 0)] if kind == "dynamic" else [(1, 5, 8, 0), (1, 6, 8, 0)]
    assert geometry == [first, *second, (6, 7, 13, 0), (1, 13, 8, 6), (3, 14, 10, 7), (1, 17, 8, 10)]
    carries = [isinstance(m, TamdMask) and m.window is not None for *_, m in seen]
    assert carries == [False, False, False, True, False, True, False]
    assert [m.window for *_, m in seen if isinstance(m, TamdMask) and m.window is not None] == [8, 8]
    for n, p, length, o, binds, m in seen:
        if isinstance(m, TamdMask) and m.window is not None:
            assert m.q_start is None and m.kv_len is None
            assert (m.key_valid is None) == (left_pad == 0)
            assert m.key_valid is None or m.key_valid.shape == (BATCH, length)
            assert _mask_kv_len(m) in (None, length)
            moved = m.to(device=torch.device("cpu"), dtype=torch.bool)
            assert isinstance(moved, TamdMask) and moved.window == m.window
            with pytest.raises(ops.TamdError):  # a block that only knows padding masks refuses it
                split_mask(m, BATCH, length)
    if kind == "static":  # the static-prefix decode steps: the count in device memory, the mask over the allocation
        for n, p, length, o, binds, m in seen[1:3]:
            assert isinstance(m, TamdMask) and m.kv_len.tolist() == [p + 1] * BATCH and m.window is None
        assert torch.is_tensor(seen[0][5]) and seen[0][5].shape == (BATCH, 5)  # the prefill: the slots in use
    else:
        assert seen[1][5] is None or torch.is_tensor(seen[1][5])
    # one query over the cropped cache sees every key it is handed: the padding mask over [o, o + L), or nothing
    n, p, length, o, binds, m = seen[4]
    assert (m is None) if left_pad == 0 else (torch.is_tensor(m) and m.shape == (BATCH, length))


@settings(max_examples=60, deadline=None)
@given(st.sampled_from(["dynamic", "static"]), st.integers(2, 12), st.lists(st.integers(1, 9), min_size=1, max_size=7),
       st.integers(0, 4))
def test_factory_matches_the_reference_mask_at_every_step(kind, window, steps, left_pad):
    """Property over (W, step lengths): every step's answer expands to the reference's own mask; the binding steps over a
    non-empty cache, and only those, carry `window` (a binding first forward is the square call: the bound planes)."""
    seen = _run(kind, window, steps, min(left_pad, steps[0] - 1))
    for n, p, length, o, binds, m in seen:
        carries = isinstance(m, TamdMask) and m.window is not None
        assert carries == (binds and p > 0), (kind, window, steps, p, n)
        if carries:
            assert n >= 2 and o + length == p + n and m.window == window
        if binds and p == 0:
            assert isinstance(m, TamdMask) and m.q_start is not None and m.window is None


def test_what_stays_refused():
    from transformers import masking_utils as mu

    fn = mu.sliding_window_causal_mask_function(8)
    kw = dict(local_size=8, device="cpu")
    # one query whose window binds: a cache that keeps keys the window has left behind (it does not crop)
    with pytest.raises(ops.TamdError, match="does not crop"):
        tamd_mask(2, 1, 21, q_offset=20, kv_offset=0, mask_function=fn, **kw)
    # a binding window over keys that do not end at the last query
    with pytest.raises(ops.TamdError, match="do not end at the last query"):
        tamd_mask(2, 3, 32, q_offset=20, kv_offset=0, mask_function=fn, **kw)
    # an offset without the aligned form
    with pytest.raises(ops.TamdError, match="not the"):
        tamd_mask(2, 1, 8, q_offset=20, kv_offset=16, mask_function=fn, **kw)
    # a device-side query offset under an overlay
    with pytest.raises(ops.TamdError, match="device tensor"):
        tamd_mask(2, 1, 32, q_offset=torch.tensor(5), kv_offset=0, mask_function=fn, **kw)
    # a caller that does not say what its cache keeps: the refusal the factory always gave
    with pytest.raises(ops.TamdError):
        tamd_mask(2, 1, 6, q_offset=5, mask_function=fn, device="cpu")
    with pytest.raises(ops.TamdError):
        tamd_mask(2, 1, 8, q_offset=13, kv_offset=6, mask_function=fn, device="cpu")
    # packed sequences and chunked attention with a cache
    ids = torch.zeros(2, 24, dtype=torch.long)
    for other in (mu.packed_sequence_mask_function(ids), mu.chunked_overlay(4, torch.zeros(2, dtype=torch.long))):
        with pytest.raises(ops.TamdError):
            tamd_mask(2, 4, 24, q_offset=20, mask_function=mu.and_masks(fn, other), **kw)
        with pytest.raises(ops.TamdError):
            tamd_mask(2, 3, 10, q_offset=14, kv_offset=7, mask_function=mu.and_masks(fn, other), **kw)
    # a bidirectional window is no causal window
    with pytest.raises(ops.TamdError):
        tamd_mask(2, 3, 10, q_offset=14, kv_offset=7, local_size=8, device="cpu",
                  mask_function=mu.and_masks(mu.causal_mask_function, mu.sliding_window_bidirectional_overlay(8)))
    # several sliding overlays: the smallest window
    two = mu.and_masks(mu.sliding_window_causal_mask_function(8), mu.sliding_window_overlay(5))
    m = tamd_mask(2, 3, 10, q_offset=14, kv_offset=7, mask_function=two, **kw)
    assert isinstance(m, TamdMask) and m.window == 5
