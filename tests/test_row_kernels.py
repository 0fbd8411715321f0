"""Row kernels, element by element: the norm family (csrc/norm.hip), cross-entropy (csrc/elementwise.hip) and the column
sums, at every (NCH, WPR) instantiation of `norm_geometry` and at the ragged edges -- rows that are no multiple of the rows
per block, a last 16-byte chunk that is partly filled, sub-waves of a row group without a column, a second grid-stride
iteration in which almost every block is past the matrix, vocabularies that are no multiple of the vector.

The SAME small shapes run under the CPU execution model (`emu`) and on the MI355X (`hip`): the backward's edges are the
hardware range check of the buffer accesses, which the CPU model only restates.  No tensor exceeds ~2.2 M elements.

Reference: float64 torch on the stored (dtype-rounded) inputs -- the statistics a backward receives are the fp32 values
the forward stored.  Every element of every output is checked:

    |got - ref| <= gate * (ulp_T(ref) + s),      gate = 2 * max(0.5, own)

ulp_T(ref): the unit in the last place of the storage type T at ref.
s:          what fp32 arithmetic may add in front of the output rounding: 2^-23 x (the float64 sum of the absolute terms
            of the element's reduction) x (the reduction length: the kernels fix no summation order), plus 2^-23 per
            elementwise operation on the term it acts on.  Worked out per output next to each check below.
            Where the kernel documents a rounding in FRONT of the last one (RMSNorm's `w * round(x * rstd)`, its dw from
            the same rounded value, dx_drop = round(round(dx) * keep / (1 - p))), s also carries the ulp_T of that inner
            value times what multiplies it: a sum that cancels keeps the inner roundings of its terms.
own:        the float64 reference's OWN error in that unit once it is rounded as the kernel documents its roundings (once
            to T for most outputs, twice for those three).  One rounding to nearest errs by at most 0.5 ulp -- the value
            `own` approaches on any tensor of a few hundred elements; the floor of 0.5 keeps a tensor of eight elements
            from a gate below one legal rounding.  The gate is twice that: one more half ulp for a last bit flipped by
            the fp32 summation order.
Neither term comes from the kernels' output.  `own`, the kernels' worst ratio and the gate go to the parity report
(conftest.record, group "row_kernels").  Bit-exact properties are asserted with torch.equal: h = x + residual,
h = round(round(x * keep / (1 - p)) + residual), the zeroed padding of dlogits, "same outputs with and without column
sums", zero gradient rows of ignored labels.

Outputs are written through the C ABI into the interior of buffers pre-filled with a sentinel (the compiled ops allocate
their own outputs, which leaves nothing to guard): the guard rows before and behind y, h_out, dx, dx_drop, the
statistics and the parameter gradients must keep the sentinel."""
import numpy as np
import pytest
import torch

from kernel_checks import BF16, F16, F32, NAME, Guarded, check, rnd, ulp  # (shared with tests/test_gemm_elements.py)
from transformers_amd import ops

VE = {BF16: 8, F16: 8, F32: 4}  # elements of a 16-byte vector
U2 = 2.0 ** -23
EPS = float(np.float32(1e-5))  # what the kernels receive
E_SHAPE, E_ARG = -2, -6
MAX_PARTIALS = 512  # csrc/colsum.h kNormMaxPartials: blocks of a norm backward


def geometry(cols, dtype):
    """csrc/norm.hip norm_geometry: (NCH, WPR) of a row of `cols` elements, None if refused."""
    ve = VE[dtype]
    if cols <= 0 or cols % ve:
        return None
    chunks = -(-cols // (64 * ve))
    wpr = 4 if chunks >= 16 else (2 if chunks >= 5 else 1)
    per = -(-chunks // wpr)
    if per > 8:
        return None
    return (1 if per <= 1 else 2 if per <= 2 else 4 if per <= 4 else 8), wpr


def ptr(t):
    return None if t is None else t.data_ptr()


_WS = {}


def workspace(dev, nbytes):
    """One scratch buffer per device, grown on demand (the norm backward's is 6 KB per column)."""
    t = _WS.get(dev.type)
    if t is None or t.numel() < nbytes:
        t = _WS[dev.type] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return t


class Call:
    """One C-ABI call of a norm entry point with every output in a guarded buffer."""

    def __init__(self, env, like):
        self.be = ops.backend()
        self.lib, self.stream = self.be.lib, self.be.stream(like)
        self.rows, self.cols = like.shape
        self.dtype, self.dev, self.code = like.dtype, like.device, ops._code(like)
        self.outs = {}

    def out(self, name, kind):
        """kind 'mat': [rows, cols] T with four guard rows (the most a block owns) on either side; 'vec': [cols] T;
        'stat': [rows] fp32"""
        if kind == "mat":
            g = Guarded((self.rows, self.cols), self.dtype, self.dev, 4 * self.cols)
        elif kind == "vec":
            g = Guarded((self.cols,), self.dtype, self.dev, self.cols)
        else:
            g = Guarded((self.rows,), F32, self.dev, 8)
        self.outs[name] = g
        return g.t

    def ws(self):
        n = self.lib.tamd_norm_bwd_workspace_bytes(self.rows, self.cols)
        return workspace(self.dev, n).data_ptr(), n

    def done(self, code, what):
        assert code == 0, f"{what}: C-ABI status {code} at rows {self.rows} cols {self.cols} {NAME[self.dtype]}"
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        for name, g in self.outs.items():
            assert g.intact(), f"{what}: the guard around {name} was written (rows {self.rows}, cols {self.cols})"
        return {k: g.t for k, g in self.outs.items()}


def norm_fwd(env, kind, x, w, b=None, res=None, drop=None):
    """kind 'rms' | 'ln'; drop = (p, seed) selects tamd_layernorm_dropout_fwd.  -> dict y, h (with res), mean (ln), rstd"""
    c = Call(env, x)
    y = c.out("y", "mat")
    h = c.out("h", "mat") if res is not None else None
    rstd = c.out("rstd", "stat")
    if kind == "rms":
        st = c.lib.tamd_rmsnorm_fwd(ptr(x), ptr(res), ptr(w), ptr(y), ptr(h), ptr(rstd), c.rows, c.cols, EPS, c.code, c.stream)
    else:
        mean = c.out("mean", "stat")
        if drop is None:
            st = c.lib.tamd_layernorm_fwd(ptr(x), ptr(res), ptr(w), ptr(b), ptr(y), ptr(h), ptr(mean), ptr(rstd), c.rows,
                                          c.cols, EPS, c.code, c.stream)
        else:
            st = c.lib.tamd_layernorm_dropout_fwd(ptr(x), ptr(res), ptr(w), ptr(b), ptr(y), ptr(h), ptr(mean), ptr(rstd),
                                                  c.rows, c.cols, EPS, drop[0], drop[1], None, c.code, c.stream)
    return c.done(st, f"{kind}_fwd")


def norm_bwd(env, kind, dy, h, w, mean, rstd, dres=None, need_db=True, csum=False, drop=None, expect=0):
    """-> dict dx, dw, db (ln, need_db), dc (csum), dxd (drop)"""
    c = Call(env, h)
    dx, dw = c.out("dx", "mat"), c.out("dw", "vec")
    ws, nbytes = c.ws()
    if kind == "rms":
        st = c.lib.tamd_rmsnorm_bwd(ptr(dy), ptr(h), ptr(w), ptr(rstd), ptr(dres), ptr(dx), ptr(dw), ws, nbytes, c.rows,
                                    c.cols, c.code, c.stream)
    else:
        db = c.out("db", "vec") if need_db else None
        dc = c.out("dc", "vec") if csum else None
        if drop is None:
            st = c.lib.tamd_layernorm_bwd(ptr(dy), ptr(h), ptr(w), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(dw), ptr(db),
                                          ptr(dc), ws, nbytes, c.rows, c.cols, c.code, c.stream)
        else:
            dxd = c.out("dxd", "mat")
            st = c.lib.tamd_layernorm_dropout_bwd(ptr(dy), ptr(h), ptr(w), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(dxd),
                                                  ptr(dw), ptr(db), ptr(dc), ws, nbytes, c.rows, c.cols, drop[0], drop[1],
                                                  None, c.code, c.stream)
    if expect != 0:
        assert st == expect, (st, expect)
        assert all(g.untouched() for g in c.outs.values()), "a refused call wrote an output"
        return None
    return c.done(st, f"{kind}_bwd")


# ---------------------------------------------------------------------------------------------------- inputs, references
def norm_inputs(rows, cols, dtype, dev, seed):
    """randn; row 1 (row 0 of a single row) sits at +100: a one-pass variance loses it; row 2 is constant: variance 0."""
    g = torch.Generator().manual_seed(seed)
    x, r, dy, dres = (torch.randn(rows, cols, generator=g) for _ in range(4))
    off, const = (1, 2) if rows >= 3 else (0, None)
    x[off] += 100.0
    if const is not None:
        x[const], r[const] = 0.75, 0.0
    w = torch.rand(cols, generator=g) + 0.5
    b = torch.randn(cols, generator=g)
    t = {k: v.to(dtype).to(dev) for k, v in dict(x=x, r=r, dy=dy, dres=dres, w=w, b=b).items()}
    t["const"] = const
    return t


def d64(t):
    return t.detach().cpu().double()


def check_fwd(tag, kind, out, h, w, b, dtype, const):
    """h: the normalised tensor as stored (x, or the h the kernel wrote).  Checks mean, rstd, y."""
    h, w = d64(h), d64(w)
    n = h.shape[1]
    absmean = h.abs().mean(-1, keepdim=True)
    if kind == "ln":
        mu = h.mean(-1, keepdim=True)
        var = (h - mu).pow(2).mean(-1, keepdim=True)
        # mean: n terms in any order
        check(f"{tag}.mean", out["mean"], mu[:, 0], U2 * n * absmean[:, 0], F32)
    else:
        mu = torch.zeros_like(h[:, :1])
        var = h.pow(2).mean(-1, keepdim=True)
    rs = (var + EPS).rsqrt()
    # rstd: d rstd = rstd / 2 * d var / (var + eps), d var <= 2^-23 n var (n positive terms); rsqrtf itself errs by ulps
    check(f"{tag}.rstd", out["rstd"], rs[:, 0], U2 * n * rs[:, 0], F32)
    xh = (h - mu) * rs
    if kind == "ln":
        bb = d64(b)
        ref = xh * w + bb
        # y: the mean moves every element by d mu * rstd * w, rstd scales it by n 2^-23; three elementwise operations
        s = U2 * (n * (absmean * rs * w.abs() + (xh * w).abs()) + 3 * ((xh * w).abs() + bb.abs()))
        check(f"{tag}.y", out["y"], ref, s, dtype)
        if const is not None:  # variance 0: rstd = rsqrt(eps) (within the bound above), y = b
            assert var[const].item() == 0.0 and torch.equal(out["y"][const].cpu(), b.cpu())
    else:
        ref = xh * w
        # reference: weight * x.to(dtype) -- the inner rounding moves y by up to |w| ulp_T(x * rstd) / 2
        s = U2 * (n + 3) * ref.abs() + w.abs() * ulp(xh, dtype)
        check(f"{tag}.y", out["y"], ref, s, dtype, chain=rnd(w * rnd(xh, dtype), dtype))


def check_bwd(tag, kind, out, dy, h, w, mean, rstd, dres, dtype, drop=None, keep=None):
    """dx, dw, db, dc, dxd against the float64 formulas on the stored h, dy, w, dres and the stored fp32 mean / rstd."""
    dy, h, w, rs = d64(dy), d64(h), d64(w), d64(rstd)[:, None]
    rows, n = h.shape
    mu = d64(mean)[:, None] if kind == "ln" else torch.zeros_like(rs)
    xh = (h - mu) * rs
    g = dy * w
    sgx = (g * xh).mean(-1, keepdim=True)
    sg = g.mean(-1, keepdim=True) if kind == "ln" else torch.zeros_like(sgx)
    ref = rs * (g - sg - xh * sgx)
    # the two row sums have n terms each; then five elementwise operations on the three terms
    s = U2 * rs * (n * (g.abs().mean(-1, keepdim=True) * (1.0 if kind == "ln" else 0.0)
                        + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
                   + 5 * (g.abs() + sg.abs() + (xh * sgx).abs()))
    if dres is not None:
        ref = ref + d64(dres)
        s = s + U2 * d64(dres).abs()
    check(f"{tag}.dx", out["dx"], ref, s, dtype)
    if drop is not None:
        scale = float(np.float32(1.0 / (1.0 - float(np.float32(drop[0])))))  # csrc/dropout.h drop_params
        f = keep.double() * scale
        # dx_drop = round(round(dx) * keep / (1 - p)): the inner rounding is scaled with the element
        check(f"{tag}.dx_drop", out["dxd"], ref * f, (s + ulp(ref, dtype)) * f, dtype, chain=rnd(rnd(ref, dtype) * f, dtype))
        assert bool((out["dxd"].cpu()[~keep] == 0).all())  # dropped elements receive no gradient, exactly
    # dw, db: `rows` terms per column in any order; xh itself carries three fp32 operations
    terms = dy * xh
    s_dw = U2 * (rows + 3) * terms.abs().sum(0)
    chain = None
    if kind == "rms":  # RMSNorm: dw from the ROUNDED x * rstd (what the forward multiplied w with): every term moves by up
        chain = rnd((dy * rnd(xh, dtype)).sum(0), dtype)  # to |dy| ulp_T(x * rstd) / 2, whatever the sum cancels to
        s_dw = s_dw + (dy.abs() * ulp(xh, dtype)).sum(0)
    check(f"{tag}.dw", out["dw"], terms.sum(0), s_dw, dtype, chain=chain)
    if "db" in out:
        check(f"{tag}.db", out["db"], dy.sum(0), U2 * rows * dy.abs().sum(0), dtype)
    if "dc" in out:  # column sums of the gradient AS STORED
        src = d64(out["dxd"] if drop is not None else out["dx"])
        check(f"{tag}.dcolsum", out["dc"], src.sum(0), U2 * rows * src.abs().sum(0), dtype)


def same(a, b, names):
    for k in names:
        assert torch.equal(a[k], b[k]), f"{k} differs"


# ---------------------------------------------------------------------------------------------------- norm family
# one width per (NCH, WPR) at the upper edge of its range or just inside a boundary, ragged widths whose last chunk is partly
# filled or in which a whole sub-wave of the row group has no column; 7680: the widest two-row-group LayerNorm, whose
# column-sum plane no longer fits beside dw and db in the LDS a launch may ask for
WIDTHS = {
    BF16: [8, 520, 1032, 1536, 2056, 4104, 5120, 7680, 7688, 8192, 8200, 16384],
    F16: [8, 520, 1536, 2056, 5120, 7680, 8192, 8200],
    F32: [4, 260, 516, 768, 1028, 2052, 2560, 3844, 4096, 4100, 8192],
}
CASES = [pytest.param(dt, c, id=f"{NAME[dt]}-{c}") for dt in (BF16, F16, F32) for c in WIDTHS[dt]]


def test_width_table_covers_every_instantiation():
    for dt in (BF16, F16, F32):
        assert {geometry(c, dt) for c in WIDTHS[dt]} == {(1, 1), (2, 1), (4, 1), (4, 2), (8, 2), (4, 4), (8, 4)}


@pytest.mark.parametrize("dtype,cols", CASES)
def test_norm_forward_every_geometry(env, dtype, cols):
    """RMSNorm and LayerNorm forward, plain and with the fused residual add, and LayerNorm(dropout(x) + residual), at
    1, 5 and 7 rows (no multiple of any rows-per-block: the last block has row groups past the matrix)."""
    for rows in (1, 5, 7):
        t = norm_inputs(rows, cols, dtype, env.device, 1000 + rows)
        x, r, w, b, const = t["x"], t["r"], t["w"], t["b"], t["const"]
        tag = "rmsnorm_fwd"
        check_fwd(tag, "rms", norm_fwd(env, "rms", x, w), x, w, None, dtype, const)
        o = norm_fwd(env, "rms", x, w, res=r)
        assert torch.equal(o["h"], x + r)  # bit for bit
        check_fwd(tag + "+res", "rms", o, o["h"], w, None, dtype, const)
        tag = "layernorm_fwd"
        check_fwd(tag, "ln", norm_fwd(env, "ln", x, w, b), x, w, b, dtype, const)
        o = norm_fwd(env, "ln", x, w, b, res=r)
        assert torch.equal(o["h"], x + r)
        check_fwd(tag + "+res", "ln", o, o["h"], w, b, dtype, const)
        p, seed = 0.1, 0x1234_5678_9ABC + rows
        o = norm_fwd(env, "ln", x, w, b, res=r, drop=(p, seed))
        keep = ops.hidden_dropout_keep_mask(seed, rows, cols, p)
        scale = torch.tensor(1.0 / (1.0 - float(np.float32(p))), dtype=F32)
        dropped = (x.cpu().float() * torch.where(keep, scale, torch.zeros(()))).to(dtype)  # the reference's dropout rounds
        assert torch.equal(o["h"].cpu(), (dropped.float() + r.cpu().float()).to(dtype))  # ... and so does its add
        check_fwd("layernorm_dropout_fwd", "ln", o, o["h"], w, b, dtype, None)  # (dropout leaves no constant row)


@pytest.mark.parametrize("dtype,cols", CASES)
def test_norm_backward_every_geometry(env, dtype, cols):
    """Every backward variant at 1, 5 and 7 rows: RMSNorm (plain, dres), LayerNorm (plain, dres, without db, with the
    column sums), LayerNorm + dropout (plain, dres, column sums).  The column-sum variants leave every other output
    bit-identical; column sums together with dres are refused before any launch."""
    for rows in (1, 5, 7):
        t = norm_inputs(rows, cols, dtype, env.device, 2000 + rows)
        dy, dres, w = t["dy"], t["dres"], t["w"]
        h = t["x"] + t["r"]
        hf = h.float()
        rstd = (hf.pow(2).mean(-1) + EPS).rsqrt()
        for dr in (None, dres):
            o = norm_bwd(env, "rms", dy, h, w, None, rstd, dres=dr)
            check_bwd("rmsnorm_bwd" + ("+dres" if dr is not None else ""), "rms", o, dy, h, w, None, rstd, dr, dtype)
        mean = hf.mean(-1)
        rstd = ((hf - mean[:, None]).pow(2).mean(-1) + EPS).rsqrt()
        plain = norm_bwd(env, "ln", dy, h, w, mean, rstd)
        check_bwd("layernorm_bwd", "ln", plain, dy, h, w, mean, rstd, None, dtype)
        o = norm_bwd(env, "ln", dy, h, w, mean, rstd, dres=dres)
        check_bwd("layernorm_bwd+dres", "ln", o, dy, h, w, mean, rstd, dres, dtype)
        o = norm_bwd(env, "ln", dy, h, w, mean, rstd, need_db=False)
        same(o, plain, ("dx", "dw"))
        o = norm_bwd(env, "ln", dy, h, w, mean, rstd, csum=True)
        same(o, plain, ("dx", "dw", "db"))
        check_bwd("layernorm_bwd+colsum", "ln", o, dy, h, w, mean, rstd, None, dtype)
        norm_bwd(env, "ln", dy, h, w, mean, rstd, dres=dres, csum=True, expect=E_ARG)
        drop = (0.1, 0x5EED_1234 + rows)
        keep = ops.hidden_dropout_keep_mask(drop[1], rows, cols, drop[0])
        dplain = norm_bwd(env, "ln", dy, h, w, mean, rstd, drop=drop)
        same(dplain, plain, ("dx", "dw", "db"))  # dx is the gradient of the residual input: dropout does not touch it
        check_bwd("layernorm_dropout_bwd", "ln", dplain, dy, h, w, mean, rstd, None, dtype, drop, keep)
        o = norm_bwd(env, "ln", dy, h, w, mean, rstd, dres=dres, drop=drop)
        check_bwd("layernorm_dropout_bwd+dres", "ln", o, dy, h, w, mean, rstd, dres, dtype, drop, keep)
        o = norm_bwd(env, "ln", dy, h, w, mean, rstd, csum=True, drop=drop)
        same(o, dplain, ("dx", "dxd", "dw", "db"))
        check_bwd("layernorm_dropout_bwd+colsum", "ln", o, dy, h, w, mean, rstd, None, dtype, drop, keep)


# 512 * RPB + 3 rows: the backward's grid is capped at 512 blocks, so a second grid-stride iteration runs in which only the
# first block has rows left -- every other block walks the "row past the matrix" path (zero-sized buffer descriptors, the
# fence-less barriers of group_sum with an inactive row group).  The narrowest width of each geometry; fp32 where only
# that keeps the tensor under 2.2 M elements.
LONG = [(BF16, 8), (BF16, 520), (F32, 516), (F32, 1028), (F32, 2052), (F32, 3844), (F32, 4100)]


@pytest.mark.parametrize("dtype,cols", [pytest.param(dt, c, id=f"{NAME[dt]}-{c}") for dt, c in LONG])
def test_norm_backward_second_grid_stride_iteration(env, dtype, cols):
    nch, wpr = geometry(cols, dtype)
    rows = MAX_PARTIALS * (4 // wpr) + 3
    assert [geometry(c, d) for d, c in LONG] == [(1, 1), (2, 1), (4, 1), (4, 2), (8, 2), (4, 4), (8, 4)]
    assert rows * cols <= 2_200_000
    t = norm_inputs(rows, cols, dtype, env.device, 3000)
    dy, dres, w = t["dy"], t["dres"], t["w"]
    h = t["x"]
    hf = h.float()
    rstd = (hf.pow(2).mean(-1) + EPS).rsqrt()
    o = norm_bwd(env, "rms", dy, h, w, None, rstd, dres=dres)
    check_bwd("long.rmsnorm_bwd+dres", "rms", o, dy, h, w, None, rstd, dres, dtype)
    mean = hf.mean(-1)
    rstd = ((hf - mean[:, None]).pow(2).mean(-1) + EPS).rsqrt()
    drop = (0.1, 0xABCD_0123)
    keep = ops.hidden_dropout_keep_mask(drop[1], rows, cols, drop[0])
    o = norm_bwd(env, "ln", dy, h, w, mean, rstd, csum=True, drop=drop)
    check_bwd("long.layernorm_dropout_bwd+colsum", "ln", o, dy, h, w, mean, rstd, None, dtype, drop, keep)


@pytest.mark.parametrize("dtype,cols", [(BF16, 16392), (BF16, 12), (F16, 16392), (F32, 8196), (F32, 6)])
def test_norm_refuses_unsupported_widths_before_any_launch(env, dtype, cols):
    """A width past the widest instantiation, or no multiple of the 16-byte vector: TAMD_E_SHAPE from the forward AND the
    backward, and no output is written."""
    assert geometry(cols, dtype) is None
    rows = 5
    x = torch.zeros(rows, cols, dtype=dtype, device=env.device)
    w = torch.ones(cols, dtype=dtype, device=env.device)
    stat = torch.ones(rows, dtype=F32, device=env.device)
    for kind in ("rms", "ln"):
        c = Call(env, x)
        y, h, mean, rstd = c.out("y", "mat"), c.out("h", "mat"), c.out("mean", "stat"), c.out("rstd", "stat")
        if kind == "rms":
            st = c.lib.tamd_rmsnorm_fwd(ptr(x), ptr(x), ptr(w), ptr(y), ptr(h), ptr(rstd), rows, cols, EPS, c.code, c.stream)
        else:
            st = c.lib.tamd_layernorm_fwd(ptr(x), ptr(x), ptr(w), ptr(w), ptr(y), ptr(h), ptr(mean), ptr(rstd), rows, cols,
                                          EPS, c.code, c.stream)
        assert st == E_SHAPE and all(g.untouched() for g in c.outs.values())
        norm_bwd(env, kind, x, x, w, stat, stat, expect=E_SHAPE)
    norm_bwd(env, "ln", x, x, w, stat, stat, csum=True, drop=(0.1, 1), expect=E_SHAPE)


# ---------------------------------------------------------------------------------------------------- cross-entropy
IGNORE = -100
CE_CASES = [(5, 8, BF16), (1000, 1000, BF16), (1003, 1008, BF16), (2049, 2056, BF16), (50257, 50264, BF16),
            (1003, 1008, F16), (1003, 1004, F32)]
PAD = 3.0e4  # what the padding columns of the logits hold: a kernel that read them would see it in every lse


def ce_logits(t, vocab, ld, dtype, dev):
    """Row 0 peaks at about +80 and row 1 at about -80 (no max-subtraction: exp leaves fp32's range or its precision),
    rows 3 / 4 at +100 / -100, past exp's fp32 range; row 2 has one element far above the rest, the LAST one: in the ragged
    tail whenever there is one."""
    g = torch.Generator().manual_seed(vocab)
    z = torch.randn(t, vocab, generator=g)
    z[0] *= 80.0 / z[0].max()
    z[1] = z[1] * 3.0 - (z[1] * 3.0).max() - 80.0
    z[2, vocab - 1] = 30.0
    z[3] *= 100.0 / z[3].max()
    z[4] = z[4] - z[4].max() - 100.0
    buf = torch.full((t, ld), PAD).to(dtype)
    buf[:, :vocab] = z.to(dtype)
    return buf.to(dev)


def ce_run(env, buf, vocab, labels, gscale):
    """-> lse, row_loss, the whole [t, ld] dlogits buffer; all three written into guarded buffers"""
    be = ops.backend()
    lib, stream = be.lib, be.stream(buf)
    t, ld = buf.shape
    dev, code = buf.device, ops._code(buf)
    lse, loss = Guarded((t,), F32, dev, 8), Guarded((t,), F32, dev, 8)
    d = Guarded((t, ld), buf.dtype, dev, ld)
    lab = labels.to(dev)
    gs = torch.tensor([gscale], dtype=F32, device=dev)
    before = buf.clone()
    st = lib.tamd_cross_entropy_fwd(ptr(buf), ptr(lab), ptr(lse.t), ptr(loss.t), t, vocab, ld, IGNORE, code, stream)
    assert st == 0
    st = lib.tamd_cross_entropy_bwd(ptr(buf), ptr(lab), ptr(lse.t), ptr(gs), ptr(d.t), t, vocab, ld, IGNORE, code, stream)
    assert st == 0
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert lse.intact() and loss.intact() and d.intact()
    assert torch.equal(buf, before)  # the logits, padding included, are read only
    return lse.t, loss.t, d.t


def ce_check(tag, buf, vocab, labels, gscale, lse, loss, d):
    t, ld = buf.shape
    dtype = buf.dtype
    z = d64(buf)[:, :vocab]
    n = vocab
    ref_lse = torch.logsumexp(z, -1)
    # lse = M + log S, S = sum exp(z - M) >= 1: n positive terms in any order move S by 2^-23 n S, lse by 2^-23 n; exp of an
    # fp32 argument and the log add a few ulps of their own
    s_lse = torch.full_like(ref_lse, U2 * (n + 16))
    check(f"{tag}.lse", lse, ref_lse, s_lse, F32)
    valid = (labels != IGNORE) & (labels >= 0) & (labels < vocab)
    picked = z.gather(1, labels.clamp(0, vocab - 1)[:, None])[:, 0]
    ref_loss = torch.where(valid, ref_lse - picked, torch.zeros_like(ref_lse))
    check(f"{tag}.row_loss", loss, ref_loss, s_lse + ulp(ref_lse, F32), F32)  # (lse is rounded before the subtraction)
    assert bool((loss.cpu()[~valid] == 0).all())
    # dlogits on the STORED lse: (exp(z - lse) - [col == label]) * gscale
    l = d64(lse)[:, None]
    p = (z - l).exp()
    onehot = torch.zeros_like(z)
    onehot[valid, labels[valid]] = 1.0
    gs = float(np.float32(gscale))
    ref = (p - onehot) * gs * valid[:, None].double()
    # exp(x), x = z - lse in fp32: the subtraction, the scaling by log2(e) and that constant's own rounding move the argument
    # by up to 1.25 * 2^-24 |x| each way, the hardware exp2 adds an ulp: 2^-23 (2 |x| + 2) relative with the factor two of
    # the other terms; the subtraction of the one-hot and the product with gscale are one operation each.  The
    # kernel's exp is the hardware's (`__expf`), which flushes results below fp32's smallest normal number, 2^-126, to
    # zero: an absolute floor under the probabilities of the rows at -80 / -100 (bf16 itself reaches down to 2^-133)
    # (and so may the product with gscale)
    s = abs(gs) * (U2 * (p * (2 * (z - l).abs() + 2) + 2 * (p - onehot).abs()) + 2.0 ** -126) + 2.0 ** -126
    dc = d.cpu()
    check(f"{tag}.dlogits", dc[:, :vocab], ref, s, dtype)
    assert bool((dc[~valid] == 0).all())  # ignored / out-of-range labels: a zero gradient row, exactly
    assert bool((dc[:, vocab:] == 0).all())  # the padding columns are zeroed (the buffer held the sentinel)


@pytest.mark.parametrize("vocab,ld,dtype", [pytest.param(v, l, dt, id=f"{NAME[dt]}-{v}-{l}") for v, l, dt in CE_CASES])
def test_cross_entropy_ragged_vocab_and_labels(env, vocab, ld, dtype):
    t = 5
    buf = ce_logits(t, vocab, ld, dtype, env.device)
    # the last (tail) element, element 0, ignore_index, a negative label that is not ignore_index, a label >= vocab
    labels = torch.tensor([vocab - 1, 0, IGNORE, -5, vocab], dtype=torch.int64)
    lse, loss, d = ce_run(env, buf, vocab, labels, 1.0)
    ce_check("cross_entropy", buf, vocab, labels, 1.0, lse, loss, d)
    # every row valid (the spike of row 2 is its label), gscale != 1
    labels2 = torch.tensor([0, vocab - 1, vocab - 1, min(1, vocab - 1), vocab // 2], dtype=torch.int64)
    lse2, loss2, d2 = ce_run(env, buf, vocab, labels2, 0.37)
    assert torch.equal(lse2, lse)
    ce_check("cross_entropy", buf, vocab, labels2, 0.37, lse2, loss2, d2)
    # every row ignored
    labels3 = torch.tensor([IGNORE, -1, vocab, IGNORE, vocab + 7], dtype=torch.int64)
    lse3, loss3, d3 = ce_run(env, buf, vocab, labels3, 1.0)
    assert torch.equal(lse3, lse) and bool((loss3 == 0).all()) and bool((d3 == 0).all())
    # the compiled ops on the [t, vocab] view: the same bits, and the padding of the buffer they allocate is zero
    view = buf[:, :vocab]
    lse_o, loss_o = ops.raw_cross_entropy_fwd(view, labels2.to(env.device), IGNORE)
    dv = ops.raw_cross_entropy_bwd(view, labels2.to(env.device), lse_o, torch.tensor([0.37], dtype=F32, device=env.device), IGNORE)
    assert torch.equal(lse_o, lse2) and torch.equal(loss_o, loss2) and torch.equal(dv, d2[:, :vocab])
    whole = torch.as_strided(dv, (t, ld), (ld, 1), dv.storage_offset())
    assert torch.equal(whole, d2)
    assert torch.equal(buf.cpu()[:, vocab:], torch.full((t, ld - vocab), PAD).to(dtype))


# ---------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_colsum_row_tails_and_slabs(env, dtype):
    """tamd_colsum: eight rows per trip and a tail (1, 7, 8, 9 rows), slabs of at least 16 rows (513 rows: 33 slabs, the
    last of one row; 1031: 64 slabs of 16 rows and one of 7), one to five threads' worth of columns."""
    be = ops.backend()
    lib = be.lib
    g = torch.Generator().manual_seed(7)
    for rows in (1, 7, 8, 9, 513, 1031):
        for cols in (8, 136, 1032):
            x = torch.randn(rows, cols, generator=g).to(dtype).to(env.device)
            out = Guarded((cols,), dtype, env.device, cols)
            n = lib.tamd_colsum_workspace_bytes(rows, cols)
            ws = workspace(env.device, n)
            st = lib.tamd_colsum(ptr(x), ptr(out.t), ptr(ws), n, rows, cols, cols, ops._code(x), be.stream(x))
            assert st == 0
            if env.device.type == "cuda":
                torch.cuda.synchronize()
            assert out.intact()
            xd = d64(x)
            check("colsum", out.t, xd.sum(0), U2 * rows * xd.abs().sum(0), dtype)
            assert torch.equal(ops.raw_colsum(x), out.t)  # (the compiled op allocates its output: nothing to guard there)
    # a column slice of a wider buffer: the op passes the row stride on
    rows, cols, off = 37, 136, VE[dtype]
    wide = torch.randn(rows, cols + 2 * off, generator=g).to(dtype).to(env.device)
    xd = d64(wide)[:, off:off + cols]
    check("colsum.slice", ops.raw_colsum(wide[:, off:off + cols]), xd.sum(0), U2 * rows * xd.abs().sum(0), dtype)
