"""What the per-element kernel tests share (tests/test_row_kernels.py, tests/test_gemm_elements.py): the unit in the last
place of a storage type, the per-element gate, and outputs that live inside sentinel-filled buffers.

    |got - ref| <= gate * (ulp_T(ref) + s),      gate = 2 * max(0.5, own)

ulp_T(ref): the unit in the last place of the storage type T at ref.
s:          what fp32 arithmetic may add in front of the output rounding; worked out by the caller, per output.
own:        the float64 reference's OWN error in that unit once it is rounded as the kernel documents its roundings.
Neither term comes from a kernel's output."""
import numpy as np
import torch

from conftest import record

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
MANT = {BF16: 7, F16: 10, F32: 23}
MINEXP = {BF16: -126, F16: -14, F32: -126}
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}
SENT = -3.0


def ulp(ref, dtype):
    m, e = torch.frexp(ref.abs())  # |ref| = m * 2^e, m in [0.5, 1)
    e = torch.where(ref != 0, e.to(torch.int64) - 1, torch.full_like(e, MINEXP[dtype], dtype=torch.int64))
    return torch.ldexp(torch.ones_like(ref), e.clamp_min(MINEXP[dtype]) - MANT[dtype])


def rnd(t64, dtype):
    return t64.to(dtype).double()


_WORST = {}


def check(name, got, ref, s, dtype, chain=None, group="row_kernels", own_floor=0.0):
    """Every element of `got` within the gate of the module docstring; `chain`: the reference rounded as the kernel
    documents (default: once to the storage type); `own_floor`: a further error of the reference's side, in the same unit
    (torch's fp32 operator on the same input), that `own` may not fall below."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    unit = ulp(ref, dtype) + s
    own = (((rnd(ref, dtype) if chain is None else chain) - ref).abs() / unit).max().item()
    own = max(own, own_floor)
    gate = 2.0 * max(0.5, own)
    ratio = (got - ref).abs() / unit
    worst = ratio.max().item()
    key = f"{name}[{NAME[dtype]}]"
    w = _WORST.setdefault((group, key), [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], worst if worst == worst else float("inf")), max(w[1], gate), max(w[2], own)
    record(group, key, w[0], w[1])
    record(group, key + " reference's own rounding", w[2])
    print(f"{key}: worst {worst:.3f} gate {gate:.3f} (reference's own {own:.3f}) over {got.numel()} elements")
    if not worst <= gate:  # (NaN fails)
        bad = torch.nonzero(~(ratio <= gate))
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{key}: {bad.shape[0]} of {got.numel()} elements beyond {gate:.3f} x (ulp + s); first at {i}: "
                             f"got {got[i].item()!r} want {ref[i].item()!r} unit {unit[i].item():.3e}; worst {worst:.3f}")


class Guarded:
    """`n` elements in the middle of a buffer filled with a sentinel, `guard` elements on either side."""

    def __init__(self, shape, dtype, device, guard):
        n = int(np.prod(shape))
        self.guard = guard
        self.buf = torch.full((n + 2 * guard,), SENT, dtype=dtype, device=device)
        self.t = self.buf[guard:guard + n].view(*shape)

    def intact(self):
        g = self.guard
        return bool((self.buf[:g] == SENT).all()) and bool((self.buf[-g:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


class GuardedMatrix(Guarded):
    """[rows, cols] with row stride ld >= cols inside a sentinel-filled buffer: at least four rows of ld elements on either
    side, and the ld - cols gap columns of every row are sentinel too.  `fill`: what the matrix holds before the call."""

    def __init__(self, rows, cols, ld, dtype, device, fill=None):
        assert ld >= cols
        super().__init__((rows, ld), dtype, device, 4 * ld + 64)
        self.full, self.cols = self.t, cols
        self.t = self.full[:, :cols]
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        return super().intact() and bool((self.full[:, self.cols:] == SENT).all())
