"""Plain/guarded operand factory, the two-run driver and the error metrics shared by the guard
test files (tests/test_gpu_guard.py: conv and vision kernels; tests/test_gpu_guard_transformer.py:
the Whisper path).  A plain module next to ``kernel_guard.py``: no fixtures; the metrics
(``rel_err``, ``row_errs`` / ``row_err``, ``pixel_channel_errs`` / ``assert_pixel_channel``) work
on the CPU."""
from __future__ import annotations

import dataclasses

import torch

from kernel_guard import BYTE_NAN, guarded

DEV = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")
# per-row bound of a bf16 output: one rounding of an fp32 value moves an element by at most 2^-8
# of itself (half an ulp of 8 significand bits) and a row's norm by about 2^-9
ROW_BOUND = 2.0 ** -8


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def rel_err(a, b):
    """Whole-tensor ``||a - b|| / ||b||``."""
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def row_errs(y, ref):
    """``||y[m] - ref[m]|| / ||ref[m]||`` of every row m of a 2-D tensor, an fp64 vector.  A row
    whose reference norm is 0 is compared exactly: any non-zero element there, like any
    non-finite element anywhere, gives ``inf``."""
    y, ref = y.double(), ref.double()
    assert y.dim() == 2 and y.shape == ref.shape, (y.shape, ref.shape)
    num, den = (y - ref).norm(dim=1), ref.norm(dim=1)
    err = torch.where(den > 0, num / den.clamp(min=1e-300), torch.where(num == 0, 0.0, float("inf")))
    return torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))


def row_err(y, ref):
    """``max_m`` of :func:`row_errs` (0 for an empty tensor)."""
    errs = row_errs(y, ref)
    return errs.max().item() if errs.numel() else 0.0


def pixel_channel_errs(y_nhwc, ref_nhwc):
    """``(per_pixel[M], per_channel[N])`` of an NHWC (or ``[M, N]``) output: :func:`row_errs` of
    the ``[M, N]`` view (M = every dimension but the last) and of its transpose."""
    assert y_nhwc.shape == ref_nhwc.shape, (y_nhwc.shape, ref_nhwc.shape)
    N = y_nhwc.shape[-1]
    y, ref = y_nhwc.reshape(-1, N).double(), ref_nhwc.reshape(-1, N).double()
    if y.device != ref.device:
        y = y.to(ref.device)
    return row_errs(y, ref), row_errs(y.T, ref.T)


def _where(idx, shape):
    """Flat pixel index -> ``(b, h, w)`` for an NHWC shape, ``(m,)`` otherwise."""
    if len(shape) != 4:
        return (int(idx),)
    _, H, W, _ = shape
    return (int(idx) // (H * W), int(idx) // W % H, int(idx) % W)


def assert_pixel_channel(y_nhwc, ref_nhwc, bound=ROW_BOUND, what=""):
    """Print the worst pixel (as ``(b, h, w)`` and flat row) and the worst channel, then assert
    both are below ``bound``.  The failure message counts the pixels and channels over the bound
    and names the first and the last of each, so a tile or border pattern shows in the log.
    Returns ``(worst pixel error, worst channel error)``."""
    pix, ch = pixel_channel_errs(y_nhwc, ref_nhwc)
    shape = tuple(y_nhwc.shape)
    pi, ci = int(pix.argmax()), int(ch.argmax())
    pe, ce = pix[pi].item(), ch[ci].item()
    print(f"parity {what}: shape {shape} worst pixel {_where(pi, shape)} (row {pi}) {pe:.3e}, "
          f"worst channel {ci} {ce:.3e}, bound {bound:.3e}")
    bad_p, bad_c = torch.nonzero(~(pix < bound)).flatten().tolist(), torch.nonzero(~(ch < bound)).flatten().tolist()
    if bad_p or bad_c:
        msg = [f"{what}: per-pixel / per-channel bound {bound:.3e} exceeded (shape {shape})"]
        if bad_p:
            msg.append(f"{len(bad_p)} of {pix.numel()} pixels: first {_where(bad_p[0], shape)} (row {bad_p[0]}) "
                       f"{pix[bad_p[0]].item():.3e}, last {_where(bad_p[-1], shape)} (row {bad_p[-1]}) "
                       f"{pix[bad_p[-1]].item():.3e}, worst row {pi} {pe:.3e}")
        if bad_c:
            msg.append(f"{len(bad_c)} of {ch.numel()} channels: first {bad_c[0]} {ch[bad_c[0]].item():.3e}, "
                       f"last {bad_c[-1]} {ch[bad_c[-1]].item():.3e}, worst {ci} {ce:.3e}")
        raise AssertionError("; ".join(msg))
    return pe, ce


def attn_split_plan(B, H, T, cus, pieces, nw=8, work_bytes=None):
    """What attention.hip's launcher does with ``AIKO_ATTN_SPLIT_S = pieces`` and a workspace:
    ``(r, sp, cnt_bytes)`` — split items per XCD, pieces per item, and the byte offset of the
    fp32 partials in the workspace — or ``(r, 0, 0)`` when it falls back to the plain grid
    (items not a multiple of 8, no partial last round, or one that is more than half full)."""
    qb = 32 * nw
    items = -(-T // qb) * H * B
    ntiles = -(-T // 64)
    if pieces <= 0 or cus < 8 or items % 8:
        return 0, 0, 0
    slots = (16 // nw) * (cus // 8)
    r = (items // 8) % slots
    if r == 0 or 2 * r > slots:
        return r, 0, 0
    sp = min(pieces, ntiles)
    cnt_b = (8 * r * 4 + 255) // 256 * 256
    if work_bytes is not None and cnt_b + 8 * r * sp * qb * 66 * 4 > work_bytes:
        return r, 0, 0
    return r, sp, cnt_b


class Operands:
    """Tensor factory of one run: plain (fresh tensors) or guarded (views between NaN guards).
    ``byte_nan``: 1-byte tensors hold fp8 values / E8M0 scales, so their guards (and an output's
    interior) are ``0xFF`` bytes — NaN in both formats — instead of ``0xA5``."""

    def __init__(self, on: bool, poison=None, byte_nan: bool = False):
        self.on, self.checks, self.poison, self.byte_nan = on, [], poison, byte_nan

    @property
    def gap(self):
        """What the gap channels of a sliced input hold: zero (plain) or the poison (guarded)."""
        return 0.0 if not self.on else NAN if self.poison is None else self.poison

    @property
    def byte_gap(self):
        """The same for fp8 / E8M0 bytes: zero (plain) or ``0xFF`` (guarded)."""
        return BYTE_NAN if self.on else 0

    def _guard(self, shape, dtype, values, name):
        poison = self.poison if dtype.is_floating_point else \
            BYTE_NAN if self.byte_nan and torch.empty(0, dtype=dtype).element_size() == 1 else None
        view, check = guarded(shape, dtype, DEV, values=values, name=name, poison=poison)
        self.checks.append(check)
        return view

    def inp(self, values, name="input"):
        """An input holding ``values`` (CPU or device tensor)."""
        if not self.on:
            return values.to(DEV).contiguous().clone()
        return self._guard(values.shape, values.dtype, values.to(DEV), name)

    def inp_slice(self, values, pitch, c0, name="input slice"):
        """``values`` [..., C] as channels [c0, c0 + C) of a [..., pitch] buffer (ld > C).  The
        gap channels are zero in the plain run (as the other test files have them) and poison in
        the guarded run."""
        C = values.shape[-1]
        gap = self.gap if values.dtype.is_floating_point else self.byte_gap
        wide = torch.full((*values.shape[:-1], pitch), gap, dtype=values.dtype)
        wide[..., c0:c0 + C] = values
        return self.inp(wide, name)[..., c0:c0 + C]

    def out(self, shape, dtype=BF16, name="output"):
        """An output: NaN (floating point) in both runs, so an unwritten element is non-finite."""
        if not self.on:
            return torch.full(shape, NAN, dtype=dtype, device=DEV) if dtype.is_floating_point else \
                torch.zeros(shape, dtype=dtype, device=DEV)
        return self._guard(shape, dtype, None, name)

    def spec(self, spec, name="spec"):
        """``spec`` with its weight and bias swapped for guarded copies: a NEW ConvSpec, so every
        derived image (patch / patchw / rows / exp / stem images) is re-derived from them."""
        if not self.on:
            return dataclasses.replace(spec)
        return dataclasses.replace(spec, weight=self.inp(spec.weight, name + ".weight"),
                                   bias=None if spec.bias is None else self.inp(spec.bias, name + ".bias"))

    def check(self):
        for c in self.checks:
            c()


def run_both(case, poison=None, byte_nan: bool = False):
    """``case(ops) -> tensor | tuple of tensors``: run plain and guarded, assert 1-3, return the
    plain outputs (for assertion 4, the caller's).  ``poison``: a finite value instead of NaN in
    the guards and gap channels (max-reductions).  ``byte_nan``: see :class:`Operands`."""
    plain_ops = Operands(False, byte_nan=byte_nan)
    plain = case(plain_ops)
    torch.cuda.synchronize()
    ops = Operands(True, poison, byte_nan)
    from aiko_services_amd.ops import conv as C
    saved = dict(C._ZERO)                   # the LDS-DMA kernels' zero page is an operand too
    try:
        dev = torch.device(DEV, torch.cuda.current_device())
        C._ZERO[dev] = ops.inp(torch.zeros(32, dtype=BF16), "zero page")
        guard = case(ops)
        torch.cuda.synchronize()
    finally:
        C._ZERO.clear()
        C._ZERO.update(saved)
    single = not isinstance(plain, (tuple, list))
    plain, guard = ((plain,), (guard,)) if single else (tuple(plain), tuple(guard))
    assert ops.checks, "the guarded run allocated no guarded tensor"
    ops.check()                                                                   # 1
    for i, t in enumerate(guard):                                                 # 2
        if t.dtype.is_floating_point:
            bad = (~torch.isfinite(t.float())).sum().item()
            assert bad == 0, f"guarded output {i}: {bad} non-finite element(s) (poison consumed or unwritten)"
    for i, (p, t) in enumerate(zip(plain, guard)):                                # 3
        if not torch.equal(_bits(p), _bits(t)):
            n = (_bits(p) != _bits(t)).sum().item()
            raise AssertionError(f"output {i}: {n} element(s) differ between the plain and the guarded run")
    return plain[0] if single else plain
