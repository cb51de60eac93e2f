"""Operands and references of the conv / fused-block parity cases, shared by the GPU tests
(tests/test_gpu_guard.py, test_gpu_bneck.py, test_gpu_conv_exp.py) and the reference-only CPU
checks (tests/test_conv_parity_reference.py).  A plain module in the style of ``guard_ops.py``: no
fixtures.  Every builder makes its operands on the CPU from a seeded generator — the seeds and
shapes the GPU tests have always used — so both files see identical data.

A :class:`Case` holds the CPU operands (``ops``), the ConvSpecs (``specs``; their packed weight
and bias on ``device``, their ``ref_weight`` / ``ref_bias`` on the CPU) and ``fn(dtype, ops,
specs) -> tuple of NHWC outputs``: the reference of the kernel, evaluated in ``dtype`` on the CPU
and rounded to bf16 exactly where the kernel stores bf16 (to LDS or to memory) before reading the
value again.  ``case.ref64`` is that function in fp64 (computed once, never modified);
``case.eval32()`` the same in fp32, rounded to bf16 at the end as a kernel's output is.

The bound of every family is ``guard_ops.ROW_BOUND`` = 2^-8 except c2f_fused's 32-channel kernel
(YOLOv8-n l2), whose fp32 evaluation alone exceeds it: see C2F_L2_BOUND.
"""
from __future__ import annotations

import dataclasses
import functools

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16

ROW_BOUND = 2.0 ** -8           # guard_ops.ROW_BOUND

# c2f_fused's l2 kernel: 32 -> (16 | 16) -> 32 channels, four bf16 roundings in a row.  With 16
# channels per intermediate one flipped rounding of [a | s], t or c is a visible part of a pixel's
# 32 outputs, so the fp32 evaluation on the CPU already differs from the fp64 one by more than
# 2^-8 at single pixels: worst per-pixel figure of check (a) over the three l2 cases 4.964e-3
# (rb = 20's input; 3.440e-3 and 3.883e-3 for the other two; per channel at most 1.764e-3).  The
# family's bound is 2^-8 plus twice that excess — a reference-only quantity, no kernel output went
# into it.  The 64-channel l15 kernel (worst 3.165e-3) and c2f_bneck (2.715e-3) keep 2^-8.
C2F_L2_CPU_WORST = 4.964e-3
C2F_L2_BOUND = ROW_BOUND + 2 * (C2F_L2_CPU_WORST - ROW_BOUND)          # 6.02e-3


def nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous()


def nchw(x_nhwc):
    return x_nhwc.permute(0, 3, 1, 2)


def rb(t):
    """Round to bf16 and back: a point where the kernel stores bf16."""
    return t.to(BF16).to(t.dtype)


def _R():
    from aiko_services_amd.ops import reference as R
    return R


def _C():
    from aiko_services_amd.ops import conv as C
    return C


@dataclasses.dataclass
class Case:
    name: str
    ops: dict
    specs: dict
    fn: object                      # fn(dtype, ops, specs) -> tuple of NHWC tensors
    last: str                       # the spec whose bias reaches the last output directly
    k3: str | None = None           # a single k x k conv (k > 1) with this spec: the border-tap corruption
    _ref64: tuple | None = None

    @property
    def ref64(self):
        """The fp64 reference outputs (NHWC, CPU), computed once."""
        if self._ref64 is None:
            self._ref64 = tuple(t.contiguous() for t in self.fn(torch.float64, self.ops, self.specs))
        return self._ref64

    def eval32(self, specs=None, ops=None):
        """The fp32 evaluation on the CPU, rounded to bf16 like a kernel's output."""
        return tuple(t.to(BF16) for t in self.fn(torch.float32, ops or self.ops, specs or self.specs))

    def with_bias(self, name, channel, factor):
        """``specs`` with ``specs[name]``'s reference bias of ``channel`` scaled by ``factor``."""
        s = self.specs[name]
        b = s.ref_bias.clone()
        b[channel] *= factor
        return {**self.specs, name: dataclasses.replace(s, ref_bias=b)}


def kernel_spec_with_bias(spec, channel, factor):
    """``spec`` for a kernel (``dataclasses.replace``) with the device bias of ``channel`` scaled
    by ``factor``; the reference fields are untouched, so the reference does not see it."""
    b = spec.bias.clone()
    b[channel] *= factor
    return dataclasses.replace(spec, bias=b)


def top_bias_channel(spec):
    return int(spec.ref_bias.abs().argmax())


def receptive(b, h, w, convs, H, W):
    """Output pixels (flat indices into [B, Ho, Wo]) that read input pixel ``(b, h, w)`` of an
    H x W image through the chain ``convs`` = [(k, stride, pad), ...]; and (Ho, Wo)."""
    pix = {(h, w)}
    for k, s, p in convs:
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        nxt = set()
        for (ih, iw) in pix:
            for r in range(k):
                for c in range(k):
                    oh, ow = ih + p - r, iw + p - c
                    if oh % s == 0 and ow % s == 0 and 0 <= oh // s < Ho and 0 <= ow // s < Wo:
                        nxt.add((oh // s, ow // s))
        pix, H, W = nxt, Ho, Wo
    return sorted((b * H + oh) * W + ow for oh, ow in pix), (H, W)


# ---- single convs --------------------------------------------------------------------------------

def _conv_fn(after=False, add_after=False):
    def fn(dtype, ops, specs):
        R = _R()
        r = ops.get("r")
        r = None if r is None else r.to(dtype)
        if add_after:                               # conv3x3_rows, res == "after": act(conv) + r
            return (nhwc(R.conv_ref(ops["x"].to(dtype), specs["conv"]) + r),)
        return (nhwc(R.conv_ref(ops["x"].to(dtype), specs["conv"], r, residual_after_act=after)),)
    return fn


_G13 = (1, 13, 9, 192, 72, 3, 2, 1, "gelu", True)
_S200 = (1, 9, 11, 128, 200, 3, 1, 1, "silu", True)
_N7 = (1, 9, 10, 16, 32, 3, 1, 1, "gelu", True)
_PW = (3, 14, 14, 256, 1024, 1, 1, 0, None, True)
_G13x3 = (3,) + _G13[1:]
G13x24 = (24,) + _G13[1:]
PW_MULTI = (11, 14, 14, 256, 2048, 1, 1, 0, "relu", True)
V4_MULTI = (3, 75, 75, 64, 72, 3, 1, 1, "gelu", True)

CONV_CASES = [
    # variants 0 / 1: register-staged and LDS-DMA igemm (N tail Cout = 24; exact-N 80)
    ((1, 9, 11, 40, 24, 3, 1, 1, None, False), (64, 64), 0),
    ((1, 9, 11, 40, 24, 3, 1, 1, None, False), (64, 64, 1), 0),
    ((1, 13, 17, 80, 80, 1, 1, 0, None, True), (128, 80, 1), 0),
    # variants 2 / 3 / 5 / 6: buffer-DMA kernels
    (_G13, (128, 64, 2), 0),
    ((1, 9, 11, 128, 64, 3, 1, 1, "silu", False), (64, 64, 3), 0),
    ((1, 9, 11, 128, 64, 3, 2, 1, "silu", False), (256, 128, 5), 0),
    ((1, 9, 11, 128, 256, 3, 2, 1, "silu", True), (128, 256, 6), 0),
    # variants 4 / 20: persistent walks, 3 workgroups; B = 3: several tiles, ending on the tail
    (_G13, (64, 64, 4), 3), (_G13, (256, 128, 20), 3),
    (_G13x3, (64, 64, 4), 3), (_G13x3, (256, 128, 20), 3),
    # ... B = 24: four 256-row tiles over 3 workgroups, workgroup 0 walks tiles 0 and 3 (the
    # tail); with and without a residual (3- and 2-slot forms)
    (G13x24, (256, 128, 20), 3), ((24,) + _G13[1:9] + (False,), (256, 256, 20), 3),
    # variant 4 sizes its grid from the CU count alone (2 workgroups per CU): 264 x 2 tiles of
    # 64 x 64 are more than 512 slots, so every workgroup walks two tiles and the last one ends
    # on the 43-row tail — the only multi-tile walk of this kernel in the suite
    (V4_MULTI, (64, 64, 4), -1),
    # variants 8 / 9 / 11 / 19: conv_wide (N tail Cout = 200 / 72)
    (_S200, (256, 128, 8), 0), (_S200, (256, 128, 11), 0), (_S200, (128, 256, 19), 0),
    (_G13, (64, 128, 9), 0), (_G13, (128, 128, 19), 0),
    # variant 18: exact-N conv_wide
    ((2, 9, 13, 128, 144, 3, 1, 1, "silu", True), (128, 144, 18), 0),
    ((1, 17, 19, 64, 160, 3, 1, 1, "relu", True), (256, 80, 18), 0),
    # variant 7: direct narrow kernel (tiles of 8 / 16 rows x 32 columns)
    (_N7, (8, 32, 7), 0), (_N7, (16, 32, 7), 0),
    ((1, 9, 10, 32, 32, 3, 1, 1, "gelu", True), (16, 64, 7), 0),
    ((1, 33, 65, 16, 32, 3, 2, 1, "silu", False), (8, 32, 7), 0),
    # variants 12 / 13 / 14: persistent pointwise kernels
    (_PW, (128, 128, 12), 0), (_PW, (64, 128, 13), 0), (_PW, (64, 128, 14), 0),
    ((1, 7, 7, 512, 2048, 1, 1, 0, "relu", True), (64, 128, 13), 0),
    ((1, 7, 7, 128, 512, 1, 1, 0, "relu", True), (64, 128, 13), 0),
    # ... with more M tiles than workgroups per channel block (CUs / (Cout / BN) of them, from
    # the CU count alone), so some workgroup walks several tiles and ends on the tail: K = 256
    # (BN 128), K = 512 (BN 64), K = 128 (BN 256)
    (PW_MULTI, (128, 128, 12), -2),
    (PW_MULTI, (64, 128, 13), -2),
    (PW_MULTI, (64, 128, 14), -2),
    ((12, 7, 7, 512, 2048, 1, 1, 0, "relu", True), (64, 128, 13), -2),
    ((3, 28, 28, 128, 2048, 1, 1, 0, "silu", False), (64, 128, 13), -2),
]
CONV_SHAPES = list(dict.fromkeys(c[0] for c in CONV_CASES))      # the distinct operand sets


@functools.lru_cache(maxsize=None)
def conv_case(shape, device=None):
    """One ``CONV_CASES`` shape ``(B, H, W, cin, cout, k, stride, pad, act, res)``, seed 1234."""
    C = _C()
    B, H, W, cin, cout, k, stride, pad, act, res = shape
    g = torch.Generator().manual_seed(1234)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    spec = C.make_conv_spec(w, b, stride=stride, pad=pad, act=act, device=device)
    x = torch.randn(B, cin, H, W, generator=g).to(BF16)
    x_nhwc = torch.zeros(B, H, W, spec.Cc, dtype=BF16)
    x_nhwc[..., :cin] = nhwc(x)
    Ho, Wo = spec.out_hw(H, W)
    r = torch.randn(B, cout, Ho, Wo, generator=g).to(BF16) if res else None
    return Case("conv-" + "x".join(str(s) for s in shape[:8]), {"x": x, "x_nhwc": x_nhwc, "r": r},
                {"conv": spec}, _conv_fn(), "conv", "conv" if k > 1 else None)


SLICE_CASES = [(32, 64, 3, (64, 64), 96, 0), (32, 64, 3, (64, 64), 96, 32), (32, 64, 3, (64, 64, 1), 96, 32),
               (40, 24, 3, (64, 64, 1), 64, 8), (16, 16, 3, (8, 32, 7), 48, 16), (32, 32, 3, (16, 64, 7), 96, 32),
               (128, 64, 3, (64, 64, 2), 192, 64), (128, 64, 3, (64, 64, 4), 192, 64),
               (128, 200, 3, (256, 128, 8), 192, 64), (128, 144, 3, (128, 144, 18), 192, 32),
               (256, 256, 1, (128, 128, 12), 384, 64), (256, 256, 1, (64, 128, 13), 384, 64),
               (128, 256, 1, (64, 128, 13), 384, 64)]
SLICE_SHAPES = list(dict.fromkeys(c[:3] for c in SLICE_CASES))


@functools.lru_cache(maxsize=None)
def slice_case(cin, cout, k, device=None):
    """test_conv2d_channel_slices_guarded: 2 x 9 x 11, SiLU, the residual after it; seed 7."""
    C = _C()
    g = torch.Generator().manual_seed(7)
    B, H, W = 2, 9, 11
    x = torch.randn(B, H, W, cin, generator=g).to(BF16)
    r = torch.randn(B, H, W, cout, generator=g).to(BF16)
    spec = C.make_conv_spec(torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5,
                            torch.randn(cout, generator=g) * 0.1, pad=k // 2, act="silu", device=device)
    return Case(f"slices-{cin}-{cout}-k{k}", {"x": nchw(x), "r": nchw(r), "x_nhwc": x, "r_nhwc": r},
                {"conv": spec}, _conv_fn(after=True), "conv", "conv" if k > 1 else None)


def _dual_fn(dtype, ops, specs):
    R = _R()
    idn = R.conv_ref(nchw(ops["x"]).to(dtype), specs["down"])
    return (nhwc(R.conv_ref(nchw(ops["t"]).to(dtype), specs["main"], idn)),)


PW_DUAL_CASES = [(1, 18, 384, 2), (2, 18, 384, 2), (13, 18, 2048, 2)]
# With the unit-variance biases of these cases a ReLU channel can be dead (all of its M outputs
# zero: a zero-norm column, which the fp64 reference may not have).  The seeds B * 100 + H + cout
# gave 4 / 2 / 1 such channels; these are the first of seed + 1000 k without one.
_PW_DUAL_SEED = {(1, 384): 35502, (2, 384): 20602, (13, 2048): 5366}


@functools.lru_cache(maxsize=None)
def pw_dual_case(B, H, cout, stride, device=None):
    """test_conv_pw_dual_guarded: relu(main(t) + down(x)), K = 128 + 256."""
    C = _C()
    g = torch.Generator().manual_seed(_PW_DUAL_SEED[(B, cout)])
    Ho = (H - 1) // stride + 1
    main = C.make_conv_spec(torch.randn(cout, 128, 1, 1, generator=g) / 128 ** 0.5, torch.randn(cout, generator=g),
                            act="relu", device=device)
    down = C.make_conv_spec(torch.randn(cout, 256, 1, 1, generator=g) / 256 ** 0.5, torch.randn(cout, generator=g),
                            stride=stride, device=device)
    t = torch.randn(B, Ho, Ho, 128, generator=g).to(BF16)
    x = torch.randn(B, H, H, 256, generator=g).to(BF16)
    return Case(f"pw_dual-{B}-{cout}", {"t": t, "x": x}, {"main": main, "down": down}, _dual_fn, "main")


@functools.lru_cache(maxsize=None)
def projection_case(device=None):
    """test_fused_projection_guarded: conv3(t) + down(x), 512 + 1024 -> 2048, M = 49; seed 21.
    The two biases are 0.25 * randn: with unit variance 30 to 53 of the 2048 ReLU channels were
    dead (zero-norm columns) at every one of 20 seeds tried — at M = 49 no seed avoids them."""
    C = _C()
    B, H, cin_main, cin_sc, cout, stride = 1, 14, 512, 1024, 2048, 2
    g = torch.Generator().manual_seed(21)
    Ho = H // stride
    main = C.make_conv_spec(torch.randn(cout, cin_main, 1, 1, generator=g) / cin_main ** 0.5,
                            0.25 * torch.randn(cout, generator=g), act="relu", device=device)
    down = C.make_conv_spec(torch.randn(cout, cin_sc, 1, 1, generator=g) / cin_sc ** 0.5,
                            0.25 * torch.randn(cout, generator=g), stride=stride, device=device)
    t = torch.randn(B, Ho, Ho, cin_main, generator=g).to(BF16)
    x = torch.randn(B, H, H, cin_sc, generator=g).to(BF16)
    return Case("projection", {"t": t, "x": x}, {"main": main, "down": down}, _dual_fn, "main")


PATCH_CASES = [(3, 1, 24, "relu"), (3, 13, 24, "silu")]
PATCHW_CASES = [(2, 5, "relu", True, 0), (4, 14, None, False, 1), (3, 30, "relu", False, 2)]
ROWS_CASES = [(2, 1, None, "after", False, 1), (4, 3, "silu", None, True, 5), (3, 7, "relu", "before", True, 4)]


@functools.lru_cache(maxsize=None)
def patch_case(B, H, W, act, device=None):
    C = _C()
    g = torch.Generator().manual_seed(B * 100 + H)
    spec = C.make_conv_spec(torch.randn(64, 64, 3, 3, generator=g) / 24, torch.randn(64, generator=g) * 0.1,
                            pad=1, act=act, device=device)
    x = torch.randn(B, 64, H, W, generator=g).to(BF16)
    return Case(f"patch-{B}-{H}", {"x": x}, {"conv": spec}, _conv_fn(), "conv", "conv")


@functools.lru_cache(maxsize=None)
def patchw_case(B, H, act, device=None):
    C = _C()
    g = torch.Generator().manual_seed(B * 100 + H)
    spec = C.make_conv_spec(torch.randn(128, 128, 3, 3, generator=g) / (128 * 9) ** 0.5,
                            torch.randn(128, generator=g) * 0.1, pad=1, act=act, device=device)
    x = torch.randn(B, 128, H, 28, generator=g).to(BF16)
    return Case(f"patchw-{B}-{H}", {"x": x}, {"conv": spec}, _conv_fn(), "conv", "conv")


@functools.lru_cache(maxsize=None)
def rows_case(B, H, act, res, device=None):
    C = _C()
    g = torch.Generator().manual_seed(B * 31 + H)
    spec = C.make_conv_spec(torch.randn(32, 32, 3, 3, generator=g) / (32 * 9) ** 0.5,
                            torch.randn(32, generator=g) * 0.1, pad=1, act=act, device=device)
    x = torch.randn(B, 32, H, 80, generator=g).to(BF16)
    r = torch.randn(B, 32, H, 80, generator=g).to(BF16) if res else None
    return Case(f"rows-{B}-{H}", {"x": x, "r": r}, {"conv": spec}, _conv_fn(add_after=res == "after"), "conv", "conv")


# ---- ResNet fused kernels ------------------------------------------------------------------------

def _chain_fn(dtype, ops, specs):
    """conv_chain.hip: Y = relu(x . W1^T + b1 + r) is rounded to bf16 in LDS — the stored output
    and the A operand of the second GEMM are that same tile."""
    R = _R()
    y = rb(R.conv_ref(nchw(ops["x"]).to(dtype), specs["c3"], nchw(ops["r"]).to(dtype)))
    return nhwc(y), nhwc(R.conv_ref(y, specs["c1"]))


CHAIN_CASES = [(k1, n1, n2, B, H, W, grid) for (k1, n1, n2) in [(64, 256, 64), (64, 256, 128), (128, 512, 128)]
               for (B, H, W, grid) in [(1, 8, 8, 0), (3, 8, 8, 2)]]


@functools.lru_cache(maxsize=None)
def chain_case(k1, n1, n2, B, H, W, device=None):
    C = _C()
    # seed n2 + k1; (128, 512, 128) had one dead ReLU channel of z at B = 3 (a zero-norm column)
    g = torch.Generator().manual_seed(1256 if (k1, n1, n2) == (128, 512, 128) else n2 + k1)
    spec3 = C.make_conv_spec(torch.randn(n1, k1, 1, 1, generator=g) / k1 ** 0.5, 0.1 * torch.randn(n1, generator=g),
                             act="relu", device=device)
    spec1 = C.make_conv_spec(torch.randn(n2, n1, 1, 1, generator=g) / n1 ** 0.5, 0.1 * torch.randn(n2, generator=g),
                             act="relu", device=device)
    x = torch.randn(B, H, W, k1, generator=g).to(BF16)
    r = torch.randn(B, H, W, n1, generator=g).to(BF16)
    return Case(f"chain-{k1}-{n1}-{n2}-{B}", {"x": x, "r": r}, {"c3": spec3, "c1": spec1}, _chain_fn, "c1")


def bneck_block(g, cin, dual, device=None):
    """c1, c2, c3, down of a stage-1 bottleneck with folded random BN (tests/test_gpu_bneck.py)."""
    from aiko_services_amd.models.resnet50 import _rand_bn, _rand_conv
    C = _C()
    c1 = C.make_conv_spec(*C.fold_bn(_rand_conv(g, 64, cin, 1), *_rand_bn(g, 64)), act="relu", device=device)
    c2 = C.make_conv_spec(*C.fold_bn(_rand_conv(g, 64, 64, 3), *_rand_bn(g, 64)), pad=1, act="relu", device=device)
    c3 = C.make_conv_spec(*C.fold_bn(_rand_conv(g, 256, 64, 1), *_rand_bn(g, 256, (0.1, 0.3))), act="relu",
                          device=device)
    down = None
    if dual:
        down = C.make_conv_spec(*C.fold_bn(_rand_conv(g, 256, cin, 1), *_rand_bn(g, 256)), device=device)
    return c1, c2, c3, down


def _chain_dual_fn(dtype, ops, specs):
    """conv_chain2.hip: Y = relu([t2 | x] . [W3 | Wd]^T + b3 + bd), rounded to bf16 in LDS, is the
    stored output and the A operand of the next block's reduction."""
    R = _R()
    idn = R.conv_ref(nchw(ops["x"]).to(dtype), specs["down"])
    y = rb(R.conv_ref(nchw(ops["t2"]).to(dtype), specs["c3"], idn))
    return nhwc(y), nhwc(R.conv_ref(y, specs["nxt"]))


@functools.lru_cache(maxsize=None)
def chain_dual_case(device=None):
    C = _C()
    g = torch.Generator().manual_seed(3)
    _, _, c3, down = bneck_block(g, 64, True, device)
    nxt = C.make_conv_spec(torch.randn(64, 256, 1, 1, generator=g) / 16, 0.1 * torch.randn(64, generator=g),
                           act="relu", device=device)
    B, H, W = 1, 8, 8
    t2 = torch.randn(B, H, W, 64, generator=g).to(BF16)
    x = torch.randn(B, H, W, 64, generator=g).to(BF16)
    return Case("chain_dual", {"t2": t2, "x": x}, {"c3": c3, "down": down, "nxt": nxt}, _chain_dual_fn, "nxt")


def _bneck_fn(dtype, ops, specs):
    """bneck_fused.hip: t1 = relu(conv1(x)) and t2 = relu(conv2(t1)) are rounded to bf16 (LDS);
    the identity (x itself) or projection shortcut is added in fp32, unrounded."""
    R = _R()
    x = ops["x"].to(dtype)
    t = rb(R.conv_ref(x, specs["c1"]))
    t = rb(R.conv_ref(t, specs["c2"]))
    idn = R.conv_ref(x, specs["down"]) if specs.get("down") is not None else x
    return (nhwc(R.conv_ref(t, specs["c3"], residual_nchw=idn)),)


BNECK_GUARD_CASES = [(B, H, dual, grid) for dual in (False, True)
                     for (B, H, grid) in [(1, 1, 1), (2, 3, 2), (3, 2, 0), (3, 3, 2)]]
BNECK_PARITY_CASES = [                            # tests/test_gpu_bneck.py
    (3, 56, False, 0), (2, 56, True, 0),          # default grid: more CUs than rows, one row each
    (3, 56, False, 7), (2, 56, True, 3),          # ranges of 24 / 37-38 rows crossing image boundaries
    (9, 56, False, 5), (5, 56, True, 2),          # ranges spanning three or more images
    (2, 20, False, 1), (2, 20, True, 1),          # one workgroup streaming two images
    (1, 56, False, 1), (2, 13, False, 4),         # one image / uneven split (26 = 7 + 7 + 6 + 6)
    (4, 1, False, 1), (3, 2, True, 2),            # images of one / two rows: a boundary every row or two
    (40, 56, False, 0), (24, 56, True, 0),        # every CU streaming several rows: counted DMA waits
]


@functools.lru_cache(maxsize=2)       # the large cases' references are hundreds of MB
def bneck_case(B, H, dual, grid, device=None):
    """A stage-1 bottleneck on [B, H, 56]; the seed depends on the grid as it always has."""
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + int(dual) + 7 * grid)
    cin = 64 if dual else 256
    c1, c2, c3, down = bneck_block(g, cin, dual, device)
    x = torch.relu(torch.randn(B, cin, H, 56, generator=g)).to(BF16)
    specs = {"c1": c1, "c2": c2, "c3": c3}
    if dual:
        specs["down"] = down
    return Case(f"bneck-{B}-{H}-{int(dual)}-{grid}", {"x": x}, specs, _bneck_fn, "c3")


def _exp_fn(dtype, ops, specs):
    """conv_exp.hip: t2 = relu(conv2(t1)) is rounded to bf16 (LDS); the residual is added in fp32."""
    R = _R()
    t = rb(R.conv_ref(ops["t1"].to(dtype), specs["c2"]))
    return (nhwc(R.conv_ref(t, specs["c3"], residual_nchw=ops["x"].to(dtype))),)


def exp_specs(g, n, device=None):
    from aiko_services_amd.models.resnet50 import _rand_bn, _rand_conv
    C = _C()
    c2 = C.make_conv_spec(*C.fold_bn(_rand_conv(g, 256, 256, 3), *_rand_bn(g, 256)), pad=1, act="relu", device=device)
    c3 = C.make_conv_spec(*C.fold_bn(_rand_conv(g, n, 256, 1), *_rand_bn(g, n, (0.1, 0.3))), act="relu",
                          device=device)
    return c2, c3


EXP_GUARD_CASES = [(1, 14, 14, 1024, 0), (3, 14, 14, 1024, 2), (5, 7, 9, 512, 1)]
EXP_PARITY_CASES = [            # tests/test_gpu_conv_exp.py
    (1, 14, 14, 1024, 0),       # M = 196: a single partial tile
    (2, 14, 14, 1024, 0),       # M = 392: a tile boundary inside image 1, then a partial tile
    (3, 14, 14, 1024, 0),       # M = 588: three tiles, a 76-row tail
    (64, 14, 14, 1024, 0),      # M = 12,544 = 49 full tiles, no tail
    (336, 14, 14, 1024, 0),     # 257.25 tiles: more tiles than CUs (a second round), plus a tail
    (5, 7, 9, 512, 0),          # no 14 x 14 geometry, no 1024
    (3, 14, 14, 1024, 2),       # two workgroups walking tiles 0, 2 / 1: a late tile and the tail
    (5, 7, 9, 512, 1),          # one workgroup walking both tiles
]


@functools.lru_cache(maxsize=2)       # the large cases' references are hundreds of MB
def exp_case(B, H, W, N, grid, device=None):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W + N + 7 * grid)
    c2, c3 = exp_specs(g, N, device)
    t1 = torch.relu(torch.randn(B, 256, H, W, generator=g)).to(BF16)
    x = torch.relu(torch.randn(B, N, H, W, generator=g)).to(BF16)
    return Case(f"exp-{B}-{H}-{W}-{N}-{grid}", {"t1": t1, "x": x}, {"c2": c2, "c3": c3}, _exp_fn, "c3")


# ---- linear --------------------------------------------------------------------------------------

def _linear_fn(dtype, ops, specs):
    return (_R().linear_ref(ops["x"].to(dtype), specs["fc"]),)


LINEAR_CASES = [(37, 1000, 2048), (1, 64, 1024)]


@functools.lru_cache(maxsize=None)
def linear_case(B, N, K, device=None):
    """Rows are batch entries, columns output features."""
    C = _C()
    g = torch.Generator().manual_seed(B + N)
    spec = C.make_linear_spec(torch.randn(N, K, generator=g) * 0.02, torch.randn(N, generator=g), device=device)
    x = torch.randn(B, K, generator=g).to(BF16)
    return Case(f"linear-{B}-{N}-{K}", {"x": x}, {"fc": spec}, _linear_fn, "fc")


# ---- stems ---------------------------------------------------------------------------------------

STEM_HW = (96, 132)


def _stem_fn(pool):
    def fn(dtype, ops, specs):
        y = _R().conv_ref(ops["pre"].to(dtype), specs["stem"])
        return (nhwc(F.max_pool2d(y, 3, 2, 1) if pool else y),)
    return fn


@functools.lru_cache(maxsize=None)
def stem_operands(device=None):
    """``(hw, frames, spec)`` of the stem tests: two 96 x 132 uint8 frames, a 7x7 / 2 stem; seed 11."""
    C = _C()
    g = torch.Generator().manual_seed(11)
    frames = torch.randint(0, 256, (2, STEM_HW[0], STEM_HW[1], 3), generator=g, dtype=torch.uint8)
    w = torch.randn(64, 3, 7, 7, generator=g) / (3 * 49) ** 0.5
    b = torch.randn(64, generator=g) * 0.1
    return STEM_HW, frames, C.make_stem_spec(w, b, act="relu", device=device)


def stem_case(pool, pre_nchw=None, device=None):
    """The stem (and 3x3 / 2 max-pool) on the bf16 stem buffer's image ``pre_nchw`` [B, 3, H, W]:
    the conv's operands are then exact.  Without one (the CPU file), the fp32 normalisation of
    :func:`reference.preprocess_ref` rounded to bf16 stands in for the device kernel's buffer."""
    hw, frames, spec = stem_operands(device)
    if pre_nchw is None:
        pre_nchw = _R().preprocess_ref(frames, hw).to(BF16)
    return Case(f"stem-pool{int(pool)}", {"pre": pre_nchw.cpu()}, {"stem": spec}, _stem_fn(pool), "stem")


def u8_tables(mean, std, dtype):
    """What stem_pool.hip's uint8 variant feeds its MFMAs, evaluated in ``dtype``: the patch entry
    ``c - 255 mean_ch`` for every (value c, channel) pair as the kernel writes it (fp32
    ``(float)c - m`` with ``m`` the fp32 of ``255 * mean``, then bf16) and the per-channel weight
    scale ``1 / (255 std_ch)`` (``ops.conv.stem_pool_u8_weight``)."""
    c = torch.arange(256, dtype=dtype).view(256, 1)
    m = torch.tensor([255.0 * float(v) for v in mean], dtype=torch.float64).to(dtype)
    scale = torch.tensor([1.0 / (255.0 * float(v)) for v in std], dtype=torch.float64).to(dtype)
    return c - m, scale


def _stem_u8_fn(dtype, ops, specs):
    y = F.conv2d(ops["patch"].to(dtype), ops["w"].to(dtype), specs["stem"].ref_bias.to(dtype), stride=2, padding=3)
    return (nhwc(F.max_pool2d(torch.relu(y), 3, 2, 1)),)


def stem_u8_case(mean, std, device=None):
    """The uint8 stem: its operands are NOT the bf16 of the normalised image and the stem's bf16
    weight — the kernel rounds ``c - 255 mean`` to bf16 and multiplies by weights
    ``bf16(w_bf16 / (255 std))`` — so the reference takes both from the kernel's formulas
    (:func:`u8_tables`); with them its operands are exact."""
    hw, frames, spec = stem_operands(device)
    table, scale = u8_tables(mean, std, torch.float32)
    table = table.to(BF16)                                            # [256, 3]
    idx = frames.long()
    patch = torch.stack([table[idx[..., ch], ch] for ch in range(3)], 1)  # [B, 3, H, W] bf16
    w = (spec.ref_weight * scale.view(1, 3, 1, 1)).to(BF16)
    return Case("stem-u8", {"patch": patch, "w": w}, {"stem": spec}, _stem_u8_fn, "stem")


# ---- YOLO fused kernels --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def yolo_specs(device="cpu"):
    """YOLOv8-n's ConvSpecs (seed 0): the same weights on every device."""
    from aiko_services_amd.models.yolov8 import YOLOv8
    return YOLOv8("n", device=device)


def c2f_ref(x_nchw, blk):
    """One C2f block (one bottleneck) from its specs, rounded where c2f_fused.hip stores bf16:
    [a | s] = silu(cv1(x)) (LDS rings), t = silu(conv_a(s)) (LDS ring), c = silu(conv_b(t)) (+ s:
    added in fp32, ONE rounding of the sum) and the output y = silu(cv2([a | s | c]))."""
    R = _R()
    a, b = blk.m[0]
    y = rb(R.conv_ref(x_nchw, blk.cv1))
    s = y[:, blk.c:]
    t = rb(R.conv_ref(s, a))
    c = rb(R.conv_ref(t, b, residual_nchw=s if blk.shortcut else None, residual_after_act=True))
    return R.conv_ref(torch.cat([y, c], 1), blk.cv2)


def _c2f_fn(dtype, ops, specs):
    blk = dataclasses.replace(specs["blk"], cv2=specs["cv2"])
    return (nhwc(c2f_ref(nchw(ops["x"]).to(dtype), blk)),)


C2F_CASES = [("l2", 160, 160, 32, 32, 10), ("l2", 160, 160, 32, 32, 20), ("l2", 160, 160, 32, 32, 160),
             ("l15", 80, 80, 192, 64, 10), ("l15", 80, 80, 192, 64, 20), ("l15", 80, 80, 192, 64, 80)]


def c2f_case(layer, H, W, cin, rb_rows, model=None):
    """test_c2f_fused_guarded: the input's seed is the band height."""
    m = model or yolo_specs()
    blk = getattr(m, layer)
    g = torch.Generator().manual_seed(rb_rows)
    x = (torch.randn(1, H, W, cin, generator=g) * 2).to(BF16)
    return Case(f"c2f-{layer}-rb{rb_rows}", {"x": x}, {"blk": blk, "cv2": blk.cv2}, _c2f_fn, "cv2")


def case_bound(name):
    """The per-pixel / per-channel bound of a case by its name."""
    return C2F_L2_BOUND if name.startswith("c2f-l2") else ROW_BOUND


def _c2f_bneck_fn(dtype, ops, specs):
    """c2f_bneck_kernel: t = silu(conv_a(x)) is rounded to bf16 (LDS); silu(conv_b(t)) + x is
    rounded once, as the output."""
    R = _R()
    x = nchw(ops["x"]).to(dtype)
    t = rb(R.conv_ref(x, specs["a"]))
    return (nhwc(R.conv_ref(t, specs["b"], residual_nchw=x, residual_after_act=True)),)


def c2f_bneck_case(model=None):
    """test_c2f_bneck_guarded: l4's first bottleneck on 80 x 80 x 32; seed 10."""
    m = model or yolo_specs()
    blk = m.l4
    g = torch.Generator().manual_seed(10)
    x = (torch.randn(1, 80, 80, blk.c, generator=g) * 2).to(BF16)
    a, b = blk.m[0]
    return Case("c2f_bneck", {"x": x}, {"a": a, "b": b}, _c2f_bneck_fn, "b")


def _tail_fn(dtype, ops, specs):
    """conv_glds TAIL: the activated 3x3 tile is rounded to bf16 in LDS, the 1x1 reads it there."""
    R = _R()
    t = rb(R.conv_ref(nchw(ops["x"]).to(dtype), specs["s1"]))
    return (nhwc(R.conv_ref(t, specs["s2"])),)


TAIL_CASES = [("box", 20), ("cls", 20), ("box", 40), ("cls", 40), ("box", 80), ("cls", 80), ("l3", None)]


def tail_geometry(branch, hw, m):
    lvl = m.heads[0]
    return {"box": (lvl.box[1], lvl.box[2], 64, 0, 144, 64, 0, 144, hw, hw),
            "cls": (lvl.cls[1], lvl.cls[2], 80, 64, 144, 80, 64, 144, hw, hw),
            "l3": (m.l3, m.l4.cv1, 32, 16, 48, 64, 0, 128, 21, 19)}[branch]


def tail_case(branch, hw, model=None):
    """test_conv_tail_guarded: seed 20."""
    m = model or yolo_specs()
    s1, s2, cin, _, _, _, _, _, H, W = tail_geometry(branch, hw, m)
    g = torch.Generator().manual_seed(20)
    x = (torch.randn(1, H, W, cin, generator=g) * 2).to(BF16)
    return Case(f"tail-{branch}-{hw}", {"x": x}, {"s1": s1, "s2": s2}, _tail_fn, "s2")


def all_cases():
    """``(id, builder)`` of every case the CPU file checks; the builders are called one at a time."""
    P = functools.partial
    out = [("conv-" + "x".join(str(v) for v in s[:8]), P(conv_case, s)) for s in CONV_SHAPES]
    out += [(f"slices-{c[0]}-{c[1]}-k{c[2]}", P(slice_case, *c)) for c in SLICE_SHAPES]
    out += [(f"pw_dual-{c[0]}-{c[2]}", P(pw_dual_case, *c)) for c in PW_DUAL_CASES]
    out += [("projection", projection_case)]
    out += [(f"patch-{c[0]}-{c[1]}", P(patch_case, *c)) for c in PATCH_CASES]
    out += [(f"patchw-{c[0]}-{c[1]}", P(patchw_case, *c[:3])) for c in PATCHW_CASES]
    out += [(f"rows-{c[0]}-{c[1]}", P(rows_case, *c[:4])) for c in ROWS_CASES]
    out += [(f"chain-{c[0]}-{c[1]}-{c[2]}-{c[3]}", P(chain_case, *c[:6])) for c in CHAIN_CASES]
    out += [("chain_dual", chain_dual_case)]
    bn = list(dict.fromkeys(BNECK_GUARD_CASES + BNECK_PARITY_CASES))
    out += [(f"bneck-{c[0]}-{c[1]}-{int(c[2])}-{c[3]}", P(bneck_case, *c)) for c in bn]
    ex = list(dict.fromkeys(EXP_GUARD_CASES + EXP_PARITY_CASES))
    out += [("exp-" + "-".join(str(v) for v in c), P(exp_case, *c)) for c in ex]
    out += [(f"linear-{c[0]}-{c[1]}", P(linear_case, *c)) for c in LINEAR_CASES]
    out += [("stem", P(stem_case, False)), ("stem-pool", P(stem_case, True))]
    from aiko_services_amd.ops.vision import IMAGENET_MEAN, IMAGENET_STD
    out += [("stem-u8", P(stem_u8_case, IMAGENET_MEAN, IMAGENET_STD))]
    out += [(f"c2f-{c[0]}-rb{c[5]}", P(c2f_case, c[0], c[1], c[2], c[3], c[5])) for c in C2F_CASES]
    out += [("c2f_bneck", c2f_bneck_case)]
    out += [(f"tail-{c[0]}-{c[1]}", P(tail_case, *c)) for c in TAIL_CASES]
    return out


# ---- positional controls -------------------------------------------------------------------------
#
# One perturbed operand that the reference does not see, placed where the case has its edge.  The
# CPU file checks that the fp32 evaluation with the same perturbation is flagged at exactly the
# predicted pixels / channel; the GPU file gives the perturbed operand to the kernel.

def negated(t, layout, b, h, w):
    """``t`` with input pixel ``(b, h, w)`` negated (every channel); layout "nchw" or "nhwc"."""
    t = t.clone()
    if layout == "nchw":
        t[b, :, h, w] = -t[b, :, h, w]
    else:
        t[b, h, w] = -t[b, h, w]
    return t


# name -> (builder(device) — for "c2f" builder(model) —, operand keys with their layouts, input pixel,
#          [(k, stride, pad), ...] of the 3x3 convs between that operand and the output,
#          input (H, W), spec whose bias the bias control scales)
CONTROLS = {
    # the tail tile (rows 768 .. 839 = images 21 .. 23) of the B = 24 variant-20 walk
    "v20-walk": (functools.partial(conv_case, G13x24), (("x", "nchw"), ("x_nhwc", "nhwc")), (23, 7, 5),
                 [(3, 2, 1)], (13, 9), "conv"),
    # the last pixel of conv_pw's multi-tile case: the last tile of the last workgroup's walk
    "pw-multi": (functools.partial(conv_case, PW_MULTI), (("x", "nchw"), ("x_nhwc", "nhwc")), (10, 13, 13),
                 [(1, 1, 0)], (14, 14), "conv"),
    # the last image row of bneck_fused's (3, 3, 2) split: the end of the second workgroup's range
    "bneck": (functools.partial(bneck_case, 3, 3, False, 2), (("x", "nchw"),), (2, 2, 30), [(3, 1, 1)], (3, 56),
              "c3"),
    # the partial tile (rows 256 .. 314) of conv3x3_exp (5, 7, 9, 512)
    "exp": (functools.partial(exp_case, 5, 7, 9, 512, 1), (("t1", "nchw"),), (4, 5, 4), [(3, 1, 1)], (7, 9), "c3"),
    # the last row of c2f_fused l15's first band (rb = 10): its 5 x 5 field spans bands 0 and 1
    "c2f": (lambda model=None: c2f_case("l15", 80, 80, 192, 10, model), (("x", "nhwc"),), (0, 9, 40),
            [(3, 1, 1), (3, 1, 1)], (80, 80), "cv2"),
}


def control(name, model=None, device=None):
    """``(case, perturbed ops, predicted output pixels, bias spec name, its channel)``."""
    build, keys, (b, h, w), convs, (H, W), bias_spec = CONTROLS[name]
    case = build(model) if name == "c2f" else build(device)
    ops = dict(case.ops)
    for key, layout in keys:
        ops[key] = negated(case.ops[key], layout, b, h, w)
    pixels, _ = receptive(b, h, w, convs, H, W)
    return case, ops, pixels, bias_spec, top_bias_channel(case.specs[bias_spec])
