"""Reference-only checks of the conv / fused-block parity cases (tests/conv_parity_cases.py), on
the CPU: before the per-pixel / per-channel bound is put on a kernel, it is shown here that

(a) the reference alone meets it — an fp32 evaluation, rounded to bf16 at the same points, stays
    within the case's bound of the fp64 reference per pixel and per channel;
(b) no pixel row and no channel column of the fp64 reference has norm 0, so the exact-compare
    branch of ``row_errs`` never decides a case;
(c) the metric sees what the whole-tensor bound 1e-2 does not: a pixel that takes its left
    neighbour's value, a dropped bias and a missing border tap column are flagged at exactly
    the pixels / the channel they touch, and for four of them the whole-tensor error stays
    below 1e-2;
(d) the positional controls of the GPU file (a bias scaled by 1.5, one negated input pixel) are
    flagged at exactly the predicted channel / output pixels when the fp32 evaluation gets the
    perturbed operand.

Each case's fp64 reference is built once and shared by the four checks.
"""
import dataclasses

import pytest
import torch

import conv_parity_cases as P
from guard_ops import ROW_BOUND, pixel_channel_errs, rel_err

CASES = P.all_cases()


def _over(errs, bound):
    return torch.nonzero(~(errs < bound)).flatten().tolist()


@pytest.mark.parametrize("build", [b for _, b in CASES], ids=[n for n, _ in CASES])
def test_reference_case(build):
    case = build()
    bound = P.case_bound(case.name)
    ref = case.ref64
    y32 = case.eval32()
    # (b) before (a): a zero-norm row would show as inf in (a)
    for i, r in enumerate(ref):
        flat = r.reshape(-1, r.shape[-1])
        assert (flat.norm(dim=1) == 0).sum().item() == 0, f"{case.name} output {i}: zero-norm pixel rows"
        assert (flat.norm(dim=0) == 0).sum().item() == 0, f"{case.name} output {i}: zero-norm channel columns"
    # (a)
    for i, (y, r) in enumerate(zip(y32, ref)):
        pix, ch = pixel_channel_errs(y, r)
        print(f"{case.name} output {i}: fp32 vs fp64 pixel {pix.max().item():.3e} channel {ch.max().item():.3e} "
              f"whole {rel_err(y, r):.3e} bound {bound:.3e}")
        assert pix.max().item() < bound and ch.max().item() < bound, (pix.max().item(), ch.max().item())
        if case.name.startswith("c2f-l2"):
            assert pix.max().item() <= P.C2F_L2_CPU_WORST * 1.0005 and ch.max().item() < ROW_BOUND
    # (c) on the last output
    y, r = y32[-1], ref[-1]
    N = y.shape[-1]
    M = y.numel() // N
    if M > 1:                                               # the last pixel takes its left neighbour's value
        bad = y.clone().reshape(M, N)
        bad[M - 1] = bad[M - 2]
        pix, _ = pixel_channel_errs(bad.reshape(y.shape), r)
        assert _over(pix, bound) == [M - 1]
        if case.name == "conv-" + "x".join(str(v) for v in P.V4_MULTI[:8]):
            assert rel_err(bad, r.reshape(M, N)) < 1e-2          # the old bound lets it through
    c = P.top_bias_channel(case.specs[case.last])           # the bias of the largest |bias| dropped
    bad = case.eval32(specs=case.with_bias(case.last, c, 0.0))[-1]
    _, ch = pixel_channel_errs(bad, r)
    assert _over(ch, bound) == [c]
    if case.name in ("conv-" + "x".join(str(v) for v in P.PW_MULTI[:8]), "conv-1x13x9x192x72x3x2x1",
                     "exp-3-14-14-1024-0"):
        # the bias of the LAST channel dropped (the N tail's): flagged, and under the old bound
        bad = case.eval32(specs=case.with_bias(case.last, N - 1, 0.0))[-1]
        _, ch = pixel_channel_errs(bad, r)
        assert _over(ch, bound) == [N - 1]
        assert rel_err(bad, r) < 1e-2, rel_err(bad, r)
    if case.k3 and y.dim() == 4 and y.shape[2] > 1:         # the last image's right-hand column misses a tap column
        s = case.specs[case.k3]
        w = s.ref_weight.clone()
        w[:, :, :, 0] = 0
        part = case.eval32(specs={**case.specs, case.k3: dataclasses.replace(s, ref_weight=w)})[-1]
        bad = y.clone()
        bad[-1, :, -1] = part[-1, :, -1]
        B, Ho, Wo, _ = y.shape
        pix, _ = pixel_channel_errs(bad, r)
        assert _over(pix, bound) == [((B - 1) * Ho + h) * Wo + Wo - 1 for h in range(Ho)]


@pytest.mark.parametrize("name", list(P.CONTROLS))
def test_positional_controls_predict_their_sets(name):
    """(d): what the GPU controls will assert of the kernels holds for the fp32 evaluation."""
    case, ops, pixels, bias_spec, c = P.control(name)
    bound = P.case_bound(case.name)
    r = case.ref64[-1]
    pix, _ = pixel_channel_errs(case.eval32(ops=ops)[-1], r)
    assert _over(pix, bound) == pixels, (name, _over(pix, bound), pixels)
    assert len(pixels) == {"v20-walk": 4, "pw-multi": 1, "bneck": 6, "exp": 9, "c2f": 25}[name]
    y = case.eval32(specs=case.with_bias(bias_spec, c, 1.5))[-1]
    _, ch = pixel_channel_errs(y, r)
    assert _over(ch, bound) == [c]
    if name == "pw-multi":
        assert rel_err(y, r) < 1e-2


def test_stem_u8_tables_fp32_equals_fp64():
    """stem_pool.hip's uint8 variant writes ``(float)c - m`` (``m`` = fp32 of 255 * mean) as bf16
    into its patch and reads weights scaled by fp32 ``1 / (255 std)``: for all 256 x 3 (value,
    channel) pairs the fp32 formula rounds to the same bf16 as the fp64 one, and the scaled
    weights of the stem case round alike too — so the operands the reference takes from these
    formulas are the kernel's, exactly."""
    from aiko_services_amd.ops.vision import IMAGENET_MEAN, IMAGENET_STD, YOLO_MEAN, YOLO_STD
    for mean, std in ((IMAGENET_MEAN, IMAGENET_STD), (YOLO_MEAN, YOLO_STD)):
        t32, s32 = P.u8_tables(mean, std, torch.float32)
        t64, s64 = P.u8_tables(mean, std, torch.float64)
        assert torch.equal(t32.to(torch.bfloat16), t64.to(torch.bfloat16))
        _, _, spec = P.stem_operands()
        w32 = (spec.ref_weight * s32.view(1, 3, 1, 1)).to(torch.bfloat16)
        w64 = (spec.ref_weight.double() * s64.view(1, 3, 1, 1)).to(torch.bfloat16)
        differ = (w32 != w64).sum().item()
        print(f"scaled stem weights: {differ} of {w32.numel()} differ between the fp32 and the fp64 formula")
        assert differ == 0


@pytest.mark.parametrize("k,stride,pad,H,W", [(1, 1, 0, 5, 7), (1, 2, 0, 18, 18), (3, 1, 1, 9, 11), (3, 2, 1, 13, 9),
                                              (7, 2, 3, 20, 23)])
def test_tap_matmul_conv_equals_conv2d(k, stride, pad, H, W):
    """reference._conv_taps (conv_ref's fp64 path on a device: one matmul per filter tap, no fp64
    convolution needed there) is the same convolution as F.conv2d — checked here in fp64."""
    import torch.nn.functional as F

    from aiko_services_amd.ops import reference as R
    g = torch.Generator().manual_seed(k * 100 + stride)
    x = torch.randn(2, 6, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(10, 6, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(10, generator=g, dtype=torch.float64)
    want = F.conv2d(x, w, b, stride=stride, padding=pad)
    got = R._conv_taps(x, w, b, stride, pad)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < 1e-12 * want.abs().max().item()
    assert torch.equal(R._conv_taps(x, w, None, stride, pad) + b.view(1, -1, 1, 1), got)
