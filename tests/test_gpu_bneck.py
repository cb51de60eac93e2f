"""Fused stage-1 ResNet bottleneck (bneck_fused.hip) vs a plain PyTorch fp32 reference of the
same block, vs the unfused kernel path (conv3x3_patch / conv_chain / igemm), and — per pixel and
per channel, bound 2^-8 — vs an fp64 reference that rounds t1 and t2 to bf16 where the kernel
keeps them as bf16 in LDS (the identity or projection shortcut is added unrounded)."""
import pytest
import torch

import conv_parity_cases as P
from guard_ops import ROW_BOUND, assert_pixel_channel

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _reference(x_nchw, c1, c2, c3, down):
    from aiko_services_amd.ops import reference as R
    t = R.conv_ref(x_nchw, c1)
    t = R.conv_ref(t.to(torch.bfloat16).float(), c2)          # the kernels round t1 / t2 to bf16
    idn = R.conv_ref(x_nchw, down) if down is not None else x_nchw
    return R.conv_ref(t.to(torch.bfloat16).float(), c3, residual_nchw=idn)


@pytest.mark.parametrize("B,H,dual,grid", P.BNECK_PARITY_CASES)
def test_bneck_fused_matches_torch(native, B, H, dual, grid):
    from aiko_services_amd.ops import conv as C
    pc = P.bneck_case(B, H, dual, grid, DEV)
    c1, c2, c3, down, x = pc.specs["c1"], pc.specs["c2"], pc.specs["c3"], pc.specs.get("down"), pc.ops["x"]
    conv3 = C.fuse_shortcut(c3, down) if dual else c3
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    out = torch.full((B, H, 56, 256), float("nan"), dtype=torch.bfloat16, device=DEV)
    y = C.bneck_fused(xd, c1, c2, conv3, out=out, grid=grid)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all(), "unwritten / non-finite output pixels"
    ref = _reference(x.float().to(DEV), c1, c2, c3, down)
    err = _rel(y.permute(0, 3, 1, 2), ref)
    assert err < 1e-2, err
    # the unfused kernel path of the same block
    t1 = C.conv2d(xd, c1)
    t2 = C.conv2d(t1, c2)
    y2 = C.conv2d(t2, conv3, x2=xd) if dual else C.conv2d(t2, c3, residual=xd)
    assert _rel(y, y2) < 5e-3
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"bneck_fused B{B} H{H} dual{int(dual)} grid{grid}")


def test_resnet50_stage1_fused_matches_unfused(native, monkeypatch):
    """The model's stage 1 on bneck_fused (default) against the round-3 kernel chain."""
    from aiko_services_amd.models.resnet50 import ResNet50
    m = ResNet50(device=DEV)
    frames = torch.randint(0, 256, (8, 224, 224, 3), dtype=torch.uint8, device=DEV)
    assert m.bneck
    a = m.logits(frames).float()
    m.bneck = False
    b = m.logits(frames).float()
    ref = m.reference_logits(frames)
    torch.cuda.synchronize()
    cos = torch.nn.functional.cosine_similarity
    assert cos(a.flatten(), b.flatten(), dim=0).item() > 0.999
    assert cos(a, ref, dim=1).min().item() > 0.995
