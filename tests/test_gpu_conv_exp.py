"""Fused 3x3 conv + 1x1 expansion + identity residual (conv_exp.hip) vs a plain PyTorch fp32
reference of the same two layers, and vs the unfused kernel path (conv2d -> conv2d(residual=x)).
Both bounds hold for every 256-row M tile on its own — the tile is the kernel's unit of work, so
a broken tail tile or a broken late tile of a workgroup's walk cannot hide in the global norm.
Per pixel and per channel the output is held to 2^-8 of an fp64 reference that rounds t2 to bf16
where the kernel keeps it as bf16 in LDS (the residual is added unrounded)."""
import pytest
import torch

import conv_parity_cases as P
from guard_ops import ROW_BOUND, assert_pixel_channel

pytestmark = pytest.mark.gpu

DEV = "cuda"
TILE = 256


def _specs(g, n):
    return P.exp_specs(g, n, DEV)


def _reference(t1_nchw, x_nchw, c2, c3):
    from aiko_services_amd.ops import reference as R
    t = R.conv_ref(t1_nchw, c2)
    return R.conv_ref(t.to(torch.bfloat16).float(), c3, residual_nchw=x_nchw)   # the kernels round t2 to bf16


def _tile_rel(a, b):
    """Relative L2 error of ``a`` against ``b`` ([M, N]) per 256-row tile, the partial last one included."""
    a, b = a.float(), b.float()
    M = a.shape[0]
    nt = (M + TILE - 1) // TILE
    idx = torch.arange(M, device=a.device) // TILE
    num = torch.zeros(nt, device=a.device).index_add_(0, idx, (a - b).pow(2).sum(1))
    den = torch.zeros(nt, device=a.device).index_add_(0, idx, b.pow(2).sum(1))
    return num.sqrt() / (den.sqrt() + 1e-12)


@pytest.mark.parametrize("B,H,W,N,grid", P.EXP_PARITY_CASES)
def test_conv3x3_exp_matches_torch(native, B, H, W, N, grid):
    from aiko_services_amd.ops import conv as C
    pc = P.exp_case(B, H, W, N, grid, DEV)
    c2, c3, t1, x = pc.specs["c2"], pc.specs["c3"], pc.ops["t1"], pc.ops["x"]
    t1d = t1.permute(0, 2, 3, 1).contiguous().to(DEV)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    assert C.conv_exp_ok(c2, c3, t1d, xd)
    out = torch.full((B, H, W, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    y = C.conv3x3_exp(t1d, c2, c3, xd, out=out, grid=grid)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all(), "unwritten / non-finite output pixels"
    ref = _reference(t1.float().to(DEV), x.float().to(DEV), c2, c3).permute(0, 2, 3, 1).reshape(-1, N)
    y2 = C.conv2d(C.conv2d(t1d, c2), c3, residual=xd)          # the unfused kernel path
    torch.cuda.synchronize()
    M = B * H * W
    e_ref = _tile_rel(y.reshape(M, N), ref)
    e_unf = _tile_rel(y.reshape(M, N), y2.reshape(M, N))
    e_base = _tile_rel(y2.reshape(M, N), ref)
    print(f"tiles {e_ref.numel()}: fused/ref max {e_ref.max().item():.3e}, fused/unfused max "
          f"{e_unf.max().item():.3e}, unfused/ref max {e_base.max().item():.3e}")
    assert e_ref.numel() == (M + TILE - 1) // TILE
    # the per-tile bound is meaningful only if the unfused path meets it on these inputs
    assert e_base.max().item() < 1e-2, e_base.max().item()
    assert e_ref.max().item() < 1e-2, (e_ref.argmax().item(), e_ref.max().item())
    assert e_unf.max().item() < 5e-3, (e_unf.argmax().item(), e_unf.max().item())
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"conv3x3_exp B{B} {H}x{W} N{N} grid{grid}")


def test_conv3x3_exp_refuses_ineligible(native):
    from aiko_services_amd.models.resnet50 import _rand_bn, _rand_conv
    from aiko_services_amd.ops import conv as C
    g = torch.Generator().manual_seed(5)
    c2 = C.make_conv_spec(*C.fold_bn(_rand_conv(g, 128, 128, 3), *_rand_bn(g, 128)), pad=1, act="relu", device=DEV)
    c3 = C.make_conv_spec(*C.fold_bn(_rand_conv(g, 512, 128, 1), *_rand_bn(g, 512)), act="relu", device=DEV)
    t1 = torch.zeros(1, 14, 14, 128, dtype=torch.bfloat16, device=DEV)
    x = torch.zeros(1, 14, 14, 512, dtype=torch.bfloat16, device=DEV)
    assert not C.conv_exp_ok(c2, c3, t1, x)
    with pytest.raises(ValueError):
        C.conv3x3_exp(t1, c2, c3, x)
    # stride 2 on the right widths
    c2s, c3s = _specs(g, 1024)
    c2s.stride = 2
    t1 = torch.zeros(1, 14, 14, 256, dtype=torch.bfloat16, device=DEV)
    x = torch.zeros(1, 14, 14, 1024, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        C.conv3x3_exp(t1, c2s, c3s, x)


def test_resnet50_stage3_fused_matches_unfused(native, monkeypatch):
    """The model's stage-3 identity blocks on conv3x3_exp against the three-launch path."""
    from aiko_services_amd.models.resnet50 import ResNet50
    from aiko_services_amd.ops import conv as C
    calls = []
    fused = C.conv3x3_exp
    monkeypatch.setattr(C, "conv3x3_exp", lambda *a, **k: (calls.append(1), fused(*a, **k))[1])
    m = ResNet50(device=DEV)
    frames = torch.randint(0, 256, (8, 224, 224, 3), dtype=torch.uint8, device=DEV)
    m.exp3 = True
    a = m.logits(frames).float()
    assert len(calls) == 5, "the five stage-3 identity blocks"
    m.exp3 = False
    b = m.logits(frames).float()
    assert len(calls) == 5
    ref = m.reference_logits(frames)
    torch.cuda.synchronize()
    cos = torch.nn.functional.cosine_similarity
    assert cos(a.flatten(), b.flatten(), dim=0).item() > 0.999
    assert cos(a, ref, dim=1).min().item() > 0.995
