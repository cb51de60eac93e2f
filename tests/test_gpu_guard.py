"""Guard-band and poison runs of the conv and vision kernels (run on MI355X: -m gpu).

Every case builds its inputs once on the CPU from a seeded generator and runs the kernel twice:
*plain*, on fresh tensors as the other test files do, and *guarded*, with every tensor the
binding receives (inputs, second source, residual, outputs, weights, biases, scratch, zero page)
a view from ``kernel_guard.guarded`` holding the same values between two NaN guards.  Then, in
this order:

1. every guard is bit-identical to its saved copy — nothing outside any tensor was written;
2. the guarded output is finite everywhere — no poison was consumed, every element was written;
3. the guarded output is bit-identical to the plain output — the kernels use no atomics and the
   tile is forced, so where the operands live must not change one bit;
4. the plain output meets the bound of the kernel's existing test, unchanged, and — for the conv,
   fused-block, stem, C2f and linear kernels — the per-pixel and per-channel bound:
   ``assert_pixel_channel(y, ref64, ROW_BOUND)``, the error norm of every pixel row and of every
   channel column of the ``[M, N]`` output below 2^-8 of that row's / column's norm in an fp64
   reference.  One RNE rounding of an fp32 value to bf16 moves an element by at most 2^-8 of
   itself, hence a row or column by at most 2^-8 of its norm; fp32 accumulation over K <= 4608,
   the erf polynomial and the rcp / exp SiLU are orders below.  The reference
   (tests/conv_parity_cases.py, shared with the CPU checks of tests/test_conv_parity_reference.py)
   starts from the same bf16 operands and, for a fused kernel, rounds to bf16 at exactly the
   points where the kernel stores bf16 — each test's docstring names them.  The whole-tensor
   bound cannot see a wrong value computed from in-bounds data (a tap dropped at a border, a
   lost bias in the N tail: about 1 % of the output's energy fits under 1e-2); this one does,
   and the positional controls at the end of the conv section show it on the device.

Each kernel family has a case whose last tile is partial; the case computes the split its
launcher makes — ``M % BM`` for the tiled convs, the row split of the row-stream kernels, the
element count over the 256-thread block (or the rows over the waves of a block) of the pointwise
ops — and asserts it is non-zero, so a case that stops exercising a tail fails loudly.  Two
families cannot have a partial tile: conv_chain's launcher refuses M % 64 != 0 and the C2f
launchers (c2f_fused.hip) refuse H % rb != 0.  The conv_chain cases assert an uneven walk of the
persistent grid instead (3 tiles over 2 workgroups); the C2f kernels are not persistent (one
workgroup per band of rb rows), so their cases run every band height of the existing tests:
several bands with halo rows recomputed at band edges, and rb == H, the single band with zero
rows on both sides.

NaN cannot show an out-of-tensor tap of a max-reduction (``fmaxf`` drops it), so the max-pool
cases run a second time with +3e38 in the guards and gap channels: it would win every maximum.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_parity_cases as P
from guard_ops import Operands, _bits, run_both  # noqa: F401  (shared with test_gpu_guard_transformer.py)
from guard_ops import ROW_BOUND, assert_pixel_channel, pixel_channel_errs
from kernel_guard import GuardError, guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")


def _rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous()


def _nchw(x_nhwc):
    return x_nhwc.permute(0, 3, 1, 2)


# ---- the helper on the device --------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.uint8])
@pytest.mark.parametrize("side,offset", [("before", -1), ("after", 0)])
def test_guard_reports_device_write(dtype, side, offset):
    vals = torch.ones(2, 5, 7, 16)
    view, check = guarded(vals.shape, dtype, DEV, values=vals)
    assert view.is_cuda and view.is_contiguous() and view.storage_offset() > 0 and view.data_ptr() % 256 == 0
    check()
    at = check.start + offset if side == "before" else check.start + check.numel + offset
    check.flat[at:at + 1] = 3
    with pytest.raises(GuardError) as e:
        check()
    assert e.value.side == side and e.value.offset == offset


@pytest.mark.parametrize("side", ["before", "after"])
def test_guard_poison_is_live(side):
    """One row of guard inside a 3x3 conv's input makes the output non-finite: a kernel that
    reads a tap outside its tensor cannot pass assertion 2."""
    g = torch.Generator().manual_seed(1)
    H, W, C = 6, 5, 8
    x, check = guarded((1, H, W, C), torch.float32, DEV, values=torch.randn(1, H, W, C, generator=g))
    w = torch.randn(4, C, 3, 3, generator=g).to(DEV)
    assert torch.isfinite(F.conv2d(_nchw(x), w, padding=1)).all()
    s = check.start - W * C if side == "before" else check.start
    ext = check.flat[s:s + (H + 1) * W * C].view(1, H + 1, W, C)
    assert not torch.isfinite(F.conv2d(_nchw(ext), w, padding=1)).all()
    check()


# ---- conv2d: every tiled variant -----------------------------------------------------------------

CONV_CASES = P.CONV_CASES                     # tests/conv_parity_cases.py: shapes, tiles, grids
_PW_BN = {128: 256, 256: 128, 512: 64}          # variant 13 / 14 channel block per K


def _conv_id(p):
    shape, tile, grid = p
    v = tile[2] if len(tile) > 2 else 0
    return f"v{v}-{'x'.join(str(s) for s in shape[:5])}-k{shape[5]}s{shape[6]}-t{tile[0]}x{tile[1]}" + \
        (f"-g{grid}" if grid > 0 else "-multi" if grid < 0 else "")


@pytest.mark.parametrize("shape,tile,grid", CONV_CASES, ids=[_conv_id(p) for p in CONV_CASES])
def test_conv2d_guarded(native, monkeypatch, shape, tile, grid):
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    B, H, W, cin, cout, k, stride, pad, act, res = shape
    variant = tile[2] if len(tile) > 2 else 0
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if grid > 0:
        monkeypatch.setenv("AIKO_CONV_PERS_GRID", str(grid))
    pc = P.conv_case(shape, DEV)
    spec0, x, x_nhwc, r = pc.specs["conv"], pc.ops["x"], pc.ops["x_nhwc"], pc.ops["r"]
    Ho, Wo = spec0.out_hw(H, W)
    M = B * Ho * Wo
    if variant == 7:
        assert Ho % tile[0] != 0 or Wo % 32 != 0, "case has no partial tile"
    else:
        assert M % tile[0] != 0, "case has no partial last M tile"
    mtiles = -(-M // tile[0])
    if grid == -1:                                          # variant 4: 2 workgroup slots per CU
        assert variant == 4 and mtiles * -(-cout // tile[1]) > 2 * cus, "one tile per workgroup"
    elif grid == -2:                                        # conv_pw: CUs / channel blocks groups per block
        bn = 128 if variant == 12 else _PW_BN[spec0.K]
        assert cout % bn == 0 and mtiles > max(1, cus // (cout // bn)), "one tile per workgroup"
    elif B == 24:
        assert mtiles * -(-cout // tile[1]) > grid, "one tile per workgroup"

    def case(ops):
        out = ops.out((B, Ho, Wo, cout))
        C.conv2d(ops.inp(x_nhwc, "x"), ops.spec(spec0), residual=None if r is None else ops.inp(_nhwc(r), "residual"),
                 out=out, tile=tile)
        return out

    y = run_both(case)
    ref = R.conv_ref(x.float().to(DEV), spec0, None if r is None else r.float().to(DEV))
    err = _rel_err(_nchw(y), ref)
    assert err < 1e-2, err
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"conv2d {_conv_id((shape, tile, grid))}")


@pytest.mark.parametrize("cin,cout,k,tile,pitch,c0", P.SLICE_CASES)
def test_conv2d_channel_slices_guarded(native, cin, cout, k, tile, pitch, c0):
    """Input and residual from channel slices (pitch > Cc: the gap channels are poison, so a K
    block that runs past its tap's channels shows), output into a slice of a NaN concat buffer
    whose other channels must stay NaN — in rows 0 and M-1 too.  M = 198: a partial last tile."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    pc = P.slice_case(cin, cout, k, DEV)
    B, H, W = 2, 9, 11
    x, r, spec0 = pc.ops["x_nhwc"], pc.ops["r_nhwc"], pc.specs["conv"]
    assert spec0.Cc == cin and (B * H * W) % tile[0] != 0 and H % tile[0] != 0
    ro = 8 * ((cout + 7) // 8)

    def case(ops):
        cat = ops.out((B, H, W, 32 + cout + 16), name="concat buffer")
        C.conv2d(ops.inp_slice(x, pitch, c0, "x"), ops.spec(spec0), residual=ops.inp_slice(r, ro + 24, 16, "residual"),
                 out=cat[..., 32:32 + cout], tile=tile, residual_after_act=True)
        torch.cuda.synchronize()
        assert torch.isnan(cat[..., :32].float()).all() and torch.isnan(cat[..., 32 + cout:].float()).all(), \
            "wrote outside the output's channel slice"
        return cat[..., 32:32 + cout]

    y = run_both(case)
    ref = R.conv_ref(_nchw(x).float().to(DEV), spec0, _nchw(r).float().to(DEV), residual_after_act=True)
    assert _rel_err(_nchw(y), ref) < 1e-2
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"slices {cin}->{cout} k{k} v{tile[2] if len(tile) > 2 else 0}")


@pytest.mark.parametrize("B,H,cout,stride", P.PW_DUAL_CASES)
def test_conv_pw_dual_guarded(native, B, H, cout, stride):
    """Variant 13 with a second source (Ho = 9, M = 81 / 162: 64-pixel tiles end in a tail;
    B = 13, Cout = 2048: 17 tiles over 16 workgroups per channel block, one walks two)."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    pc = P.pw_dual_case(B, H, cout, stride, DEV)
    Ho = (H - 1) // stride + 1
    main, down, t, x = pc.specs["main"], pc.specs["down"], pc.ops["t"], pc.ops["x"]
    fused = C.fuse_shortcut(main, down)
    assert (B * Ho * Ho) % 64 != 0
    if cout == 2048:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert -(-B * Ho * Ho // 64) > max(1, cus // (cout // 128)), "one tile per workgroup"

    def case(ops):
        out = ops.out((B, Ho, Ho, cout))
        C.conv2d(ops.inp(t, "t"), ops.spec(fused), x2=ops.inp(x, "x2"), out=out, tile=(64, 128, 13))
        return out

    y = run_both(case)
    idn = R.conv_ref(_nchw(x).float().to(DEV), down)
    ref = R.conv_ref(_nchw(t).float().to(DEV), main, idn)
    assert _rel_err(_nchw(y), ref) < 1e-2
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"conv_pw dual B{B} N{cout}")


@pytest.mark.parametrize("variant,grid", [(0, 0), (2, 0), (8, 0), (20, 5)])
def test_fused_projection_guarded(native, monkeypatch, variant, grid):
    """conv3(t) + down(x) as one K-concatenated igemm with two A sources, M = 49."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    if grid:
        monkeypatch.setenv("AIKO_CONV_PERS_GRID", str(grid))
    B, H, cout, stride = 1, 14, 2048, 2
    Ho = H // stride
    pc = P.projection_case(DEV)
    main, down, t, x = pc.specs["main"], pc.specs["down"], pc.ops["t"], pc.ops["x"]
    fused = C.fuse_shortcut(main, down)
    tile = (256, 128, variant) if variant in (8, 20) else (64, 128, variant)
    assert (B * Ho * Ho) % tile[0] != 0

    def case(ops):
        out = ops.out((B, Ho, Ho, cout))
        C.conv2d(ops.inp(t, "t"), ops.spec(fused), x2=ops.inp(x, "x2"), out=out, tile=tile)
        return out

    y = run_both(case)
    idn = R.conv_ref(_nchw(x).float().to(DEV), down)
    ref = R.conv_ref(_nchw(t).float().to(DEV), main, idn)
    assert _rel_err(_nchw(y), ref) < 1e-2
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"fused projection v{variant}")


# ---- patch / patchw / rows kernels ---------------------------------------------------------------

@pytest.mark.parametrize("B,H,W,act", P.PATCH_CASES)
def test_conv3x3_patch_guarded(native, B, H, W, act):
    """Variant 10: 8-row tiles, H = 1 / 13: every image ends in a partial tile."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    pc = P.patch_case(B, H, W, act, DEV)
    spec0, x = pc.specs["conv"], pc.ops["x"]
    assert H % 8 != 0

    def case(ops):
        out = ops.out((B, H, W, 64))
        C.conv2d(ops.inp(_nhwc(x), "x"), ops.spec(spec0), out=out, tile=(8, 64, 10))
        return out

    y = run_both(case)
    assert _rel_err(_nchw(y), R.conv_ref(x.float().to(DEV), spec0)) < 1e-2
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"conv3x3_patch B{B} H{H}")


@pytest.mark.parametrize("B,H,act,slices,grid", P.PATCHW_CASES)
def test_conv3x3_patchw_guarded(native, B, H, act, slices, grid):
    """Variant 16: 14-row tiles; H = 5 / 30 end each image in a partial tile, grid 1 / 2 walks
    several tiles per workgroup; a channel-slice input (pitch 192, gap channels poison)."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    pc = P.patchw_case(B, H, act, DEV)
    spec0, x = pc.specs["conv"], pc.ops["x"]
    assert H % 14 != 0 or grid == 1

    def case(ops):
        spec = ops.spec(spec0)
        xin = ops.inp_slice(_nhwc(x), 192, 32, "x") if slices else ops.inp(_nhwc(x), "x")
        if slices:
            ybig = ops.out((B, H, 28, 256), name="concat buffer")
            out = ybig[..., 64:192]
        else:
            out = ops.out((B, H, 28, 128))
        assert C.patchw_variant_ok(spec, xin, None, None, out)
        torch.ops.aiko.conv3x3_patchw_out(xin, ops.inp(C.patchw_weight(spec), "weight image"), spec.bias, out,
                                          spec.act, grid)
        if slices:
            torch.cuda.synchronize()
            assert torch.isnan(ybig[..., :64].float()).all() and torch.isnan(ybig[..., 192:].float()).all()
        return out

    y = run_both(case)
    assert _rel_err(_nchw(y), R.conv_ref(x.float().to(DEV), spec0)) < 1e-2
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"conv3x3_patchw B{B} H{H}")


@pytest.mark.parametrize("B,H,act,res,slices,grid", P.ROWS_CASES)
def test_conv3x3_rows_guarded(native, B, H, act, res, slices, grid):
    """Variant 17: B * H rows split over ``grid`` workgroups (12 over 5, 21 over 4: uneven
    ranges crossing image boundaries); channel-slice input / residual / output."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    pc = P.rows_case(B, H, act, res, DEV)
    spec0, x, r = pc.specs["conv"], pc.ops["x"], pc.ops["r"]
    if grid > 1:
        assert (B * H) % grid != 0, "even row split"

    def case(ops):
        spec = ops.spec(spec0)
        if slices:
            xin = ops.inp_slice(_nhwc(x), 96, 32, "x")
            rin = ops.inp_slice(_nhwc(r), 96, 64, "residual") if r is not None else None
            ybig = ops.out((B, H, 80, 128), name="concat buffer")
            out = ybig[..., 96:128]
        else:
            xin = ops.inp(_nhwc(x), "x")
            rin = ops.inp(_nhwc(r), "residual") if r is not None else None
            out = ops.out((B, H, 80, 32))
        assert C.rows_variant_ok(spec, xin, rin, None, out)
        act_code = spec.act | (C.ACT_RESIDUAL_AFTER if res == "after" else 0)
        torch.ops.aiko.conv3x3_rows_out(xin, ops.inp(C.rows_weight(spec), "weight image"), spec.bias, rin, out,
                                        act_code, grid)
        if slices:
            torch.cuda.synchronize()
            assert torch.isnan(ybig[..., :96].float()).all()
        return out

    y = run_both(case)
    ref = R.conv_ref(x.float().to(DEV), spec0, None if (r is None or res == "after") else r.float().to(DEV))
    if res == "after":
        ref = ref + r.float().to(DEV)
    assert _rel_err(_nchw(y), ref) < 1e-2
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"conv3x3_rows B{B} H{H}")


# ---- ResNet fused kernels ------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W,grid", [(1, 8, 8, 0), (3, 8, 8, 2)])
@pytest.mark.parametrize("k1,n1,n2", [(64, 256, 64), (64, 256, 128), (128, 512, 128)])
def test_conv_chain_guarded(native, k1, n1, n2, B, H, W, grid):
    """conv_chain / conv_chain2: 64-pixel tiles, M % 64 == 0 by contract (no partial tile); the
    kernels prefetch the NEXT tile's rows, so the edge is the last tile of each workgroup's walk
    (grid 2 over 3 tiles: an uneven walk).  The fp64 reference rounds y to bf16 where the kernel
    does — in LDS, the tile that is both stored and read by the second GEMM — so y and z are
    each held to the per-pixel / per-channel bound."""
    from aiko_services_amd.ops import conv as C
    pc = P.chain_case(k1, n1, n2, B, H, W, DEV)
    spec3, spec1, x, r = pc.specs["c3"], pc.specs["c1"], pc.ops["x"], pc.ops["r"]
    assert C.chain_ok(spec3, spec1)
    M = B * H * W
    assert M % 64 == 0
    if grid:
        assert (M // 64) % grid != 0, "even walk"

    def case(ops):
        y, z = ops.out((B, H, W, n1), name="y"), ops.out((B, H, W, n2), name="z")
        C.conv_chain(ops.inp(x, "x"), ops.spec(spec3), ops.inp(r, "residual"), y, ops.spec(spec1), z, grid=grid)
        return y, z

    y, z = run_both(case)
    xd, rd = x.to(DEV), r.to(DEV)
    y2 = C.conv2d(xd, spec3, residual=rd)
    z2 = C.conv2d(y2, spec1)
    assert ((y.float() - y2.float()).abs() > 0.02 * (1 + y2.float().abs())).float().mean() < 1e-3
    assert ((z.float() - z2.float()).abs().max() / z2.float().abs().max()) < 2e-2
    yr = torch.relu(xd.float() @ spec3.ref_weight[:, :, 0, 0].T.to(DEV) + spec3.ref_bias.to(DEV) + rd.float())
    assert ((y.float() - yr).norm() / yr.norm()).item() < 1e-2
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"conv_chain y {k1}-{n1}-{n2} B{B}")
    assert_pixel_channel(z, pc.ref64[1], ROW_BOUND, f"conv_chain z {k1}-{n1}-{n2} B{B}")


def test_conv_chain_dual_guarded(native):
    """The dual-source chain ([t2 | x] . W^T, K = 64 + 64 -> 256 -> 64) at M = 64: one tile.  The
    fp64 reference rounds y to bf16 where the kernel does (the LDS tile stored and read by the
    second GEMM)."""
    from aiko_services_amd.ops import conv as C
    pc = P.chain_dual_case(DEV)
    fused = C.fuse_shortcut(pc.specs["c3"], pc.specs["down"])
    nxt, t2, x = pc.specs["nxt"], pc.ops["t2"], pc.ops["x"]
    assert C.chain_dual_ok(fused, nxt)
    B, H, W = 1, 8, 8

    def case(ops):
        y, z = ops.out((B, H, W, 256), name="y"), ops.out((B, H, W, 64), name="z")
        C.conv_chain(ops.inp(t2, "t2"), ops.spec(fused), None, y, ops.spec(nxt), z, x2=ops.inp(x, "x2"))
        return y, z

    y, z = run_both(case)
    y2 = C.conv2d(t2.to(DEV), fused, x2=x.to(DEV))
    z2 = C.conv2d(y2, nxt)
    assert ((y.float() - y2.float()).norm() / y2.float().norm()).item() < 5e-3
    assert ((z.float() - z2.float()).norm() / z2.float().norm()).item() < 1e-2
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, "conv_chain dual y")
    assert_pixel_channel(z, pc.ref64[1], ROW_BOUND, "conv_chain dual z")


@pytest.mark.parametrize("B,H,grid", [(1, 1, 1), (2, 3, 2), (3, 2, 0), (3, 3, 2)])
@pytest.mark.parametrize("dual", [False, True])
def test_bneck_fused_guarded(native, B, H, dual, grid):
    """bneck_fused streams 56-pixel image rows through 64 pixel slots (a partial tile in every
    row) over contiguous per-workgroup row ranges; (3, 3, 2): 9 rows over 2 workgroups.  The
    fp64 reference rounds t1 and t2 to bf16 (the kernel keeps them as bf16 in LDS); the identity
    or projection shortcut is added unrounded, as in the kernel's fp32 epilogue."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    pc = P.bneck_case(B, H, dual, grid, DEV)
    c1, c2, c3, down, x = pc.specs["c1"], pc.specs["c2"], pc.specs["c3"], pc.specs.get("down"), pc.ops["x"]
    conv3 = C.fuse_shortcut(c3, down) if dual else c3
    assert 56 % 64 != 0
    if (B, H, grid) == (3, 3, 2):
        assert (B * H) % grid != 0, "even row split"

    def case(ops):
        out = ops.out((B, H, 56, 256))
        C.bneck_fused(ops.inp(_nhwc(x), "x"), ops.spec(c1, "conv1"), ops.spec(c2, "conv2"), ops.spec(conv3, "conv3"),
                      out=out, grid=grid)
        return out

    y = run_both(case)
    xf = x.float().to(DEV)
    t = R.conv_ref(xf, c1)
    t = R.conv_ref(t.to(BF16).float(), c2)
    idn = R.conv_ref(xf, down) if down is not None else xf
    ref = R.conv_ref(t.to(BF16).float(), c3, residual_nchw=idn)
    err = _rel_err(_nchw(y), ref)
    assert err < 1e-2, err
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"bneck_fused B{B} H{H} dual{int(dual)} grid{grid}")


@pytest.mark.parametrize("B,H,W,N,grid", P.EXP_GUARD_CASES)
def test_conv3x3_exp_guarded(native, B, H, W, N, grid):
    """conv_exp.hip: 256-row tiles, M = 196 / 588 / 315: the last tile is partial.  The fp64
    reference rounds t2 to bf16 (the kernel's LDS tile); the residual is added unrounded."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    pc = P.exp_case(B, H, W, N, grid, DEV)
    c2, c3, t1, x = pc.specs["c2"], pc.specs["c3"], pc.ops["t1"], pc.ops["x"]
    M = B * H * W
    assert M % 256 != 0

    def case(ops):
        out = ops.out((B, H, W, N))
        s2, s3 = ops.spec(c2, "conv2"), ops.spec(c3, "conv3")
        t1d, xd = ops.inp(_nhwc(t1), "t1"), ops.inp(_nhwc(x), "residual")
        assert C.conv_exp_ok(s2, s3, t1d, xd)
        C.conv3x3_exp(t1d, s2, s3, xd, out=out, grid=grid)
        return out

    y = run_both(case)
    t = R.conv_ref(t1.float().to(DEV), c2)
    ref = _nhwc(R.conv_ref(t.to(BF16).float(), c3, residual_nchw=x.float().to(DEV))).reshape(M, N)
    a = y.reshape(M, N).float()
    for r0 in range(0, M, 256):                                 # the per-tile bound of test_gpu_conv_exp
        e = _rel_err(a[r0:r0 + 256], ref[r0:r0 + 256])
        assert e < 1e-2, (r0, e)
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"conv3x3_exp B{B} {H}x{W} N{N} grid{grid}")


# ---- stems ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stem_case():
    return P.stem_operands(DEV)


def _stem_image(pre, hw):
    """The image inside a bf16 stem buffer [B, Hp, Wp, 4] as NCHW: what the stem conv reads."""
    return _nchw(pre[:, 3:3 + hw[0], 3:3 + hw[1], :3])


def _stem_ref(frames, spec, hw, pool):
    from aiko_services_amd.ops import reference as R
    xr = R.preprocess_ref(frames.to(DEV), hw)
    y = R.conv_ref(xr.to(BF16).float(), spec)
    return F.max_pool2d(y, 3, 2, 1) if pool else y


def test_preprocess_and_stem_conv_guarded(native, stem_case):
    """preprocess_frames (row kernel: aligned base) -> the stem through conv2d(image_hw=...),
    M = 2 * 48 * 66 = 6336 on 128-row tiles (a 64-row tail).  The fp64 reference of the conv
    takes the bf16 stem buffer the kernel read as its input, so the conv's operands are exact."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    from aiko_services_amd.ops import vision as V
    hw, frames, spec0 = stem_case
    B = frames.shape[0]
    Hp, Wp = C.stem_geometry(*hw)
    Ho, Wo = spec0.out_hw(*hw)
    assert (B * Ho * Wo) % 128 != 0

    def case(ops):
        pre = V.preprocess_frames(ops.inp(frames, "frames"), hw, out=ops.out((B, Hp, Wp, 4), name="stem buffer"))
        out = ops.out((B, Ho, Wo, 64))
        C.conv2d(pre, ops.spec(spec0), image_hw=hw, out=out, tile=(128, 64))
        return pre, out

    pre, y = run_both(case)
    xr = R.preprocess_ref(frames.to(DEV), hw)
    assert _rel_err(_nchw(pre[:, 3:3 + hw[0], 3:3 + hw[1], :3]), xr) < 5e-3
    assert pre[:, :3].abs().max().item() == 0 and pre[..., 3].abs().max().item() == 0
    assert pre[:, :, :3].abs().max().item() == 0 and pre[:, :, 3 + hw[1]:].abs().max().item() == 0
    assert _rel_err(_nchw(y), _stem_ref(frames, spec0, hw, False)) < 1e-2
    assert_pixel_channel(y, P.stem_case(False, _stem_image(pre, hw), DEV).ref64[0], ROW_BOUND, "stem conv2d")


@pytest.mark.parametrize("variant", [0, 1])
def test_stem_pool_guarded(native, stem_case, variant):
    """Fused stem + max-pool: pooled tiles of 8 x 7 / 8 x 14 over a 24 x 33 pooled image.  The
    fp64 reference (conv, ReLU, pool) takes the bf16 stem buffer as its input."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import vision as V
    hw, frames, spec0 = stem_case
    B = frames.shape[0]
    Ho, Wo = spec0.out_hw(*hw)
    Hm, Wm = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    assert Wm % (7, 14)[variant] != 0
    pre0 = V.preprocess_frames(frames.to(DEV), hw)

    def case(ops):
        out = ops.out((B, Hm, Wm, 64))
        C.stem_pool(ops.inp(pre0, "stem buffer"), ops.spec(spec0), hw, out=out, variant=variant)
        return out

    y = run_both(case)
    assert _rel_err(_nchw(y), _stem_ref(frames, spec0, hw, True)) < 1e-2
    unfused = V.maxpool2d(C.conv2d(pre0, spec0, image_hw=hw), 3, 2, 1)
    assert torch.equal(y, unfused)
    assert_pixel_channel(y, P.stem_case(True, _stem_image(pre0, hw), DEV).ref64[0], ROW_BOUND, f"stem_pool v{variant}")


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_stem_pool_u8_guarded(native, stem_case, variant):
    """uint8 frames straight into the fused stem: the image edges are tap masks on the FRAME
    (no zero-bordered buffer), so the guards sit directly against rows 0 and H-1.

    The kernel does not form bf16((c / 255 - mean) / std): its patch holds bf16(c - 255 mean) and
    its weights are bf16(w / (255 std)) (stem_pool.hip, ops.conv.stem_pool_u8_weight), so both
    operands differ from the bf16 stem buffer's and the stem spec's.  The fp64 reference takes
    both tables from the kernel's formulas; tests/test_conv_parity_reference.py shows on the CPU
    that the fp32 formulas round all 256 x 3 (value, channel) pairs, and the scaled weights, to
    the same bf16 as the fp64 ones — no pair differs — so the reference's operands are exact."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import vision as V
    hw, frames, spec0 = stem_case
    B = frames.shape[0]
    Ho, Wo = spec0.out_hw(*hw)
    Hm, Wm = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    assert Wm % 7 != 0 and hw[1] % 4 == 0

    def case(ops):
        out = ops.out((B, Hm, Wm, 64))
        C.stem_pool_u8(ops.inp(frames, "frames"), ops.spec(spec0), V.IMAGENET_MEAN, V.IMAGENET_STD, out=out,
                       variant=variant)
        return out

    y = run_both(case)
    assert _rel_err(_nchw(y), _stem_ref(frames, spec0, hw, True)) < 1e-2
    assert_pixel_channel(y, P.stem_u8_case(V.IMAGENET_MEAN, V.IMAGENET_STD, DEV).ref64[0], ROW_BOUND,
                         f"stem_pool_u8 v{variant}")


@pytest.fixture(scope="module")
def yolo(native):
    from aiko_services_amd.models.yolov8 import YOLOv8
    return YOLOv8("n", device=DEV)


@pytest.mark.parametrize("hw,S", [((360, 500), 640), ((120, 200), 200), ((90, 125), 200)])
def test_stem_direct_guarded(native, yolo, hw, S):
    """stem_direct_out: (360, 500) -> 640 is the resizing kernel at the model's geometry; the
    200 x 200 canvases give a 100 x 100 output (partial 16 x 32 tiles) without (120, 200: the
    fast kernel) and with (90, 125) a resize, letterbox bars above and below.  Only the
    no-resize case gets the per-pixel / per-channel bound.  Its kernel (stem_fast_kernel) keeps
    the RAW pixel values 0 .. 255 and the raw canvas colour in its tile — exact in bf16 — and
    applies 1 / (255 std) to the fp32 accumulator, so no input rounding exists: the fp64 reference
    is the conv of the exact canvas (c - 255 mean) / (255 std), not of the bf16 stem buffer (whose
    rounding of c / 255 the kernel does not share: against it 118 of 20,000 pixels, all inside
    the frame, measured up to 5.1e-3).  The resizing cases keep their present bounds: the
    in-kernel bilinear weights need not round like preprocess_frames', so neither input is the
    kernel's operand."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    from aiko_services_amd.ops import vision as V
    m = yolo
    g = torch.Generator().manual_seed(hw[0])
    B = 2
    frames = torch.randint(0, 256, (B,) + hw + (3,), generator=g, dtype=torch.uint8)
    Ho, Wo, top, left, _ = V.letterbox_geometry(hw[0], hw[1], S)
    h0, w0 = C.stem_out_hw(S, S, 3, 2, 1)
    if S != 640:
        assert h0 % 16 != 0 and w0 % 32 != 0
    if m._stem_w is None:
        m.stem_from_frames(frames.to(DEV))
    stem_w = m._stem_w.clone()

    def case(ops):
        out = ops.out((B, h0, w0, m.ch[0]))
        torch.ops.aiko.stem_direct_out(ops.inp(frames, "frames"), ops.inp(stem_w, "weight"), ops.inp(m.l0.bias, "bias"),
                                       out, [Ho, Wo, S, S, top, left, 3, 2, 1, 2], 114.0, list(V.YOLO_MEAN),
                                       list(V.YOLO_STD), False)
        return out

    y = run_both(case)
    Hp, Wp = C.stem_geometry(S, S, 3, 2, 1)
    pre = V.preprocess_frames(frames.to(DEV), (Ho, Wo), V.YOLO_MEAN, V.YOLO_STD, stem=(3, 2, 1),
                              out=torch.empty(B, Hp, Wp, 4, dtype=BF16, device=DEV), canvas=(S, S, top, left, 114.0))
    unfused = C.conv2d(pre, m.l0, image_hw=(S, S))
    assert _rel_err(y.float(), unfused.float()) < 5e-3
    ref = R.conv_ref(_nchw(pre[:, 1:S + 1, 1:S + 1, :3]).float(), m.l0)
    assert _rel_err(_nchw(y), ref) < 1e-2
    if (Ho, Wo) == hw:
        canvas = torch.full((B, 3, S, S), 114.0, dtype=torch.float64)
        canvas[:, :, top:top + Ho, left:left + Wo] = _nchw(frames).double()
        mean = torch.tensor(V.YOLO_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
        std = torch.tensor(V.YOLO_STD, dtype=torch.float64).view(1, 3, 1, 1)
        ref64 = R.conv_ref((canvas - 255.0 * mean) / (255.0 * std), m.l0)
        assert_pixel_channel(y, _nhwc(ref64), ROW_BOUND, f"stem_direct {hw}")


# ---- YOLO fused kernels --------------------------------------------------------------------------

def _c2f_bound(a, b):
    a, b = a.float(), b.float()
    cos = F.cosine_similarity(a.flatten(), b.flatten(), dim=0).item()
    assert cos > 0.9995, cos
    assert (a - b).abs().max().item() < 0.05 * b.abs().max().item()


@pytest.mark.parametrize("layer,H,W,cin,cout,rb", P.C2F_CASES)
def test_c2f_fused_guarded(native, yolo, monkeypatch, layer, H, W, cin, cout, rb):
    """c2f_fused.hip (l2: weights in registers; l15: the LDS-weights variant), one workgroup per
    band of rb rows: halo rows recomputed at band edges, zero rows at the image edges; rb == H is
    the single band with zero rows on both sides and no halo.  The launcher refuses
    H % rb != 0, so no band is partial.

    Two references: the project's unfused device path (as before), and an fp64 evaluation of the
    block from its specs (cv1, the chunk, m[0], the concat, cv2, the shortcut), rounded to bf16
    where the kernel stores bf16: [a | s] = silu(cv1(x)) and t = silu(conv_a(s)) in their LDS
    rings, c = silu(conv_b(t)) (+ s, added in fp32: one rounding of the sum), and the output.
    l15 is held to 2^-8; l2 to conv_parity_cases.C2F_L2_BOUND, because the fp32 evaluation of
    its 16-channel intermediates alone exceeds 2^-8 at single pixels (see that constant)."""
    m, blk = yolo, getattr(yolo, layer)
    pc = P.c2f_case(layer, H, W, cin, rb, yolo)
    x = pc.ops["x"]
    a, b = blk.m[0]
    assert H % rb == 0

    def case(ops):
        out = ops.out((1, H, W, cout))
        xd = ops.inp(x, "x")
        assert m._c2f_fused_ok(blk, xd, out)
        sp = [ops.spec(s, n) for s, n in ((blk.cv1, "cv1"), (a, "m.a"), (b, "m.b"), (blk.cv2, "cv2"))]
        torch.ops.aiko.c2f_fused_out(xd, sp[0].weight, sp[0].bias, sp[1].weight, sp[1].bias, sp[2].weight, sp[2].bias,
                                     sp[3].weight, sp[3].bias, out, blk.cv1.Cc, blk.shortcut, rb, None)
        return out

    y = run_both(case)
    monkeypatch.setenv("AIKO_C2F_FUSED", "0")
    out_u = torch.empty_like(y)
    m._run_c2f(layer + "g", blk, x.to(DEV), out_u)
    torch.cuda.synchronize()
    _c2f_bound(y, out_u)
    assert_pixel_channel(y, pc.ref64[0], P.case_bound(pc.name), f"c2f_fused {layer} rb{rb}")


def test_c2f_fused_upsample_guarded(native, yolo):
    """l15's fused C2f reading channels [0, 128) of its input as the nearest 2x upsample of
    ``xu`` (a channel slice of a 192-channel buffer): those channels of ``x`` are never
    materialised — poison in the guarded run — and must not be read.  Bit-identical to the same
    kernel on the materialised input."""
    m, blk = yolo, yolo.l15
    g = torch.Generator().manual_seed(15)
    H = W = 80
    rb = 10
    tail = (torch.randn(1, H, W, 64, generator=g) * 2).to(BF16)
    xu0 = (torch.randn(1, H // 2, W // 2, 128, generator=g) * 2).to(BF16)
    a, b = blk.m[0]

    def launch(xd, xu, out, sp):
        torch.ops.aiko.c2f_fused_out(xd, sp[0].weight, sp[0].bias, sp[1].weight, sp[1].bias, sp[2].weight, sp[2].bias,
                                     sp[3].weight, sp[3].bias, out, blk.cv1.Cc, blk.shortcut, rb, xu)

    def case(ops):
        wide = torch.full((1, H, W, 192), NAN if ops.on else 0.0, dtype=BF16)
        wide[..., 128:] = tail
        out = ops.out((1, H, W, 64))
        xd = ops.inp(wide, "x")
        assert m._c2f_fused_ok(blk, xd, out)
        launch(xd, ops.inp_slice(xu0, 192, 64, "upsample source"), out,
               [ops.spec(s, n) for s, n in ((blk.cv1, "cv1"), (a, "m.a"), (b, "m.b"), (blk.cv2, "cv2"))])
        return out

    y = run_both(case)
    up = xu0.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    ref = torch.empty_like(y)
    launch(torch.cat([up, tail], -1).to(DEV), None, ref, [blk.cv1, a, b, blk.cv2])
    torch.cuda.synchronize()
    assert torch.equal(y, ref)


@pytest.mark.parametrize("rb", [10, 20, 80])
def test_c2f_bneck_guarded(native, yolo, monkeypatch, rb):
    """c2f_bneck_kernel on l4's first bottleneck: reads channels [32, 64) and writes channels
    [64, 96) of the 128-channel concat buffer; every other channel of it is poison.  Bands of
    10 / 20 rows (the existing test's) and the single band rb == H.  Next to the unfused device
    path, an fp64 reference from the two specs: t = silu(conv_a(x)) rounded to bf16 (the LDS
    ring), silu(conv_b(t)) + x rounded once, as the output."""
    from aiko_services_amd.ops import conv as C
    m, blk = yolo, yolo.l4
    pc = P.c2f_bneck_case(yolo)
    H = W = 80
    c = blk.c
    assert c == 32 and blk.shortcut and H % rb == 0
    x = pc.ops["x"]
    a, b = blk.m[0]

    def case(ops):
        wide = torch.full((1, H, W, 4 * c), NAN, dtype=BF16)
        wide[..., c:2 * c] = x
        cat = ops.inp(wide, "concat buffer")
        sa, sb = ops.spec(a, "m.a"), ops.spec(b, "m.b")
        torch.ops.aiko.c2f_bneck_out(cat[..., c:2 * c], sa.weight, sa.bias, sb.weight, sb.bias, cat[..., 2 * c:3 * c],
                                     blk.shortcut, rb)
        torch.cuda.synchronize()
        assert torch.isnan(cat[..., :c].float()).all() and torch.isnan(cat[..., 3 * c:].float()).all()
        assert torch.equal(cat[..., c:2 * c], x.to(DEV))
        return cat[..., 2 * c:3 * c]

    y = run_both(case)
    xd = x.to(DEV)
    t = C.conv2d(xd, a)
    ref = C.conv2d(t, b, residual=xd, residual_after_act=True)
    _c2f_bound(y, ref)
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"c2f_bneck rb{rb}")


@pytest.mark.parametrize("branch,hw", P.TAIL_CASES)
def test_conv_tail_guarded(native, yolo, branch, hw):
    """conv_glds TAIL (3x3 + SiLU with the 1x1 in its epilogue, 128-row tiles), B = 1.  box / cls:
    the three head levels (20 x 20 and 40 x 40 end in a partial tile, 80 x 80 = 50 whole tiles),
    input and output channel slices of [.., 64 + 80] buffers whose other slice is poison.  l3:
    the 3x3 / stride 2 conv 32 -> 64 with l4's cv1 (1x1 + SiLU) in its epilogue on an odd 21 x 19
    image, from a slice of a 48-channel buffer into the first half of l4's concat.  The fp64
    reference rounds the activated 3x3 tile to bf16, as the kernel does in LDS before the 1x1."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    s1, s2, cin, c0, pitch, n, o0, opitch, H, W = P.tail_geometry(branch, hw, yolo)
    pc = P.tail_case(branch, hw, yolo)
    x = pc.ops["x"]
    Ho, Wo = s1.out_hw(H, W)
    M = Ho * Wo
    if hw != 80:
        assert n in (64, 80) and M % 128 != 0, "no partial last tile"

    def case(ops):
        xs = ops.inp_slice(x, pitch, c0, "input buffer")
        big = ops.out((1, Ho, Wo, opitch), name="output buffer")
        a, b = ops.spec(s1, "3x3"), ops.spec(s2, "1x1")
        assert C.conv_tail_ok(xs, a, b)
        C.conv2d_tail(xs, a, b, big[..., o0:o0 + n])
        torch.cuda.synchronize()
        other = torch.cat([big[..., :o0], big[..., o0 + n:]], -1)
        assert torch.isnan(other.float()).all(), "wrote outside the output's channel slice"
        return big[..., o0:o0 + n]

    y = run_both(case)
    xr = _nchw(x.to(DEV).float())
    yr = _nhwc(R.conv_ref(R.conv_ref(xr, s1), s2))
    assert ((y.float() - yr).norm() / yr.norm()).item() < 1e-2
    t = C.conv2d(x.to(DEV), s1)
    ref = C.conv2d(t, s2).float()
    assert F.cosine_similarity(y.float().flatten(), ref.flatten(), dim=0).item() > 0.9999
    assert (y.float() - ref).abs().max().item() < 0.02 * ref.abs().max().item()
    assert_pixel_channel(y, pc.ref64[0], ROW_BOUND, f"conv_tail {branch} {hw}")


def test_conv_tail_decode_guarded(native):
    """The tail launches that decode in their epilogue (box: DFL -> xyxy; class: sigmoid(max) /
    argmax) writing rows [astart, astart + H * W) of [B, A] outputs: the anchors before and after
    the level are poison and must stay so.  Against the stored head output + yolo_decode."""
    from aiko_services_amd.models import yolov8 as Y
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import detect as DT
    m = Y.YOLOv8("n", device=DEV, cls_bias=0.0)
    assert m._decode_fused_ok()
    lvl = m.heads[1]
    g = torch.Generator().manual_seed(13)
    B, H, W = 1, 20, 20
    M, astart, A = H * W, 24, H * W + 64
    assert M % 64 != 0 and M % 128 != 0 and M % 256 != 0
    h1 = (torch.randn(B, H, W, 144, generator=g) * 2).to(BF16)

    def case(ops):
        hd = ops.inp(h1, "head buffer")
        zp = C.zero_page(hd.device)
        boxes = ops.out((B, A, 4), torch.float32, "boxes")
        scores = ops.out((B, A), torch.float32, "scores")
        cls = ops.out((B, A), torch.int32, "cls")
        if not ops.on:
            cls.fill_(-1515870811)                           # 0xA5A5A5A5: the guarded run's poison
        for xs, (s1, s2), mode, nc in ((hd[..., :64], (lvl.box[1], lvl.box[2]), 1, 64),
                                       (hd[..., 64:], (lvl.cls[1], lvl.cls[2]), 2, 80)):
            a, b = ops.spec(s1), ops.spec(s2)
            torch.ops.aiko.conv_glds_tail_decode_out(xs, a.weight, a.bias, b.weight, b.bias, boxes, scores, cls,
                                                     s1.R, s1.pad, s1.act, mode, nc, 16, astart, zp)
        torch.cuda.synchronize()
        for t in (boxes, scores):
            assert torch.isnan(t[:, :astart]).all() and torch.isnan(t[:, astart + M:]).all()
        assert (cls[:, :astart] == -1515870811).all() and (cls[:, astart + M:] == -1515870811).all()
        return boxes[:, astart:astart + M], scores[:, astart:astart + M], cls[:, astart:astart + M]

    bf, sf, cf = run_both(case)
    hd = h1.to(DEV)
    feat = torch.empty(B, H, W, 144, dtype=BF16, device=DEV)
    C.conv2d_tail(hd[..., :64], lvl.box[1], lvl.box[2], feat[..., :64])
    C.conv2d_tail(hd[..., 64:], lvl.cls[1], lvl.cls[2], feat[..., 64:])
    bd, sd, cd = DT.yolo_decode([feat], (16,), 80)
    torch.cuda.synchronize()
    assert torch.equal(cf, cd) and torch.equal(sf, sd)
    assert (bf - bd).abs().max().item() < 1e-3 * bd.abs().max().item()


# ---- pointwise ops -------------------------------------------------------------------------------

# The launchers in vision_ops.hip / detect_ops.hip: one thread per output element (a pixel, or 8
# channels of a pixel) in blocks of 256 threads, or one wave per row in blocks of 4 waves.  Each
# case computes that split and asserts the last block is partial.
BLOCK = 256
WAVES = 4


def test_preprocess_rows_guarded(native):
    """No-resize frames at an aligned base: preprocess_rows_kernel (dword loads, a wave per row;
    W * 3 = 300 bytes per row), BGR; the zero border is written over the output's poison."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    from aiko_services_amd.ops import vision as V
    g = torch.Generator().manual_seed(136)
    B, H, W = 3, 36, 100
    frames = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    Hp, Wp = C.stem_geometry(H, W)
    assert Hp % WAVES != 0, "a wave per output row, 4 rows per block: no partial block"
    assert (W * 3 // 4) % 64 != 0 and Wp % 64 != 0, "no partial 64-lane pass over a row"

    def case(ops):
        fr = ops.inp(frames, "frames")
        assert fr.data_ptr() % 4 == 0
        return V.preprocess_frames(fr, (H, W), bgr=True, out=ops.out((B, Hp, Wp, 4)))

    pre = run_both(case)
    ref = R.preprocess_ref(frames.to(DEV), (H, W), bgr=True)
    assert _rel_err(_nchw(pre[:, 3:3 + H, 3:3 + W, :3]), ref) < 5e-3
    assert pre[:, :3].abs().max().item() == 0 and pre[..., 3].abs().max().item() == 0
    assert pre[:, :, :3].abs().max().item() == 0 and pre[:, :, 3 + W:].abs().max().item() == 0
    assert pre[:, 3 + H:].abs().max().item() == 0


def test_preprocess_resize_guarded(native):
    """The resizing kernel: a thread per stem-buffer pixel, blocks of 256 per image."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    from aiko_services_amd.ops import vision as V
    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (2, 480, 640, 3), generator=g, dtype=torch.uint8)
    Hp, Wp = C.stem_geometry(224, 224)
    assert (Hp * Wp) % BLOCK != 0 and Hp * Wp <= 1024 * BLOCK, "no partial last block per image"

    def case(ops):
        return V.preprocess_frames(ops.inp(frames, "frames"), (224, 224), out=ops.out((2, Hp, Wp, 4)))

    pre = run_both(case)
    ref = R.preprocess_ref(frames.to(DEV), (224, 224))
    assert _rel_err(_nchw(pre[:, 3:227, 3:227, :3]), ref) < 1e-2


def test_preprocess_letterbox_guarded(native):
    """The YOLO form: /255 into a 200 x 200 canvas of colour 114 (bars above and below the
    120-row frame) inside the 1-pixel zero border of a 3x3 / 2 stem buffer."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import vision as V
    g = torch.Generator().manual_seed(7)
    B, H, W, S = 2, 120, 200, 200
    frames = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    Ho, Wo, top, left, _ = V.letterbox_geometry(H, W, S)
    assert (Ho, Wo, top, left) == (120, 200, 40, 0)
    Hp, Wp = C.stem_geometry(S, S, 3, 2, 1)
    assert (Hp * Wp) % BLOCK != 0 and Hp * Wp <= 1024 * BLOCK, "no partial last block per image"

    def case(ops):
        return V.preprocess_frames(ops.inp(frames, "frames"), (Ho, Wo), V.YOLO_MEAN, V.YOLO_STD,
                                   out=ops.out((B, Hp, Wp, 4)), stem=(3, 2, 1), canvas=(S, S, top, left, 114.0))

    pre = run_both(case)
    canvas = torch.full((B, 3, S, S), 114.0 / 255, device=DEV)
    canvas[:, :, top:top + Ho, left:left + Wo] = _nchw(frames.to(DEV)).float() / 255
    assert _rel_err(_nchw(pre[:, 1:S + 1, 1:S + 1, :3]), canvas) < 5e-3
    assert pre[:, 0].abs().max().item() == 0 and pre[:, :, 0].abs().max().item() == 0
    assert pre[:, S + 1:].abs().max().item() == 0 and pre[:, :, S + 1:].abs().max().item() == 0
    assert pre[..., 3].abs().max().item() == 0


def test_resize_u8_guarded(native):
    """A thread per output pixel: 2 * 63 * 80 = 10080 pixels = 39 blocks and 96 threads."""
    from aiko_services_amd.ops import vision as V
    g = torch.Generator().manual_seed(6)
    B, Ho, Wo = 2, 63, 80
    frames = torch.randint(0, 256, (B, 37, 53, 3), generator=g, dtype=torch.uint8)
    assert (B * Ho * Wo) % BLOCK != 0, "no partial last block"

    def case(ops):
        return V.resize_u8(ops.inp(frames, "frames"), (Ho, Wo), out=ops.out((B, Ho, Wo, 3), torch.uint8))

    y = run_both(case)
    ref = F.interpolate(_nchw(frames.to(DEV)).float(), size=(Ho, Wo), mode="bilinear",
                        align_corners=False).round().clamp(0, 255).permute(0, 2, 3, 1)
    assert (y.float() - ref).abs().max().item() <= 1


def test_maxpool_guarded(native):
    """3x3 / 2 / pad 1 on odd sizes (taps outside the first and the last image), and the 5x5 / 1
    pool between channel slices of one concat buffer (SPPF form).  A thread per 8 channels of an
    output pixel.  Run with NaN and with +3e38 in the guards: the kernel's max drops a NaN tap."""
    from aiko_services_amd.ops import vision as V
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 13, 15, 64, generator=g).to(BF16)
    cat0 = torch.randn(3, 20, 20, 128, generator=g).to(BF16)
    assert (2 * 7 * 8 * (64 // 8)) % BLOCK != 0 and (3 * 20 * 20 * (32 // 8)) % BLOCK != 0, "no partial last block"

    def case(ops):
        y = V.maxpool2d(ops.inp(x, "x"), 3, 2, 1, out=ops.out((2, 7, 8, 64)))
        cat = ops.inp(cat0, "concat buffer")
        V.maxpool2d(cat[..., :32], 5, 1, 2, out=cat[..., 32:64])
        return y, cat

    run_both(case, poison=3e38)
    y, cat = run_both(case)
    assert torch.equal(_nchw(y).float(), F.max_pool2d(_nchw(x.to(DEV)).float(), 3, 2, 1))
    assert torch.equal(_nchw(cat[..., 32:64]).float(), F.max_pool2d(_nchw(cat0[..., :32].to(DEV)).float(), 5, 1, 2))
    keep = torch.cat([cat[..., :32], cat[..., 64:]], -1)
    assert torch.equal(keep, torch.cat([cat0[..., :32], cat0[..., 64:]], -1).to(DEV))


def test_avgpool_upsample_guarded(native):
    from aiko_services_amd.ops import detect as DT
    from aiko_services_amd.ops import vision as V
    g = torch.Generator().manual_seed(12)
    Ca = 2040                                    # 3 * 255 threads: the last block is partial
    x = torch.randn(3, 7, 7, Ca, generator=g).to(BF16)
    u = torch.randn(2, 5, 7, 32, generator=g).to(BF16)
    assert (3 * (Ca // 8)) % BLOCK != 0, "avgpool (a thread per 8 channels of an image): no partial last block"
    assert (7 * (32 // 8)) % BLOCK != 0, "upsample2x (a thread per 8 channels of an input row pixel): no partial block"

    def case(ops):
        a = V.avgpool(ops.inp(x, "x"), out=ops.out((3, Ca)))
        big = ops.out((2, 10, 14, 80), name="concat buffer")
        DT.upsample2x(ops.inp_slice(u, 48, 16, "x slice"), out=big[..., 48:80])
        torch.cuda.synchronize()
        assert torch.isnan(big[..., :48].float()).all()
        return a, big[..., 48:80]

    a, up = run_both(case)
    assert _rel_err(a, x.to(DEV).float().mean(dim=(1, 2))) < 5e-3
    ref = F.interpolate(_nchw(u.to(DEV)).float(), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(up.float(), ref)


@pytest.mark.parametrize("B,H,W,c", [(2, 7, 33, 16), (3, 20, 20, 128)])
def test_sppf_pool_guarded(native, B, H, W, c):
    """A block per (8 channels, image), its 256 threads striding over the H * W pixels.  Run with
    NaN and with +3e38 in the guards: the kernel's max drops a NaN tap."""
    from aiko_services_amd.ops import vision as V
    g = torch.Generator().manual_seed(H * W + c)
    cat0 = (torch.randn(B, H, W, 4 * c, generator=g) * 4).round().to(BF16)
    assert (H * W) % BLOCK != 0, "no partial last pass over the image"

    def case(ops):
        return V.sppf_pool(ops.inp(cat0, "concat buffer"), c, 5)

    run_both(case, poison=3e38)
    cat = run_both(case)
    ref = cat0.to(DEV).clone()
    for i in range(3):
        V.maxpool2d(ref[..., i * c:(i + 1) * c], 5, 1, 2, out=ref[..., (i + 1) * c:(i + 2) * c])
    torch.cuda.synchronize()
    assert torch.equal(cat, ref)


def test_batchnorm_guarded(native):
    from aiko_services_amd.ops import vision as V
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 9, 11, 32, generator=g).to(BF16)
    gamma, beta = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g)
    mean, var = torch.randn(32, generator=g), torch.rand(32, generator=g) + 0.5
    scale, shift = V.bn_scale_shift(gamma, beta, mean, var)
    assert (2 * 9 * 11 * (32 // 8)) % BLOCK != 0, "a thread per 8 channels of a pixel: no partial last block"

    def case(ops):
        big = ops.out((2, 9, 11, 64), name="concat buffer")
        V.batchnorm(ops.inp_slice(x, 64, 32, "x slice"), ops.inp(scale, "scale"), ops.inp(shift, "shift"), act=1,
                    out=big[..., :32])
        torch.cuda.synchronize()
        assert torch.isnan(big[..., 32:].float()).all()
        return big[..., :32]

    y = run_both(case)
    ref = F.batch_norm(_nchw(x.to(DEV)).float(), mean.to(DEV), var.to(DEV), gamma.to(DEV), beta.to(DEV), False, 0.0,
                       1e-5).relu()
    assert _rel_err(_nchw(y), ref) < 1e-2


def test_softmax_topk_guarded(native):
    from aiko_services_amd.ops import vision as V
    N, k = 1000, 5
    g = torch.Generator().manual_seed(N)
    lg = torch.randint(-4, 5, (19, N), generator=g).float()
    lg[:, ::3] *= -0.0
    lg = lg.to(BF16)
    assert lg.shape[0] % WAVES != 0, "a wave per row, 4 rows per block: no partial last block"
    assert 64 * 4 < N <= 64 * 16 and N % 64 != 0, "no partial 64-lane pass over a row (the 16-per-lane kernel)"

    def case(ops):
        return V.softmax_topk(ops.inp(lg, "logits"), k, prob=ops.out((19, k), torch.float32, "prob"),
                              index=ops.out((19, k), torch.int32, "index"))

    p, i = run_both(case)
    order = torch.stack([torch.tensor(sorted(range(N), key=lambda c: (-float(r[c]), c))) for r in lg.float()])[:, :k]
    assert torch.equal(i.cpu().long(), order)
    assert torch.allclose(p.cpu(), torch.softmax(lg.float(), -1).gather(1, order), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("B,N,K", P.LINEAR_CASES)
def test_linear_guarded(native, B, N, K):
    """The igemm linear and the split-K linear with a guarded ``work`` buffer of exactly
    S * B * N elements (32 x 32 one-wave tiles: M = 37 / 1 and N = 1000 end in partial tiles)."""
    from aiko_services_amd.ops import conv as C
    from aiko_services_amd.ops import reference as R
    pc = P.linear_case(B, N, K, DEV)
    spec0, x = pc.specs["fc"], pc.ops["x"]
    assert B % 32 != 0 and (N % 32 != 0 or B == 1), "split-K: no partial 32 x 32 tile"
    pick = C.pick_tile(B, N)
    assert B % pick[0] != 0 and (N % pick[1] != 0 or B == 1), "igemm: no partial tile"

    def case(ops):
        spec, xd = ops.spec(spec0), ops.inp(x, "x")
        assert C.linear_splitk_ok(xd, spec)
        work = ops.out((C.LINEAR_SPLITK * B * N,), torch.float32, "work")
        y1 = C.linear(xd, spec, out=ops.out((B, N), name="split-K y"), work=work)
        y0 = C.linear(xd, spec, out=ops.out((B, N), name="igemm y"))
        return y1, y0

    y1, y0 = run_both(case)
    ref = R.linear_ref(x.to(DEV).float(), spec0)
    assert _rel_err(y1, ref) < 1e-2
    assert _rel_err(y0, ref) < 1e-2
    assert _rel_err(y1.float(), y0.float()) < 1e-2
    assert_pixel_channel(y1, pc.ref64[0], ROW_BOUND, f"linear split-K {B}x{N}")    # rows: batch entries
    assert_pixel_channel(y0, pc.ref64[0], ROW_BOUND, f"linear igemm {B}x{N}")      # columns: features


# ---- positional liveness controls of the per-pixel / per-channel bound ---------------------------
#
# The new assertion must fail for a kernel that is wrong in one place.  No kernel is sabotaged:
# each control gives the kernel one perturbed operand that the reference does not see — a bias
# scaled by 1.5, or one negated input pixel placed where the family's cases have their edge
# (conv_parity_cases.CONTROLS) — and asserts that exactly the predicted channel / output pixels
# exceed the bound.  tests/test_conv_parity_reference.py shows the same of the fp32 evaluation.

def _control_launch(name, ops, specs, monkeypatch):
    from aiko_services_amd.ops import conv as C

    def nan_out(*shape):
        return torch.full(shape, NAN, dtype=BF16, device=DEV)

    if name in ("v20-walk", "pw-multi"):
        if name == "v20-walk":
            monkeypatch.setenv("AIKO_CONV_PERS_GRID", "3")
        spec, x = specs["conv"], ops["x_nhwc"]
        B, H, W, _ = x.shape
        out = nan_out(B, *spec.out_hw(H, W), spec.cout)
        C.conv2d(x.to(DEV), spec, residual=_nhwc(ops["r"]).to(DEV), out=out,
                 tile=(256, 128, 20) if name == "v20-walk" else (64, 128, 13))
    elif name == "bneck":
        x = _nhwc(ops["x"])
        out = nan_out(*x.shape[:3], 256)
        C.bneck_fused(x.to(DEV), specs["c1"], specs["c2"], specs["c3"], out=out, grid=2)
    elif name == "exp":
        t1, x = _nhwc(ops["t1"]).to(DEV), _nhwc(ops["x"]).to(DEV)
        out = nan_out(*x.shape)
        assert C.conv_exp_ok(specs["c2"], specs["c3"], t1, x)
        C.conv3x3_exp(t1, specs["c2"], specs["c3"], x, out=out, grid=1)
    else:
        blk, cv2, x = specs["blk"], specs["cv2"], ops["x"].to(DEV)
        a, b = blk.m[0]
        out = nan_out(*x.shape[:3], cv2.cout)
        torch.ops.aiko.c2f_fused_out(x, blk.cv1.weight, blk.cv1.bias, a.weight, a.bias, b.weight, b.bias, cv2.weight,
                                     cv2.bias, out, blk.cv1.Cc, blk.shortcut, 10, None)
    torch.cuda.synchronize()
    return out


def _over(errs, bound):
    return torch.nonzero(~(errs < bound)).flatten().tolist()


@pytest.mark.parametrize("name", list(P.CONTROLS))
def test_parity_control_bias(native, yolo, monkeypatch, name):
    """The bias of the channel with the largest |bias| times 1.5 in the kernel's spec only
    (``dataclasses.replace``): exactly that channel exceeds the bound — and in the 2048-channel
    pointwise case the whole-tensor error stays below the old 1e-2."""
    case, _, _, bias_spec, c = P.control(name, yolo, DEV)
    specs = {**case.specs, bias_spec: P.kernel_spec_with_bias(case.specs[bias_spec], c, 1.5)}
    y = _control_launch(name, case.ops, specs, monkeypatch)
    pix, ch = pixel_channel_errs(y, case.ref64[-1])
    print(f"control bias {name}: channel {c} {ch[c].item():.3e}, others at most "
          f"{torch.cat([ch[:c], ch[c + 1:]]).max().item():.3e}, whole tensor {_rel_err(y.cpu(), case.ref64[-1]):.3e}")
    assert _over(ch, P.case_bound(case.name)) == [c]
    if name == "pw-multi":
        assert _rel_err(y.cpu(), case.ref64[-1]) < 1e-2


@pytest.mark.parametrize("name", list(P.CONTROLS))
def test_parity_control_input_pixel(native, yolo, monkeypatch, name):
    """One input pixel negated in the kernel's input only: exactly the output pixels of its
    receptive field exceed the bound (1 for a 1x1, the 3 x 3 neighbourhood through the stride,
    radius 2 for C2f's two 3x3 convs), no other pixel does."""
    case, ops, pixels, _, _ = P.control(name, yolo, DEV)
    y = _control_launch(name, ops, case.specs, monkeypatch)
    pix, _ = pixel_channel_errs(y, case.ref64[-1])
    got = _over(pix, P.case_bound(case.name))
    print(f"control input pixel {name}: {len(got)} pixels over the bound, predicted {len(pixels)}: {pixels}")
    assert got == pixels


# ---- whole models on a guarded workspace ---------------------------------------------------------
#
# The per-kernel cases above force one tile each.  Here every activation buffer of a model's
# workspace is a guarded view (``_buf`` swapped), so each kernel runs with the tile the model
# picks, on the views the model makes: batch slices ``buf[c0:c0 + ch]`` of full-batch buffers,
# channel slices of concat buffers, buffers only partly written by design.

def _guard_workspace(m, monkeypatch):
    checks, ws = [], {}

    def _buf(key, shape, dtype=BF16):
        k = (getattr(m, "ws_tag", "") + key, tuple(shape), dtype)
        if k not in ws:
            ws[k], check = guarded(shape, dtype, DEV, name=key)
            checks.append(check)
        return ws[k]

    monkeypatch.setattr(m, "_buf", _buf)
    return checks


@pytest.fixture(scope="module")
def resnet(native):
    from aiko_services_amd.models.resnet50 import ResNet50
    m = ResNet50(seed=0, device=DEV)
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (3, 224, 224, 3), dtype=torch.uint8, generator=g).to(DEV)
    return m, frames, m.reference_logits(frames)


@pytest.mark.parametrize("flags", [
    {},                                                                     # the benchmarked path
    {"mall_chunk": 1},                                                      # stage 1 on batch-slice views
    {"stem_u8": False, "bneck": False, "mall_chunk": 1},                    # preprocess + stem_pool, patch / chain
    {"stem_u8": False, "fuse_stem_pool": False, "bneck": False, "chain": False, "exp3": False},   # one conv per launch
], ids=["default", "chunked", "chained", "unfused"])
def test_resnet50_on_guarded_workspace(resnet, monkeypatch, flags):
    m, frames, ref = resnet
    for k, v in flags.items():
        monkeypatch.setattr(m, k, v)
    m.release_workspace()
    plain = m.logits(frames).clone()
    torch.cuda.synchronize()
    checks = _guard_workspace(m, monkeypatch)
    guard = m.logits(frames)
    torch.cuda.synchronize()
    assert len(checks) > 4
    for c in checks:
        c()
    assert torch.isfinite(guard.float()).all()
    assert torch.equal(_bits(guard), _bits(plain))
    cos = F.cosine_similarity(plain.float(), ref, dim=1)
    assert cos.min().item() > 0.995, cos


@pytest.mark.parametrize("decode", [False, True])
def test_yolov8n_on_guarded_workspace(native, monkeypatch, decode):
    """YOLOv8-n's conv side (stem to head outputs, or to decoded boxes / scores / classes) on one
    480 x 640 frame; the upsampled half of l15's input buffer is never written and stays poison."""
    from aiko_services_amd.models import yolov8 as Y
    m = Y.YOLOv8("n", device=DEV, cls_bias=0.0)
    assert not decode or m._decode_fused_ok()
    g = torch.Generator().manual_seed(12)
    frames = torch.randint(0, 256, (1, 480, 640, 3), generator=g, dtype=torch.uint8).to(DEV)

    def run():
        if decode:
            return m.head_outputs(None, a0=m.stem_from_frames(frames), decode=True)
        return m.head_outputs(m.preprocess(frames))

    plain = [t.clone() for t in run()]
    torch.cuda.synchronize()
    checks = _guard_workspace(m, monkeypatch)
    guard = run()
    torch.cuda.synchronize()
    assert len(checks) > 10
    for c in checks:
        c()
    for p, t in zip(plain, guard):
        if t.dtype.is_floating_point:
            assert torch.isfinite(t.float()).all()
        assert torch.equal(_bits(p), _bits(t))
    if not decode:
        for o, r in zip(plain, m.reference_head_outputs(frames)):         # the bound of test_gpu_detect
            cos = F.cosine_similarity(_nchw(o).float().flatten(), r.flatten(), dim=0).item()
            assert cos > 0.99, cos
    else:
        from aiko_services_amd.ops import detect as DT
        feats = m.head_outputs(None, a0=m.stem_from_frames(frames))
        A = sum(f.shape[1] * f.shape[2] for f in feats)
        bd, sd, cd = DT.yolo_decode(feats, Y.STRIDES, m.nc_pad, boxes=torch.empty(1, A, 4, device=DEV),
                                    scores=torch.empty(1, A, device=DEV),
                                    cls=torch.empty(1, A, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        assert torch.equal(plain[2], cd) and torch.equal(plain[1], sd)
        assert (plain[0] - bd).abs().max().item() < 1e-3 * bd.abs().max().item()
