"""Guard-band, poison and per-row parity runs of the Whisper path (run on MI355X: -m gpu): the fp8
GEMM and row-norm kernels of gemm_fp8.hip, attention.hip and the log-mel kernels of audio_ops.hip.

Every case follows ``guard_ops.run_both``: the kernel runs *plain*, on fresh tensors, and
*guarded*, with every tensor the binding receives a view between two poison guards the test owns
(NaN for bf16 / fp32, ``0xFF`` — NaN as e4m3fn and as an E8M0 scale — for fp8 storage), column
gaps and padding rows holding the same poison.  Then, in this order: every guard is bit-identical
to its saved copy; the guarded output is finite; it is bit-identical to the plain output (no
floating-point atomics, the tile is forced); the numeric bound holds.

The numeric bound of a bf16 output is per row, ``row_err < 2^-8``: the kernel and the fp64
reference start from the same dequantised operands, a bf16 output is one rounding of an fp32 value
(at most 2^-8 of an element, about 2^-9 of a row's norm), fp32 summation order over K <= 3072 and
the erf approximation (1.5e-7) are orders below that; 2^-8 leaves a factor 2 over a clean row.  MX and fp8 outputs keep the scale-equality
shares (> 0.98, > 0.97) and dequantised bounds of tests/test_gpu_transformer.py, applied to every
block of 128 rows instead of once.  Attention and log-mel keep their bounds (1e-2 of the tensor's
norm, 2e-2 max-abs per clip).

Every case asserts the property that makes it an edge case (a partial tile, more tiles than CUs,
the kernel its D selects, ...), so a case cannot go stale silently.  Each kernel family has a
liveness control: poison *inside* the valid range makes exactly the affected rows non-finite.
"""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from guard_ops import BF16, DEV, NAN, ROW_BOUND, Operands, _bits, attn_split_plan, rel_err, row_err, run_both  # noqa: F401
from kernel_guard import BYTE_NAN, guarded

pytestmark = pytest.mark.gpu

SENT = 0x5A                      # sentinel byte of output regions no kernel may write
FP8 = torch.float8_e4m3fn


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _up(v, m):
    return -(-v // m) * m


def _blocks(M):
    return [(m0, min(m0 + 128, M)) for m0 in range(0, M, 128)]


# ---- fp8 GEMM --------------------------------------------------------------------------------------

def _act64(v, act):
    if act == 1:
        return F.relu(v)
    if act == 2:
        return F.silu(v)
    if act == 3:
        return F.gelu(v)
    return v


def _gemm_data(TR, M, N, K, mx_in, res, seed):
    """CPU operands and the fp64 reference of the pre-activation product (on the device)."""
    g = torch.Generator().manual_seed(seed)
    lin = TR.make_fp8_linear(torch.randn(N, K, generator=g) / 30, torch.randn(N, generator=g) * 0.1, DEV)
    if mx_in:                                        # a wide dynamic range across the 32-wide blocks
        x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-6, 6, (M, K // 32), generator=g).float()
                                                        ).repeat_interleave(32, dim=1)
        aq, asc = TR.mx_quantize_ref(x)
        xs, xd = None, TR.mx_dequant(aq, asc)
    else:
        aq, xs = TR.quantize_rows_ref(torch.randn(M, K, generator=g))
        asc, xd = None, aq.view(FP8).float() * xs[:, None]
    r = torch.randn(M, N, generator=g).to(BF16) if res else None
    pre = xd.double().to(DEV) @ lin.ref_weight.double().to(DEV).T + lin.bias.double()
    return lin, aq, xs, asc, r, pre


def _gemm_launch(TR, ops, lin, aq, xs, asc, r, M, N, K, tile, act, mx_out):
    """One launch on ``ops``' tensors: A as the byte-column slice [128, 128 + K) of a wider buffer
    (``lda > K``), ``sa`` five entries longer than M, MX input scale rows past M poisoned, residual
    and output as column slices of wider NaN buffers, an MX output's pitch gap and scale rows
    past M prefilled with a sentinel."""
    a = ops.inp_slice(aq, K + 256, 128, "A")
    assert a.stride(0) > K
    sa = amx = None
    rows = _up(M, 128)
    if asc is not None:
        sc = asc.clone()
        assert sc.shape == (K // 128, rows, 4)
        sc[:, M:] = ops.byte_gap if ops.on else 127
        amx = ops.inp(sc, "A scales")
    else:
        sa = ops.inp(torch.cat([xs, torch.full((5,), ops.gap)]), "sa")
    res = None if r is None else ops.inp_slice(r, N + 24, 16, "residual")
    w = lin if not ops.on else dataclasses.replace(lin, weight=ops.inp(lin.weight, "W"), scale=ops.inp(lin.scale, "sb"),
                                                   bias=ops.inp(lin.bias, "bias"))
    if mx_out:
        yq_w = ops.inp(torch.full((M, N + 32), SENT, dtype=torch.uint8), "yq")
        ysc = ops.inp(torch.full((N // 128, rows + 128, 4), SENT, dtype=torch.uint8), "ysc")
        TR.linear_fp8(a, sa, w, act=act, tile=tile, x_mx=amx, out_mx=(yq_w[:, 16:16 + N], ysc))
        torch.cuda.synchronize()
        assert (yq_w[:, :16] == SENT).all() and (yq_w[:, 16 + N:] == SENT).all(), "wrote into yq's pitch gap"
        assert (ysc[:, M:] == SENT).all(), "wrote a scale row >= M"
        return yq_w, ysc
    cat = ops.out((M, 32 + N + 16), name="y")
    TR.linear_fp8(a, sa, w, out=cat[:, 32:32 + N], residual=res, act=act, tile=tile, x_mx=amx)
    torch.cuda.synchronize()
    assert torch.isnan(cat[:, :32].float()).all() and torch.isnan(cat[:, 32 + N:].float()).all(), \
        "wrote outside the output's column slice"
    return cat[:, 32:32 + N]


def _check_mx_out(TR, yq_w, ysc, full, M, N):
    """The MX-output checks of test_gpu_transformer.py, per block of 128 rows."""
    yq, ysc = yq_w[:, 16:16 + N].cpu().contiguous(), ysc.cpu()
    full = full.float().cpu()
    rq, rsc = TR.mx_quantize_ref(full)
    got, want = TR.mx_dequant(yq, ysc), TR.mx_dequant(rq, rsc)
    assert torch.isfinite(got).all()
    for m0, m1 in _blocks(M):
        share = (ysc[:, m0:m1] == rsc[:, m0:m1]).float().mean().item()
        e_full, e_q = rel_err(got[m0:m1], full[m0:m1]), rel_err(got[m0:m1], want[m0:m1])
        print(f"rows {m0}-{m1}: scale share {share:.4f} rel(full) {e_full:.3e} rel(quantised ref) {e_q:.3e}")
        assert share > 0.98, (m0, share)
        assert e_full < 4e-2, (m0, e_full)
        assert e_q < 1e-2, (m0, e_q)


def _gemm_case(TR, M, N, K, tile, act=0, res=False, mx_in=False, mx_out=False, seed=0):
    lin, aq, xs, asc, r, pre = _gemm_data(TR, M, N, K, mx_in, res, seed)
    out = run_both(lambda ops: _gemm_launch(TR, ops, lin, aq, xs, asc, r, M, N, K, tile, act, mx_out), byte_nan=True)
    full = _act64(pre, act)
    if mx_out:
        _check_mx_out(TR, out[0], out[1], full, M, N)
        return
    ref = full if r is None else full + r.double().to(DEV)
    e_row, e_all = row_err(out, ref), rel_err(out, ref)
    print(f"M={M} N={N} K={K} tile={tile}: row_err {e_row:.3e} (bound {ROW_BOUND:.3e}) rel {e_all:.3e}")
    assert e_all < 5e-3, e_all
    assert e_row < ROW_BOUND, e_row


_T01 = [(64, 64), (128, 128), (128, 64), (64, 128)]
GEMM_SMALL = [(t + ((v,) if v else ()), K) for v in (0, 1) for t in _T01 for K in (256, 384)]


@pytest.mark.parametrize("tile,K", GEMM_SMALL, ids=[f"v{t[2] if len(t) > 2 else 0}-{t[0]}x{t[1]}-k{K}" for t, K in GEMM_SMALL])
def test_gemm_fp8_small_tiles_guarded(native, tile, K):
    """Variants 0 / 1, M = 77 x N = 200: an M tail and an N tail on every tile size, two and
    three 128-wide K chunks; K = 256 with no activation, K = 384 with GELU; both with a residual."""
    from aiko_services_amd.ops import transformer as TR
    M, N = 77, 200
    assert M % tile[0] != 0 and N % tile[1] != 0 and N % 8 == 0 and K // 128 in (2, 3)
    _gemm_case(TR, M, N, K, tile, act=3 if K == 384 else 0, res=True, seed=K + tile[0])


# (tile, M, N, K, act, res, mx_in, mx_out)
GEMM_BIG = [
    ((256, 128, 2), 300, 384, 256, 0, True, False, False), ((256, 128, 2), 300, 384, 384, 3, True, False, False),
    ((256, 256, 3), 300, 512, 256, 0, True, False, False), ((256, 256, 3), 300, 512, 384, 2, False, False, False),
    ((256, 256, 3), 300, 512, 384, 0, True, True, False), ((256, 256, 3), 300, 512, 256, 3, False, False, True),
    ((256, 256, 4), 300, 512, 256, 0, False, False, False), ((256, 256, 4), 300, 512, 384, 1, False, False, False),
    ((256, 256, 4), 300, 512, 384, 2, False, False, False), ((256, 256, 4), 300, 512, 256, 3, False, False, True),
    ((256, 256, 4), 300, 512, 384, 0, True, True, False),
    # variant 5: the launcher's four forms
    ((128, 256, 5), 300, 512, 256, 0, False, False, False), ((128, 256, 5), 300, 512, 384, 3, False, False, False),
    ((128, 256, 5), 300, 512, 384, 3, False, False, True), ((128, 256, 5), 300, 512, 256, 0, True, True, False),
    # MX in / out on the 128-wide LDS-DMA tiles (variant 1)
    ((128, 128, 1), 77, 256, 384, 0, True, True, False), ((64, 128, 1), 77, 256, 256, 3, False, False, True),
    # M = 1 on every kernel
    ((64, 64), 1, 200, 256, 0, True, False, False), ((128, 128, 1), 1, 200, 256, 3, True, False, False),
    ((256, 128, 2), 1, 384, 256, 0, True, False, False), ((256, 256, 3), 1, 512, 256, 0, True, False, False),
    ((256, 256, 4), 1, 512, 256, 3, False, False, False), ((128, 256, 5), 1, 512, 256, 0, True, True, False),
]


def _big_id(p):
    tile, M, N, K, act, res, mx_in, mx_out = p
    return f"v{tile[2] if len(tile) > 2 else 0}-{tile[0]}x{tile[1]}-{M}x{N}x{K}-a{act}" + \
        ("-res" if res else "") + ("-mxin" if mx_in else "") + ("-mxout" if mx_out else "")


@pytest.mark.parametrize("p", GEMM_BIG, ids=[_big_id(p) for p in GEMM_BIG])
def test_gemm_fp8_guarded(native, p):
    """Variants 2 - 5 (and the MX forms of variant 1) at M = 300 (a partial last tile on 64, 128
    and 256 rows) and M = 1, K = 256 / 384, with the operand layout of ``_gemm_launch``."""
    from aiko_services_amd.ops import transformer as TR
    tile, M, N, K, act, res, mx_in, mx_out = p
    assert M % tile[0] != 0 and K // 128 in (2, 3)
    _gemm_case(TR, M, N, K, tile, act=act, res=res, mx_in=mx_in, mx_out=mx_out, seed=M + N + K + act)


@pytest.mark.parametrize("tile,M", [((256, 256, 4), 5500), ((128, 256, 5), 2800)], ids=["v4-5500", "v5-2800"])
def test_gemm_fp8_persistent_walk_guarded(native, tile, M):
    """The persistent kernels with more tiles than workgroups (N = 3072, K = 256: 22 x 12 = 264
    tiles on the CUs), so some workgroups walk a second tile, the last one ending on the M tail."""
    from aiko_services_amd.ops import transformer as TR
    N, K = 3072, 256
    ntiles = -(-M // tile[0]) * (N // tile[1])
    assert ntiles > _cus(), f"{ntiles} tiles on {_cus()} CUs: one tile per workgroup"
    assert M % tile[0] != 0
    _gemm_case(TR, M, N, K, tile, act=3, seed=M)


@pytest.mark.parametrize("tile,kw", [
    ((128, 256, 5), dict(act=1)),                       # variant 5 has no ReLU / SiLU instantiation
    ((128, 256, 5), dict(res=True)),                    # variants 4 / 5: a residual only with MX input
    ((256, 256, 4), dict(res=True)),
    ((256, 256, 4), dict(mx_in=True)),                  # ... and MX input only with a residual
    ((256, 256, 4), dict(K=128)),                       # K < 256
    ((128, 256, 5), dict(K=128)),
    ((256, 256, 4), dict(N=384)),                       # N % 256 != 0
    ((256, 64, 2), dict()),                             # variant 2 is 256 x 128 only
], ids=["v5-relu", "v5-res", "v4-res", "v4-mxin-nores", "v4-k128", "v5-k128", "v4-n384", "v2-bn64"])
def test_gemm_fp8_launcher_refusals(native, tile, kw):
    """Shapes and forms the launcher refuses are errors, not silent fall-backs; nothing is written."""
    from aiko_services_amd.ops import transformer as TR
    M, N, K = 77, kw.get("N", 512), kw.get("K", 256)
    lin, aq, xs, asc, r, _ = _gemm_data(TR, M, N, K, kw.get("mx_in", False), kw.get("res", False), 1)
    out = torch.full((M, N), NAN, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported configuration"):
        TR.linear_fp8(aq.to(DEV), None if xs is None else xs.to(DEV), lin, out=out,
                      residual=None if r is None else r.to(DEV), act=kw.get("act", 0), tile=tile,
                      x_mx=None if asc is None else asc.to(DEV))
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()


@pytest.mark.parametrize("tile", [(64, 64), (64, 64, 1), (256, 128, 2), (256, 256, 3), (256, 256, 4), (128, 256, 5)],
                         ids=lambda t: f"v{t[2] if len(t) > 2 else 0}")
def test_gemm_fp8_poison_is_live(native, tile):
    """Liveness control, one per kernel: a single ``0xFF`` byte (e4m3 NaN) inside the valid K range
    of one A row — a normal launch on valid memory — makes exactly that output row non-finite.
    A kernel that multiplied in a poisoned byte of a gap, a guard or a row past M could not pass
    the finite check of the guarded cases."""
    from aiko_services_amd.ops import transformer as TR
    M, N, K, row = 77, 256, 256, 41
    lin, aq, xs, _, _, _ = _gemm_data(TR, M, N, K, False, False, 3)
    aq = aq.clone()
    aq[row, 200] = BYTE_NAN
    y = TR.linear_fp8(aq.to(DEV), xs.to(DEV), lin, tile=tile)
    torch.cuda.synchronize()
    bad = ~torch.isfinite(y.float()).all(dim=1)
    assert bad.nonzero().flatten().tolist() == [row]
    assert not torch.isfinite(y[row].float()).any()


# ---- row-norm ----------------------------------------------------------------------------------------

def _rownorm_x(M, D, g):
    x = torch.randn(M, D, generator=g) * torch.exp2(torch.randint(-2, 4, (M, 1), generator=g).float()) + \
        0.5 * torch.randn(M, 1, generator=g)
    if M >= 3:
        x[1] = 0.0                      # an all-zero row: LayerNorm gives beta, quantise-only scale 1
        x[2] = 0.5                      # a constant row: zero variance, rstd = eps^-1/2
    return x.to(BF16)


def _rownorm_case(TR, M, D, mode, seed):
    """mode "ln": LayerNorm writing bf16, e4m3 and scales in one pass; "ln_q": LayerNorm writing
    e4m3 + scales only (the model's LN1 / LN2); "ln_y": bf16 only (ln_post); "quant":
    quantise-only.  x is a column slice of a NaN buffer, yb and q go into slices with a padded
    pitch, qs is seven entries longer than M."""
    g = torch.Generator().manual_seed(seed)
    x = _rownorm_x(M, D, g)
    ln = mode != "quant"
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    want_y, want_q = mode in ("ln", "ln_y"), mode != "ln_y"

    def case(ops):
        xs = ops.inp_slice(x, D + 24, 8, "x")
        assert xs.stride(0) > D
        gb = (ops.inp(gamma, "gamma"), ops.inp(beta, "beta")) if ln else (None, None)
        outs = []
        yb = q = qs = None
        if want_y:
            cat = ops.out((M, D + 16), name="yb")
            yb = cat[:, 8:8 + D]
        if want_q:
            q_w = ops.inp(torch.full((M, _up(D + 32, 16)), SENT, dtype=torch.uint8), "q")
            q = q_w[:, 16:16 + D]
            qs = ops.inp(torch.full((M + 7,), 7.0), "qs")
        TR.rownorm(xs, gb[0], gb[1], 1e-5, out=yb, q=q, qs=qs)
        torch.cuda.synchronize()
        if want_y:
            assert torch.isnan(cat[:, :8].float()).all() and torch.isnan(cat[:, 8 + D:].float()).all(), \
                "wrote outside yb's column slice"
            outs.append(yb)
        if want_q:
            assert (q_w[:, :16] == SENT).all() and (q_w[:, 16 + D:] == SENT).all(), "wrote into q's pitch gap"
            assert (qs[M:] == 7.0).all(), "wrote a scale past row M"
            outs += [q, qs[:M]]
        return tuple(outs)

    outs = list(run_both(case, byte_nan=True))
    ref = x.double()
    if ln:
        ref = F.layer_norm(ref, (D,), gamma.double(), beta.double(), 1e-5)
    if want_y:
        e = row_err(outs.pop(0), ref.to(DEV))
        print(f"rownorm {M}x{D} {mode}: row_err {e:.3e} (bound {ROW_BOUND:.3e})")
        assert e < ROW_BOUND, e
    if want_q:
        q, qs = outs[0].cpu(), outs[1].cpu()
        rq, rs = TR.quantize_rows_ref(ref.float())
        assert torch.allclose(qs, rs, rtol=1e-5, atol=0), (qs - rs).abs().max()
        if M >= 3 and not ln:
            assert qs[1].item() == 1.0 and (q[1] == 0).all()            # the all-zero row: scale 1
        deq = q.view(FP8).float() * qs[:, None]
        rdeq = rq.view(FP8).float() * rs[:, None]
        assert torch.isfinite(deq).all()
        for m0, m1 in _blocks(M):
            share = (q[m0:m1] == rq[m0:m1]).float().mean().item()
            e = rel_err(deq[m0:m1], rdeq[m0:m1])
            assert share > 0.97, (m0, share)
            assert e < 2e-2, (m0, e)


ROWNORM = [(101, 384), (101, 776), (5, 1024), (5, 1032), (7, 1280), (3, 8192), (1, 768)]


@pytest.mark.parametrize("mode", ["ln", "ln_q", "ln_y", "quant"])
@pytest.mark.parametrize("M,D", ROWNORM, ids=[f"{m}x{d}" for m, d in ROWNORM])
def test_rownorm_guarded(native, M, D, mode):
    """Every kernel aiko_rownorm_quant selects by D, with the chunk counts no other test has."""
    from aiko_services_amd.ops import transformer as TR
    nchunk = D // 8
    if (M, D) == (101, 384):          # persistent <3>: lanes 0-15 hold two chunks, 16-31 one; odd M: a dead half
        assert D <= 768 and 32 < nchunk < 64 and M % 2 == 1
    elif (M, D) == (101, 776):        # <2>: the second 64-lane pass is partial
        assert 768 < D <= 1024 and 64 < nchunk < 128
    elif (M, D) == (5, 1024):         # <2>: both passes full
        assert nchunk == 128
    elif (M, D) == (5, 1032):         # the first D of <6>, one chunk in its third pass
        assert 1024 < D <= 3072 and nchunk == 129
    elif (M, D) == (7, 1280):         # <6>: Whisper-large's width
        assert 1024 < D <= 3072 and nchunk % 64 != 0
    elif (M, D) == (3, 8192):         # <16>, the widest row the binding accepts
        assert 3072 < D and nchunk == 64 * 16
    else:                             # persistent, one row: the second half of its wave is dead
        assert (M, D) == (1, 768)
    _rownorm_case(TR, M, D, mode, seed=M + D)


@pytest.mark.parametrize("mode", ["ln", "quant"])
def test_rownorm_persistent_walk_guarded(native, mode):
    """More row pairs than the persistent grid has waves (4 x 4 x CUs): every wave takes a second
    pair through the ``nxt -> cur`` prefetch, some a third, and the odd M ends on a dead half."""
    from aiko_services_amd.ops import transformer as TR
    cus = _cus()
    M, D = 2 * 16 * cus + 515, 768
    pairs = (M + 1) // 2
    assert pairs > 16 * cus and M % 2 == 1
    _rownorm_case(TR, M, D, mode, seed=5)


def test_rownorm_poison_is_live(native):
    """Liveness control: one NaN inside row 3 of x makes exactly that row of the LayerNorm output
    non-finite (persistent kernel, D = 768, and the <2> kernel, D = 1024)."""
    from aiko_services_amd.ops import transformer as TR
    for D in (768, 1024):
        g = torch.Generator().manual_seed(D)
        x = _rownorm_x(9, D, g)
        x[3, D - 5] = NAN
        gamma, beta = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
        y = torch.zeros(9, D, dtype=BF16, device=DEV)
        TR.rownorm(x.to(DEV), gamma, beta, 1e-5, out=y)
        torch.cuda.synchronize()
        bad = ~torch.isfinite(y.float()).all(dim=1)
        assert bad.nonzero().flatten().tolist() == [3], D


# ---- attention ---------------------------------------------------------------------------------------

ATTN_VARIANTS = list(range(0, 9)) + list(range(10, 16))
_ATTN_NW = {3: 4, 4: 4, 7: 4, 8: 4, 13: 4, 14: 4}              # 4-wave variants; the others have 8
_ATTN_SM = (0, 11, 12, 13, 14, 15)                              # variants whose softmax the split path supports
ATTN_SHAPES = [(2, 3, 77, 80), (2, 2, 257, 264), (1, 2, 64, 64)]


def _attn_qkv(B, H, T, Tpad, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B * Tpad, 3 * H * 64, generator=g) * 1.5).to(BF16)


def _attn_ref(qkv, B, H, T, Tpad):
    x = qkv.float().to(DEV).view(B, Tpad, 3, H, 64)[:, :T]
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    return F.scaled_dot_product_attention(q, k, v, scale=0.125).transpose(1, 2).reshape(B, T, H * 64)


def _attn_case(TR, B, H, T, Tpad, seed, mx=False, work_bytes=0, part_off=0):
    """q / k / v are column slices of one fused buffer; in the guarded run its rows T .. Tpad-1
    (every sequence's padding) are NaN and the output is prefilled with NaN (bf16) or ``0xFF``
    (MX), whose padding rows must come back bit for bit.  Returns the valid rows of the plain run."""
    d = H * 64
    qkv = _attn_qkv(B, H, T, Tpad, seed)

    def case(ops):
        vals = qkv.clone()
        if ops.on:
            vals.view(B, Tpad, 3 * d)[:, T:] = NAN
        t = ops.inp(vals, "qkv")
        work = ops.inp(torch.zeros(work_bytes // 4), "workspace") if work_bytes else None
        if ops.on:
            out = ops.out((B * Tpad, d), name="out")
        else:
            out = torch.zeros(B * Tpad, d, dtype=BF16, device=DEV)
        before = _bits(out).clone()
        out_mx = None
        if mx:
            rows = _up(B * Tpad, 128)
            oq = ops.inp(torch.full((B * Tpad, d), BYTE_NAN if ops.on else SENT, dtype=torch.uint8), "oq")
            osc = ops.inp(torch.full((d // 128, rows, 4), BYTE_NAN if ops.on else SENT, dtype=torch.uint8), "osc")
            out_mx, fill = (oq, osc), BYTE_NAN if ops.on else SENT
        TR.attention(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], out, B, H, T, Tpad, 0.125, work=work, out_mx=out_mx)
        torch.cuda.synchronize()
        if work is not None:
            assert work.view(torch.int32)[:part_off // 4].abs().max().item() == 0, "arrival counters not re-armed"
            assert work[part_off // 4:].abs().max().item() > 0, "the split path did not run: no partials written"
        if mx:
            assert torch.equal(_bits(out), before), "bf16 out written beside the MX output"
            assert (oq.view(B, Tpad, d)[:, T:] == fill).all(), "wrote a padding row of oq"
            pad = torch.ones(rows, dtype=torch.bool, device=DEV)
            pad[:B * Tpad].view(B, Tpad)[:, :T] = False
            assert (osc[:, pad] == fill).all(), "wrote a padding row of osc"
            return oq.view(B, Tpad, d)[:, :T], osc[:, ~pad]
        pad = _bits(out).view(B, Tpad, d)[:, T:]
        assert (pad == (0x7FC0 if ops.on else 0)).all(), "wrote a padding row of out"
        return out.view(B, Tpad, d)[:, :T]

    return qkv, run_both(case, byte_nan=True)


@pytest.mark.parametrize("B,H,T,Tpad", ATTN_SHAPES, ids=[f"{b}x{h}x{t}" for b, h, t, _ in ATTN_SHAPES])
@pytest.mark.parametrize("variant", ATTN_VARIANTS)
def test_attention_guarded(native, monkeypatch, variant, B, H, T, Tpad):
    """Every launcher variant (LDS-DMA ring / register staging, 8 / 4 waves, the three softmax
    forms) with NaN in every padding row of q, k and v: keys >= T must never be multiplied in —
    the DMA variants rely on the buffer descriptor returning zeros past T, the register-staged
    ones clamp to key T-1.  T = 77 and 257 end in a ragged key tile (and a ragged query block),
    T = 64 = Tpad is one exact tile whose successor is the guard."""
    from aiko_services_amd.ops import transformer as TR
    monkeypatch.setenv("AIKO_ATTN_VARIANT", str(variant))
    monkeypatch.delenv("AIKO_ATTN_SPLIT_S", raising=False)
    assert H > 1 and (T % 64 != 0 or T == Tpad)
    qkv, got = _attn_case(TR, B, H, T, Tpad, seed=T + variant)
    e = rel_err(got, _attn_ref(qkv, B, H, T, Tpad))
    assert e < 1e-2, e


@pytest.mark.parametrize("T,Tpad", [(1, 8), (63, 64), (65, 72)])
def test_attention_short_sequences_guarded(native, monkeypatch, T, Tpad):
    """Variant 0 at one key, one key short of a tile, and one key into the second tile."""
    from aiko_services_amd.ops import transformer as TR
    monkeypatch.delenv("AIKO_ATTN_VARIANT", raising=False)
    monkeypatch.delenv("AIKO_ATTN_SPLIT_S", raising=False)
    assert T in (1, 64 - 1, 64 + 1)
    qkv, got = _attn_case(TR, 2, 2, T, Tpad, seed=T)
    e = rel_err(got, _attn_ref(qkv, 2, 2, T, Tpad))
    assert e < 1e-2, e


@pytest.mark.parametrize("B,H,T,Tpad", [(2, 4, 77, 80), (2, 2, 257, 264), (1, 2, 64, 64)],
                         ids=["2x4x77", "2x2x257", "1x2x64"])
@pytest.mark.parametrize("variant", [0, 3, 7, 12, 15])
def test_attention_mx_output_guarded(native, monkeypatch, variant, B, H, T, Tpad):
    """The MX-fp8 epilogue (H * 64 must be a multiple of 128, so H = 4 at T = 77): padding rows of
    ``oq`` and ``osc`` unchanged, dequantised output within e4m3 rounding of the reference and the
    scales those of a reference MX quantisation of the bf16 output, as test_flash_attention_mx_output."""
    from aiko_services_amd.ops import transformer as TR
    monkeypatch.setenv("AIKO_ATTN_VARIANT", str(variant))
    monkeypatch.delenv("AIKO_ATTN_SPLIT_S", raising=False)
    d = H * 64
    assert d % 128 == 0
    qkv, (oq, osc) = _attn_case(TR, B, H, T, Tpad, seed=T + variant, mx=True)
    t = qkv.to(DEV)
    out = torch.zeros(B * Tpad, d, dtype=BF16, device=DEV)
    TR.attention(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], out, B, H, T, Tpad, 0.125)
    valid = out.view(B, Tpad, d)[:, :T].reshape(B * T, d).float().cpu()
    oq, osc = oq.reshape(B * T, d).cpu(), osc.cpu()
    sc = torch.full((d // 128, _up(B * T, 128), 4), 127, dtype=torch.uint8)
    sc[:, :B * T] = osc
    got = TR.mx_dequant(oq, sc)
    rq, rsc = TR.mx_quantize_ref(valid)
    assert torch.isfinite(got).all()
    e = rel_err(got, _attn_ref(qkv, B, H, T, Tpad).reshape(B * T, d).cpu())
    assert e < 4e-2, e
    for m0, m1 in _blocks(B * T):
        share = (osc[:, m0:m1] == rsc[:, m0:m1]).float().mean().item()
        assert share > 0.98, (m0, share)


@pytest.mark.parametrize("mx", [False, True], ids=["bf16", "mx"])
@pytest.mark.parametrize("variant,B,H,T,Tpad", [(0, 2, 4, 77, 80), (0, 2, 2, 257, 264), (15, 2, 2, 257, 264),
                                               (12, 2, 4, 257, 264), (13, 2, 4, 257, 264)])
def test_attention_split_guarded(native, monkeypatch, variant, B, H, T, Tpad, mx):
    """The split-KV tail (``AIKO_ATTN_SPLIT_S`` = 2 with a workspace) on poisoned padding rows and
    a guarded workspace.  The launcher falls back to the plain grid without a word when the items
    are not a multiple of 8 or leave no partial round on the device's CUs; this test computes what
    it will do and fails — it does not pass on the fallback — and then asserts that partials
    were written.  (B * H * query blocks is a multiple of 8 here, hence H = 4 at T = 77.)"""
    from aiko_services_amd.ops import transformer as TR
    monkeypatch.setenv("AIKO_ATTN_VARIANT", str(variant))
    monkeypatch.setenv("AIKO_ATTN_SPLIT_S", "2")
    assert variant in _ATTN_SM
    nw = _ATTN_NW.get(variant, 8)
    work_bytes = 4 << 20
    r, sp, part_off = attn_split_plan(B, H, T, _cus(), 2, nw, work_bytes)
    assert sp == 2, f"the launcher would fall back to the plain grid: r = {r} on {_cus()} CUs"
    qkv, got = _attn_case(TR, B, H, T, Tpad, seed=T + variant, mx=mx, work_bytes=work_bytes, part_off=part_off)
    if not mx:
        e = rel_err(got, _attn_ref(qkv, B, H, T, Tpad))
        assert e < 1e-2, e
    else:
        d = H * 64
        sc = torch.full((d // 128, _up(B * T, 128), 4), 127, dtype=torch.uint8)
        sc[:, :B * T] = got[1].cpu()
        deq = TR.mx_dequant(got[0].reshape(B * T, d).cpu(), sc)
        e = rel_err(deq, _attn_ref(qkv, B, H, T, Tpad).reshape(B * T, d).cpu())
        assert torch.isfinite(deq).all() and e < 4e-2, e


@pytest.mark.parametrize("variant", [0, 5, 3, 13])
def test_attention_poison_is_live(native, monkeypatch, variant):
    """Liveness control (DMA and register staging, 8 and 4 waves): NaN in the *valid* key row T-1
    of one (sequence, head) makes that head's outputs non-finite and leaves every other head
    finite — so a padded key that was multiplied in would show in the guarded cases."""
    from aiko_services_amd.ops import transformer as TR
    monkeypatch.setenv("AIKO_ATTN_VARIANT", str(variant))
    monkeypatch.delenv("AIKO_ATTN_SPLIT_S", raising=False)
    B, H, T, Tpad = 2, 3, 77, 80
    d = H * 64
    qkv = _attn_qkv(B, H, T, Tpad, 9)
    b, h = 1, 2
    qkv[b * Tpad + T - 1, d + h * 64:d + (h + 1) * 64] = NAN
    t = qkv.to(DEV)
    out = torch.zeros(B * Tpad, d, dtype=BF16, device=DEV)
    TR.attention(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], out, B, H, T, Tpad, 0.125)
    torch.cuda.synchronize()
    fin = torch.isfinite(out.float()).view(B, Tpad, H, 64)[:, :T]
    assert not fin[b, :, h].any()
    fin[b, :, h] = True
    assert fin.all()


# ---- log-mel ---------------------------------------------------------------------------------------------

def test_log_mel_guarded(native, monkeypatch):
    """A loud clip, digital silence and a nearly silent clip side by side: the ``max - 8`` floor
    (clip 0: a 0.5-amplitude tone that ends after 1.5 s, so its zero-padded tail sits on the
    floor), the 1e-10 clamp with a per-clip maximum of exactly -10 (clip 1) and a negative
    maximum whose integer key must order correctly (clip 2: 0.2 s of 1e-3 noise, then zeros).
    A per-clip maximum leaking across clips, or a reflect-padded frame at a clip's start reading
    its neighbour, would move the silent clip off -1.5.  The guards hold 1e4 instead of NaN:
    ``fmaxf(e, 1e-10)`` drops a NaN energy, which would make an over-read look like silence."""
    from aiko_services_amd.ops import audio as AU
    g = torch.Generator().manual_seed(6)
    B, N, pad, ld = 3, 32000, 2, 88
    t = torch.arange(N) / 16000
    audio = torch.zeros(B, N)
    audio[0, :24000] = 0.5 * torch.sin(2 * torch.pi * 440 * t[:24000])
    audio[2, :3200] = 1e-3 * torch.randn(3200, generator=g)
    filters = AU.mel_filters().to(DEV)
    F_ = N // AU.HOP
    rows = F_ + pad + 2
    assert F_ % 16 != 0                                  # the last workgroup of a clip has dead frames
    ref = AU.log_mel_ref(audio.to(DEV), filters, frames=F_)             # [B, 80, F]
    top = ref.amax(dim=(1, 2))

    def share(clip, value):
        return ((ref[clip] - value).abs() < 1e-5).float().mean().item()

    assert top[0] > 1.0 and share(0, top[0] - 2.0) > 0.2                 # the floor max - 8, above the clamp
    assert share(1, -1.5) == 1.0                                         # log10(1e-10) everywhere
    assert -1.4 < top[2] < 1.0 and share(2, -1.5) > 0.5                  # raw maximum < 0; most frames clamped

    def case(ops):
        big = ops.out((B * rows, ld), name="out")
        AU.log_mel(ops.inp(audio, "audio"), filters, big[:, :80], rows, pad,
                   work=ops.out((B * F_ * 80,), torch.float32, name="work"),
                   gmax=ops.inp(torch.zeros(B, dtype=torch.int32), "gmax"), frames=F_)
        torch.cuda.synchronize()
        assert torch.isnan(big[:, 80:].float()).all(), "wrote the pitch columns"
        return big[:, :80]

    outs = []
    for scalar in ("0", "1"):
        monkeypatch.setenv("AIKO_LOGMEL_SCALAR", scalar)
        outs.append(run_both(case, poison=1e4))
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))                  # both finalize kernels
    got = outs[0].view(B, rows, 80)
    assert (got[:, :pad] == 0).all() and (got[:, pad + F_:] == 0).all()
    y = got[:, pad:pad + F_].float().transpose(1, 2)
    for b in range(B):
        e = (y[b] - ref[b]).abs().max().item()
        assert e < 2e-2, (b, e)
    assert (y[1] == -1.5).all()


# ---- the whole encoder on a guarded workspace ------------------------------------------------------------

def test_whisper_tiny_on_guarded_workspace(native, monkeypatch):
    """Whisper-tiny on two 4 s clips with every workspace buffer a guarded view: ``_buf`` swapped
    (``zero=`` honoured), the two MX hand-offs (attention -> out-projection, fc1 -> fc2) guarded
    with ``0xFF`` interiors.  The attention epilogue never writes the spare token row of ``a8``,
    the out-projection reads it as e4m3 NaN and adds it into ``x``: from the first block on the
    spare rows of x, qkv, a8 and u8 are non-finite — what production sees whenever the allocator
    leaves 0x7F / 0xFF bytes there.  With B = 2, clip 0's spare row sits directly in front of
    clip 1's keys.  The output must not notice."""
    from aiko_services_amd.models.whisper import WhisperEncoder
    from aiko_services_amd.ops import transformer as TR
    enc = WhisperEncoder("tiny", device=DEV)
    g = torch.Generator().manual_seed(4)
    audio = (0.1 * torch.randn(2, 16000 * 4, generator=g)).to(DEV)
    B, T, d = 2, 200, 384
    plain = enc.encode(audio).clone()
    torch.cuda.synchronize()
    enc.release_workspace()
    checks, ws = [], {}

    def _buf(key, shape, dtype=BF16, zero=False):
        k = (key, tuple(shape), dtype)
        if k not in ws:
            ws[k], check = guarded(shape, dtype, DEV, fill=0 if zero else None, name=key)
            checks.append(check)
        return ws[k]

    def mx_buffers(M, K, device):
        q, c0 = guarded((M, K), torch.uint8, DEV, poison=BYTE_NAN, name=f"mx q {K}")
        sc, c1 = guarded((K // 128, _up(M, 128), 4), torch.uint8, DEV, poison=BYTE_NAN, name=f"mx sc {K}")
        assert (q == BYTE_NAN).all() and (sc == BYTE_NAN).all()
        checks.extend([c0, c1])
        return q, sc

    monkeypatch.setattr(enc, "_buf", _buf)
    monkeypatch.setattr(TR, "mx_buffers", mx_buffers)
    assert enc.mx_attention
    try:
        guard = enc.encode(audio)
        torch.cuda.synchronize()
    finally:
        enc.release_workspace()
    assert len(checks) > 10
    x = ws[("x", (B * (T + 1), d), BF16)].view(B, T + 1, d)
    assert not torch.isfinite(x[0, T].float()).all(), "precondition: the spare row of x is still finite"
    for c in checks:
        c()
    assert guard.shape == (B, T, d) and torch.isfinite(guard.float()).all()
    assert torch.equal(_bits(guard), _bits(plain))
    cos = F.cosine_similarity(plain.float().flatten(), enc.reference_encode(audio).flatten(), dim=0).item()
    assert cos > 0.99, cos
