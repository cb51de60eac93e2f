"""fp8 GEMM, LayerNorm/quantise, flash attention, log-mel and the Whisper encoder on MI355X
vs plain PyTorch fp32 references (BASELINE config 5)."""
import pytest
import torch
import torch.nn.functional as F

from guard_ops import ROW_BOUND, attn_split_plan, row_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.parametrize("tile", [(128, 128), (128, 64), (64, 64), (64, 128),
                                  (128, 128, 1), (128, 64, 1), (64, 64, 1), (64, 128, 1), (256, 128, 2), (256, 256, 3)])
@pytest.mark.parametrize("act", [0, 3])
def test_gemm_fp8(native, tile, act):
    from aiko_services_amd.ops import transformer as TR
    g = torch.Generator().manual_seed(1)
    M, N, K = 333, 384, 768
    x = torch.randn(M, K, generator=g)
    lin = TR.make_fp8_linear(torch.randn(N, K, generator=g) / 30, torch.randn(N, generator=g) * 0.1, DEV)
    xq, xs = TR.quantize_rows_ref(x)
    res = torch.randn(M, N, generator=g).to(DEV, torch.bfloat16)
    y = TR.linear_fp8(xq.to(DEV), xs.to(DEV), lin, residual=res, act=act, tile=tile)
    xd = xq.view(torch.float8_e4m3fn).float() * xs[:, None]
    ref = xd.to(DEV) @ lin.ref_weight.T.to(DEV) + lin.bias
    if act == 3:
        ref = F.gelu(ref)
    ref = ref + res.float()
    assert _rel(y, ref) < 5e-3
    assert row_err(y, ref) < ROW_BOUND


@pytest.mark.parametrize("M,N,K,act", [(333, 512, 768, 0), (333, 512, 768, 3), (3000, 2304, 768, 0),
                                       (21014, 3072, 768, 3), (700, 768, 3072, 0), (1, 256, 256, 0),
                                       (3000, 1024, 512, 1), (600, 256, 256, 2)])
def test_gemm_fp8_persistent(native, M, N, K, act):
    """Variant 4 (persistent 256 x 256, transposed product, register-direct epilogue): M tails,
    one and several tiles per workgroup (21014 x 3072: 996 tiles on the CUs), a single-row M,
    long K; rows past M untouched."""
    from aiko_services_amd.ops import transformer as TR
    g = torch.Generator().manual_seed(M + N + act)
    x = torch.randn(M, K, generator=g)
    lin = TR.make_fp8_linear(torch.randn(N, K, generator=g) / 30, torch.randn(N, generator=g) * 0.1, DEV)
    xq, xs = TR.quantize_rows_ref(x)
    out = torch.full((M + 3, N), 7.0, dtype=torch.bfloat16, device=DEV)
    TR.linear_fp8(xq.to(DEV), xs.to(DEV), lin, out=out[:M], act=act, tile=(256, 256, 4))
    ref = (xq.view(torch.float8_e4m3fn).float() * xs[:, None]).to(DEV) @ lin.ref_weight.T.to(DEV) + lin.bias
    ref = {0: ref, 1: F.relu(ref), 2: F.silu(ref), 3: F.gelu(ref)}[act]
    assert _rel(out[:M], ref) < 5e-3
    assert row_err(out[:M], ref) < ROW_BOUND
    assert bool((out[M:] == 7.0).all())


@pytest.mark.parametrize("M,N", [(300, 512), (5000, 3072)])
def test_gemm_fp8_persistent_mx_out(native, M, N):
    """Variant 4 with GELU + MX-fp8 output (the fc1 -> fc2 hand-off): block max over the four
    lane rows of a fragment pair (two permlane swaps), same E8M0 scales as the reference."""
    from aiko_services_amd.ops import transformer as TR
    g = torch.Generator().manual_seed(N + 5)
    K = 768
    lin = TR.make_fp8_linear(torch.randn(N, K, generator=g) / 20, torch.randn(N, generator=g) * 0.1, DEV)
    xq, xs = TR.quantize_rows_ref(torch.randn(M, K, generator=g))
    oq, osc = TR.mx_buffers(M, N, DEV)
    TR.linear_fp8(xq.to(DEV), xs.to(DEV), lin, act=TR.ACT_GELU, out_mx=(oq, osc), tile=(256, 256, 4))
    full = F.gelu((xq.view(torch.float8_e4m3fn).float() * xs[:, None]).to(DEV) @ lin.ref_weight.T.to(DEV) + lin.bias)
    rq, rsc = TR.mx_quantize_ref(full.cpu())
    got = TR.mx_dequant(oq.cpu(), osc.cpu())
    assert (osc.cpu()[:, :M] == rsc[:, :M]).float().mean() > 0.98
    assert _rel(got, full.cpu()) < 4e-2
    assert _rel(got, TR.mx_dequant(rq, rsc)) < 1e-2


def test_rownorm_quant(native):
    from aiko_services_amd.ops import transformer as TR
    g = torch.Generator().manual_seed(2)
    M, D = 100, 768
    big = torch.randn(M, 2 * D, generator=g).to(DEV, torch.bfloat16)
    x = big[:, D:]                                    # column slice, pitch 2D
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(D, generator=g)).to(DEV)
    out = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
    q = torch.empty(M, D, dtype=torch.uint8, device=DEV)
    qs = torch.empty(M, dtype=torch.float32, device=DEV)
    TR.rownorm(x, gamma, beta, 1e-5, out=out, q=q, qs=qs)
    ref = F.layer_norm(x.float(), (D,), gamma, beta, 1e-5)
    assert _rel(out, ref) < 5e-3
    assert row_err(out, ref) < ROW_BOUND
    rq, rs = TR.quantize_rows_ref(ref)
    assert torch.allclose(qs, rs.to(DEV), rtol=1e-5)
    deq = q.view(torch.float8_e4m3fn).float() * qs[:, None]
    rdeq = rq.to(DEV).view(torch.float8_e4m3fn).float() * rs.to(DEV)[:, None]
    assert _rel(deq, rdeq) < 2e-2
    assert (q == rq.to(DEV)).float().mean().item() > 0.97
    # quantise-only (no LayerNorm) on a 3072-wide row
    u = torch.randn(50, 3072, generator=g).to(DEV, torch.bfloat16)
    uq = torch.empty(50, 3072, dtype=torch.uint8, device=DEV)
    us = torch.empty(50, dtype=torch.float32, device=DEV)
    TR.rownorm(u, q=uq, qs=us)
    rq, rs = TR.quantize_rows_ref(u.float())
    assert torch.allclose(us, rs.to(DEV), rtol=1e-5)
    assert (uq == rq.to(DEV)).float().mean().item() > 0.97


@pytest.mark.parametrize("B,T,Tpad,H", [(2, 1500, 1501, 12), (3, 77, 80, 4)])
def test_flash_attention(native, B, T, Tpad, H):
    from aiko_services_amd.ops import transformer as TR
    g = torch.Generator().manual_seed(T)
    d = H * 64
    qkv = (torch.randn(B * Tpad, 3 * d, generator=g) * 1.5).to(DEV, torch.bfloat16)
    out = torch.zeros(B * Tpad, d, dtype=torch.bfloat16, device=DEV)
    TR.attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], out, B, H, T, Tpad, 0.125)
    x = qkv.float().view(B, Tpad, 3, H, 64)[:, :T]
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    ref = F.scaled_dot_product_attention(q, k, v, scale=0.125).transpose(1, 2).reshape(B, T, d)
    got = out.view(B, Tpad, d)[:, :T]
    assert _rel(got, ref) < 1e-2
    assert out.view(B, Tpad, d)[:, T:].abs().max().item() == 0


@pytest.mark.parametrize("case", ["growing", "negative", "spiky"])
def test_flash_attention_rescale_paths(native, case):
    """Data that drives the online softmax's rare branches (guide rule: bounded random data
    never takes them): per-query maxima that keep growing across key tiles (lazy rescale fires
    mid-sequence), scores far below zero everywhere (first-tile max, no underflow to l = 0),
    and isolated huge scores late in the sequence."""
    from aiko_services_amd.ops import transformer as TR
    g = torch.Generator().manual_seed(11)
    B, H, T, Tpad = 2, 3, 700, 704
    d = H * 64
    q = torch.randn(B, Tpad, H, 64, generator=g)
    k = torch.randn(B, Tpad, H, 64, generator=g)
    v = torch.randn(B, Tpad, H, 64, generator=g)
    if case == "growing":
        k = k * torch.linspace(0.2, 6.0, Tpad).view(1, Tpad, 1, 1)      # later keys score higher
        q = q * 2
    elif case == "negative":
        q = q.abs() * 4 + 4
        k = -(k.abs() * 4 + 4)                                          # every score << 0
    else:
        k[:, 650] = q[:, :, :, :].mean(dim=1) * 40                     # one dominant late key
    qkv = torch.cat([q, k, v], dim=2).reshape(B * Tpad, 3 * d).to(DEV, torch.bfloat16)   # [q | k | v] heads
    out = torch.zeros(B * Tpad, d, dtype=torch.bfloat16, device=DEV)
    TR.attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], out, B, H, T, Tpad, 0.125)
    x = qkv.float().view(B, Tpad, 3, H, 64)[:, :T]
    qq, kk, vv = (x[:, :, i].transpose(1, 2) for i in range(3))
    ref = F.scaled_dot_product_attention(qq, kk, vv, scale=0.125).transpose(1, 2).reshape(B, T, d)
    got = out.view(B, Tpad, d)[:, :T].float()
    assert torch.isfinite(got).all()
    assert _rel(got, ref) < 2e-2, _rel(got, ref)


@pytest.mark.parametrize("B,H,T,Tpad,scale_k", [(1, 8, 256, 256, 1.0), (16, 12, 1500, 1504, 1.0), (2, 4, 1000, 1024, 6.0)])
@pytest.mark.parametrize("pieces", [2, 4])
def test_flash_attention_split_tail(native, B, H, T, Tpad, scale_k, pieces, monkeypatch):
    """Split-KV tail (``work`` given): the items of a partial last round per XCD run as key-range
    pieces merged in-kernel by the last arriver.  Same result as the unsplit grid (within bf16
    rounding of the merge order) and the fp32 reference; the arrival counters re-arm, so
    repeated launches agree; keys scaled up (scale_k) so pieces see very different maxima."""
    from aiko_services_amd.ops import transformer as TR
    monkeypatch.setenv("AIKO_ATTN_SPLIT_S", str(pieces))       # opt-in (attention.hip)
    # the launcher falls back to the plain grid without a word when the items leave no partial last
    # round on this device's CUs: every assertion below would still hold, so say so here
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    r, sp, part_off = attn_split_plan(B, H, T, cus, pieces, work_bytes=TR.ATTN_WORKSPACE_BYTES)
    assert sp >= 2, f"the launcher would not split: r = {r} on {cus} CUs"
    g = torch.Generator().manual_seed(T + B)
    d = H * 64
    qkv = torch.randn(B * Tpad, 3 * d, generator=g) * 1.5
    qkv.view(B, Tpad, 3, H, 64)[:, :, 1] *= torch.linspace(0.3, scale_k, Tpad).view(1, Tpad, 1, 1)
    qkv = qkv.to(DEV, torch.bfloat16)
    plain = torch.zeros(B * Tpad, d, dtype=torch.bfloat16, device=DEV)
    TR.attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], plain, B, H, T, Tpad, 0.125)   # no workspace
    ws = TR.attention_workspace(DEV)
    outs = []
    for _ in range(3):
        o = torch.zeros(B * Tpad, d, dtype=torch.bfloat16, device=DEV)
        TR.attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], o, B, H, T, Tpad, 0.125, work=ws)
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    cnt = ws[:8 * r].view(torch.int32)                      # the 8 x r arrival counters
    assert cnt.abs().max().item() == 0                       # counters re-armed
    assert ws[part_off // 4:].abs().max().item() > 0         # the split ran: partials were written
    x = qkv.float().view(B, Tpad, 3, H, 64)[:, :T]
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    ref = F.scaled_dot_product_attention(q, k, v, scale=0.125).transpose(1, 2).reshape(B, T, d)
    got = outs[0].view(B, Tpad, d)[:, :T]
    assert _rel(got, ref) < 1e-2
    assert _rel(got, plain.view(B, Tpad, d)[:, :T].float()) < 1e-2
    if Tpad > T:
        assert outs[0].view(B, Tpad, d)[:, T:].abs().max().item() == 0


def test_flash_attention_pingpong_identical(native, monkeypatch):
    """Variant 15 (the two query tiles ping-ponged: tile 0's PV MFMAs issued before tile 1's
    softmax) runs the same operations per accumulator in the same order as the default softmax:
    bit-identical output, ragged last tile and the lazy-rescale path included."""
    from aiko_services_amd.ops import transformer as TR
    g = torch.Generator().manual_seed(5)
    B, H, T, Tpad = 2, 3, 1000, 1024
    d = H * 64
    qkv = torch.randn(B * Tpad, 3 * d, generator=g) * 1.5
    qkv.view(B, Tpad, 3, H, 64)[:, :, 1] *= torch.linspace(0.3, 6.0, Tpad).view(1, Tpad, 1, 1)
    qkv = qkv.to(DEV, torch.bfloat16)
    outs = []
    for variant in ("0", "15"):
        monkeypatch.setenv("AIKO_ATTN_VARIANT", variant)
        o = torch.zeros(B * Tpad, d, dtype=torch.bfloat16, device=DEV)
        TR.attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], o, B, H, T, Tpad, 0.125)
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])


def test_log_mel(native):
    from aiko_services_amd.ops import audio as AU
    g = torch.Generator().manual_seed(3)
    B, N = 2, 16000 * 5
    t = torch.arange(N) / 16000
    audio = (0.3 * torch.sin(2 * torch.pi * 440 * t) + 0.05 * torch.randn(B, N, generator=g)).float()
    filters = AU.mel_filters().to(DEV)
    F_ = N // AU.HOP
    rows = F_ + 2
    out = torch.full((B * rows, 80), 7.0, dtype=torch.bfloat16, device=DEV)
    AU.log_mel(audio.to(DEV), filters, out, rows, 1, frames=F_)
    ref = AU.log_mel_ref(audio.to(DEV), filters, frames=F_)         # [B, 80, F]
    got = out.view(B, rows, 80)
    assert (got[:, 0] == 0).all() and (got[:, -1] == 0).all()
    assert (got[:, 1:-1].float().transpose(1, 2) - ref).abs().max().item() < 2e-2


@pytest.mark.parametrize("pad,ld", [(1, 80), (3, 88), (2, 96)])
def test_log_mel_finalize8_matches_scalar(native, monkeypatch, pad, ld):
    """The 8-mels-per-thread finalize kernel is bit-identical to the scalar one, with conv
    padding rows (pad > 0, tail rows) and a padded row pitch."""
    from aiko_services_amd.ops import audio as AU
    g = torch.Generator().manual_seed(5)
    B, N = 3, 16000 * 2
    audio = (0.2 * torch.randn(B, N, generator=g)).float().to(DEV)
    filters = AU.mel_filters().to(DEV)
    F_ = N // AU.HOP
    rows = F_ + pad + 2
    outs = []
    for scalar in ("0", "1"):
        monkeypatch.setenv("AIKO_LOGMEL_SCALAR", scalar)
        big = torch.full((B * rows, ld), 9.0, dtype=torch.bfloat16, device=DEV)
        AU.log_mel(audio, filters, big[:, :80], rows, pad, frames=F_)
        outs.append(big)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    got = outs[0].view(B, rows, ld)
    assert (got[:, :pad, :80] == 0).all() and (got[:, pad + F_:, :80] == 0).all()
    assert (got[..., 80:] == 9.0).all()                 # the pitch padding is never written


def test_whisper_tiny_matches_reference(native):
    from aiko_services_amd.models.whisper import WhisperEncoder
    enc = WhisperEncoder("tiny", device=DEV)
    g = torch.Generator().manual_seed(4)
    audio = (0.1 * torch.randn(2, 16000 * 4, generator=g)).to(DEV)
    y = enc.encode(audio)
    ref = enc.reference_encode(audio)
    assert y.shape == ref.shape == (2, 200, 384)
    cos = F.cosine_similarity(y.float().flatten(), ref.flatten(), dim=0).item()
    assert cos > 0.99, cos


def test_whisper_small_matches_reference_at_bench_shape(native):
    """the PRODUCTION encoder (Whisper-small, 30 s windows) at the config-5
    bench's shape — 14 windows per batch, so the tuner picks what the bench runs (fp8 GEMM
    variants 4/5 with MX-fp8 A operand + residual, MX-fp8 attention output, persistent rownorm)
    — against the fp32 PyTorch reference of the same weights: cosine > 0.99 for every window."""
    from aiko_services_amd.models.whisper import WhisperEncoder
    enc = WhisperEncoder("small", device=DEV)
    g = torch.Generator().manual_seed(11)
    amp = torch.linspace(0.02, 0.3, 14).unsqueeze(1)             # a range of signal levels
    audio = (amp * torch.randn(14, 480000, generator=g)).to(DEV)
    y = enc.encode(audio)
    torch.cuda.synchronize()
    ref = enc.reference_encode(audio)
    assert y.shape == ref.shape == (14, 1500, 768)
    cos = F.cosine_similarity(y.float().flatten(1), ref.flatten(1), dim=1)
    assert bool((cos > 0.99).all()), cos.tolist()


def test_whisper_small_30s(native):
    from aiko_services_amd.models.whisper import WhisperEncoder
    enc = WhisperEncoder("small", device=DEV)
    audio = (0.1 * torch.randn(1, 480000)).to(DEV)
    y = enc.encode(audio)
    torch.cuda.synchronize()
    assert y.shape == (1, 1500, 768)
    assert torch.isfinite(y.float()).all()


@pytest.mark.parametrize("tile", [(128, 128, 1), (64, 128, 1), (256, 256, 3)])
def test_gemm_fp8_mx_in_and_out(native, tile):
    """MX-fp8 activations: E8M0 block scales straight into the scaled MFMA (A side), and an
    epilogue that quantises GELU(out) to MX-fp8 (fc1 -> fc2 without a bf16 round trip); the
    128-wide LDS-DMA tiles and the 256 x 256 8-wave tile."""
    from aiko_services_amd.ops import transformer as TR
    g = torch.Generator().manual_seed(5)
    M, N, K = 300, 512, 512
    lin = TR.make_fp8_linear(torch.randn(N, K, generator=g) / 20, torch.randn(N, generator=g) * 0.1, DEV)
    # A side: MX-quantised input with a wide dynamic range across blocks
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-6, 6, (M, K // 32), generator=g).float()
                                                    ).repeat_interleave(32, dim=1)
    q, sc = TR.mx_quantize_ref(x)
    y = TR.linear_fp8(q.to(DEV), None, lin, x_mx=sc.to(DEV), tile=tile)
    ref = TR.mx_dequant(q, sc).to(DEV) @ lin.ref_weight.T.to(DEV) + lin.bias
    assert _rel(y, ref) < 5e-3
    assert row_err(y, ref) < ROW_BOUND
    # output side: GELU then MX quantisation in the epilogue
    xq, xs = TR.quantize_rows_ref(torch.randn(M, K, generator=g))
    oq, osc = TR.mx_buffers(M, N, DEV)
    TR.linear_fp8(xq.to(DEV), xs.to(DEV), lin, act=TR.ACT_GELU, out_mx=(oq, osc), tile=tile)
    full = F.gelu((xq.view(torch.float8_e4m3fn).float() * xs[:, None]).to(DEV) @ lin.ref_weight.T.to(DEV) + lin.bias)
    rq, rsc = TR.mx_quantize_ref(full.cpu())
    got = TR.mx_dequant(oq.cpu(), osc.cpu())
    assert (osc.cpu()[:, :M] == rsc[:, :M]).float().mean() > 0.98          # same E8M0 scales
    assert _rel(got, full.cpu()) < 4e-2                                    # fp8 rounding only
    assert _rel(got, TR.mx_dequant(rq, rsc)) < 1e-2


@pytest.mark.parametrize("B,T,Tpad,H,split", [(2, 1500, 1501, 12, 0), (3, 77, 80, 4, 0), (16, 1500, 1504, 12, 2)])
def test_flash_attention_mx_output(native, B, T, Tpad, H, split, monkeypatch):
    """Attention writing MX-fp8 directly (the out-projection's A operand; each head's 64
    columns = two E8M0 blocks quantised in the epilogue, split-KV merge included): the
    dequantised output matches the fp32 reference within e4m3 rounding, the scales equal a
    reference MX quantisation of the bf16 output path, and padding rows stay unwritten."""
    from aiko_services_amd.ops import transformer as TR
    if split:
        monkeypatch.setenv("AIKO_ATTN_SPLIT_S", str(split))
    g = torch.Generator().manual_seed(T + H)
    d = H * 64
    qkv = (torch.randn(B * Tpad, 3 * d, generator=g) * 1.5).to(DEV, torch.bfloat16)
    ws = TR.attention_workspace(DEV) if split else None
    out = torch.zeros(B * Tpad, d, dtype=torch.bfloat16, device=DEV)
    TR.attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], out, B, H, T, Tpad, 0.125, work=ws)
    aq, asc = TR.mx_buffers(B * Tpad, d, DEV)
    aq.fill_(0x7f)
    TR.attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], torch.empty_like(out), B, H, T, Tpad, 0.125,
                 work=ws, out_mx=(aq, asc))
    torch.cuda.synchronize()
    x = qkv.float().view(B, Tpad, 3, H, 64)[:, :T]
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    ref = F.scaled_dot_product_attention(q, k, v, scale=0.125).transpose(1, 2).reshape(B, T, d)
    got = TR.mx_dequant(aq.cpu(), asc.cpu()).view(B, Tpad, d)[:, :T].to(DEV)
    assert _rel(got, ref) < 4e-2, _rel(got, ref)
    rq, rsc = TR.mx_quantize_ref(out.float().cpu())
    valid = torch.zeros(B, Tpad, dtype=torch.bool)
    valid[:, :T] = True
    valid = valid.flatten()
    assert (asc.cpu()[:, :B * Tpad][:, valid] == rsc[:, :B * Tpad][:, valid]).float().mean() > 0.98
    assert (aq.view(B, Tpad, d)[:, T:] == 0x7f).all()                   # padding rows untouched


@pytest.mark.parametrize("tile", [(128, 256, 5), (256, 256, 4)])
@pytest.mark.parametrize("M,N,K", [(300, 768, 768), (2000, 768, 3072), (21014, 768, 768), (1, 256, 256)])
def test_gemm_fp8_persistent_128_mx_in_residual(native, M, N, K, tile):
    """Variant 5 (persistent 128 x 256, epilogue overlapped with the next tile): the out-projection
    / fc2 form — MX-fp8 activations (E8M0 scale tile DMA'd with each K block into the MFMA's B-side
    scale) plus a bf16 residual prefetched a fragment group ahead; M tails, one and several tiles
    per workgroup, rows past M untouched."""
    from aiko_services_amd.ops import transformer as TR
    g = torch.Generator().manual_seed(M + K)
    lin = TR.make_fp8_linear(torch.randn(N, K, generator=g) / 20, torch.randn(N, generator=g) * 0.1, DEV)
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-6, 6, (M, K // 32), generator=g).float()
                                                    ).repeat_interleave(32, dim=1)
    q, sc = TR.mx_quantize_ref(x)
    res = torch.randn(M, N, generator=g).to(DEV, torch.bfloat16)
    out = torch.full((M + 3, N), 7.0, dtype=torch.bfloat16, device=DEV)
    TR.linear_fp8(q.to(DEV), None, lin, out=out[:M], residual=res, x_mx=sc.to(DEV), tile=tile)
    ref = TR.mx_dequant(q, sc).to(DEV) @ lin.ref_weight.T.to(DEV) + lin.bias + res.float()
    assert _rel(out[:M], ref) < 5e-3
    assert row_err(out[:M], ref) < ROW_BOUND
    assert bool((out[M:] == 7.0).all())


@pytest.mark.parametrize("M,N,act,mxo", [(3000, 768, 0, False), (333, 2304, 3, False), (5000, 3072, 3, True)])
def test_gemm_fp8_persistent_128(native, M, N, act, mxo):
    """Variant 5 without MX input / residual: bf16 out (none / GELU) and GELU + MX-fp8 out."""
    from aiko_services_amd.ops import transformer as TR
    g = torch.Generator().manual_seed(N + act)
    K = 768
    lin = TR.make_fp8_linear(torch.randn(N, K, generator=g) / 20, torch.randn(N, generator=g) * 0.1, DEV)
    xq, xs = TR.quantize_rows_ref(torch.randn(M, K, generator=g))
    full = (xq.view(torch.float8_e4m3fn).float() * xs[:, None]).to(DEV) @ lin.ref_weight.T.to(DEV) + lin.bias
    if act == 3:
        full = F.gelu(full)
    if mxo:
        oq, osc = TR.mx_buffers(M, N, DEV)
        TR.linear_fp8(xq.to(DEV), xs.to(DEV), lin, act=act, out_mx=(oq, osc), tile=(128, 256, 5))
        rq, rsc = TR.mx_quantize_ref(full.cpu())
        assert (osc.cpu()[:, :M] == rsc[:, :M]).float().mean() > 0.98
        assert _rel(TR.mx_dequant(oq.cpu(), osc.cpu()), TR.mx_dequant(rq, rsc)) < 1e-2
    else:
        y = TR.linear_fp8(xq.to(DEV), xs.to(DEV), lin, act=act, tile=(128, 256, 5))
        assert _rel(y, full) < 5e-3
        assert row_err(y, full) < ROW_BOUND
