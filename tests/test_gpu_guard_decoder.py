"""Guard-band, poison and per-row parity runs of the decoder step kernels of decode_ops.hip (run on
MI355X: -m gpu): embed_kernel, attn_decode_kernel + attn_decode_combine, the four instances of
dec_linear_kernel and argmax_step_kernel, then the whole Whisper-tiny decoder on a guarded
workspace.  The references, launch plans and case tables are tests/decoder_refs.py (checked on the
CPU by tests/test_decoder_refs.py).

Every case follows ``guard_ops.run_both``: a *plain* run on fresh tensors and a *guarded* run in
which every tensor the binding receives is a view between two poison guards, inputs and outputs are
column slices of wider buffers whose gaps hold poison (so every ``ld*`` argument is proven), and
outputs are prefilled with NaN.  Guards intact, guarded outputs finite and bit-identical to the
plain run, slack columns untouched; then the numeric check, per row:

* embed, argmax / step state and the KV cache contents are bit-exact;
* attention: each (sequence, head) row of 64 outputs has ``row_err < ROW_BOUND`` (2^-8) against
  the fp64 softmax of the bf16 operands.  Worst rows measured on MI355X: 1.7e-3 to 2.2e-3, the
  bf16 rounding of the output (``ATTN_WORST``);
* dec_linear without LayerNorm: planted rows (exact scale, exact e4m3 ties), every row below
  ``ROW_BOUND``; with LayerNorm: every row below ``flip_bound``, at most M // 8 rows at or above
  ``ROW_BOUND`` (the kernel's fp32 LayerNorm may land on the other side of an e4m3 boundary), and
  the unfused device path (rownorm + linear_fp8) is held to the same rule.

Each case asserts the property that makes it an edge (its split plan, its kernel instance, its tile
count), so it cannot go stale silently, and each family has liveness controls: poison *inside* the
valid range shows in exactly the affected outputs.

Two things a NaN does not do here, which shape the checks.  (1) ``argmax_step`` compares with
``>``, which drops a NaN, so its logits gap and guards hold a *finite* value above every logit
(3e30).  (2) ``dec_linear`` swallows a NaN in ``x``: the row maximum is an ``fmaxf`` chain and the
quantiser clamps with ``fminf(fmaxf(v, -448), 448)``, which turns NaN into a finite code (the
unfused ``rownorm`` quantiser behaves the same).  A NaN read from an x gap would therefore leave
the output finite; the x gaps are judged by bit-identity with the plain run, whose gaps hold
zero (a consumed NaN becomes ±448 and moves the row), and the liveness control for x is a finite
spike that must change exactly its own row.
"""
import functools

import pytest
import torch

import decoder_refs as R
from guard_ops import BF16, DEV, NAN, ROW_BOUND, _bits, row_errs, run_both
from kernel_guard import BYTE_NAN, guarded

pytestmark = pytest.mark.gpu

# worst (sequence, head) row of the attention cases as measured on MI355X (bound 2^-8 = 3.91e-3;
# documentation only).  One key gives 0: the output is the value row itself.
ATTN_WORST = {"cross 1x1x1": 0.0, "cross 2x2x255": 1.73e-3, "cross 2x2x256": 1.80e-3, "cross 2x2x257": 1.89e-3,
              "cross 2x2x600": 1.71e-3, "cross 16x8x300": 2.20e-3, "cross 13x8x1300": 2.15e-3,
              "append 2x4 pos 0": 0.0, "append 2x4 pos 5": 1.86e-3, "append 2x4 pos 255": 1.78e-3,
              "append 2x4 pos 256": 1.68e-3, "append 2x4 pos 300": 2.02e-3, "append 2x4 pos 447": 1.97e-3,
              "append 2x4 pos 448": 1.95e-3, "append 16x8 pos 0": 0.0, "append 16x8 pos 256": 2.15e-3,
              "append 16x8 pos 447": 2.07e-3}
# dec_linear on the same run: worst row 2.63e-3 without LayerNorm (16x1536x16, GELU) and 2.24e-3 with
# it (16x1024x32); no LayerNorm row reached ROW_BOUND, so no seed had to be changed, and the unfused
# path gave the same worst rows to three digits.


def _up(v, m):
    return -(-v // m) * m


def _nan_slack(cat, c0, n, what):
    assert torch.isnan(cat[:, :c0].float()).all() and torch.isnan(cat[:, c0 + n:].float()).all(), \
        f"wrote outside {what}'s column slice"


# ---- embed_tokens ----------------------------------------------------------------------------------

@pytest.mark.parametrize("pos", [0, 11, 14], ids=["pos0", "last", "past"])
@pytest.mark.parametrize("d", [8, 384, 1280])
def test_embed_tokens_guarded(native, d, pos):
    """d = 8: one live thread of 128; d = 384: 48; d = 1280: 160 chunks, so 32 threads take a
    second pass.  Ids below 0 and past the vocabulary and a position past the table clamp."""
    vocab, n_pos, B = 50, 12, 4
    assert pos in (0, n_pos - 1, n_pos + 2) and (d != 1280 or d // 8 > 128)
    g = torch.Generator().manual_seed(d + pos)
    tok = torch.randn(vocab, d, generator=g).to(BF16)
    pemb = torch.randn(n_pos, d, generator=g).to(BF16)
    ids = torch.tensor([-3, 0, vocab - 1, vocab + 5, 1, 2], dtype=torch.int32)
    assert ids.numel() > B

    def case(ops):
        cat = ops.out((B, d + 24), name="x")
        x = cat[:, 8:8 + d]
        assert x.stride(0) == d + 24
        torch.ops.aiko.embed_tokens_out(ops.inp(ids, "ids"), ops.inp(torch.tensor([pos], dtype=torch.int32), "pos"),
                                        ops.inp(tok, "tok"), ops.inp(pemb, "pemb"), x)
        torch.cuda.synchronize()
        _nan_slack(cat, 8, d, "x")
        return x

    out = run_both(case)
    rows = ids[:B].clamp(0, vocab - 1).long()
    want = (tok.float()[rows] + pemb.float()[min(max(pos, 0), n_pos - 1)]).to(BF16)
    assert torch.equal(_bits(out.cpu()), _bits(want))


# ---- attn_decode ---------------------------------------------------------------------------------------

def _worst_rows(out, ref, B, H, what):
    errs = row_errs(out.reshape(B * H, 64), ref.to(out.device))
    w = int(errs.argmax())
    print(f"attn_decode {what}: worst row (b {w // H}, h {w % H}) {errs[w].item():.3e}, bound {ROW_BOUND:.3e}")
    return errs


def _cross_launch(ops, q, kv, B, H, T, S, nsplit):
    """q as columns [d, 2d) of a 3d-wide buffer; k | v as columns [8, 8 + 2d) of one 2d + 16 wide
    buffer whose rows T .. S-1 of every sequence are poison in the guarded run; out as columns
    [32, 32 + d) of a NaN buffer; work guarded, NaN, exactly the elements the binding demands."""
    from aiko_services_amd.models.whisper_decoder import attn_decode
    d = H * 64
    qs = ops.inp_slice(q, 3 * d, d, "q")
    wide = torch.full((B * S, 2 * d + 16), ops.gap, dtype=BF16)
    wide[:, 8:8 + 2 * d] = kv
    if ops.on:
        wide.view(B, S, -1)[:, T:] = NAN
    t = ops.inp(wide, "kv")
    cat = ops.out((B, d + 48), name="out")
    work = ops.out((R.attn_decode_work_elems(B, H, T),), torch.float32, name="work")
    out = cat[:, 32:32 + d]
    assert qs.stride(0) == 3 * d and t.stride(0) == 2 * d + 16 and out.stride(0) == d + 48
    attn_decode(qs, t[:, 8:8 + d], t[:, 8 + d:8 + 2 * d], out, B, H, S, T, 0.125, work)
    torch.cuda.synchronize()
    _nan_slack(cat, 32, d, "out")
    if nsplit > 1:
        assert not torch.isnan(work).any(), "a split left its partials unwritten"
    else:
        assert torch.isnan(work).all(), "one split wrote the workspace"
    return out


@pytest.mark.parametrize("B,H,T,S", R.ATTN_CROSS_CASES, ids=[f"{b}x{h}x{t}" for b, h, t, _ in R.ATTN_CROSS_CASES])
def test_attn_decode_cross_guarded(native, B, H, T, S):
    nsplit, chunks = R.attn_decode_plan(B, H, T)
    if T == 1:                                     # one key: the output is that value row
        assert (nsplit, chunks) == (1, 1)
    elif (B, H) == (2, 2):                         # a workgroup per chunk; 255 / 256 / 257 sit around the
        assert nsplit == chunks == -(-T // 256)    # chunk edge (masked-lane clamp), 600 gives three splits
        assert T != 256 or S == T                  # T = S = 256: key 256 of the last sequence is the guard
    elif B * H >= 128:                             # one workgroup streams both chunks, no combine
        assert (nsplit, chunks) == (1, 2)
    else:                                          # split 0 walks chunks 0 and 5, chunk 5 has 20 live keys
        assert 1 < nsplit < chunks and (nsplit, chunks) == (5, 6) and T - 5 * 256 == 20
    q, kv = R.attn_cross_data(B, H, T, S, seed=T + B)
    d = H * 64
    out = run_both(lambda ops: _cross_launch(ops, q, kv, B, H, T, S, nsplit))
    ref = R.attn_decode_ref(q, kv[:, :d].reshape(B, S, d), kv[:, d:].reshape(B, S, d), [T] * B, H, 0.125)
    errs = _worst_rows(out, ref, B, H, f"cross {B}x{H}x{T}")
    if T == 1:
        assert torch.equal(_bits(out.cpu()), _bits(kv.view(B, S, 2 * d)[:, 0, d:]))
    assert errs.max().item() < ROW_BOUND, errs.max().item()


APPEND = [(2, 4, p) for p in (0, 5, 255, 256, 300, 447, 448)] + [(16, 8, p) for p in (0, 256, 447)]


@pytest.mark.parametrize("B,H,pos", APPEND, ids=[f"{b}x{h}-pos{p}" for b, h, p in APPEND])
def test_attn_decode_append_guarded(native, B, H, pos):
    """Append mode on a 448-row cache whose rows past ``pos`` are poison in k and in v.  The cache
    comes back as an output: the old cache with row ``pos`` of every sequence replaced, bit for
    bit, gaps and poison rows included.  pos = 448 = S (a full cache): nothing is appended, the
    cache is unchanged, the S cached keys are attended and no guard is touched."""
    from aiko_services_amd.models.whisper_decoder import attn_decode
    S, d = 448, H * 64
    nsplit, chunks = R.attn_decode_plan(B, H, S)
    full = pos >= S
    n = S if full else pos + 1
    if B * H < 128:
        assert (nsplit, chunks) == (2, 2)          # pos < 256: split 1 has no chunk, the combine skips it;
        owner = (pos // 256) % nsplit              # pos = 256: the owner of the append flips to split 1
        assert full or owner == (0 if pos < 256 else 1)
    else:
        assert (nsplit, chunks) == (1, 2)
    g = torch.Generator().manual_seed(100 + pos + B)
    cache = torch.randn(B * S, 2 * d, generator=g).to(BF16)
    qkv = torch.randn(B, 3 * d, generator=g).to(BF16)

    def case(ops):
        wide = torch.full((B * S, 2 * d + 16), ops.gap, dtype=BF16)
        wide[:, 8:8 + 2 * d] = cache
        if ops.on:
            wide.view(B, S, -1)[:, n:] = NAN       # rows > pos (row pos itself is overwritten)
            if not full:
                wide.view(B, S, -1)[:, pos] = NAN
        t = ops.inp(wide, "kv cache")
        x = ops.inp_slice(qkv, 3 * d + 24, 8, "qkv")
        cat = ops.out((B, d + 48), name="out")
        work = ops.out((R.attn_decode_work_elems(B, H, S),), torch.float32, name="work")
        out = cat[:, 32:32 + d]
        attn_decode(x[:, :d], t[:, 8:8 + d], t[:, 8 + d:8 + 2 * d], out, B, H, S, 0, 0.125, work,
                    pos=ops.inp(torch.tensor([pos], dtype=torch.int32), "pos"), knew=x[:, d:2 * d], vnew=x[:, 2 * d:])
        torch.cuda.synchronize()
        _nan_slack(cat, 32, d, "out")
        want = wide.clone().view(B, S, -1)
        if not full:
            want[:, pos, 8:8 + 2 * d] = qkv[:, d:]
        assert torch.equal(_bits(t.cpu()), _bits(want.view(B * S, -1))), "the cache is not the old cache with row pos replaced"
        return out, t.view(B, S, -1)[:, :n, 8:8 + 2 * d]

    out, rows = run_both(case)
    kk, vv = rows[..., :d].cpu(), rows[..., d:].cpu()
    if not full:
        assert torch.equal(_bits(kk[:, pos]), _bits(qkv[:, d:2 * d])) and torch.equal(_bits(vv[:, pos]), _bits(qkv[:, 2 * d:]))
    ref = R.attn_decode_ref(qkv[:, :d], kk, vv, [n] * B, H, 0.125)
    errs = _worst_rows(out, ref, B, H, f"append {B}x{H} pos {pos}")
    assert errs.max().item() < ROW_BOUND, errs.max().item()


@pytest.mark.parametrize("which", ["v", "k"])
@pytest.mark.parametrize("B,H,T,S,key", [(2, 3, 77, 80, 76), (2, 2, 600, 601, 300)], ids=["one-split", "three-splits"])
def test_attn_decode_poison_is_live(native, B, H, T, S, key, which):
    """Liveness control: NaN in a *valid* value row, or in a valid key row, of one (sequence, head)
    makes exactly that head's 64 outputs non-finite — so a poisoned row past T that was read in
    the guarded cases would show.  (A NaN key gives a NaN softmax sum; the kernel divides by it
    unless the sum is exactly zero.)"""
    from aiko_services_amd.models.whisper_decoder import attn_decode
    nsplit, _ = R.attn_decode_plan(B, H, T)
    assert nsplit == (1 if T <= 256 else 3)
    d = H * 64
    q, kv = R.attn_cross_data(B, H, T, S, seed=9)
    b, h = 1, 1
    c0 = (d if which == "v" else 0) + h * 64
    kv = kv.clone()
    kv[b * S + key, c0:c0 + 64] = NAN
    t = kv.to(DEV)
    out = torch.zeros(B, d, dtype=BF16, device=DEV)
    work = torch.zeros(R.attn_decode_work_elems(B, H, T), dtype=torch.float32, device=DEV)
    attn_decode(q.to(DEV), t[:, :d], t[:, d:], out, B, H, S, T, 0.125, work)
    torch.cuda.synchronize()
    fin = torch.isfinite(out.float()).view(B, H, 64).cpu()
    assert not fin[b, h].any(), f"a NaN {which} row left its head finite"
    fin[b, h] = True
    assert fin.all()


# ---- dec_linear ------------------------------------------------------------------------------------------

def _dec_linear_launch(ops, d, M, K, N, byte_w=None):
    """x as columns [8, 8 + K) of a K + 24 wide buffer, y as columns [32, 32 + N) of a NaN buffer
    (pitch N + 48, N rounded up to whole 16-byte rows), the residual as columns [8, 8 + N) of an
    N + 24 wide buffer or — in place — y itself; W, sw, bias, gamma and beta guarded."""
    from aiko_services_amd.models.whisper_decoder import dec_linear
    from aiko_services_amd.ops import transformer as TR
    Np = _up(N, 8)
    x = ops.inp_slice(d["x"], K + 24, 8, "x")
    lin = TR.Fp8Linear(ops.inp(d["w"], "W"), ops.inp(d["sw"], "sw"), None if d["bias"] is None else ops.inp(d["bias"], "bias"), N, K)
    ln = None if d["ln"] is None else (ops.inp(d["ln"][0], "gamma"), ops.inp(d["ln"][1], "beta"))
    if d["mode"] == "inplace":
        wide = torch.full((M, Np + 48), NAN, dtype=BF16)
        wide[:, 32:32 + N] = d["res"]
        cat = ops.inp(wide, "y (in place)")
        res = cat[:, 32:32 + N]
    else:
        cat = ops.out((M, Np + 48), name="y")
        res = None if d["res"] is None else ops.inp_slice(d["res"], Np + 24, 8, "residual")
        assert res is None or res.stride(0) == Np + 24
    y = cat[:, 32:32 + N]
    assert x.stride(0) == K + 24 and y.stride(0) == Np + 48
    dec_linear(x, lin, y, ln, residual=res, act=d["act"])
    torch.cuda.synchronize()
    _nan_slack(cat, 32, N, "y")
    return y


def _check_plan(M, K, N):
    p = R.dec_linear_plan(M, N, K)
    inst, nkb = p["instance"], p["nkb"]
    if (M, K, N) == (17, 128, 40):
        assert M % 16 == 1 and N % 16 and nkb == 1 and inst == (2, 4, 2)
    elif (M, K, N) == (5, 640, 48):
        assert nkb == 5 and nkb % 4
    elif K in (1024, 1536, 3072) and not p["wide"]:
        assert inst[0] * 512 == K                     # the largest K of the instance
    elif K in (1152, 1664):
        assert inst[0] * 512 > K > {3: 1024, 6: 1536}[inst[0]] and (K // 8) % 64
    elif (M, K, N) == (5, 128, 8192):
        assert p["wide"] and N == 8192
    elif (M, K, N) == (17, 1024, 8200):
        assert p["wide"] and nkb == inst[2] == 8 and N % 64 == 8
    elif (M, K, N) == (3, 128, 8191):
        assert not p["wide"] and p["ntiles"] == 512 and N % 16
    elif (M, K, N) == (1, 128, 65600):
        assert p["wide"] and p["ntiles"] == 1025 and p["grid"][0] == 512      # workgroup 0: tiles 0, 512, 1024
    else:
        assert (M, K, N) == (1, 128, 16) and inst == (2, 4, 2)
    return p


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("case", R.DEC_LINEAR_CASES, ids=[R.dec_linear_id(c) for c in R.DEC_LINEAR_CASES])
def test_dec_linear_guarded(native, case, ln):
    from aiko_services_amd.ops import transformer as TR
    M, K, N, act, _, mode = case
    _check_plan(M, K, N)
    d = dict(R.dec_linear_data(case, ln), mode=mode)
    if M >= 3:
        assert (d["x"][1] == 0).all() and (d["x"][2] == d["x"][2, 0]).all()
    y = run_both(lambda ops: _dec_linear_launch(ops, d, M, K, N), byte_nan=True)
    ref, deq, Wd = R.dec_linear_ref(d["x"], d["w"], d["sw"], d["bias"], d["ln"], 1e-5, act, d["res"])
    errs = row_errs(y.cpu(), ref)
    print(f"dec_linear {R.dec_linear_id(case)} ln={ln}: worst row {int(errs.argmax())} {errs.max().item():.3e}, "
          f"bound {ROW_BOUND:.3e}")
    if not ln:
        assert (errs < ROW_BOUND).all(), errs.max().item()
        return
    bounds = R.flip_bound(ref, deq, Wd)
    ok, over = R.ln_rule(errs, bounds, M)
    assert ok, (over, errs[over].tolist(), bounds[over].tolist())
    if N % 8:                                          # the tiled fp8 GEMM takes N % 8 == 0 only
        return
    # the rule is attainable: the unfused device path (rownorm + linear_fp8) is held to it too
    lin = TR.Fp8Linear(d["w"].to(DEV), d["sw"].to(DEV), None if d["bias"] is None else d["bias"].to(DEV), N, K)
    q = torch.empty(M, K, dtype=torch.uint8, device=DEV)
    s = torch.empty(M, dtype=torch.float32, device=DEV)
    TR.rownorm(d["x"].to(DEV), d["ln"][0].to(DEV), d["ln"][1].to(DEV), q=q, qs=s)
    y2 = TR.linear_fp8(q, s, lin, residual=None if d["res"] is None else d["res"].to(DEV), act=act)
    errs2 = row_errs(y2.cpu(), ref)
    ok2, over2 = R.ln_rule(errs2, bounds, M)
    print(f"  unfused: worst row {errs2.max().item():.3e}")
    assert ok2, (over2, errs2[over2].tolist())


@pytest.mark.parametrize("M,K,N", [(17, 128, 40), (5, 128, 8192)], ids=["narrow", "wide"])
def test_dec_linear_poison_is_live(native, M, K, N):
    """Liveness controls on plain tensors.  A ``0xFF`` byte (e4m3 NaN) in W row n, NaN in sw[n] or
    in bias[n] make exactly column n non-finite; NaN in res[m, n] exactly that element.  A NaN in
    x does NOT propagate (see the module docstring): the output stays finite.  The control for x
    is a finite spike at one valid element of row m, which changes bits in exactly that row."""
    case = (M, K, N, 0, True, "yes")
    base = dict(R.dec_linear_data(case, False), mode="yes")
    m, n = M - 1, N - 3

    def run(**kw):
        d = dict(base)
        for k, v in kw.items():
            d[k] = v
        return _dec_linear_launch(_plain_ops(), d, M, K, N).float().cpu()

    clean = run()
    assert torch.isfinite(clean).all()

    def bad_columns(y):
        return (~torch.isfinite(y)).all(dim=0).nonzero().flatten().tolist(), (~torch.isfinite(y)).sum().item()

    w = base["w"].clone()
    w[n, K - 7] = BYTE_NAN
    assert bad_columns(run(w=w)) == ([n], M), "W"
    sw = base["sw"].clone()
    sw[n] = NAN
    assert bad_columns(run(sw=sw)) == ([n], M), "sw"
    bias = base["bias"].clone()
    bias[n] = NAN
    assert bad_columns(run(bias=bias)) == ([n], M), "bias"
    res = base["res"].clone()
    res[m, n] = NAN
    assert (~torch.isfinite(run(res=res))).nonzero().tolist() == [[m, n]], "res"
    x = base["x"].clone()
    x[m, 5] = NAN
    assert torch.isfinite(run(x=x)).all(), "a NaN in x is expected to be swallowed by the quantiser's clamp"
    x = base["x"].clone()
    x[m, 5] = 3e4
    changed = (_bits(run(x=x).to(BF16)) != _bits(clean.to(BF16))).any(dim=1).nonzero().flatten().tolist()
    assert changed == [m], changed


def _plain_ops():
    from guard_ops import Operands
    return Operands(False, byte_nan=True)


# ---- argmax_step ------------------------------------------------------------------------------------------

_SCEN = [("first", 1), ("last", 1), ("chunk", 4), ("lanes", 13), ("waves", 601), ("passes", 8270), ("zeros", 4),
         ("nan_mixed", 5), ("all_nan", 1), ("all_ninf", 1), ("done", 1)]
TOP = 9.0


def _argmax_rows(B, V, launch, offset, g):
    """Logits [B, V] (fp32 holding bf16 values, |x| <= 8) with one scenario per row, and the
    scenario names.  Ties are two ``TOP`` entries: the smaller index must win."""
    names = [s for s, need in _SCEN if V >= need]
    x = (2 * torch.randn(B, V, generator=g)).clamp(-8, 8).to(BF16).float()
    used = []
    for b in range(B):
        s = names[(offset + launch * B + b) % len(names)]
        used.append(s)
        r = x[b]
        if s == "first":
            r[0] = TOP
        elif s == "last":
            r[V - 1] = TOP
        elif s == "chunk":                          # one thread's 8-element chunk
            r[1] = r[3] = TOP
        elif s == "lanes":                          # threads 0 and 1 of a wave: the shuffle tie rule
            r[3] = r[12] = TOP
        elif s == "waves":                          # threads 1 and 75: waves 0 and 1, met in LDS
            r[10] = r[600] = TOP
        elif s == "passes":                         # thread 9's first and second pass
            r[77] = r[77 + 8192] = TOP
        elif s == "zeros":                          # -0.0 == +0.0: index 1 wins over index 3
            r.copy_(-r.abs() - 1)
            r[1], r[3] = -0.0, 0.0
        elif s == "nan_mixed":
            r[0] = r[4] = r[V - 1] = NAN
            r[2] = TOP
        elif s == "all_nan":
            r.fill_(NAN)
        elif s == "all_ninf":
            r.fill_(float("-inf"))
    return x, used


ARGMAX = [(1, 5, 8), (4, 1001, 1008), (33, 51865, 51968)]


@pytest.mark.parametrize("phase", ["forced", "end"])
@pytest.mark.parametrize("B,V,ld", ARGMAX, ids=[f"{b}x{v}" for b, v, _ in ARGMAX])
def test_argmax_step_guarded(native, B, V, ld, phase):
    """Three consecutive launches on one state (new logits each time), every piece of state compared
    with ``step_ref`` after every launch: the counter is re-armed and ``pos`` advances by exactly 1.
    ``forced``: nxt = 1 (end-of-text inside the forced prefix sets no ``done``), 2 = n_forced - 1,
    3 = n_forced.  ``end``: nxt = 6, 7 = max_len - 1, 8 = max_len, where ``out_tokens`` stays as it
    is.  The logits gap [V, ld) and the guards hold 3e30, above every logit."""
    eot = V - 2
    forced = [V - 1, eot, 0]
    pos0, max_len, offset = (0, 16, 0) if phase == "forced" else (5, 8, 3)
    assert (pos0 + 1 < len(forced) - 1 and pos0 + 3 == len(forced)) or pos0 + 3 == max_len
    assert ld % 8 == 0 and ld >= _up(V, 8) and (V <= 8192 or V % 8)
    g = torch.Generator().manual_seed(B + V)
    logits, names = zip(*[_argmax_rows(B, V, i, offset, g) for i in range(3)])
    if B >= 11:
        assert set(names[0]) == {s for s, _ in _SCEN}           # every scenario in one launch
    done0 = [1 if s == "done" else 0 for s in names[0]]
    state = ([5] * B + [-7, -7], pos0, [[-1] * max_len for _ in range(B)], done0)
    want = []
    for i in range(3):
        state = R.step_ref([r.to(BF16).float() for r in logits[i]], V, state[0], state[1], state[2], forced, eot, state[3])
        want.append(state)
    if phase == "end":
        assert want[2][1] == max_len and want[2][2] == want[1][2]
    else:
        assert all(t == eot for r in want[0][2] for t in [r[1]]) and want[0][3] == done0

    def case(ops):
        wide = torch.full((B, ld), ops.gap, dtype=BF16)
        wide[:, :V] = logits[0].to(BF16)
        lg = ops.inp(wide, "logits")
        ids = ops.inp(torch.tensor([5] * B + [-7, -7], dtype=torch.int32), "ids")
        pos = ops.inp(torch.tensor([pos0], dtype=torch.int32), "pos")
        out = ops.inp(torch.full((B, max_len), -1, dtype=torch.int32), "out_tokens")
        fz = ops.inp(torch.tensor(forced, dtype=torch.int32), "forced")
        done = ops.inp(torch.tensor(done0, dtype=torch.int32), "done")
        counter = ops.inp(torch.zeros(1, dtype=torch.int32), "counter")
        for i in range(3):
            if i:
                lg[:, :V].copy_(logits[i].to(BF16))
            torch.ops.aiko.argmax_step_out(lg, V, ids, pos, out, fz, eot, done, counter)
            torch.cuda.synchronize()
            got = (ids.tolist(), pos.item(), out.tolist(), done.tolist())
            assert got[1] == want[i][1] == pos0 + i + 1 and counter.item() == 0, (i, got[1], counter.item())
            assert got[0] == want[i][0], (i, "ids", [(b, names[i][b]) for b in range(B) if got[0][b] != want[i][0][b]])
            assert got[3] == want[i][3], (i, "done")
            assert got[2] == want[i][2], (i, "out_tokens")
        return ids, done, out, pos, counter

    run_both(case, poison=3e30)


# ---- the whole decoder on a guarded workspace --------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _tiny():
    from aiko_services_amd.models.whisper_decoder import WhisperDecoder
    return WhisperDecoder("tiny", device=DEV)


def _eight_steps(dec, feats, B, poison_spare):
    dec.prepare(feats)
    _, T, S = dec._geom
    assert S == T + 1, "features did not take the zero-copy path"
    st = dec._state(B)
    st["forced"].copy_(torch.tensor(dec.prompt, dtype=torch.int32))
    if poison_spare:
        for i in range(dec.layers_n):
            dec._buf(f"kv_cross{i}", (B * S, 2 * dec.d)).view(B, S, -1)[:, T:] = NAN
    logits = [dec.step().clone() for _ in range(8)]
    torch.cuda.synchronize()
    return logits, st["tokens"][:, :9].clone()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_decoder_tiny_on_guarded_workspace(native, monkeypatch, fused):
    """Eight eager steps of Whisper-tiny, B = 2, with every workspace buffer a guarded view whose
    interior starts as poison (``zero=`` honoured): the self-attention cache rows past ``pos`` are
    NaN, as ``torch.empty`` may leave them, and so are the spare encoder rows that sit inside every
    ``kv_cross`` (sequence 0's directly in front of sequence 1's keys).  Logits of every step and
    the tokens are finite and bit-identical to the run on a plain workspace."""
    dec = _tiny()
    B, T, d = 2, 120, 384
    g = torch.Generator().manual_seed(8)
    vals = torch.randn(B, T + 1, d, generator=g).to(BF16)
    vals[:, T] = NAN
    monkeypatch.setattr(dec, "fused_linear", fused)
    dec.release_workspace()
    try:
        plain_logits, plain_tokens = _eight_steps(dec, vals.to(DEV)[:, :T], B, False)
    finally:
        dec.release_workspace()
    checks, ws = [], {}

    def _buf(key, shape, dtype=BF16, zero=False):
        k = (dec.ws_tag + key, tuple(shape), dtype)
        if k not in ws:
            ws[k], check = guarded(shape, dtype, DEV, fill=0 if zero else None, name=key)
            checks.append(check)
        return ws[k]

    monkeypatch.setattr(dec, "_buf", _buf)
    feats, fcheck = guarded((B, T + 1, d), BF16, DEV, values=vals, name="features")
    try:
        logits, tokens = _eight_steps(dec, feats[:, :T], B, True)
    finally:
        monkeypatch.undo()
        dec.release_workspace()
    assert len(checks) > 10
    kvs = ws[("kv_self0", (B * dec.n_ctx, 2 * d), BF16)].view(B, dec.n_ctx, -1)
    assert torch.isfinite(kvs[:, :8].float()).all() and torch.isnan(kvs[:, 8:].float()).all(), \
        "precondition: exactly the eight appended cache rows are finite"
    kvc = ws[("kv_cross0", (B * (T + 1), 2 * d), BF16)].view(B, T + 1, -1)
    assert torch.isnan(kvc[:, T].float()).all()
    fcheck()
    for c in checks:
        c()
    for i, (a, b) in enumerate(zip(plain_logits, logits)):
        assert torch.isfinite(b.float()).all(), i
        assert torch.equal(_bits(a), _bits(b)), f"step {i}: logits differ between the plain and the guarded workspace"
    assert torch.equal(plain_tokens, tokens)
    assert tokens[:, :4].tolist() == [list(dec.prompt)] * B
