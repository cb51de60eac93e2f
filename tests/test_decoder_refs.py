"""tests/decoder_refs.py against slow, obvious code on tiny inputs, and the conditions the numeric
bounds of tests/test_gpu_guard_decoder.py rest on: planted rows quantise without a rounding
choice, an fp32 emulation of the fused LayerNorm path keeps every row of every case below
``ROW_BOUND`` (so the chosen seeds ask nothing unattainable), and an fp32 emulation of the chunked
online softmax stays below it too.  No GPU needed."""
import math

import pytest
import torch
import torch.nn.functional as F

import decoder_refs as R
from guard_ops import ROW_BOUND, row_errs


# ---- plans ---------------------------------------------------------------------------------------

def test_attn_decode_plan_matches_claims():
    want = {(1, 1, 1, 8): (1, 1), (2, 2, 255, 264): (1, 1), (2, 2, 256, 256): (1, 1), (2, 2, 257, 264): (2, 2),
            (2, 2, 600, 601): (3, 3), (16, 8, 300, 304): (1, 2), (13, 8, 1300, 1304): (5, 6)}
    assert set(want) == set(R.ATTN_CROSS_CASES)
    for (B, H, T, S), plan in want.items():
        assert R.attn_decode_plan(B, H, T) == plan, (B, H, T)
    # append mode plans by S = 448
    assert R.attn_decode_plan(2, 4, 448) == (2, 2) and R.attn_decode_plan(16, 8, 448) == (1, 2)
    # up to the encoder's 1500 frames the only way to 1 < nsplit < chunks: 103 <= B*H <= 127 and
    # more than 1280 keys
    for bh in range(1, 140):
        for maxlen in (1, 256, 257, 1280, 1281, 1500, 1536):
            ns, ch = R.attn_decode_plan(1, bh, maxlen)
            assert 1 <= ns <= ch == -(-maxlen // 256)
            if 1 < ns < ch:
                assert 103 <= bh <= 127 and maxlen > 1280
    assert R.attn_decode_work_elems(13, 8, 1300) == 13 * 8 * 5 * 66


def test_dec_linear_plan_matches_claims():
    want = [((2, 4, 2), False, 1), ((2, 4, 2), False, 3), ((2, 4, 2), False, 3), ((2, 4, 2), False, 2),
            ((3, 4, 3), False, 3), ((3, 4, 3), False, 1), ((6, 4, 6), False, 3), ((6, 4, 6), False, 2),
            ((2, 1, 8), True, 128), ((2, 1, 8), True, 129), ((2, 4, 2), False, 512), ((2, 1, 8), True, 1025)]
    for (M, K, N, *_), (inst, wide, ntiles) in zip(R.DEC_LINEAR_CASES, want):
        p = R.dec_linear_plan(M, N, K)
        assert (p["instance"], p["wide"], p["ntiles"]) == (inst, wide, ntiles), (M, K, N)
        assert p["grid"] == (min(ntiles, 512) if wide else ntiles, -(-M // 16))
    assert R.dec_linear_plan(1, 65600, 128)["grid"] == (512, 1)
    with pytest.raises(ValueError):
        R.dec_linear_plan(1, 16, 3200)
    # every act, bias on and off, and the three residual forms are covered, with both kernels
    cases = R.DEC_LINEAR_CASES
    assert {c[3] for c in cases} == {0, 1, 2, 3} and {c[4] for c in cases} == {True, False}
    assert {c[5] for c in cases} == {"none", "yes", "inplace"}
    assert {R.dec_linear_plan(c[0], c[2], c[1])["instance"] for c in cases} == {(2, 4, 2), (3, 4, 3), (6, 4, 6), (2, 1, 8)}


# ---- attention -----------------------------------------------------------------------------------

def test_attn_decode_ref_against_loops():
    g = torch.Generator().manual_seed(0)
    B, H, S = 2, 2, 5
    q = torch.randn(B, H * 64, generator=g).to(R.BF16)
    k = torch.randn(B, S, H * 64, generator=g).to(R.BF16)
    v = torch.randn(B, S, H * 64, generator=g).to(R.BF16)
    counts = [3, 5]
    got = R.attn_decode_ref(q, k, v, counts, H, 0.125)
    assert got.shape == (B * H, 64) and got.dtype == torch.float64
    for b in range(B):
        for h in range(H):
            qq = [float(t) for t in q[b, h * 64:(h + 1) * 64]]
            s = [0.125 * sum(a * float(c) for a, c in zip(qq, k[b, j, h * 64:(h + 1) * 64])) for j in range(counts[b])]
            w = [math.exp(t - max(s)) for t in s]
            for e in (0, 17, 63):
                want = sum(wj * float(v[b, j, h * 64 + e]) for j, wj in enumerate(w)) / sum(w)
                assert abs(got[b * H + h, e].item() - want) < 1e-12
    # one key: the output is that value row
    one = R.attn_decode_ref(q, k, v, [1, 1], H, 0.125)
    assert torch.equal(one.view(B, H * 64), v[:, 0].double())


def _attn_emulate_fp32(q, k, v, T, H, scale, nsplit):
    """The kernel's order of work in fp32: 256-key chunks, online softmax in the exp2 domain per
    split, partials combined; returns bf16-rounded rows [B*H, 64]."""
    B = q.shape[0]
    qf = q.float().view(B, H, 64) * torch.tensor(scale * 1.4426950408889634, dtype=torch.float32)
    kf, vf = k.float().view(B, -1, H, 64), v.float().view(B, -1, H, 64)
    parts = []
    for split in range(nsplit):
        m = torch.full((B, H), -math.inf)
        l = torch.zeros(B, H)
        acc = torch.zeros(B, H, 64)
        for start in range(split * 256, T, nsplit * 256):
            end = min(start + 256, T)
            s = torch.einsum("bhd,bthd->bht", qf, kf[:, start:end])
            mn = torch.maximum(m, s.amax(dim=-1))
            corr = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - mn))
            p = torch.exp2(s - mn[..., None])
            l = l * corr + p.sum(-1)
            acc = acc * corr[..., None] + torch.einsum("bht,bthd->bhd", p, vf[:, start:end])
            m = mn
        parts.append((m, l, acc))
    M = torch.stack([p[0] for p in parts]).amax(dim=0)
    L, A = torch.zeros(B, H), torch.zeros(B, H, 64)
    for m, l, acc in parts:
        w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - M))
        L, A = L + w * l, A + w[..., None] * acc
    return (A / L[..., None]).to(R.BF16).view(B * H, 64)


@pytest.mark.parametrize("B,H,T,S", [c for c in R.ATTN_CROSS_CASES if c[0] * c[2] < 5000])
def test_attention_bound_is_attainable_in_fp32(B, H, T, S):
    q, kv = R.attn_cross_data(B, H, T, S, seed=T + B)
    d = H * 64
    k, v = kv[:, :d].reshape(B, S, d), kv[:, d:].reshape(B, S, d)
    ref = R.attn_decode_ref(q, k, v, [T] * B, H, 0.125)
    got = _attn_emulate_fp32(q, k, v, T, H, 0.125, R.attn_decode_plan(B, H, T)[0])
    errs = row_errs(got, ref)
    assert errs.max().item() < ROW_BOUND, errs.max().item()


# ---- argmax / step -------------------------------------------------------------------------------

def _argmax_slow(row, V, eot):
    best, besti = -math.inf, None
    for i in range(V):
        x = float(row[i])
        if x > best:                      # False for NaN; strictly greater: the first maximum stays
            best, besti = x, i
    return eot if besti is None else besti


def test_argmax_ref_against_scan():
    nan, inf = math.nan, math.inf
    rows = [[1.0, 3.0, 3.0, 2.0], [nan, 1.0, nan, 1.0], [nan, nan, nan, nan], [-inf, -inf, -inf, -inf],
            [-inf, nan, -inf, nan], [-1.0, -0.0, 0.0, -2.0], [-1.0, 0.0, -0.0, -2.0], [nan, -inf, -5.0, nan],
            [inf, 1.0, inf, nan], [0.0, 1.0, 2.0, 9.0]]
    want = [1, 1, 99, 99, 99, 1, 1, 2, 0, 2]      # the last row: 9.0 sits at index V = 3, outside
    for r, w in zip(rows, want):
        t = torch.tensor(r).to(R.BF16)
        assert R.argmax_ref(t, 3 if r[-1] == 9.0 else 4, 99) == w, r
        assert _argmax_slow(t, 3 if r[-1] == 9.0 else 4, 99) == w, r
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-3, 4, (50, 37), generator=g).float()
    x[torch.rand(50, 37, generator=g) < 0.2] = nan
    for r in x:
        assert R.argmax_ref(r, 33, 7) == _argmax_slow(r, 33, 7)
    assert int(torch.argmax(torch.tensor([nan, 1.0]))) == 0     # why torch.argmax is not the reference


def test_step_ref_rules():
    eot, V = 3, 5
    logits = torch.tensor([[0.0, 9.0, 0, 0, 0], [0, 0, 0, 9.0, 0], [0, 0, 9.0, 0, 0]])   # 1, eot, 2
    forced = [7, eot, 8]
    ids, pos, out, done = [5, 5, 5, -7], 0, [[-1] * 5 for _ in range(3)], [0, 0, 1]
    # nxt = 1 < n_forced: the forced token wins everywhere, eot inside the prefix sets no done
    ids, pos, out, done = R.step_ref(logits, V, ids, pos, out, forced, eot, done)
    assert (ids, pos, done) == ([eot, eot, eot, -7], 1, [0, 0, 1]) and [r[1] for r in out] == [eot] * 3
    # nxt = 2 = n_forced - 1: still forced
    ids, pos, out, done = R.step_ref(logits, V, ids, pos, out, forced, eot, done)
    assert (ids, pos, done) == ([8, 8, 8, -7], 2, [0, 0, 1])
    # nxt = 3 = n_forced: free; row 1 emits eot and is done, row 2 was done and gives eot
    ids, pos, out, done = R.step_ref(logits, V, ids, pos, out, forced, eot, done)
    assert (ids, pos, done) == ([1, eot, eot, -7], 3, [0, 1, 1]) and [r[3] for r in out] == [1, eot, eot]
    # nxt = 4 = max_len - 1 is written, nxt = 5 = max_len is not
    ids, pos, out, done = R.step_ref(logits, V, ids, pos, out, forced, eot, done)
    assert pos == 4 and [r[4] for r in out] == [1, eot, eot]
    before = [list(r) for r in out]
    ids, pos, out2, done = R.step_ref(logits, V, ids, pos, out, forced, eot, done)
    assert pos == 5 and out2 == before and ids[:3] == [1, eot, eot]
    assert out == before                                           # inputs are left alone


# ---- dec_linear ----------------------------------------------------------------------------------

def _e4m3_values():
    b = torch.arange(256, dtype=torch.uint8)
    v = b.view(R.FP8).double()
    return torch.unique(v[~torch.isnan(v)])


def _e4m3_slow(x: float, grid) -> float:
    """Nearest grid value; on a tie the one whose code is even (its distance to zero is an even
    multiple of the local step)."""
    best = sorted(grid, key=lambda c: (abs(c - x), 0))[:2]
    if abs(best[0] - x) != abs(best[1] - x):
        return best[0]
    step = abs(best[0] - best[1])
    return next(c for c in best if round(abs(c) / step) % 2 == 0)


def test_e4m3_rne_against_grid_search():
    grid = _e4m3_values().tolist()
    assert max(grid) == 448.0 and len(grid) == 253 and 2.0 ** -9 in grid
    mids = [(a + b) / 2 for a, b in zip(grid, grid[1:])]                 # every tie of the format
    g = torch.Generator().manual_seed(2)
    xs = mids + grid + (torch.rand(300, generator=g).double() * 896 - 448).tolist() + \
        (torch.randn(300, generator=g).double() * 0.02).tolist() + [m + 1e-12 for m in mids] + [m - 1e-12 for m in mids]
    got = R.e4m3_rne(torch.tensor(xs, dtype=torch.float64)).tolist()
    for x, y in zip(xs, got):
        assert y == _e4m3_slow(x, grid), (x, y)
    # and torch's own fp32 -> e4m3 conversion agrees wherever fp32 holds the input exactly
    x32 = torch.tensor(mids + grid, dtype=torch.float32)
    assert torch.equal(R.e4m3_rne(x32.double()), x32.to(R.FP8).double())


def test_planted_rows_quantise_without_a_choice():
    """Condition 1 of the bounds: the largest magnitude of every row is ±1.75 * 2^j, so the fp32
    arithmetic of the kernel (scale = amax / 448, v * (1 / scale)) is exact and its quantised row
    equals the reference's bit for bit — exact ties included."""
    g = torch.Generator().manual_seed(3)
    M, K = 64, 256
    x = R.planted_rows(M, K, g)
    assert x.dtype == R.BF16 and (x[1] == 0).all() and (x[2] == x[2, 0]).all() and x[2, 0] != 0
    xf = x.float()
    amax = xf.abs().amax(dim=1)
    live = amax > 0
    frac, _ = torch.frexp(amax[live])
    assert (frac == 0.875).all()                                         # 1.75 * 2^j
    scale = torch.where(live, amax / 448.0, torch.ones_like(amax))       # fp32, as the kernel
    zk = xf * (1.0 / scale)[:, None]
    z64 = x.double() / torch.where(live, amax.double() / 448.0, torch.ones(M, dtype=torch.float64))[:, None]
    assert torch.equal(zk.double(), z64)
    assert torch.equal(zk.to(R.FP8).double(), R.e4m3_rne(z64))
    ties = (R.e4m3_rne(z64 + 1e-9) != R.e4m3_rne(z64 - 1e-9)).sum().item()
    assert ties > 0                                                      # the rows do hold exact ties


def test_dec_linear_ref_against_loops():
    g = torch.Generator().manual_seed(4)
    M, K, N = 4, 128, 3
    c = (M, K, N, 3, True, "yes")
    for ln in (False, True):
        d = R.dec_linear_data(c, ln)
        ref, deq, Wd = R.dec_linear_ref(d["x"], d["w"], d["sw"], d["bias"], d["ln"], 1e-5, d["act"], d["res"])
        grid = _e4m3_values().tolist()
        for m in (0, 1, 3):
            z = [float(t) for t in d["x"][m]]
            if ln:
                mu = sum(z) / K
                var = sum((t - mu) ** 2 for t in z) / K
                z = [(t - mu) / math.sqrt(var + 1e-5) * float(d["ln"][0][k]) + float(d["ln"][1][k]) for k, t in enumerate(z)]
            amax = max(abs(t) for t in z)
            s = amax / 448 if amax > 0 else 1.0
            dq = [_e4m3_slow(min(max(t / s, -448.0), 448.0), grid) * s for t in z]
            assert max(abs(a - float(b)) for a, b in zip(dq, deq[m])) <= 1e-12 * max(amax, 1)
            for n in range(N):
                w = d["w"][n].view(R.FP8).double() * float(d["sw"][n])
                pre = sum(a * float(b) for a, b in zip(dq, w)) + float(d["bias"][n])
                want = 0.5 * pre * (1 + math.erf(pre / math.sqrt(2))) + float(d["res"][m, n])
                assert abs(ref[m, n].item() - want) < 1e-9
        if not ln:
            assert (deq[1] == 0).all() and torch.allclose(ref[1], F.gelu(d["bias"].double()) + d["res"][1].double())
    del g


def test_flip_bound_covers_one_code_step():
    c = (6, 256, 24, 0, True, "none")
    d = R.dec_linear_data(c, True)
    ref, deq, Wd = R.dec_linear_ref(d["x"], d["w"], d["sw"], d["bias"], d["ln"], 1e-5, 0, None)
    fb = R.flip_bound(ref, deq, Wd)
    assert fb.shape == (6,) and (fb > ROW_BOUND).all()
    for m in range(6):
        k = int((deq[m].abs() * Wd.norm(dim=0)).argmax())
        flipped = deq.clone()
        flipped[m, k] *= 1 + 2.0 ** -3                                   # one code step at most
        y = flipped @ Wd.T + d["bias"].double()
        e = row_errs(y, ref)
        assert e[m] < fb[m] - ROW_BOUND + 1e-12 and (e[torch.arange(6) != m] == 0).all()
    ok, over = R.ln_rule(torch.tensor([1e-3, 5e-3, 1e-3]), torch.tensor([4e-3, 6e-3, 4e-3]), 3)
    assert not ok and over == [1]                                        # M < 8: no row may reach ROW_BOUND
    ok, over = R.ln_rule(torch.tensor([1e-3] * 7 + [5e-3]), torch.tensor([6e-3] * 8), 8)
    assert ok and over == [7]
    assert not R.ln_rule(torch.tensor([1e-3] * 7 + [7e-3]), torch.tensor([6e-3] * 8), 8)[0]


@pytest.mark.parametrize("case", R.DEC_LINEAR_CASES, ids=[R.dec_linear_id(c) for c in R.DEC_LINEAR_CASES])
def test_ln_seeds_are_attainable_in_fp32(case):
    """Condition 2 of the bounds: with the seeds of the table, an fp32 emulation of the fused path
    (fp32 LayerNorm, per-row e4m3 quantisation, exact GEMM) has no row at or above ``ROW_BOUND``
    against ``dec_linear_ref``, before the output's own bf16 rounding."""
    from aiko_services_amd.ops.transformer import quantize_rows_ref
    M, K, N, act, _, _ = case
    d = R.dec_linear_data(case, True)
    ref, deq, Wd = R.dec_linear_ref(d["x"], d["w"], d["sw"], d["bias"], d["ln"], 1e-5, act, d["res"])
    h = F.layer_norm(d["x"].float(), (K,), d["ln"][0], d["ln"][1], 1e-5)
    q, s = quantize_rows_ref(h)
    pre = (q.view(R.FP8).double() * s.double()[:, None]) @ Wd.T
    if d["bias"] is not None:
        pre = pre + d["bias"].double()
    y = R.act_ref(pre, act)
    if d["res"] is not None:
        y = y + d["res"].double()
    errs = row_errs(y, ref)
    assert (errs < ROW_BOUND).all(), errs.max().item()
    assert (errs < R.flip_bound(ref, deq, Wd)).all()
