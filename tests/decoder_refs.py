"""Plain references, launch plans and case tables for the decoder step kernels of
``csrc/kernels/decode_ops.hip`` (tests/test_gpu_guard_decoder.py runs them on the device,
tests/test_decoder_refs.py checks them here against slow, obvious code).  A plain module next to
``guard_ops.py``: no fixtures, everything works on the CPU.

References start from the operands the kernel receives (bf16 activations, e4m3 weight bytes, fp32
scales) and compute in fp64, so the only difference to a clean kernel is the kernel's own fp32
arithmetic and the final bf16 rounding — what ``guard_ops.ROW_BOUND`` (2^-8 per row) allows.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from guard_ops import ROW_BOUND

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
KC = 256                  # keys per chunk of attn_decode_kernel (kDecKC)
DH = 64                   # head dim


# ---- launch plans --------------------------------------------------------------------------------

def attn_decode_plan(B: int, H: int, maxlen: int):
    """``(nsplit, chunks)`` of aiko_attn_decode (a copy of ``attn_decode_splits``): ``maxlen`` is
    S in append mode and T in cross mode.  Workgroup ``split`` walks chunks split, split + nsplit,
    ...; ``nsplit > 1`` also launches the combine kernel and needs B*H*nsplit*66 fp32 of work."""
    chunks = -(-maxlen // KC)
    bh = B * H
    if bh >= 128:
        return 1, chunks
    want = -(-512 // bh)
    return min(want, chunks), chunks


def attn_decode_work_elems(B: int, H: int, maxlen: int) -> int:
    """fp32 elements the binding demands of ``work`` (aiko_attn_decode_work)."""
    return B * H * attn_decode_plan(B, H, maxlen)[0] * (DH + 2)


def dec_linear_plan(M: int, N: int, K: int) -> dict:
    """What aiko_dec_linear launches: ``instance`` (MAXC, KS, KBW), ``wide`` (the persistent
    64-column kernel), ``ntiles`` column tiles and the ``grid`` (x, y)."""
    if K % 128 or K > 3072 or M <= 0 or N <= 0:
        raise ValueError("dec_linear: K % 128 == 0, K <= 3072")
    nkb = K // 128
    wide = N >= 8192 and nkb <= 8
    if wide:
        inst = (2, 1, 8)
    elif K <= 1024:
        inst = (2, 4, 2)
    elif K <= 1536:
        inst = (3, 4, 3)
    else:
        inst = (6, 4, 6)
    ntiles = -(-N // (64 if wide else 16))
    return {"instance": inst, "wide": wide, "ntiles": ntiles, "nkb": nkb,
            "grid": (min(ntiles, 512) if wide else ntiles, -(-M // 16))}


# ---- attention -----------------------------------------------------------------------------------

def attn_decode_ref(q, k, v, counts, H: int, scale: float) -> torch.Tensor:
    """fp64 softmax attention of one query row per sequence.  ``q`` [B, H*64]; ``k`` / ``v``
    [B, S, H*64] (any float dtype, used as given); ``counts[b]`` keys of sequence b are attended.
    Returns fp64 [B*H, 64], row b*H + h."""
    B = q.shape[0]
    qd = q.double().reshape(B, H, DH)
    kd, vd = k.double().reshape(B, -1, H, DH), v.double().reshape(B, -1, H, DH)
    out = torch.empty(B * H, DH, dtype=torch.float64, device=q.device)
    for b in range(B):
        n = int(counts[b])
        s = torch.einsum("hd,thd->ht", qd[b], kd[b, :n]) * scale
        out[b * H:(b + 1) * H] = torch.einsum("ht,thd->hd", torch.softmax(s, dim=-1), vd[b, :n])
    return out


# (B, H, T, S) of the cross-mode cases and the property each one claims
ATTN_CROSS_CASES = [(1, 1, 1, 8), (2, 2, 255, 264), (2, 2, 256, 256), (2, 2, 257, 264), (2, 2, 600, 601),
                    (16, 8, 300, 304), (13, 8, 1300, 1304)]


def attn_cross_data(B, H, T, S, seed):
    """CPU bf16 operands of a cross-mode case: q [B, d], kv [B*S, 2d] (k | v)."""
    g = torch.Generator().manual_seed(seed)
    d = H * DH
    return torch.randn(B, d, generator=g).to(BF16), torch.randn(B * S, 2 * d, generator=g).to(BF16)


# ---- argmax step -----------------------------------------------------------------------------------

def argmax_ref(row, V: int, eot: int) -> int:
    """The smallest index among the maxima of ``row[:V]``, NaN left out; ``-0.0 == +0.0``.  The
    kernel starts from -inf and takes a value only if it is greater, so a row that holds nothing
    above -inf (all NaN, all -inf, or a mix) has no candidate and gives ``eot``."""
    v = row[:V].double()
    ok = ~torch.isnan(v) & (v > -math.inf)
    if not bool(ok.any()):
        return int(eot)
    m = v[ok].max()
    return int(torch.nonzero(ok & (v == m))[0].item())


def step_ref(logits, V, ids, pos, out_tokens, forced, eot, done):
    """One launch of argmax_step_kernel on Python lists: returns new ``(ids, pos, out_tokens,
    done)`` (the inputs are left alone).  ``ids`` may be longer than B = len(logits)."""
    B, max_len, n_forced = len(logits), len(out_tokens[0]), len(forced)
    ids, done = list(ids), list(done)
    out_tokens = [list(r) for r in out_tokens]
    nxt = pos + 1
    for b in range(B):
        tok = argmax_ref(logits[b], V, eot)
        if done[b]:
            tok = eot
        if nxt < n_forced:
            tok = forced[nxt]
        if nxt < max_len:
            out_tokens[b][nxt] = tok
        ids[b] = tok
        if tok == eot and nxt >= n_forced:
            done[b] = 1
    return ids, nxt, out_tokens, done


# ---- dec_linear ------------------------------------------------------------------------------------

def e4m3_rne(v: torch.Tensor) -> torch.Tensor:
    """fp64 values in [-448, 448] rounded to the nearest e4m3fn value, ties to even, in one step
    (no detour over fp32).  The spacing is 2^(e-3) in the binade [2^e, 2^(e+1)), 2^-9 below 2^-6."""
    v = v.double()
    a = v.abs()
    _, ex = torch.frexp(a)                                   # a = m * 2^ex, m in [0.5, 1)
    step = torch.exp2((ex.double() - 1).clamp(min=-6.0) - 3)
    return torch.sign(v) * torch.round(a / step) * step      # torch.round: half to even


def act_ref(v, act: int):
    if act == 1:
        return F.relu(v)
    if act == 2:
        return F.silu(v)
    if act == 3:
        return F.gelu(v)
    return v


def dec_linear_ref(x, w_u8, sw, bias=None, ln=None, eps: float = 1e-5, act: int = 0, res=None):
    """fp64 reference of dec_linear_kernel from its own operands: optional LayerNorm (``ln`` =
    (gamma, beta)), per-row ``s = amax / 448`` (1 for a zero row), e4m3 round-to-nearest-even of
    ``clamp(z / s)``, GEMM with the dequantised weight ``e4m3(w) * sw``, bias, activation,
    residual.  Returns ``(ref [M, N], deq [M, K], Wd [N, K])``, all fp64."""
    z = x.double()
    if ln is not None:
        z = F.layer_norm(z, (z.shape[1],), ln[0].double(), ln[1].double(), eps)
    amax = z.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    deq = e4m3_rne((z / s[:, None]).clamp(-FP8_MAX, FP8_MAX)) * s[:, None]
    Wd = w_u8.view(FP8).double() * sw.double()[:, None]
    pre = deq @ Wd.T
    if bias is not None:
        pre = pre + bias.double()
    ref = act_ref(pre, act)
    if res is not None:
        ref = ref + res.double()
    return ref, deq, Wd


def planted_rows(M: int, K: int, g: torch.Generator) -> torch.Tensor:
    """bf16 activations [M, K] whose largest magnitude in row m is ``±1.75 * 2^j`` (j per row in
    -3 .. 3): the row scale is then exactly 2^(j-8), ``z / s`` is exact in fp32 as in fp64, and a
    value half-way between two e4m3 codes is an exact tie that kernel and reference both round to
    even.  With M >= 3, row 1 is all zero (scale 1) and row 2 is constant."""
    top = 1.75 * torch.exp2(torch.randint(-3, 4, (M,), generator=g).double())
    x = torch.randn(M, K, generator=g).double() * (0.5 * top)[:, None]
    cap = (top * (1.5 / 1.75))[:, None]                      # every other element within ±1.5 * 2^j
    x = torch.minimum(torch.maximum(x, -cap), cap)
    at = torch.randint(0, K, (M,), generator=g)
    sign = torch.randint(0, 2, (M,), generator=g).double() * 2 - 1
    x[torch.arange(M), at] = sign * top
    if M >= 3:
        x[1] = 0.0
        x[2] = top[2]
    return x.to(BF16)


def flip_bound(ref, deq, Wd) -> torch.Tensor:
    """Per-row bound [M] of a run whose fp32 LayerNorm put ONE element on the other side of an
    e4m3 rounding boundary than the fp64 reference: ``ROW_BOUND`` plus one code step (2^-3 of the
    element, times 1.2 for the slope of GELU / SiLU) on the element with the largest effect,
    ``1.2 * 2^-3 * max_k(|deq[m, k]| * ||Wd[:, k]||) / ||ref[m]||``."""
    impact = (deq.double().abs() * Wd.double().norm(dim=0)[None, :]).amax(dim=1)
    return ROW_BOUND + 1.2 * 2.0 ** -3 * impact / ref.double().norm(dim=1)


# (M, K, N, act, bias, res) — res: "none", "yes" (a separate tensor) or "inplace" (y is res, as
# WhisperDecoder.step calls it).  Every case runs without and with LayerNorm.
DEC_LINEAR_CASES = [
    (1, 128, 16, 0, True, "none"),          # smallest shape on <2,4,2>
    (17, 128, 40, 1, False, "yes"),         # second row tile with one live row; ragged column tile; waves 1-3 idle
    (5, 640, 48, 2, True, "inplace"),       # nkb = 5: uneven K split
    (16, 1024, 32, 3, True, "yes"),         # largest K on <2,4,2>
    (5, 1152, 40, 0, False, "inplace"),     # first K of <3,4,3>: third pass partly live
    (16, 1536, 16, 3, True, "none"),        # largest K on <3,4,3>
    (5, 1664, 40, 1, True, "yes"),          # first K of <6,4,6>
    (37, 3072, 24, 0, True, "inplace"),     # largest K on <6,4,6>
    (5, 128, 8192, 0, False, "none"),       # N at the wide threshold
    (17, 1024, 8200, 3, True, "yes"),       # wide, nkb = KBW = 8, last 64-column tile has 8 live columns
    (3, 128, 8191, 2, True, "yes"),         # one short of the threshold: narrow, 512 tiles
    (1, 128, 65600, 0, True, "inplace"),    # 1025 tiles on 512 workgroups: a third tile, both buffers reused
]
# seed of the LayerNorm run of a case, where the default (M + K + N) had to be changed
DEC_LINEAR_LN_SEEDS: dict = {}


def dec_linear_id(c) -> str:
    M, K, N, act, bias, res = c
    return f"{M}x{K}x{N}-a{act}" + ("-bias" if bias else "") + ("" if res == "none" else "-" + res)


def dec_linear_data(case, ln: bool) -> dict:
    """CPU operands of a case: x bf16 [M, K] (planted rows), w uint8 e4m3 [N, K], sw fp32 [N],
    bias fp32 [N] or None, ln (gamma, beta) fp32 [K] or None, res bf16 [M, N] or None."""
    M, K, N, act, bias, res = case
    seed = DEC_LINEAR_LN_SEEDS.get(case, M + K + N) + 1000 if ln else M + K + N
    g = torch.Generator().manual_seed(seed)
    x = planted_rows(M, K, g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    sw = w.abs().amax(dim=1).clamp(min=1e-12) / FP8_MAX
    wq = (w / sw[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8).view(torch.uint8)
    return {"x": x, "w": wq.contiguous(), "sw": sw.contiguous(),
            "bias": 0.1 * torch.randn(N, generator=g) if bias else None,
            "ln": (1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)) if ln else None,
            "res": None if res == "none" else torch.randn(M, N, generator=g).to(BF16), "act": act}


def ln_rule(errs: torch.Tensor, bounds: torch.Tensor, M: int):
    """The LayerNorm rule: every row below its ``flip_bound``, at most ``M // 8`` rows (none for
    M < 8) at or above ``ROW_BOUND``.  Returns ``(ok, rows at or above ROW_BOUND)``."""
    over = torch.nonzero(~(errs < ROW_BOUND)).flatten().tolist()
    return bool((errs < bounds).all()) and len(over) <= M // 8, over
