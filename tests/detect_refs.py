"""Plain references, launch plans and case tables for the detection post-processing kernels of
``csrc/kernels/detect_ops.hip`` (``yolo_decode_kernel``, ``yolo_decode_tiled_kernel``,
``nms_fused_kernel``).  No fixtures, no device: everything here runs on the CPU (numpy / Python)
and is checked by tests/test_detect_refs.py; tests/test_gpu_guard_detect.py holds the kernels to it.

* :func:`decode_ref64` is the fp64 DFL decode of the bf16 head values, :func:`decode_emul32` the
  kernel's order of operations in fp32 (its distance from ``decode_ref64`` is what fp32 alone
  costs) and :func:`decode_expf_margin` what the kernel's ``__expf`` may add on top.
* :func:`nms_slow` is a per-class greedy NMS in numpy fp32, independent of the one-pass offset
  trick of ``ops.reference.nms_ref``; it also builds the fixed-size ``det`` / ``count`` image.
* ``nms_groups`` / ``nms_radix_plan`` / ``nms_blocks`` / ``decode_plan`` mirror the launchers, so
  a test can assert the property that makes its case an edge.
* ``IOU_PAIRS`` holds nested integer boxes whose exact IoU sits at, just above and just past the
  midpoint above an fp32 threshold (:func:`search_iou_pairs` found them).
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import torch

F32 = np.float32
MAX_WH = 7680.0
REG_MAX = 16
U24 = 2.0 ** -24                 # half an ulp of 1.0 in fp32: the relative error of one rounding


# ---- decode ----------------------------------------------------------------------------------------

def _levels(feats_nhwc, nc):
    for f in feats_nhwc:
        assert f.dtype == torch.bfloat16 and f.shape[-1] == 4 * REG_MAX + nc, (f.dtype, f.shape)
        B, H, W, _ = f.shape
        v = f.float().cpu().numpy().reshape(B, H * W, 4 * REG_MAX + nc)
        yield v, H, W


def _anchors(H, W, dtype):
    r = np.arange(H * W)
    return ((r % W).astype(dtype) + dtype(0.5)), ((r // W).astype(dtype) + dtype(0.5))


def _class_max(cl):
    """(max, first index of the max) of the class logits with NaN dropped (the kernels compare
    with ``>``); an anchor without a logit above -inf gives (-inf, 0)."""
    c = np.where(np.isnan(cl), -np.inf, cl)
    return c.max(-1), c.argmax(-1).astype(np.int32)            # argmax: first occurrence


def decode_ref64(feats_nhwc, strides, nc):
    """fp64 decode of the bf16 values: per side the softmax expectation over the 16 DFL bins,
    ``(anchor + 0.5 -/+ distance) * stride``; fp64 sigmoid of the class maximum; class = FIRST
    index of the maximum (NaN logits are dropped, all -inf gives class 0 and score 0).
    Returns ``boxes [B, A, 4]``, ``scores [B, A]`` (fp64) and ``cls [B, A]`` (int32) as numpy."""
    boxes, scores, classes = [], [], []
    for (v, H, W), s in zip(_levels(feats_nhwc, nc), strides):
        v = v.astype(np.float64)
        box = v[..., :4 * REG_MAX].reshape(v.shape[0], H * W, 4, REG_MAX)
        e = np.exp(box - box.max(-1, keepdims=True))
        d = (e * np.arange(REG_MAX)).sum(-1) / e.sum(-1)
        ax, ay = _anchors(H, W, np.float64)
        boxes.append(np.stack([ax - d[..., 0], ay - d[..., 1], ax + d[..., 2], ay + d[..., 3]], -1) * s)
        m, c = _class_max(v[..., 4 * REG_MAX:])
        with np.errstate(over="ignore"):
            scores.append(1.0 / (1.0 + np.exp(-m)))
        classes.append(c)
    return np.concatenate(boxes, 1), np.concatenate(scores, 1), np.concatenate(classes, 1)


def decode_emul32(feats_nhwc, strides, nc):
    """The kernels' order of operations in fp32 on the CPU: max, ``exp(v - m)``, the two sums in
    index order, one division, ``(ax -/+ d) * s``; ``1 / (1 + exp(-best))``.  (numpy's fp32 exp
    stands in for ``__expf`` and ``sk += e * k`` is rounded twice where the compiler may fuse it:
    this is the cost of fp32, not a bit-exact model.)"""
    boxes, scores, classes = [], [], []
    for (v, H, W), s in zip(_levels(feats_nhwc, nc), strides):
        box = v[..., :4 * REG_MAX].reshape(v.shape[0], H * W, 4, REG_MAX).astype(F32)
        m = box.max(-1)
        se, sk = np.zeros_like(m), np.zeros_like(m)
        for k in range(REG_MAX):
            e = np.exp(box[..., k] - m, dtype=F32)
            se = se + e
            sk = sk + e * F32(k)
        d = sk / se
        ax, ay = _anchors(H, W, F32)
        s32 = F32(s)
        boxes.append(np.stack([(ax - d[..., 0]) * s32, (ay - d[..., 1]) * s32, (ax + d[..., 2]) * s32,
                               (ay + d[..., 3]) * s32], -1))
        best, c = _class_max(v[..., 4 * REG_MAX:].astype(F32))
        with np.errstate(over="ignore"):
            scores.append(F32(1) / (F32(1) + np.exp(-best, dtype=F32)))
        classes.append(c)
    out = np.concatenate(boxes, 1), np.concatenate(scores, 1), np.concatenate(classes, 1)
    assert out[0].dtype == F32 and out[1].dtype == F32
    return out


def expf_rel(d):
    """Relative error allowed to ``__expf(-|d|)``: the kernel evaluates ``exp2(fl(d * log2e))``.
    The product's rounding and the rounding of the constant each move the exponent by at most
    ``|d| log2e 2^-24``, i.e. the result by ``|d| 2^-24`` relative each (times ln 2 < 1); the
    hardware exp2 is good to 1 ulp (2^-23) and is allowed two.  ``(2 |d| + 4) 2^-24``."""
    return (2.0 * np.abs(d) + 4.0) * U24


def decode_expf_margin(feats_nhwc, strides, nc):
    """What ``__expf`` may add to :func:`decode_emul32`'s error, per output element, to first order,
    from the fp64 softmax weights w_k: a relative error eps_k of e_k moves the expectation by
    ``|k - dist| w_k eps_k``, hence a box coordinate by ``stride * sum_k |k - dist| w_k
    expf_rel(v_k - m)`` pixels; the score ``1 / (1 + e)`` moves by ``score (1 - score)
    expf_rel(best)``.  Returns ``(box margin [B, A, 4] pixels, score margin [B, A])``."""
    bm, sm = [], []
    for (v, H, W), s in zip(_levels(feats_nhwc, nc), strides):
        v = v.astype(np.float64)
        box = v[..., :4 * REG_MAX].reshape(v.shape[0], H * W, 4, REG_MAX)
        dlt = box - box.max(-1, keepdims=True)
        e = np.exp(dlt)
        w = e / e.sum(-1, keepdims=True)
        dist = (w * np.arange(REG_MAX)).sum(-1, keepdims=True)
        bm.append(s * (np.abs(np.arange(REG_MAX) - dist) * w * expf_rel(dlt)).sum(-1))
        m, _ = _class_max(v[..., 4 * REG_MAX:])
        with np.errstate(over="ignore", invalid="ignore"):
            sc = 1.0 / (1.0 + np.exp(-m))
            sm.append(np.where(np.isfinite(m), sc * (1.0 - sc) * expf_rel(m), 0.0))
    return np.concatenate(bm, 1), np.concatenate(sm, 1)


def decode_plan(levels, nc, ld, aligned=True):
    """``("tiled" | "flat", tiles)`` as ``aiko_yolo_decode`` chooses (``AIKO_DECODE_FLAT`` unset):
    tiled when the 64-row LDS image fits 64 KiB, ``(64 + nc) * 2 * 64 + 1024 <= 65536``, every
    pitch is a multiple of 8 and at least ``64 + nc``, and the pointers are 16-byte aligned.
    ``levels``: ``(H, W)`` per level; ``ld``: one pitch or one per level; ``tiles``: 64-anchor
    tiles, which never straddle a level."""
    lds = [ld] * len(levels) if isinstance(ld, int) else list(ld)
    tiles = sum(-(-(h * w) // 64) for h, w in levels)
    tiled = (4 * REG_MAX + nc) * 2 * 64 + 16 * 64 <= 64 * 1024 and aligned and \
        all(p % 8 == 0 and p >= 4 * REG_MAX + nc for p in lds)
    return ("tiled" if tiled else "flat"), tiles


# ---- NMS -----------------------------------------------------------------------------------------

def score_keys(scores, conf):
    """The kernel's selection keys: the fp32 bit pattern of a score above ``conf``, else 0 (NaN is
    not above anything).  Monotone in the score only for non-negative floats: a negative score has
    its sign bit set and sorts above every positive one, and +0.0 is key 0, "no candidate" — which
    is why ``topk_nms_out`` refuses ``conf < 0``."""
    s = np.asarray(scores, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.where(s > F32(conf), s.view(np.uint32), np.uint32(0))


def nms_groups(B, cus):
    """Workgroups per image: ``clamp(cus // B, 1, 4)``."""
    return max(1, min(4, cus // max(B, 1)))


def nms_radix_plan(keys, max_cand):
    """Bit shifts of the 12-bit radix-select passes over ``key - min live key``: none when every
    live key is a candidate or all live keys are equal; otherwise from the top of the live range
    down to shift 0 (the last two passes overlap unless the range is a multiple of 12 bits)."""
    live = np.asarray(keys, dtype=np.uint32)
    live = live[live != 0]
    if live.size <= max_cand or live.size == 0:
        return []
    nbits = int(int(live.max()) - int(live.min())).bit_length()
    if nbits == 0:
        return []
    shifts, shift = [], max(0, nbits - 12)
    while shift >= 0:
        shifts.append(shift)
        shift = -1 if shift == 0 else max(0, shift - 12)
    return shifts


def nms_blocks(K, pcls):
    """Count of the 64 x 64 mask blocks ``(rb, w >= rb)`` the kernel computes for ``K`` candidates
    whose classes in (class, rank) position order are ``pcls``: the diagonal ones, and those where
    the class of the first position of block ``w`` is that of the last position of block ``rb``."""
    assert len(pcls) == K
    W = (K + 63) // 64
    return sum(1 for rb in range(W) for w in range(rb, W) if w == rb or pcls[w * 64] == pcls[rb * 64 + 63])


def position_classes(keep_order_cls, neg=False):
    """Classes in the kernel's position order (class ascending, then score rank) of candidates
    given in rank order; one run of class 0 for a negative IoU threshold."""
    return [0] * len(keep_order_cls) if neg else sorted(int(c) for c in keep_order_cls)


def _iou_row(b, area, i, js):
    """fp32 IoU of box i against boxes js, each operation rounded once in ``box_iou_ref``'s order:
    (min - max) clamped at 0 per axis, their product, ``inter / ((area_i + area_j) - inter)``."""
    iw = np.maximum(np.minimum(b[i, 2], b[js, 2]) - np.maximum(b[i, 0], b[js, 0]), F32(0))
    ih = np.maximum(np.minimum(b[i, 3], b[js, 3]) - np.maximum(b[i, 1], b[js, 1]), F32(0))
    inter = iw * ih
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / ((area[i] + area[js]) - inter)


def nms_slow(boxes, scores, cls, conf, iou, max_cand, max_det, max_wh=MAX_WH,
             letterbox=(1.0, 0.0, 0.0, 1e9, 1e9)):
    """Class-aware greedy NMS of ONE image in numpy fp32, without ``nms_ref``'s one pass over all
    candidates: candidates ``score > conf`` ordered by (score descending, index ascending), the
    first ``max_cand`` of them; then an independent greedy loop per class over the class-offset
    boxes (``box + fp32(class) * fp32(max_wh)``, as the kernel and ``nms_ref`` round them) in rank
    order, suppressing ``iou > thr`` with the fp32 division; the kept candidates of all classes in
    rank order, the first ``max_det``.  ``iou < 0``: one run over all candidates (every pair with
    a non-NaN IoU suppresses, across classes too).

    Returns ``(keep, det, count)``: kept anchor indices, and the ``[max_det, 6]`` fp32 rows the
    kernel must write — ``min(max((q - pad) * inv, 0), frame)`` per coordinate with
    ``inv = fp32(1) / fp32(gain)``, the score's bits, the class as a float, then rows
    ``0, 0, 0, 0, 0, -1``."""
    bx = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    sc = np.asarray(scores, dtype=F32).reshape(-1)
    cl = np.asarray(cls, dtype=np.int32).reshape(-1)
    with np.errstate(invalid="ignore"):
        cand = np.nonzero(sc > F32(conf))[0].tolist()
    cand.sort(key=lambda i: (-float(sc[i]), i))
    cand = np.asarray(cand[:max_cand], dtype=np.int64)
    K = cand.size
    off = cl[cand].astype(F32) * F32(max_wh)
    b = bx[cand] + off[:, None]
    assert b.dtype == F32
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    thr = F32(iou)
    runs = [np.arange(K)] if iou < 0 else [np.nonzero(cl[cand] == c)[0] for c in np.unique(cl[cand])]
    kept = np.zeros(K, dtype=bool)
    for run in runs:                                  # ranks of one class, ascending
        removed = np.zeros(run.size, dtype=bool)
        for n in range(run.size):
            if removed[n]:
                continue
            kept[run[n]] = True
            later = run[n + 1:]
            if later.size:
                with np.errstate(invalid="ignore"):
                    removed[n + 1:] |= _iou_row(b, area, run[n], later) > thr
    keep = cand[np.nonzero(kept)[0][:max_det]]
    gain, pad_l, pad_t, fw, fh = (F32(v) for v in letterbox)
    inv = F32(1) / gain
    det = np.zeros((max_det, 6), dtype=F32)
    det[:, 5] = -1
    n = keep.size
    q = bx[keep]
    for j, (pad, lim) in enumerate(((pad_l, fw), (pad_t, fh), (pad_l, fw), (pad_t, fh))):
        det[:n, j] = np.minimum(np.maximum((q[:, j] - pad) * inv, F32(0)), lim)
    det[:n, 4] = sc[keep]
    det[:n, 5] = cl[keep].astype(F32)
    return keep, det, n


# ---- planted IoU pairs -------------------------------------------------------------------------------

IOU_THRESHOLDS = (0.3, 0.45, 0.5, 0.7)


def iou_cuts(t):
    """``(t, m, s)`` as exact fractions: the fp32 threshold, the midpoint above it, the next float."""
    t32 = F32(t)
    s32 = np.nextafter(t32, F32(np.inf))
    tf, sf = Fraction(float(t32)), Fraction(float(s32))
    return tf, (tf + sf) / 2, sf


def classify_iou(pair, t):
    """Where the exact IoU ``x y / (X Y)`` of a nested pair ``((x, y), (X, Y))`` lies: "eq"
    (== t: ``RN(q) == t``, no suppression), "below_m" (t < q < m: rounds to t, no suppression),
    "tie" (q == m), "above_m" (m < q < s: rounds to s, suppression), or None (elsewhere)."""
    (x, y), (X, Y) = pair
    q = Fraction(x * y, X * Y)
    tf, mf, sf = iou_cuts(t)
    return "eq" if q == tf else "below_m" if tf < q < mf else "tie" if q == mf else "above_m" if mf < q < sf else None


def search_iou_pairs(t, draws=4_000_000, seed=0, side=4096):
    """Random nested integer boxes ``[0, 0, x, y]`` in ``[0, 0, X, Y]`` with ``x y + X Y <= 2^24`` (sides
    below ``side``: the areas, their sum and so inter = x y and union = X Y are exact in fp32).  ``X``, ``Y`` and ``x`` are
    drawn; ``y`` is aimed: the integers next to ``t X Y / x`` and ``m X Y / x``, the only ones that
    can land in [t, s).  Returns the pairs whose exact IoU does, by class: ``{"eq": [...],
    "below_m": [...], "tie": [...], "above_m": [...]}`` of ``((x, y), (X, Y))``.  Integer
    arithmetic: the cuts are dyadic fractions n / 2^k, ``x y 2^k`` vs ``n X Y`` fits 64 bits."""
    rng = np.random.default_rng(seed)
    X = rng.integers(2, side, draws, dtype=np.int64)
    Y = rng.integers(2, side, draws, dtype=np.int64)
    x = rng.integers(1, X + 1)
    ok = X * Y < (1 << 24)
    X, Y, x = X[ok], Y[ok], x[ok]
    tf, mf, sf = iou_cuts(t)
    den = max(tf.denominator, mf.denominator, sf.denominator)
    assert den & (den - 1) == 0 and den <= 1 << 26
    tn, mn, sn = (int(f * den) for f in (tf, mf, sf))
    U = X * Y
    found = {"eq": [], "below_m": [], "tie": [], "above_m": []}
    for cut in (tn, mn):
        for up in (0, 1):
            y = cut * U // (den * x) + up
            lhs = x * y * den
            hit = np.nonzero((y >= 1) & (y <= Y) & (x * y + U <= 1 << 24) & (lhs >= tn * U) & (lhs < sn * U))[0]
            for i in hit.tolist():
                pair = ((int(x[i]), int(y[i])), (int(X[i]), int(Y[i])))
                found[classify_iou(pair, t)].append(pair)
    return {k: sorted(set(v)) for k, v in found.items()}


# Found by search_iou_pairs (seed 0, 4e6 draws) plus the ratios 63/140, 70/140 and 98/140 (the
# decimals 0.45 and 0.7 themselves lie just above t: fp32(0.45) and fp32(0.7) round DOWN).
# Classes that do not exist, hence the empty lists:
#   * "eq" at 0.3f / 0.45f / 0.7f: t = n / 2^24 with n odd, so x y 2^24 = n X Y needs
#     2^24 | X Y, while X Y < 2^24;
#   * "below_m" at 0.5: 2 inter - union is an integer, so q is 0.5 or at least 1 / (2 union)
#     > 2^-25 above it, past m = 0.5 + 2^-25 (and below s = 0.5 + 2^-24 once union > 2^23:
#     "above_m" does exist there);
#   * "tie" at every threshold (see test_detect_refs.py).
IOU_PAIRS = {
    0.3: {"eq": [],
          "below_m": [((332, 3470), (1067, 3599)), ((685, 2053), (1911, 2453))],
          "above_m": [((346, 2281), (751, 3503)), ((1388, 1135), (2227, 2358))]},
    0.45: {"eq": [],
           "below_m": [((63, 744), (140, 744)), ((3939, 816), (4040, 1768))],
           "above_m": [((1021, 1961), (2057, 2163)), ((1241, 1165), (1869, 1719))]},
    0.5: {"eq": [((70, 744), (140, 744)), ((4068, 589), (4068, 1178))],
          "below_m": [],
          "above_m": [((1171, 3620), (2253, 3763)), ((2938, 1469), (2939, 2937))]},
    0.7: {"eq": [],
          "below_m": [((98, 744), (140, 744)), ((3920, 195), (4000, 273))],
          "above_m": [((552, 3040), (677, 3541)), ((3658, 1035), (3974, 1361))]},
}
SUPPRESSES = {"eq": False, "below_m": False, "above_m": True}


def planted_pairs():
    """``(t, class, pair)`` for every pair of the table."""
    return [(t, k, p) for t in IOU_THRESHOLDS for k in ("eq", "below_m", "above_m") for p in IOU_PAIRS[t][k]]


def pair_boxes(pair, origin=(0.0, 0.0)):
    """The two xyxy boxes of a nested pair (inner first), moved to ``origin`` (an integer offset
    keeps every side exact)."""
    (x, y), (X, Y) = pair
    ox, oy = origin
    return [ox, oy, ox + x, oy + y], [ox, oy, ox + X, oy + Y]
