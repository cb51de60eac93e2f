"""CPU tests of tests/detect_refs.py: the references, launch plans and planted cases that
tests/test_gpu_guard_detect.py holds the detection kernels to."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import detect_refs as D
from aiko_services_amd.ops import reference as R

F32 = np.float32
BF16 = torch.bfloat16


# ---- nms_slow against nms_ref (both on the CPU) ------------------------------------------------------

def _random_dets(A, g, n_centers=40, n_cls=3):
    centers = torch.rand(n_centers, 2, generator=g) * 600
    pick = torch.randint(0, n_centers, (A,), generator=g)
    c = centers[pick] + torch.randn(A, 2, generator=g) * 6
    wh = 20 + torch.rand(A, 2, generator=g) * 60
    boxes = torch.cat([c - wh / 2, c + wh / 2], -1)
    scores = (torch.rand(A, generator=g) * 256).floor() / 256      # many exact ties
    cls = torch.randint(0, n_cls, (A,), generator=g, dtype=torch.int32)
    return boxes, scores, cls


def _ref_image(boxes, scores, cls, keep, max_det):
    det = torch.zeros(max_det, 6)
    det[:, 5] = -1
    n = keep.numel()
    det[:n] = torch.cat([boxes[keep].clamp(min=0), scores[keep, None], cls[keep, None].float()], 1)
    return det.numpy(), n


@pytest.mark.parametrize("A,conf,max_cand,max_det,n_cls,iou", [
    (3000, 0.25, 1024, 300, 3, 0.5), (2000, 0.1, 256, 50, 3, 0.5), (33, 0.0, 1024, 300, 3, 0.5),
    (3000, 0.25, 1024, 1024, 1, 0.3), (3000, 0.25, 1024, 300, 80, 0.7), (3000, 0.25, 1000, 100, 1000, 0.5),
    (700, 0.1, 1024, 300, 80, -1.0), (2500, 0.5, 777, 13, 7, 0.45), (100, 2.0, 64, 8, 3, 0.5)])
def test_nms_slow_matches_nms_ref(A, conf, max_cand, max_det, n_cls, iou):
    g = torch.Generator().manual_seed(A + max_det + n_cls)
    boxes, scores, cls = _random_dets(A, g, n_cls=n_cls)
    keep = R.nms_ref(boxes, scores, cls, conf, iou, max_cand, max_det)
    k2, det, n = D.nms_slow(boxes.numpy(), scores.numpy(), cls.numpy(), conf, iou, max_cand, max_det)
    assert k2.tolist() == keep.tolist()
    want, nw = _ref_image(boxes, scores, cls, keep, max_det)
    assert n == nw and np.array_equal(det.view(np.uint32), want.view(np.uint32))


def _pair_scene(t, pair):
    inner, outer = D.pair_boxes(pair, origin=(16.0, 32.0))
    boxes = torch.tensor([outer, inner, [5000.0, 5000.0, 5010.0, 5010.0]])
    return boxes, torch.tensor([0.9, 0.8, 0.7]), torch.zeros(3, dtype=torch.int32)


@pytest.mark.parametrize("t,kind,pair", D.planted_pairs(), ids=lambda v: str(v).replace(" ", ""))
def test_planted_pairs(t, kind, pair):
    """Each pair is where the table says (exact rational arithmetic), fp32 division on the CPU
    rounds it to the side the table claims, and both references act on it accordingly."""
    (x, y), (X, Y) = pair
    assert 0 < x <= X and 0 < y <= Y and x * y + X * Y <= 1 << 24 and max(X, Y) + 32 < D.MAX_WH
    assert D.classify_iou(pair, t) == kind
    tf, mf, sf = D.iou_cuts(t)
    q = Fraction(x * y, X * Y)
    rn = F32(x * y) / F32(X * Y)
    assert float(F32(x * y)) == x * y and float(F32(X * Y)) == X * Y
    if kind == "eq":
        assert q == tf and rn == F32(t)
    elif kind == "below_m":
        assert tf < q < mf and rn == F32(t)
    else:
        assert mf < q < sf and rn == np.nextafter(F32(t), F32(np.inf)) and rn > F32(t)
    assert D.SUPPRESSES[kind] == bool(rn > F32(t))
    boxes, scores, cls = _pair_scene(t, pair)
    iou = float(R.box_iou_ref(boxes[:2], boxes[:2])[0, 1])
    assert F32(iou) == rn                                   # the offset origin keeps the sides exact
    want = [0, 2] if D.SUPPRESSES[kind] else [0, 1, 2]
    assert R.nms_ref(boxes, scores, cls, 0.1, t, 8, 8).tolist() == want
    assert D.nms_slow(boxes.numpy(), scores.numpy(), cls.numpy(), 0.1, t, 8, 8)[0].tolist() == want


def test_pair_table_covers_what_exists():
    """Every class that exists has pairs; the classes the table leaves empty are the ones the
    search cannot find either."""
    for t in D.IOU_THRESHOLDS:
        found = D.search_iou_pairs(t, draws=400_000, seed=1)
        for kind in ("eq", "below_m", "above_m"):
            if not D.IOU_PAIRS[t][kind]:
                assert not found[kind], (t, kind, found[kind][:2])
            else:
                assert len(D.IOU_PAIRS[t][kind]) >= 2
    assert not D.IOU_PAIRS[0.5]["below_m"] and all(not D.IOU_PAIRS[t]["eq"] for t in (0.3, 0.45, 0.7))


# The `thr_tie && in == d` branch of mask_word cannot be reached.  m is the midpoint of two
# adjacent fp32 numbers t < s, so m = n / 2^k with n an odd 25-bit integer.  A tie needs
# inter == m * union exactly, i.e. inter * 2^k == n * union with inter and union fp32 numbers (24-bit
# significands I, U times powers of two): n * U must then be I times a power of two, but n is odd
# and has 25 significant bits, so n * U has at least 25 significant bits after its trailing zeros are
# removed (the odd part of n * U is n times the odd part of U, >= n >= 2^24), while I has at most
# 24.  The branch is kept for the argument's sake (a threshold whose m had fewer bits); no input
# reaches it, and a mutant that drops it is equivalent.
@pytest.mark.parametrize("t", D.IOU_THRESHOLDS)
def test_iou_tie_is_unreachable(t):
    tf, mf, sf = D.iou_cuts(t)
    assert mf.numerator % 2 == 1 and mf.numerator.bit_length() == 25
    found = D.search_iou_pairs(t, draws=1_000_000, seed=2)
    assert found["tie"] == []
    assert len(found["eq"]) + len(found["below_m"]) + len(found["above_m"]) > 0    # the search does hit [t, s)
    # the integer form of the argument, on random 24-bit significands
    rng = np.random.default_rng(3)
    n = mf.numerator
    for U in rng.integers(1 << 23, 1 << 24, 2000).tolist():
        odd = n * U
        odd //= odd & -odd
        assert odd.bit_length() >= 25


# ---- keys ----------------------------------------------------------------------------------------

def test_score_keys_order_only_non_negative_scores():
    """Why topk_nms_out refuses conf < 0: the keys order scores as floats only from +0 up."""
    s = np.array([0.0, 1e-45, 1e-38, 0.1, 0.5, 1.0, np.inf], dtype=F32)
    k = D.score_keys(s, -1.0)
    assert (np.diff(k[1:].astype(np.int64)) > 0).all()        # positive floats: monotone
    assert k[0] == 0                                          # 0.0 > -1 is a candidate but has key 0: dropped
    neg = D.score_keys(np.array([-0.5, -0.25], dtype=F32), -1.0)
    assert (neg > k.max()).all()                              # negative scores sort above +inf
    assert neg[0] > neg[1]                                    # and among themselves backwards
    # with conf >= 0 none of these is a candidate, NaN and -0.0 neither, and conf itself is not
    c = F32(0.1)
    edge = np.array([np.nan, -0.0, -3.0, c, np.nextafter(c, F32(1))], dtype=F32)
    assert D.score_keys(edge, 0.1).tolist() == [0, 0, 0, 0, int(np.nextafter(c, F32(1)).view(np.uint32))]
    assert D.score_keys(np.array([0.0, -0.0, 1e-45], dtype=F32), 0.0).tolist() == [0, 0, 1]


# ---- decode --------------------------------------------------------------------------------------

def _heads(B, sizes, nc, g, scale=2.0):
    return [(torch.randn(B, h, w, 64 + nc, generator=g) * scale).to(BF16) for h, w in sizes]


def test_decode_ref64_matches_yolo_decode_ref_away_from_ties():
    g = torch.Generator().manual_seed(5)
    feats = _heads(2, [(8, 8), (5, 5), (3, 2)], 80, g)
    b, s, c = D.decode_ref64(feats, (8, 16, 32), 80)
    rb, rs, rc = R.yolo_decode_ref([f.permute(0, 3, 1, 2) for f in feats], (8, 16, 32), 80)
    srt = torch.cat([f[..., 64:].reshape(2, -1, 80) for f in feats], 1).float().sort(-1).values
    clear = (srt[..., -1] > srt[..., -2]).numpy()
    assert clear.mean() > 0.9
    assert (c == rc.numpy())[clear].all()
    assert np.abs(b - rb.double().numpy()).max() < 1e-3 and np.abs(s - rs.double().numpy()).max() < 1e-6


def test_decode_first_index_rule_on_planted_ties():
    g = torch.Generator().manual_seed(6)
    nc = 40
    f = _heads(1, [(2, 4)], nc, g)[0]
    cl = f[0].reshape(8, 64 + nc)[:, 64:]
    cl.clamp_(max=3.0)
    cl[0, [5, 13]] = 4.0            # tie across quad chunks k, k + 8
    cl[1, [21, 5 + 24, 37]] = 4.0   # k + 16, k + 24, k + 32
    cl[2, [9, 10]] = 4.0            # inside one chunk
    cl[3, :] = float("-inf")        # nothing above -inf: class 0, score 0
    cl[4, 7] = float("nan")         # a NaN is never the maximum
    cl[4, 30] = 3.5
    cl[5, :] = 1.0                  # every class tied
    for fn in (D.decode_ref64, D.decode_emul32):
        _, s, c = fn([f], (8,), nc)
        assert c[0, :6].tolist() == [5, 21, 9, 0, 30, 0], fn.__name__
        assert s[0, 3] == 0 and abs(s[0, 4] - 1 / (1 + np.exp(-3.5))) < 1e-6


def test_decode_one_hot_rows_and_emul32_error():
    """A one-hot DFL row gives the distance k exactly; on random heads decode_emul32 stays within a
    few fp32 roundings of decode_ref64, and the __expf margin is of the same order — both orders
    below the 1e-2 the old decode test allowed."""
    g = torch.Generator().manual_seed(7)
    f = _heads(1, [(3, 3)], 8, g)[0]
    rows = f[0].reshape(9, 72)
    rows[:, :64] = -60.0
    for a in range(9):
        for side in range(4):
            rows[a, side * 16 + (a + 3 * side) % 16] = 60.0
    b64, _, _ = D.decode_ref64([f], (16,), 8)
    b32, _, _ = D.decode_emul32([f], (16,), 8)
    for a in range(9):
        k = [(a + 3 * side) % 16 for side in range(4)]
        ax, ay = a % 3 + 0.5, a // 3 + 0.5
        want = [(ax - k[0]) * 16, (ay - k[1]) * 16, (ax + k[2]) * 16, (ay + k[3]) * 16]
        assert b64[0, a].tolist() == want and b32[0, a].tolist() == want
    feats = _heads(2, [(8, 8), (5, 5), (1, 1)], 80, g, scale=3.0)
    strides = (8, 16, 32)
    b64, s64, c64 = D.decode_ref64(feats, strides, 80)
    b32, s32, c32 = D.decode_emul32(feats, strides, 80)
    assert np.array_equal(c64, c32)
    lvl_s = np.repeat(np.array(strides, dtype=np.float64), [64, 25, 1])
    e_box = (np.abs(b32 - b64) / lvl_s[None, :, None]).max()
    e_sc = np.abs(s32 - s64).max()
    bm, sm = D.decode_expf_margin(feats, strides, 80)
    print(f"decode_emul32 vs decode_ref64: boxes {e_box:.3e} strides, scores {e_sc:.3e}; "
          f"__expf margin: boxes {(bm / lvl_s[None, :, None]).max():.3e} strides, scores {sm.max():.3e}")
    assert e_box < 64 * D.U24 * 16 and e_sc < 8 * D.U24          # a few dozen roundings of values below 16
    assert (bm / lvl_s[None, :, None]).max() < 1e-4 and sm.max() < 1e-5


# ---- plans ----------------------------------------------------------------------------------------

def test_nms_groups_hand_checked():
    assert [D.nms_groups(B, 256) for B in (64, 65, 85, 86, 128, 129)] == [4, 3, 3, 2, 2, 1]
    assert [D.nms_groups(B, 256) for B in (1, 2, 256, 257, 1000)] == [4, 4, 1, 1, 1]
    assert [D.nms_groups(B, 304) for B in (76, 77, 101, 102, 152, 153)] == [4, 3, 3, 2, 2, 1]


def test_nms_radix_plan_hand_checked():
    k0 = 0x3F000000
    few = np.arange(k0, k0 + 100, dtype=np.uint32)
    assert D.nms_radix_plan(few, 100) == [] and D.nms_radix_plan(few, 99) == [0]     # 7-bit range
    assert D.nms_radix_plan(np.full(500, k0, dtype=np.uint32), 64) == []             # range 0
    assert D.nms_radix_plan(np.array([k0, k0 + 1] * 50, dtype=np.uint32), 64) == [0]   # 1 bit
    assert D.nms_radix_plan(np.array([k0, k0 + 4095] * 50, dtype=np.uint32), 64) == [0]  # 12 bits: one pass
    assert D.nms_radix_plan(np.array([k0, k0 + 4096] * 50, dtype=np.uint32), 64) == [1, 0]
    assert D.nms_radix_plan(np.array([k0, k0 + (1 << 24)] * 50, dtype=np.uint32), 64) == [13, 1, 0]   # 25 bits
    assert D.nms_radix_plan(np.array([1, 0x3F800000] * 50, dtype=np.uint32), 64) == [18, 6, 0]        # 30 bits
    assert D.nms_radix_plan(np.array([1, 0x7F800000] * 50, dtype=np.uint32), 64) == [19, 7, 0]        # 31 bits
    assert D.nms_radix_plan(np.array([0, 0, k0, 0], dtype=np.uint32), 1) == []       # dead keys do not count
    keys = D.score_keys(np.array([1e-45, 1.0, np.inf, 0.0, np.nan], dtype=F32).repeat(30), 0.0)
    assert D.nms_radix_plan(keys, 64) == [19, 7, 0]


def test_nms_blocks_hand_checked():
    assert D.nms_blocks(1, [0]) == 1 and D.nms_blocks(64, [0] * 64) == 1 and D.nms_blocks(65, [0] * 65) == 3
    assert D.nms_blocks(1024, [0] * 1024) == 136                          # one class: the whole triangle
    assert D.nms_blocks(1024, list(range(1024))) == 16                    # a run per candidate: the diagonal
    assert D.nms_blocks(192, [0] * 192) == 6                              # one class over three blocks
    assert D.nms_blocks(192, [0] * 64 + [1] * 128) == 4                   # runs end on block edges
    assert D.nms_blocks(192, [0] * 63 + [1] * 129) == 6                   # block 0 ends in the class block 1, 2 start with
    assert D.nms_blocks(192, [0] * 65 + [1] * 127) == 5                   # (0, 1) shares class 0; (0, 2) does not; (1, 2) does
    assert D.position_classes([2, 0, 1, 0]) == [0, 0, 1, 2] and D.position_classes([2, 0], neg=True) == [0, 0]


def test_decode_plan_hand_checked():
    lv = [(8, 8), (5, 5), (1, 1)]
    assert D.decode_plan(lv, 80, 144) == ("tiled", 3)
    assert D.decode_plan([(8, 8), (13, 5), (1, 1), (3, 21)], 80, 160) == ("tiled", 1 + 2 + 1 + 1)
    assert D.decode_plan(lv, 440, 504) == ("tiled", 3) and (64 + 440 + 8) * 2 * 64 == 65536
    assert D.decode_plan(lv, 448, 512) == ("flat", 3)
    assert D.decode_plan(lv, 80, [144, 160, 148]) == ("flat", 3)          # a pitch that is no multiple of 8
    assert D.decode_plan(lv, 80, 144, aligned=False) == ("flat", 3)
    assert D.decode_plan(lv, 80, 136) == ("flat", 3)
