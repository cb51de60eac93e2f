"""The torch references of the ROI crop op (``ops/reference.py``): rects against hand-worked
values, the crop against a plain slice.  CPU only."""
import torch

from aiko_services_amd.ops.reference import roi_crop_ref, roi_rects_ref

H, W = 37, 53
NAN = float("nan")


def _det(rows, max_det=None):
    """[1, max_det, 6] detections from (x1, y1, x2, y2) rows; score 0.5, class 0."""
    max_det = max_det or len(rows)
    d = torch.zeros(1, max_det, 6)
    d[:, :, 5] = -1
    for i, r in enumerate(rows):
        d[0, i] = torch.tensor([*r, 0.5, 0.0])
    return d


def _rects(rows, count, k, margin=0.0, max_det=None):
    return roi_rects_ref(_det(rows, max_det), torch.tensor([count], dtype=torch.int32), k, (H, W), margin).tolist()


def test_fractional_box_rounds_outwards():
    # floor(10.3) = 10, floor(5.7) = 5, ceil(20.2) = 21, ceil(9.1) = 10
    assert _rects([(10.3, 5.7, 20.2, 9.1)], 1, 1) == [[10, 5, 21, 10]]


def test_margin_grows_the_box_by_its_own_size():
    # bw = 8, bh = 4 -> ex = 2, ey = 1 (0.25 is exact in fp32): x 10 - 2 .. 18 + 2, y 8 - 1 .. 12 + 1
    assert _rects([(10.0, 8.0, 18.0, 12.0)], 1, 1, margin=0.25) == [[8, 7, 20, 13]]
    # bw = 8.5, bh = 5 -> ex = 2.125, ey = 1.25: floor(8.375) = 8, ceil(21.125) = 22, floor(6.75) = 6, ceil(14.25) = 15
    assert _rects([(10.5, 8.0, 19.0, 13.0)], 1, 1, margin=0.25) == [[8, 6, 22, 15]]


def test_box_past_the_right_and_bottom_edges_is_clamped():
    assert _rects([(40.0, 30.0, 80.0, 90.0)], 1, 1) == [[40, 30, W, H]]
    # wholly outside: X0 = clamp(60, 0, W - 1) = 52, X1 = clamp(70, 53, 53); the same for Y
    assert _rects([(60.0, 50.0, 70.0, 55.0)], 1, 1) == [[W - 1, H - 1, W, H]]


def test_negative_coordinates_are_clamped_to_zero():
    assert _rects([(-7.5, -3.2, 12.5, 9.0)], 1, 1) == [[0, 0, 13, 9]]
    # wholly left of / above the frame: X0 = 0, X1 = clamp(-5, 1, W) = 1
    assert _rects([(-20.0, -30.0, -5.0, -4.0)], 1, 1) == [[0, 0, 1, 1]]


def test_zero_area_box_gives_one_pixel():
    assert _rects([(12.0, 7.0, 12.0, 7.0)], 1, 1) == [[12, 7, 13, 8]]
    # sub-pixel box inside one pixel
    assert _rects([(12.25, 7.5, 12.75, 7.75)], 1, 1) == [[12, 7, 13, 8]]


def test_nan_row_is_invalid_and_zero():
    rows = [(1.0, 2.0, 5.0, 6.0), (NAN, 2.0, 5.0, 6.0), (1.0, 2.0, 5.0, float("inf")), (3.0, 4.0, 9.0, 8.0)]
    assert _rects(rows, 4, 4) == [[1, 2, 5, 6], [0, 0, 0, 0], [0, 0, 0, 0], [3, 4, 9, 8]]


def test_count_zero_and_negative_use_no_row():
    rows = [(1.0, 2.0, 5.0, 6.0), (3.0, 4.0, 9.0, 8.0)]
    assert _rects(rows, 0, 2) == [[0, 0, 0, 0]] * 2
    assert _rects(rows, -3, 2) == [[0, 0, 0, 0]] * 2


def test_count_above_k_is_truncated_and_rows_past_count_are_ignored():
    rows = [(1.0, 2.0, 5.0, 6.0), (3.0, 4.0, 9.0, 8.0), (2.0, 2.0, 4.0, 4.0)]
    assert _rects(rows, 3, 2) == [[1, 2, 5, 6], [3, 4, 9, 8]]                 # count > K
    assert _rects(rows, 300, 2, max_det=3) == [[1, 2, 5, 6], [3, 4, 9, 8]]
    assert _rects(rows, 1, 3) == [[1, 2, 5, 6], [0, 0, 0, 0], [0, 0, 0, 0]]   # K > count
    garbage = [(1.0, 2.0, 5.0, 6.0), (NAN, NAN, NAN, NAN), (1e30, -1e30, 7.0, 7.0)]
    assert _rects(garbage, 1, 3) == [[1, 2, 5, 6], [0, 0, 0, 0], [0, 0, 0, 0]]


def test_slots_are_frame_major():
    det = torch.cat([_det([(1.0, 2.0, 5.0, 6.0), (0.0, 0.0, 2.0, 2.0)]), _det([(3.0, 4.0, 9.0, 8.0), (0.0, 0.0, 2.0, 2.0)])])
    got = roi_rects_ref(det, torch.tensor([1, 2], dtype=torch.int32), 2, (H, W), 0.0)
    assert got.dtype == torch.int32 and got.shape == (4, 4)
    assert got.tolist() == [[1, 2, 5, 6], [0, 0, 0, 0], [3, 4, 9, 8], [0, 0, 2, 2]]


def test_products_are_rounded_before_the_sums():
    # fp32(0.1) * 1000 = 100.0000015 rounds to 100.0, so 104 - ex = 4 exactly (a fused multiply-add
    # would give 3.9999986 -> 3) and -96 + ex = 4 exactly (fused: 4.0000014 -> 5)
    assert _rects([(104.0, 0.0, 1104.0, 1.0)], 1, 1, margin=0.1)[0][0] == 4
    assert _rects([(-1096.0, 0.0, -96.0, 1.0)], 1, 1, margin=0.1)[0][2] == 4


def test_crop_of_an_aligned_box_is_the_slice():
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, generator=g)
    Ho, Wo = 20, 24
    det = torch.cat([_det([(5.0, 3.0, 5.0 + Wo, 3.0 + Ho)], 2), _det([(29.0, 17.0, 29.0 + Wo, 17.0 + Ho)], 2)])
    crops, rois = roi_crop_ref(frames, det, torch.tensor([1, 1], dtype=torch.int32), 2, (Ho, Wo), 0.0)
    assert crops.dtype == torch.uint8 and crops.shape == (4, Ho, Wo, 3)
    assert rois.tolist() == [[5, 3, 29, 23], [0, 0, 0, 0], [29, 17, 53, 37], [0, 0, 0, 0]]
    assert torch.equal(crops[0], frames[0, 3:23, 5:29])
    assert torch.equal(crops[2], frames[1, 17:37, 29:53])
    assert not crops[1].any() and not crops[3].any()
