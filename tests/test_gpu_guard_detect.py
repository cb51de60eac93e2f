"""Guard-band, poison and exact-parity runs of the detection post-processing kernels of
detect_ops.hip (run on MI355X: -m gpu): yolo_decode_kernel, yolo_decode_tiled_kernel and
nms_fused_kernel, reached through ``ops.detect.yolo_decode`` and ``ops.detect.topk_nms``.  The
references, launch plans and planted cases are tests/detect_refs.py (checked on the CPU by
tests/test_detect_refs.py); every reference here is evaluated on the CPU.

Every case follows ``guard_ops.run_both``: a *plain* run on fresh tensors and a *guarded* run in
which every tensor the binding receives is a view between two poison guards (the decode heads also
as channel slices of wider buffers whose gaps hold poison), outputs prefilled with NaN / 0xA5 bytes.
Guards intact, guarded outputs written and bit-identical to the plain run; then the numeric check.

Decode.  The tiled and the per-anchor kernel (``AIKO_DECODE_FLAT=1``) are bit-identical; classes
equal ``decode_ref64`` on EVERY anchor (first index of the maximum, NaN dropped, all -inf -> 0);
boxes and scores are held per element to

    |box - ref64|   <= E_BOX * stride + box margin      (pixels)
    |score - ref64| <= E_SCORE + score margin

where E_BOX / E_SCORE are the worst errors of ``decode_emul32`` (the kernel's operation order in
fp32 on the CPU) against ``decode_ref64`` over this file's whole decode case table, and the margins
are ``decode_expf_margin``: what ``__expf`` may add, per element, with ``expf_rel(d) = (2 |d| + 4)
2^-24`` (two roundings of the argument scaling, which grow with the logit spread, and 2 ulp for
the hardware exp2).  CPU figures: E_BOX = 3.5e-6 strides, E_SCORE = 8.5e-8; the largest bounds of
the table are 1.8e-4 pixels (stride 32) and 1.6e-7 (score).  Measured on MI355X: worst box error
1.05e-4 pixels (nc 448, 4 levels; bound there 1.77e-4), worst score error 8.5e-8.  The old decode
test allowed 1e-2.

NMS.  ``det`` / ``count`` are compared BIT FOR BIT with ``nms_slow``'s image.  The poison is 3e38,
not NaN: the kernel selects with ``score > conf``, which drops a NaN, so a read past ``A`` of a
NaN-filled score guard would be invisible, while 3e38 wins every selection and shows as row 0.
``det`` is prefilled with NaN and ``count`` with 0xA5 bytes in both runs.  Each case asserts the
plan property that makes it an edge (workgroups per image, radix passes, mask blocks, chunk
boundaries).  The IoU threshold cases use every planted pair of ``detect_refs.IOU_PAIRS`` on both
sides of the midpoint m above the fp32 threshold; m itself (the ``thr_tie`` branch of
``mask_word``) cannot be reached, see tests/test_detect_refs.py.
"""
import functools

import numpy as np
import pytest
import torch

import detect_refs as D
from guard_ops import BF16, DEV, _bits, run_both

pytestmark = pytest.mark.gpu

F32 = np.float32
I32_POISON = -1515870811          # 0xA5A5A5A5: what an unwritten int32 output holds in both runs
NEG_INF = float("-inf")


# ---- decode ----------------------------------------------------------------------------------------

# H*W of 1, 25, 63, 64 and 65 appear: a level smaller than one tile, full tiles, a partial last tile
DECODE_LEVELS = {
    "1lvl": ([(5, 5)], (8,)),
    "3lvl": ([(9, 7), (8, 8), (1, 1)], (8, 16, 32)),
    "4lvl": ([(13, 5), (5, 5), (1, 1), (8, 8)], (4, 8, 16, 32)),
}
DECODE_NC = (8, 16, 40, 80, 88, 440, 448)
DECODE_B = 2


@functools.lru_cache(maxsize=None)
def _decode_heads(nc, key):
    """Random bf16 heads (logits * 3, so class ties among the few bf16 values near the maximum do
    occur) with planted anchors in level 0 of image 0 — and the same ties in the LAST anchor of
    the last level of image 1, the last row of a partial tile."""
    sizes, _ = DECODE_LEVELS[key]
    g = torch.Generator().manual_seed(1000 + nc + len(sizes))
    feats = [(torch.randn(DECODE_B, h, w, 64 + nc, generator=g) * 3).to(BF16) for h, w in sizes]
    rows = feats[0][0].reshape(-1, 64 + nc)
    assert rows.shape[0] >= 8
    cross = [k for k in (5, 13, 21, 29) if k < nc]             # the same place in quad chunks k, k+8, k+16, k+24
    for r in (rows[0], feats[-1][1].reshape(-1, 64 + nc)[-1]):
        r[64:].clamp_(max=3.0)
        r[64 + torch.tensor(cross)] = 4.0
    rows[1, 64:].clamp_(max=3.0)
    rows[1, 64 + 2] = rows[1, 64 + 3] = 4.0                     # a tie inside one chunk
    rows[2, 64:] = NEG_INF                                      # nothing above -inf: class 0, score 0
    rows[3, :64] = -60.0                                        # one-hot DFL rows: distance exactly k
    for side, k in enumerate((0, 15, 7, 8)):
        rows[3, side * 16 + k] = 60.0
    rows[4, :64] = torch.tensor([30.0, -30.0] * 32)             # spread +-30
    rows[5, 64 + 1] = float("nan")                              # a NaN logit is never the maximum
    rows[6, 64:] = 1.0                                          # every class tied
    rows[7, 64:] = NEG_INF
    rows[7, 64 + nc - 1] = -5.0                                 # the only finite logit is the last one
    return tuple(feats)


@functools.lru_cache(maxsize=None)
def _decode_refs(nc, key):
    feats = _decode_heads(nc, key)
    sizes, strides = DECODE_LEVELS[key]
    lvl_s = np.repeat(np.array(strides, dtype=np.float64), [h * w for h, w in sizes])
    b64, s64, c64 = D.decode_ref64(feats, strides, nc)
    b32, s32, c32 = D.decode_emul32(feats, strides, nc)
    assert np.array_equal(c64, c32)
    bm, sm = D.decode_expf_margin(feats, strides, nc)
    e_box = (np.abs(b32 - b64) / lvl_s[None, :, None]).max()
    e_score = np.abs(s32 - s64).max()
    return b64, s64, c64, bm, sm, lvl_s, e_box, e_score


@functools.lru_cache(maxsize=None)
def _decode_cpu_figures():
    """(E_BOX in strides, E_SCORE): decode_emul32 against decode_ref64 over the whole case table."""
    figs = [_decode_refs(nc, key)[6:] for nc in DECODE_NC for key in DECODE_LEVELS]
    return max(f[0] for f in figs), max(f[1] for f in figs)


def _decode_case(feats, strides, nc, sliced):
    from aiko_services_amd.ops import detect as DT
    B = feats[0].shape[0]
    A = sum(f.shape[1] * f.shape[2] for f in feats)
    pitch = 64 + nc + 16

    def case(ops):
        if sliced:
            fs = [ops.inp_slice(f, pitch, 8, f"head {i}") for i, f in enumerate(feats)]
            assert all(f.stride(2) == pitch and f.storage_offset() % 8 == 0 for f in fs)
        else:
            fs = [ops.inp(f, f"head {i}") for i, f in enumerate(feats)]
        boxes = ops.out((B, A, 4), torch.float32, "boxes")
        scores = ops.out((B, A), torch.float32, "scores")
        cls = ops.out((B, A), torch.int32, "cls")
        if not ops.on:
            cls.fill_(I32_POISON)
        DT.yolo_decode(fs, strides, nc, boxes=boxes, scores=scores, cls=cls)
        return boxes, scores, cls

    return case


@pytest.mark.parametrize("sliced", [False, True], ids=["contiguous", "sliced"])
@pytest.mark.parametrize("key", list(DECODE_LEVELS))
@pytest.mark.parametrize("nc", DECODE_NC)
def test_yolo_decode_guarded(native, monkeypatch, nc, key, sliced):
    """nc = 8: three lanes of a quad have no class chunk; 440: the largest tiled (64 KiB of LDS);
    448: flat by the LDS rule.  Heads contiguous, or channels [8, 8 + 64 + nc) of a buffer of
    pitch 64 + nc + 16 whose gaps are poison."""
    sizes, strides = DECODE_LEVELS[key]
    feats = _decode_heads(nc, key)
    pitch = 64 + nc + 16 if sliced else 64 + nc
    kind, tiles = D.decode_plan(sizes, nc, pitch)
    assert kind == ("flat" if nc >= 448 else "tiled")
    assert tiles == sum(-(-h * w // 64) for h, w in sizes) and (nc != 440 or (64 + nc + 8) * 128 == 65536)
    case = _decode_case(feats, strides, nc, sliced)
    monkeypatch.delenv("AIKO_DECODE_FLAT", raising=False)
    tiled = [t.cpu() for t in run_both(case)]
    monkeypatch.setenv("AIKO_DECODE_FLAT", "1")
    flat = [t.cpu() for t in run_both(case)]
    for name, a, b in zip(("boxes", "scores", "cls"), tiled, flat):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: the tiled and the per-anchor kernel differ"
    boxes, scores, cls = (t.numpy() for t in tiled)
    b64, s64, c64, bm, sm, lvl_s, _, _ = _decode_refs(nc, key)
    wrong = np.argwhere(cls != c64)
    assert wrong.size == 0, f"{len(wrong)} anchor(s) with the wrong class, first (b, a) = {wrong[0].tolist()}: " \
        f"{cls[tuple(wrong[0])]} for {c64[tuple(wrong[0])]}"
    e_box, e_score = _decode_cpu_figures()
    berr, serr = np.abs(boxes.astype(np.float64) - b64), np.abs(scores.astype(np.float64) - s64)
    bbound, sbound = e_box * lvl_s[None, :, None] + bm, e_score + sm
    print(f"decode nc {nc} {key} {'sliced' if sliced else 'contiguous'}: worst box error {berr.max():.3e} px "
          f"(largest bound {bbound.max():.3e}, E_BOX {e_box:.3e} strides), worst score error {serr.max():.3e} "
          f"(largest bound {sbound.max():.3e}, E_SCORE {e_score:.3e})")
    assert bbound.max() < 1e-3 and sbound.max() < 1e-5         # orders below the old atol = 1e-2
    bad = np.argwhere(~(berr <= bbound))
    assert bad.size == 0, f"{len(bad)} box coordinate(s) over the bound, first {bad[0].tolist()}: " \
        f"{berr[tuple(bad[0])]:.3e} > {bbound[tuple(bad[0])]:.3e}"
    bad = np.argwhere(~(serr <= sbound))
    assert bad.size == 0, f"{len(bad)} score(s) over the bound, first {bad[0].tolist()}: " \
        f"{serr[tuple(bad[0])]:.3e} > {sbound[tuple(bad[0])]:.3e}"
    # the planted anchors, by hand: one-hot rows are exact, -inf rows give class 0 and score 0
    assert boxes[0, 3].tolist() == [(3.5 - 0) * strides[0], (0.5 - 15) * strides[0], (3.5 + 7) * strides[0],
                                    (0.5 + 8) * strides[0]]
    assert cls[0, :3].tolist() == [5, 2, 0] and scores[0, 2] == 0 and cls[0, 6] == 0 and cls[0, 7] == nc - 1
    assert cls[1, -1] == 5


@pytest.mark.parametrize("flat", [False, True], ids=["tiled", "flat"])
def test_yolo_decode_liveness(native, monkeypatch, flat):
    """A NaN planted in one anchor's DFL row changes exactly that anchor's box (so the rows are
    read, and read where the reference reads them); a spike in a gap channel changes nothing."""
    from aiko_services_amd.ops import detect as DT
    nc, key = 80, "3lvl"
    sizes, strides = DECODE_LEVELS[key]
    if flat:
        monkeypatch.setenv("AIKO_DECODE_FLAT", "1")
    else:
        monkeypatch.delenv("AIKO_DECODE_FLAT", raising=False)
    pitch = 64 + nc + 16

    def run(edit):
        wides = []
        for f in _decode_heads(nc, key):
            w = torch.zeros(*f.shape[:3], pitch, dtype=BF16)
            w[..., 8:8 + 64 + nc] = f
            wides.append(w)
        edit(wides)
        out = DT.yolo_decode([w.to(DEV)[..., 8:8 + 64 + nc] for w in wides], strides, nc)
        torch.cuda.synchronize()
        return [t.cpu() for t in out]

    base = run(lambda w: None)

    def nan_dfl(w):
        w[1][1, 3, 2, 8 + 2 * 16 + 9] = float("nan")           # image 1, level 1, anchor (3, 2), side 2, bin 9

    a = 63 + 3 * 8 + 2
    hit = run(nan_dfl)
    assert torch.isnan(hit[0][1, a, 2]) and torch.isfinite(hit[0][1, a, [0, 1, 3]]).all()
    same = torch.ones(DECODE_B, base[0].shape[1], dtype=torch.bool)
    same[1, a] = False
    assert torch.equal(_bits(hit[0])[same], _bits(base[0])[same])
    assert torch.equal(_bits(hit[1]), _bits(base[1])) and torch.equal(hit[2], base[2])

    def gap_spike(w):
        for t in w:
            t[..., :8] = 3e4
            t[..., 8 + 64 + nc:] = float("nan")

    quiet = run(gap_spike)
    for x, y in zip(quiet, base):
        assert torch.equal(_bits(x), _bits(y))


def test_yolo_decode_refusals(native):
    from aiko_services_amd.ops import detect as DT
    f = lambda c, n=1: [torch.zeros(1, 2, 2, c, dtype=BF16, device=DEV) for _ in range(n)]  # noqa: E731
    with pytest.raises(RuntimeError, match="nc % 8"):
        DT.yolo_decode(f(76), (8,), 12)
    with pytest.raises(RuntimeError, match="reg_max 16"):
        DT.yolo_decode(f(32 + 80), (8,), 80, reg_max=8)
    with pytest.raises(RuntimeError, match="1..4 levels"):
        DT.yolo_decode(f(144, 5), (4, 8, 16, 32, 64), 80)
    with pytest.raises(RuntimeError, match="level channels"):
        DT.yolo_decode(f(144), (8,), 88)
    with pytest.raises(RuntimeError, match="bf16"):
        DT.yolo_decode([torch.zeros(1, 2, 2, 144, device=DEV)], (8,), 80)


# ---- NMS -----------------------------------------------------------------------------------------

NMS_CLASSES = (0, 79, 1000)


def _filler(B, A, seed, classes=NMS_CLASSES, n_centers=40):
    """Clustered boxes (so suppression happens), scores with full mantissas and some exact ties."""
    g = torch.Generator().manual_seed(seed)
    centers = torch.rand(B, n_centers, 2, generator=g) * 600
    pick = torch.randint(0, n_centers, (B, A), generator=g)
    c = torch.gather(centers, 1, pick[..., None].expand(B, A, 2)) + torch.randn(B, A, 2, generator=g) * 6
    wh = 20 + torch.rand(B, A, 2, generator=g) * 60
    boxes = torch.cat([c - wh / 2, c + wh / 2], -1)
    scores = torch.rand(B, A, generator=g)
    tie = torch.rand(B, A, generator=g) < 0.3
    scores = torch.where(tie, (scores * 64).floor() / 64, scores)
    cls = torch.tensor(classes, dtype=torch.int32)[torch.randint(0, len(classes), (B, A), generator=g)]
    return boxes, scores, cls


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run_nms(boxes, scores, cls, *, conf, iou, max_cand, max_det, letterbox=None, bits=False):
    """run_both of one topk_nms call with poison 3e38; ``bits``: return det as int32 (a +inf score
    is a legitimate output that run_both's finiteness check would refuse)."""
    from aiko_services_amd.ops import detect as DT
    B = scores.shape[0]
    kw = {} if letterbox is None else {"letterbox": letterbox}

    def case(ops):
        bx, sc, cl = ops.inp(boxes, "boxes"), ops.inp(scores, "scores"), ops.inp(cls, "cls")
        det = ops.out((B, max_det, 6), torch.float32, "det")
        count = ops.out((B,), torch.int32, "count")
        if not ops.on:
            count.fill_(I32_POISON)
        assert torch.isnan(det).all() and (count == I32_POISON).all()
        DT.topk_nms(bx, sc, cl, conf=conf, iou=iou, max_candidates=max_cand, max_det=max_det, det=det, count=count, **kw)
        return (det.view(torch.int32) if bits else det), count

    det, count = run_both(case, poison=3e38)
    return det.cpu().numpy().view(np.uint32), count.cpu().numpy()


def _check_nms(boxes, scores, cls, *, images=None, what="", **kw):
    """Run, then compare ``images`` (default all) bit for bit with nms_slow.  Returns
    ``{b: (keep, det, n)}`` of the checked images."""
    run_kw = {k: kw[k] for k in ("conf", "iou", "max_cand", "max_det")}
    det, count = _run_nms(boxes, scores, cls, letterbox=kw.get("letterbox"), bits=kw.get("bits", False), **run_kw)
    out = {}
    for b in (range(scores.shape[0]) if images is None else images):
        keep, want, n = D.nms_slow(boxes[b].numpy(), scores[b].numpy(), cls[b].numpy(), kw["conf"], kw["iou"],
                                   kw["max_cand"], kw["max_det"], **({"letterbox": kw["letterbox"]} if kw.get("letterbox") else {}))
        assert count[b] == n, f"{what} image {b}: count {count[b]} for {n}"
        diff = np.argwhere(det[b] != want.view(np.uint32))
        assert diff.size == 0, f"{what} image {b}: {len(diff)} det element(s) differ, first (row, col) {diff[0].tolist()}: " \
            f"{det[b].view(F32)[tuple(diff[0])]!r} for {want[tuple(diff[0])]!r}"
        out[b] = (keep, want, n)
    return out


def _live(scores, b, conf):
    return D.score_keys(scores[b].numpy(), conf)


NMS_STD = dict(conf=0.25, iou=0.5, max_cand=1024, max_det=300)


@pytest.mark.parametrize("A", [1, 33, 1023, 1024, 1025, 16384, 16385, 32768])
def test_nms_sizes_guarded(native, A):
    """A = 1023 / 1024 / 1025: around one element per thread (chunk 1 -> 2); 16384 / 16385: one and
    two trips of the 16-loads-in-flight loop; 32768: the key region exactly full, total > max_cand."""
    boxes, scores, cls = _filler(2, A, A)
    if A == 1:
        scores[0, 0], scores[1, 0] = 0.9, 0.1                  # one candidate; none
    res = _check_nms(boxes, scores, cls, what=f"A {A}", **NMS_STD)
    if A == 1:
        assert res[0][2] == 1 and res[1][2] == 0
    if A >= 16384:
        keys = _live(scores, 0, 0.25)
        assert (keys != 0).sum() > 1024 and len(D.nms_radix_plan(keys, 1024)) >= 2


@pytest.mark.parametrize("G", [1, 2, 3, 4])
def test_nms_workgroups_per_image_guarded(native, G):
    """G workgroups per image (the last arriver runs the scan): B chosen from the CU count; two
    classes, so runs span blocks and the split mask blocks matter.  Every 7th image is compared."""
    cus = _cus()
    B = {1: cus + 1, 2: cus // 2, 3: cus // 3, 4: 2}[G]
    assert D.nms_groups(B, cus) == G
    boxes, scores, cls = _filler(B, 700, 50 + G, classes=(3, 4))
    res = _check_nms(boxes, scores, cls, images=range(0, B, 7), what=f"G {G}", conf=0.1, iou=0.5, max_cand=1024, max_det=300)
    assert len(res) >= 1
    live = torch.from_numpy(_live(scores, 0, 0.1) != 0)
    K = int(live.sum())                                        # fewer than max_cand: every live anchor is a candidate
    assert 512 < K <= 700 and D.nms_blocks(K, D.position_classes(cls[0][live].tolist())) > 2 * ((K + 63) // 64)


def _selection_case(name):
    """(boxes, scores, cls, params, check(scores) -> None)"""
    if name == "all_equal_full":                               # range 0: the first max_cand by index
        boxes, scores, cls = _filler(2, 32768, 1)
        scores[:] = 0.5
        scores[1, ::3] = 0.2                                   # image 1: every third anchor below conf
        p = dict(NMS_STD)

        def check(res):
            for b in (0, 1):
                keys = _live(scores, b, 0.25)
                assert (keys != 0).sum() > 1024 and D.nms_radix_plan(keys, 1024) == []
            assert res[0][0].max() < 1024 and res[1][0].max() < 1536 and (res[1][0] % 3 != 0).all()
        return boxes, scores, cls, p, check
    if name == "two_adjacent":                                 # a 1-bit range
        boxes, scores, cls = _filler(2, 3000, 2)
        up = torch.nextafter(torch.tensor(0.5), torch.tensor(1.0))
        scores = torch.where(scores < 0.5, torch.tensor(0.5), up)
        p = dict(conf=0.25, iou=0.5, max_cand=64, max_det=300)
        return boxes, scores, cls, p, lambda res: _assert(D.nms_radix_plan(_live(scores, 0, 0.25), 64) == [0])
    if name == "wide_range":                                   # subnormals .. 1.0 and +inf, conf = 0
        boxes, _, cls = _filler(2, 5000, 3)
        rng = np.random.default_rng(3)
        bits = rng.integers(1, 0x3F800001, (2, 5000), dtype=np.int64).astype(np.uint32)
        s = bits.view(F32).copy()
        s[:, 10:5000:97] = np.inf
        s[:, 11:5000:89] = 0.0
        s[:, 12:5000:83] = -0.0
        s[:, 13:5000:79] = np.nan
        s[:, 14:5000:73] = -1.0
        s[0, 4999], s[1, 0] = 1e-45, 1e-45                     # the smallest subnormal
        scores = torch.from_numpy(s)
        p = dict(conf=0.0, iou=0.5, max_cand=1024, max_det=300, bits=True)

        def check(res):
            plan = D.nms_radix_plan(_live(scores, 0, 0.0), 1024)
            assert len(plan) == 3 and plan[0] - plan[1] == 12 and plan[1] < 12 and plan[2] == 0, plan
            assert np.isinf(res[0][1][0, 4])
        return boxes, scores, cls, p, check
    if name == "tie_straddles_K_and_chunk":
        A, K = 2500, 65
        boxes, scores, cls = _filler(2, A, 4)
        scores = scores * 0.2 + 0.26
        top = torch.arange(40) * 23 + 3
        scores[:, top] = 0.6 + torch.arange(40) / 100.0
        scores[:, 1000:1060] = 0.5                             # 60 tied anchors; places 41 .. 100
        scores[1, 1010:1012] = 0.1                             # image 1: a hole of two in the group
        p = dict(conf=0.25, iou=0.5, max_cand=K, max_det=300)

        def check(res):
            chunk = -(-A // 1024)
            assert chunk == 3 and not set(top.tolist()) & set(range(1000, 1060))
            # the K-th place is inside the group: its first 25 (27 past the hole) anchors by index are candidates,
            # and that cut falls inside one thread's chunk (not on a chunk boundary)
            cut = {0: 1025, 1: 1027}
            for b in (0, 1):
                assert (cut[b] % chunk) != 0 and 1000 // chunk != (cut[b] - 1) // chunk
                keep = res[b][0]
                assert keep[(keep >= 1000) & (keep < 1060)].max(initial=0) < cut[b]
        return boxes, scores, cls, p, check
    if name == "total_eq_max_cand":
        boxes, scores, cls = _filler(2, 500, 5)
        scores = scores * 0.4                                  # all below conf = 0.5
        scores[0, 3:3 + 64 * 7:7] = 0.6 + torch.arange(64) / 256.0
        scores[1, 3:3 + 65 * 7:7] = 0.6 + torch.arange(65) / 256.0
        p = dict(conf=0.5, iou=0.5, max_cand=64, max_det=300)

        def check(res):
            assert [(int((_live(scores, b, 0.5) != 0).sum())) for b in (0, 1)] == [64, 65]
            assert D.nms_radix_plan(_live(scores, 0, 0.5), 64) == [] and D.nms_radix_plan(_live(scores, 1, 0.5), 64) != []
        return boxes, scores, cls, p, check
    if name == "special_scores":
        boxes, scores, cls = _filler(2, 300, 6)
        c = torch.tensor(0.1)
        scores[:, 0::9] = float("nan")
        scores[:, 1::9] = -0.0
        scores[:, 2::9] = -0.7
        scores[:, 3::9] = c                                    # exactly fp32(conf): not above it
        scores[:, 4::9] = torch.nextafter(c, torch.tensor(1.0))
        scores[:, 5::9] = NEG_INF
        p = dict(conf=0.1, iou=0.5, max_cand=1024, max_det=300)

        def check(res):
            for b in (0, 1):
                keep, live = res[b][0], _live(scores, b, 0.1) != 0
                assert ((keep % 9 == 4) | (keep % 9 > 5)).all()
                assert live[4::9].all() and not live[3::9].any() and not live[0::9].any() and not live[1::9].any()
        return boxes, scores, cls, p, check
    if name == "no_candidate":
        boxes, scores, cls = _filler(2, 1500, 7)
        scores = scores * 0.25
        scores[1] = float("nan")
        p = dict(NMS_STD)

        def check(res):
            for b in (0, 1):
                want = np.zeros((300, 6), dtype=F32)
                want[:, 5] = -1
                assert res[b][2] == 0 and np.array_equal(res[b][1], want)
        return boxes, scores, cls, p, check
    raise KeyError(name)


def _assert(cond):
    assert cond


@pytest.mark.parametrize("name", ["all_equal_full", "two_adjacent", "wide_range", "tie_straddles_K_and_chunk",
                                  "total_eq_max_cand", "special_scores", "no_candidate"])
def test_nms_selection_guarded(native, name):
    boxes, scores, cls, p, check = _selection_case(name)
    check(_check_nms(boxes, scores, cls, what=name, **p))


@pytest.mark.parametrize("max_cand,max_det", [(1, 1), (1, 1024), (64, 1), (64, 1024), (65, 1024), (1024, 1), (1024, 1024)])
def test_nms_caps_guarded(native, max_cand, max_det):
    """The candidate and detection caps at their ends, max_det > max_cand included."""
    boxes, scores, cls = _filler(2, 3000, max_cand + max_det)
    res = _check_nms(boxes, scores, cls, what=f"caps {max_cand} {max_det}", conf=0.25, iou=0.5, max_cand=max_cand, max_det=max_det)
    assert all(1 <= n <= min(max_cand, max_det) for _, _, n in res.values())


def _grid_boxes(n, y0=4300.0):
    """n disjoint 10 x 10 boxes, far from the planted ones."""
    i = torch.arange(n, dtype=torch.float32)
    x = (i % 300) * 20
    y = y0 + (i // 300) * 20
    return torch.stack([x, y, x + 10, y + 10], 1)


def test_nms_chain_guarded(native):
    """A chain in which each box overlaps only its successor: the keep flags alternate, the worst
    case of the ballot fixed point (64 rounds).  Chains of 64, 65 and 63 boxes: K % 64 = 0, 1, 63
    In the chain of 65 the first box stands apart, so the odd boxes are kept and the 65th, alone in
    block 1, is suppressed by the 64th through an off-diagonal word."""
    B, A = 3, 100
    boxes = _grid_boxes(A).repeat(B, 1, 1)
    scores = torch.full((B, A), 0.05)
    cls = torch.zeros(B, A, dtype=torch.int32)
    lengths = (64, 65, 63)
    for b, n in enumerate(lengths):
        i = torch.arange(n, dtype=torch.float32)
        boxes[b, 20:20 + n] = torch.stack([i * 10, i * 0, i * 10 + 16, i * 0 + 10], 1)     # IoU 60 / 260 with the next
        scores[b, 20:20 + n] = 0.9 - i / 256
    boxes[1, 20, 1::2] += 100.0
    res = _check_nms(boxes, scores, cls, what="chain", conf=0.1, iou=0.2, max_cand=1024, max_det=1024)
    assert res[0][0].tolist() == list(range(20, 84, 2)) and res[2][0].tolist() == list(range(20, 83, 2))
    assert res[1][0].tolist() == [20] + list(range(21, 84, 2)) and D.nms_blocks(65, [0] * 65) == 3


def test_nms_class_runs_guarded(native):
    """Image 0: one class over three blocks, the suppressor at rank 0 (block 0) and its victim at
    rank 150 (block 2): only the (0, 2) mask block holds the pair.  Image 1: runs that end exactly
    on a block edge, start on one, and start mid-block.  Image 2: the same with a run per block
    edge shifted by one."""
    B, A = 3, 230
    boxes = _grid_boxes(A).repeat(B, 1, 1)
    scores = (0.9 - torch.arange(A) / 1024.0).repeat(B, 1)     # rank = index
    cls = torch.zeros(B, A, dtype=torch.int32)
    scores[0, 192:] = 0.01                                     # image 0: K = 192, one class
    boxes[0, 150] = boxes[0, 0] + torch.tensor([1.0, 0.0, 1.0, 0.0])          # IoU 90 / 110
    fb, fs, _ = _filler(2, A, 8)
    boxes[1:] = fb                                             # clustered boxes: suppression inside every run
    scores[1:, 224:] = 0.01                                    # K = 224
    cls[1, 64:164], cls[1, 164:] = 1, 2                        # runs of 64 | 100 | 60 candidates
    cls[2, 63:164], cls[2, 164:] = 1, 2                        # 63 | 101 | 60
    res = _check_nms(boxes, scores, cls, what="class runs", conf=0.1, iou=0.5, max_cand=1024, max_det=1024)
    assert D.nms_blocks(192, [0] * 192) == 6
    assert res[0][2] == 191 and 150 not in res[0][0].tolist()
    # ranks equal indices here, so the position order is the class order of the first K anchors
    assert D.nms_blocks(224, D.position_classes(cls[1, :224].tolist())) == 4 + 2    # + (1, 2), (2, 3)
    assert D.nms_blocks(224, D.position_classes(cls[2, :224].tolist())) == 4 + 4    # + (0, 1), (0, 2), (1, 2), (2, 3)


def test_nms_degenerate_boxes_guarded(native):
    """Zero-area boxes, identical zero-area pairs and inverted corners among ordinary boxes: the
    reference's IoU is 0 or NaN there, never above the threshold."""
    boxes, scores, cls = _filler(2, 400, 9, classes=(0, 1))
    boxes[:, 0::10, 2] = boxes[:, 0::10, 0]                    # zero width
    boxes[:, 1::10, 3] = boxes[:, 1::10, 1]                    # zero height
    boxes[:, 2::10] = boxes[:, 3::10]                          # identical pairs ...
    boxes[:, 2::20, 2:] = boxes[:, 2::20, :2]                  # ... half of them zero-area points
    boxes[:, 3::20] = boxes[:, 2::20]
    boxes[:, 4::10] = boxes[:, 4::10][..., [2, 3, 0, 1]]       # both corners inverted (positive "area")
    boxes[:, 5::10] = boxes[:, 5::10][..., [2, 1, 0, 3]]       # x inverted (negative area)
    cls[:, 2::10] = cls[:, 3::10]
    res = _check_nms(boxes, scores, cls, what="degenerate", conf=0.1, iou=0.5, max_cand=1024, max_det=1024)
    for b in (0, 1):
        keep = set(res[b][0].tolist())
        live = {i for i in range(400) if scores[b, i] > 0.1}
        assert {i for i in live if i % 10 in (0, 1, 4, 5)} <= keep        # never suppressed


def test_nms_negative_iou_guarded(native):
    """iou < 0: one run in rank order over a partial last block, every pair with a non-NaN IoU
    suppresses, across classes too."""
    boxes, scores, cls = _filler(2, 100, 10)
    scores[1, 50:] = 0.01
    boxes[1, :50, 2:] = boxes[1, :50, :2]                      # image 1: points only (IoU 0 / 0 within a class)
    res = _check_nms(boxes, scores, cls, what="iou < 0", conf=0.1, iou=-1.0, max_cand=1024, max_det=300)
    assert res[0][2] == 1 and res[1][2] >= 1


@pytest.mark.parametrize("G", [4, 1])
@pytest.mark.parametrize("cross", [False, True], ids=["same_block", "cross_block"])
@pytest.mark.parametrize("t", D.IOU_THRESHOLDS)
def test_nms_iou_threshold_guarded(native, t, cross, G):
    """Every planted pair at its threshold, one pair per image: the outer box at rank 0, the inner
    one at rank 1 (same 64-block: caught by the transposed diagonal word) or at rank 100 (block 1
    of the same class run: an off-diagonal word); odd images swap the two.  At G = 4 and G = 1."""
    pairs = [(k, p) for tt, k, p in D.planted_pairs() if tt == t]
    assert pairs
    cus = _cus()
    B = len(pairs) if G == 4 else cus + 1
    assert D.nms_groups(B, cus) == G
    A, K = 160, 130
    boxes = _grid_boxes(A).repeat(B, 1, 1)
    scores = (0.8 - torch.arange(A) / 1024.0).repeat(B, 1)
    scores[:, K:] = 0.01
    cls = torch.zeros(B, A, dtype=torch.int32)
    second = 100 if cross else 1
    for b in range(B):
        inner, outer = D.pair_boxes(pairs[b % len(pairs)][1], origin=(16.0, 32.0))
        first_box, second_box = (outer, inner) if b % 2 == 0 else (inner, outer)
        boxes[b, 0], boxes[b, second] = torch.tensor(first_box), torch.tensor(second_box)
    images = sorted(set(range(len(pairs))) | {B - 1, B // 2})
    res = _check_nms(boxes, scores, cls, images=images, what=f"t {t}", conf=0.1, iou=t, max_cand=1024, max_det=300)
    assert D.nms_blocks(K, [0] * K) == 6
    for b in images:
        kind = pairs[b % len(pairs)][0]
        keep = res[b][0].tolist()
        assert (second not in keep) == D.SUPPRESSES[kind], (b, kind, pairs[b % len(pairs)][1])
        assert res[b][2] == K - int(D.SUPPRESSES[kind])


@pytest.mark.parametrize("gain", [0.5, 1.3333])
def test_nms_letterbox_guarded(native, gain):
    """Letterbox -> frame mapping with non-zero pads and a frame smaller than the boxes: all four
    clips fire; ``inv = 1 / gain`` and the products round as the reference's."""
    boxes, scores, cls = _filler(2, 900, 11)
    lb = (gain, 212.0, 107.5, 300.0, 200.0)
    res = _check_nms(boxes, scores, cls, what=f"gain {gain}", letterbox=lb, **NMS_STD)
    for b in (0, 1):
        _, det, n = res[b]
        assert (det[:n, 0] == 0).any() and (det[:n, 1] == 0).any() and (det[:n, 2] == 300).any() and (det[:n, 3] == 200).any()
        inside = (det[:n, :4] > 0) & (det[:n, :4] < 200)
        assert inside.any()


def test_nms_liveness_last_score(native):
    """3e38 written at scores[b, A - 1] comes out as det[b, 0] (the last element is read); the
    same value one element past A is where the guarded run's guard already has it, and run_both
    has shown that it changes nothing."""
    A = 1025
    boxes, scores, cls = _filler(2, A, 12)
    base = _check_nms(boxes, scores, cls, what="liveness base", **NMS_STD)
    scores[:, A - 1] = 3e38
    res = _check_nms(boxes, scores, cls, what="liveness", **NMS_STD)
    for b in (0, 1):
        keep, det, n = res[b]
        assert keep[0] == A - 1 and det[0, 4] == F32(3e38) and det[0, 5] == float(cls[b, A - 1])
        assert np.array_equal(det[0, :4], np.maximum(boxes[b, A - 1].numpy(), 0))
        assert base[b][0][0] != A - 1


def test_nms_refusals(native):
    from aiko_services_amd.ops import detect as DT
    boxes, scores, cls = (t.to(DEV) for t in _filler(2, 64, 13))
    ok = dict(conf=0.25, iou=0.5, max_candidates=64, max_det=16)
    DT.topk_nms(boxes, scores, cls, **ok)
    DT.topk_nms(boxes, scores, cls, **{**ok, "conf": 0.0, "iou": -1.0})      # conf = 0 and iou < 0 stay legal
    big = torch.zeros(1, 32769, device=DEV)
    with pytest.raises(RuntimeError, match="32768 anchors"):
        DT.topk_nms(torch.zeros(1, 32769, 4, device=DEV), big, torch.zeros(1, 32769, dtype=torch.int32, device=DEV), **ok)
    for bad in ({"max_candidates": 0}, {"max_candidates": 1025}, {"max_det": 1025}):
        with pytest.raises(RuntimeError, match="max_candidates, max_det"):
            DT.topk_nms(boxes, scores, cls, **{**ok, **bad})
    with pytest.raises(RuntimeError, match="scores fp32"):
        DT.topk_nms(boxes[:, ::2], torch.cat([scores, scores], 1)[:, ::2], cls[:, ::2], **ok)
    with pytest.raises(RuntimeError, match="scores fp32"):
        DT.topk_nms(boxes, scores.double(), cls, **ok)
    with pytest.raises(RuntimeError, match="boxes fp32"):
        DT.topk_nms(boxes.half(), scores, cls, **ok)
    with pytest.raises(RuntimeError, match="cls int32"):
        DT.topk_nms(boxes, scores, cls.long(), **ok)
    with pytest.raises(RuntimeError, match="det fp32"):                       # the operator's own check
        torch.ops.aiko.topk_nms_out(boxes, scores, cls, 64, [0.25, 0.5, 7680.0, 1.0, 0.0, 0.0, 640.0, 640.0],
                                    torch.empty(2, 16, 6, dtype=torch.float64, device=DEV),
                                    torch.empty(2, dtype=torch.int32, device=DEV))
    for bad in ({"conf": -0.25}, {"conf": float("nan")}, {"iou": float("nan")}, {"conf": NEG_INF}):
        with pytest.raises(RuntimeError, match="conf must be >= 0"):
            DT.topk_nms(boxes, scores, cls, **{**ok, **bad})
    torch.cuda.synchronize()
