"""The overlay's CPU side: ``draw_detections_ref`` on cases small enough to spell out, label
placement, painting order, the percentage's rounding, colours, rects against ``roi_rects_ref``,
the name table and the project's font."""
import itertools

import torch

from aiko_services_amd.ops import overlay_font
from aiko_services_amd.ops.overlay import default_font, default_palette, pack_names
from aiko_services_amd.ops.reference import draw_detections_ref, overlay_text_ref, roi_rects_ref

NAN = float("nan")
RED = [200, 0, 0]               # luma 59800: white text


def _det(rows, max_det=None):
    """[1, max_det, 6] from (x1, y1, x2, y2, score, class) rows; padding rows as the detector's."""
    det = torch.zeros(1, max_det or len(rows), 6)
    det[:, :, 5] = -1
    for i, r in enumerate(rows):
        det[0, i] = torch.tensor([float(v) for v in r])
    return det


def _x_font():
    """3 x 3 glyphs for codes 32..65, all blank but 'A' = an X."""
    font = torch.zeros(34, 3, dtype=torch.uint8)
    font[ord("A") - 32] = torch.tensor([0b10100000, 0b01000000, 0b10100000], dtype=torch.uint8)
    return font


def _draw(hw, rows, names, font, palette, count=None, **kw):
    H, W = hw
    frames = torch.zeros(1, H, W, 3, dtype=torch.uint8)
    det = _det(rows)
    count = torch.tensor([len(rows) if count is None else count], dtype=torch.int32)
    return draw_detections_ref(frames, det, count, len(rows), names, font,
                               torch.tensor(palette, dtype=torch.uint8), **kw)[0]


def _picture(img, legend):
    """One character per pixel by colour; a colour outside ``legend`` is '?'."""
    return ["".join(legend.get(tuple(px), "?") for px in row) for row in img.tolist()]


def test_hand_written_box_and_label():
    img = _draw((12, 16), [(4, 5, 12, 11, 0.5, 0)], pack_names(["A"], 4), _x_font(), [RED],
                thickness=1, text_scale=1, show_score=False, glyph_width=3)
    # 8 x 6 box at (4, 5); the label (1 character of 3 x 3 plus a 1-pixel border: 5 x 5) sits on top
    # of it at rows 0..4; the X is white on red
    assert _picture(img, {(0, 0, 0): ".", tuple(RED): "c", (255, 255, 255): "w"}) == [
        "....ccccc.......",
        "....cwcwc.......",
        "....ccwcc.......",
        "....cwcwc.......",
        "....ccccc.......",
        "....cccccccc....",
        "....c......c....",
        "....c......c....",
        "....c......c....",
        "....c......c....",
        "....cccccccc....",
        "................",
    ]


def _label_box(img, colour=RED):
    """Bounding box (x0, y0, x1, y1) of the pixels that are ``colour`` or white."""
    t = torch.tensor(colour, dtype=torch.uint8)
    m = (img == t).all(-1) | (img == 255).all(-1)
    ys, xs = torch.nonzero(m, as_tuple=True)
    return int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1


def test_label_placement():
    names, font = pack_names(["AAAA"], 4), _x_font()
    kw = dict(thickness=1, show_score=False, glyph_width=3)
    legend = {(0, 0, 0): ".", tuple(RED): "c", (255, 255, 255): "w"}
    # Lw = 4 * 3 + 2 = 14, Lh = 5.  Room above: rows Y0 - 5 .. Y0 - 1
    img = _draw((20, 30), [(3, 8, 25, 18, 0.5, 0)], names, font, [RED], **kw)
    assert img[3:8, 3:17].any(-1).all() and not img[:3].any() and not img[3:8, 17:].any()
    assert _picture(img[4:5, 3:17], legend) == ["cwcwwcwwcwwcwc"]
    # no room above (Y0 = 4 < Lh): inside the top of the box, over its outline
    img = _draw((20, 30), [(3, 4, 25, 18, 0.5, 0)], names, font, [RED], **kw)
    assert not img[:4].any()
    assert _picture(img[4:10, 3:19], legend) == ["cccccccccccccccc", "cwcwwcwwcwwcwc..", "ccwccwccwccwcc..",
                                                 "cwcwwcwwcwwcwc..", "cccccccccccccc..", "c..............."]
    # X0 + Lw > W: shifted left so that it ends at the frame's edge
    img = _draw((20, 30), [(22, 8, 29, 18, 0.5, 0)], names, font, [RED], **kw)
    assert img[3:8, 16:30].any(-1).all() and not img[3:8, :16].any()
    assert _picture(img[4:5, 16:30], legend) == ["cwcwwcwwcwwcwc"]
    # Lw > W: starts at column 0 and is cut at the frame's edge
    img = _draw((20, 10), [(2, 8, 9, 18, 0.5, 0)], names, font, [RED], **kw)
    assert _picture(img[3:8], legend) == ["cccccccccc", "cwcwwcwwcw", "ccwccwccwc", "cwcwwcwwcw", "cccccccccc"]
    # the bottom clip: a 1-row frame keeps the label's first row only
    img = _draw((1, 30), [(3, 0, 25, 1, 0.5, 0)], names, font, [RED], **kw)
    assert _picture(img, legend) == ["...cccccccccccccccccccccc....."]


def test_lowest_index_is_on_top():
    names, font = pack_names(["A", "A"], 4), _x_font()
    green = [0, 200, 0]
    rows = [(6, 8, 20, 18, 0.9, 0), (4, 6, 16, 14, 0.8, 1)]
    both = _draw((24, 24), rows, names, font, [RED, green], thickness=2, show_score=False, glyph_width=3)
    alone = _draw((24, 24), rows[:1], names, font, [RED, green], thickness=2, show_score=False, glyph_width=3)
    red_or_white = ((alone == torch.tensor(RED, dtype=torch.uint8)).all(-1) | (alone == 255).all(-1))
    # everything row 0 paints alone is there unchanged with row 1 underneath
    assert torch.equal(both[red_or_white], alone[red_or_white])
    g = torch.tensor(green, dtype=torch.uint8)
    # row 1's outline crosses row 0's outline at (6..7, 8..9)... and its label (rows 1..5, columns
    # 4..8) meets row 0's label (rows 3..7, columns 6..10): those pixels are row 0's
    assert (both[8:10, 6:8] == torch.tensor(RED, dtype=torch.uint8)).all()
    assert not (both[3:6, 6:9] == g).all(-1).any()
    assert (both[1:3, 4:9] == g).all(-1).any() and (both[6:14, 4:6] == g).all()
    # with the rows swapped the other one wins
    swapped = _draw((24, 24), [rows[1], rows[0]], names, font, [green, RED], thickness=2, show_score=False,
                    glyph_width=3)
    assert (swapped[8:10, 6:8] == g).all()


def test_percentage_rounding():
    names = pack_names(["ab"], 4)
    digits = lambda p, show=True: bytes(overlay_text_ref(0, torch.tensor(p), names, show)).decode()  # noqa: E731
    assert digits(0.005) == "ab 00"          # fp32(0.005) * 100 = 0.49999997
    assert digits(0.995) == "ab 99"          # fp32(0.995) * 100 = 99.5 exactly in fp32? rint -> 100 or 99: both clamp to 99
    assert digits(1.7) == "ab 99"
    assert digits(-0.2) == "ab 00"
    assert digits(NAN) == "ab 00"
    assert digits(0.125) == "ab 12"          # 12.5: half to even
    assert digits(0.375) == "ab 38"          # 37.5: half to even
    assert digits(0.87) == "ab 87"
    assert digits(0.87, False) == "ab"
    assert bytes(overlay_text_ref(3, torch.tensor(0.5), names, True)).decode() == "50"     # no name: no space
    assert overlay_text_ref(-1, torch.tensor(0.5), names, False) == []


def test_class_outside_the_table_has_no_name_and_a_defined_colour():
    names, font = pack_names(["A", "A"], 4), _x_font()
    palette = [RED, [0, 200, 0], [0, 0, 200]]
    kw = dict(thickness=1, show_score=False, glyph_width=3)
    for cls, colour in ((-1, palette[0]), (-7, palette[0]), (2, palette[2]), (4, palette[1]), (300, palette[0])):
        img = _draw((20, 30), [(3, 8, 25, 18, 0.5, cls)], names, font, palette, **kw)
        assert not img[:8].any(), cls                                  # no label
        assert (img[8, 3:25] == torch.tensor(colour, dtype=torch.uint8)).all(), cls
        assert not img[9:17, 4:24].any()
    # a class inside the table with the same colour index does have its label
    img = _draw((20, 30), [(3, 8, 25, 18, 0.5, 1)], names, font, palette, **kw)
    assert img[3:8, 3:8].any(-1).all()


def test_text_is_black_or_white_by_luma():
    names, font = pack_names(["A"] * 6, 4), _x_font()
    # lumas 127886, 128000 (the threshold itself: black), 0, 255000, 76245 (red), 149685 (green)
    palette = [[128, 128, 127], [128, 128, 128], [0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0]]
    lumas = [299 * r + 587 * g + 114 * b for r, g, b in palette]
    assert lumas[0] == 127886 and lumas[1] == 128000
    for cls, (colour, luma) in enumerate(zip(palette, lumas)):
        frames = torch.full((1, 20, 30, 3), 77, dtype=torch.uint8)
        out = draw_detections_ref(frames, _det([(3, 8, 25, 18, 0.5, cls)]), torch.tensor([1], dtype=torch.int32), 1,
                                  names, font, torch.tensor(palette, dtype=torch.uint8), thickness=1,
                                  show_score=False, glyph_width=3)[0]
        ink = out[4, 4].tolist()                                        # the X's top-left pixel
        assert ink == ([0, 0, 0] if luma >= 128000 else [255, 255, 255]), (cls, luma)
        assert out[4, 5].tolist() == colour                             # the gap in the X's first row


def test_drawn_rects_equal_roi_rects():
    H, W, K = 37, 53, 6
    rows = [(0, 0, 53, 37), (10, 8, 15, 15), (20.3, 11.6, 20.7, 11.9), (NAN, 5, 20, 20),
            (44.5, 29.25, 52.5, 36.75), (3.3, 2.2, 30.9, 20.1)]
    names, font = pack_names([], 4), _x_font()
    palette = torch.tensor([[9, 9, 9]], dtype=torch.uint8)
    for margin in (0.0, 0.15):
        for i, r in enumerate(rows):
            det = _det([(*r, 0.5, 0)], K)
            count = torch.tensor([1], dtype=torch.int32)
            out = draw_detections_ref(torch.zeros(1, H, W, 3, dtype=torch.uint8), det, count, K, names, font,
                                      palette, thickness=16, margin=margin, show_score=False)[0]
            x0, y0, x1, y1 = roi_rects_ref(det, count, K, (H, W), margin)[0].tolist()
            want = torch.zeros(H, W, dtype=torch.bool)
            want[y0:y1, x0:x1] = True          # thickness 16 fills all but the interior of a big box
            if x1 - x0 > 32 and y1 - y0 > 32:
                want[y0 + 16:y1 - 16, x0 + 16:x1 - 16] = False
            assert torch.equal(out.any(-1), want), (margin, i)
            assert (x1 > x0) == (i != 3)


def test_pack_names():
    t = pack_names(["cat", "person", "", "zz9_x"], 5)
    assert t.dtype == torch.uint8 and t.shape == (4, 5)
    assert bytes(t[0].tolist()) == b"cat\0\0" and bytes(t[1].tolist()) == b"perso"
    assert not t[2].any() and bytes(t[3].tolist()) == b"zz9_x"
    assert pack_names([], 7).shape == (0, 7)
    try:
        pack_names(["café"], 8)
    except UnicodeEncodeError:
        pass
    else:
        raise AssertionError("a non-ASCII name must be refused")


def test_default_font_and_palette():
    font, gw = default_font()
    assert font.dtype == torch.uint8 and font.shape == (95, 8) and gw == 6
    assert not (font & 0x07).any()            # every glyph fits 5 columns ...
    assert not font[:, 7].any()               # ... and 7 rows
    required = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_-.:%"
    glyphs = {ch: tuple(font[ord(ch) - 32].tolist()) for ch in required}
    for ch, g in glyphs.items():
        assert any(g), ch
    for a, b in itertools.combinations(required, 2):
        assert glyphs[a] != glyphs[b], (a, b)
    assert not font[0].any()                  # space
    box = tuple(overlay_font.glyph_rows("\x7f"))
    assert tuple(font[ord("#") - 32].tolist()) == box and box not in glyphs.values()
    pal = default_palette(20)
    assert pal.dtype == torch.uint8 and pal.shape == (20, 3) and torch.equal(pal, default_palette(20))
    assert len({tuple(c) for c in pal.tolist()}) == 20
    d = (pal[:, None].int() - pal[None].int()).abs().sum(-1) + torch.eye(20, dtype=torch.int32) * 999
    assert int(d.min()) >= 40                 # no two entries close in every channel
