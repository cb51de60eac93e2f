"""``ops.reference.jpeg_encode_ref`` — the definition the JPEG kernels are held to (test_gpu_jpeg.py)
— against the world: Pillow (libjpeg) decodes every stream, the tables are Pillow's own, the
decoded picture is as close to the source as Pillow's encoder gets, and the scenes of jpeg_scenes.py
really hold the cases they claim.  CPU only."""
import io
import re
from pathlib import Path

import pytest
import torch
from PIL import Image

import jpeg_scenes as S

KERNEL = Path(__file__).resolve().parents[1] / "aiko_services_amd" / "csrc" / "kernels" / "jpeg_ops.hip"


def _ref(raw, H, W, fmt, quality, **kw):
    from aiko_services_amd.ops.reference import jpeg_encode_ref
    return jpeg_encode_ref(raw, H, W, fmt, quality, **kw)


@pytest.mark.parametrize("fmt", S.FORMATS)
@pytest.mark.parametrize("H,W", S.SHAPES)
def test_pillow_loads_every_stream(fmt, H, W):
    from aiko_services_amd.ops import jpeg as J
    my = J.geometry(fmt, H, W)[3]
    for quality in S.QUALITIES:
        stream, nbytes = S.reference(fmt, H, W, quality)
        for b in range(3):
            data = S.stream_bytes(stream, nbytes, b)
            assert data.startswith(J.header(fmt, H, W, quality)) and data.endswith(b"\xff\xd9")
            assert not stream[b, int(nbytes[b]):].any()
            assert S.decode(data).shape == (H, W, 3)
            # my - 1 restart markers, 0..7 cyclically
            assert S.restart_markers(data, len(J.header(fmt, H, W, quality))) == [r % 8 for r in range(my - 1)]
    assert J.geometry("i420", 152, 24)[3] == 10          # the RST counter wraps in that shape


def test_tables_are_the_rule():
    import math
    from aiko_services_amd.ops import jpeg as J
    assert J.DCT_MATRIX[0][0] == 2896 and J.DCT_MATRIX[1][0] == 4017
    for k in range(8):
        for n in range(8):
            a = math.sqrt(1 / 8) if k == 0 else 0.5
            assert J.DCT_MATRIX[k][n] == round(8192 * a * math.cos((2 * n + 1) * k * math.pi / 16))
            assert J.DCT_MATRIX[k][7 - n] == (-1) ** k * J.DCT_MATRIX[k][n]      # what the kernel folds
    assert sorted(J.ZIGZAG) == list(range(64))
    assert J.ZIGZAG[:10] == (0, 1, 8, 16, 9, 2, 3, 10, 17, 24) and J.ZIGZAG[-3:] == (55, 62, 63)
    # the kernel's copy of the matrix
    text = re.search(r"JP_DCT\[64\]\s*=\s*\{([^}]*)\}", KERNEL.read_text()).group(1)
    assert tuple(int(v) for v in text.replace("\n", " ").split(",")) == tuple(v for row in J.DCT_MATRIX for v in row)
    # the device tables: codes by symbol, quantisers with exact reciprocals, the zigzag map
    ints = J._table_ints(75)
    assert len(ints) == J.TABLE_INTS
    for tc, base in ((0x10, 0), (0x11, 256), (0x00, 512), (0x01, 528)):
        for symbol, (code, length) in J.huffman_codes(tc).items():
            assert ints[base + symbol] == code | length << 16 and code < 1 << length <= 1 << 16
    for t, table in enumerate(J.quant_tables(75)):
        for z in range(64):
            assert ints[544 + 64 * t + z] == table[J.ZIGZAG[z]]
    for quality in (1, 100):
        ints = J._table_ints(quality)
        for i in range(128):
            q, rcp = ints[544 + i], ints[672 + i]
            assert (q == 1 and rcp == 0) or all((a * rcp) >> 32 == a // q for a in range(0, 1 << 16, 7))
    assert all(ints[800 + n] == z for z, n in enumerate(J.ZIGZAG))


@pytest.mark.parametrize("quality", [1, 30, 50, 75, 90, 95, 100])
def test_quantisation_tables_equal_pillows(quality):
    from aiko_services_amd.ops import jpeg as J
    rgb = S.structured_rgb(16, 16)
    for fmt in S.FORMATS:
        ours = Image.open(io.BytesIO(S.stream_bytes(*_ref(S.raw_from_rgb(rgb, fmt), 16, 16, fmt, quality))))
        theirs = Image.open(io.BytesIO(S.pillow_encode(rgb, fmt, quality)))
        got = {k: list(v) for k, v in ours.quantization.items()}
        assert got == {k: list(v) for k, v in theirs.quantization.items()}
        assert got == {0: list(J.quant_tables(quality)[0]), 1: list(J.quant_tables(quality)[1])}


def test_huffman_tables_equal_pillows():
    from aiko_services_amd.ops import jpeg as J
    rgb = S.structured_rgb(16, 16)
    theirs = dict((body[0], body[1:]) for m, body in S.segments(S.pillow_encode(rgb, "i420", 75)) if m == 0xC4)
    ours = [(body[0], body[1:]) for m, body in S.segments(J.header("i420", 16, 16, 75)) if m == 0xC4]
    assert [tc for tc, _ in ours] == [0x00, 0x10, 0x01, 0x11] and sorted(theirs) == [0x00, 0x01, 0x10, 0x11]
    for tc, body in ours:
        assert body == theirs[tc] == bytes(J.HUFFMAN[tc][0]) + bytes(J.HUFFMAN[tc][1])


def test_header_layout():
    from aiko_services_amd.ops import jpeg as J
    for fmt, luma in (("i420", 0x22), ("i444", 0x11)):
        head = J.header(fmt, 17, 23, 90)
        segs = S.segments(head)
        assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
        assert segs[0][1] == b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"
        assert segs[1][1][0] == 0 and segs[2][1][0] == 1 and len(segs[1][1]) == 65
        assert segs[3][1] == bytes([8, 0, 17, 0, 23, 3, 1, luma, 0, 2, 0x11, 1, 3, 0x11, 1])
        assert segs[8][1] == bytes([0, J.geometry(fmt, 17, 23)[4]])
        assert segs[9][1] == bytes([3, 1, 0, 2, 0x11, 3, 0x11, 0, 0x3F, 0])
        assert sum(len(b) + 4 for _, b in segs) + 2 == len(head)
    assert J.header("i444", 8, 8, 90)[-14:-12] == b"\xff\xda"
    assert J.capacities("i420", 480, 640) == (len(J.header("i420", 480, 640, 90)) + 460800, 15360)
    assert J.capacities("i420", 16, 4096)[1] == 96 * 1024 == J.MAX_SEG_CAP
    assert J.workspace_bytes("i420", 480, 640, 2) == 2 * 30 * (4 + 15360)


# Fidelity: our decoded frame against Pillow's own encoder at the same quality and subsampling, from
# the same RGB.  The margin of 0.5 dB is three times the 0.17 dB worst case of a prototype of the rule
# on smooth-plus-noise images of these sizes; the values seen are in profiles/jpeg_encode.md.
@pytest.mark.parametrize("fmt", S.FORMATS)
@pytest.mark.parametrize("H,W", [(40, 56), (33, 47), (64, 64)])
def test_fidelity_against_pillows_encoder(fmt, H, W):
    for quality in (30, 75, 95):
        rgb = S.smooth_noise_rgb(H, W)
        ours = S.psnr(S.decode(S.stream_bytes(*_ref(S.raw_from_rgb(rgb, fmt), H, W, fmt, quality))), rgb.numpy())
        theirs = S.psnr(S.decode(S.pillow_encode(rgb, fmt, quality)), rgb.numpy())
        print(f"fidelity {fmt} {H} x {W} quality {quality}: ours {ours:.2f} dB, Pillow {theirs:.2f} dB, "
              f"difference {ours - theirs:+.2f} dB")
        assert ours >= theirs - 0.5


# ---- the cases a coder gets wrong: each asserts that the condition really occurs -------------

def test_only_coefficient_63():
    raw, H, W, fmt = S.only_63_raw()
    trace = []
    stream, nbytes = _ref(raw, H, W, fmt, 100, trace=trace)
    y = [t for t in trace if t[2] == 0]
    assert [(t[3], t[4]) for t in y] == [("dc", 0), ("ac", 0xF0), ("ac", 0xF0), ("ac", 0xF0), ("ac", 0xE9)]
    assert y[-1][5] == 440                                 # run 14 after three ZRLs = 62 zeros; no EOB
    assert S.decode(S.stream_bytes(stream, nbytes)).shape == (8, 8, 3)


def test_largest_sizes():
    raw, H, W, fmt = S.checker_raw()
    trace = []
    stream, nbytes = _ref(raw, H, W, fmt, 100, trace=trace)
    assert max(t[4] for t in trace if t[3] == "dc") == 11
    assert {abs(t[5]) for t in trace if t[3] == "dc" and t[4] == 11} == {2039}
    assert max(t[4] & 15 for t in trace if t[3] == "ac") == 10
    got = S.decode(S.stream_bytes(stream, nbytes)).astype(int)[..., 1]
    want = raw[0, :H * W].view(H, W).numpy().astype(int)
    assert abs(got - want).max() <= 3                      # every quantiser is 1; the DC clamp costs 1


def test_noise_is_stuffed_and_flat_is_all_eob():
    from aiko_services_amd.ops import jpeg as J
    H, W = 17, 23
    for fmt in S.FORMATS:
        stream, nbytes = S.reference(fmt, H, W, 90)
        head = len(J.header(fmt, H, W, 90))
        noise, flat = S.stream_bytes(stream, nbytes, 0), S.stream_bytes(stream, nbytes, 1)
        assert b"\xff\x00" in noise[head:]
        # no 0xFF in the coded data is followed by anything but a stuffed zero or a marker
        assert all(noise[i + 1] == 0 or 0xD0 <= noise[i + 1] <= 0xD9 for i in range(head, len(noise) - 1)
                   if noise[i] == 0xFF)
        trace = []
        _ref(S.flat_raw(fmt, H, W), H, W, fmt, 90, trace=trace)
        assert {t[4] for t in trace if t[3] == "ac"} == {0x00}
        _, _, nblk, my, mx = J.geometry(fmt, H, W)
        assert len([t for t in trace if t[3] == "ac"]) == nblk * mx * my
        assert len(flat) < head + 4 * my * mx * nblk


# ---- the overflow rule, both ways ---------------------------------------------------------------

def test_overflow_of_cap():
    from aiko_services_amd.ops import jpeg as J
    H, W = S.OVERFLOW_SHAPE
    raw = S.noise_raw("i420", H, W)
    cap, seg_cap = J.capacities("i420", H, W)
    fits = _ref(raw, H, W, "i420", 90)
    assert 0 < int(fits[1][0]) <= cap and fits[0].shape == (1, cap)
    over = _ref(raw, H, W, "i420", 100)
    assert int(over[1][0]) == -1
    big = _ref(raw, H, W, "i420", 100, cap=4 * cap, seg_cap=4 * seg_cap)
    assert int(big[1][0]) > cap                            # the whole stream is longer than cap
    print(f"noise 152 x 24 i420: {int(fits[1][0])} bytes at quality 90, {int(big[1][0])} at 100, cap {cap}")
    exact = int(fits[1][0])
    assert int(_ref(raw, H, W, "i420", 90, cap=exact)[1][0]) == exact
    assert int(_ref(raw, H, W, "i420", 90, cap=exact - 1)[1][0]) == -1


def test_overflow_of_seg_cap():
    from aiko_services_amd.ops import jpeg as J
    raw, H, W, fmt = S.one_noisy_row_raw()
    cap, seg_cap = J.capacities(fmt, H, W)
    roomy = _ref(raw, H, W, fmt, 100, seg_cap=4 * seg_cap)
    total = int(roomy[1][0])
    assert 0 < total <= cap                                # the whole stream fits cap
    assert int(_ref(raw, H, W, fmt, 100)[1][0]) == -1      # one segment is past seg_cap
    # the longest stuffed segment, from the stream itself: it is the noisy row's
    data = S.stream_bytes(*roomy)
    head = len(J.header(fmt, H, W, 100))
    cuts = [i for i in range(head, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD9]
    lengths = [b - a for a, b in zip([head] + [c + 2 for c in cuts[:-1]], cuts)]
    assert len(lengths) == 10 and max(lengths) == lengths[2] > seg_cap
    assert int(_ref(raw, H, W, fmt, 100, seg_cap=lengths[2])[1][0]) == total
    assert int(_ref(raw, H, W, fmt, 100, seg_cap=lengths[2] - 1)[1][0]) == -1


def test_front_end_refusals_need_no_device():
    from aiko_services_amd.ops import jpeg as J
    raw = torch.zeros(1, 384, dtype=torch.uint8)
    for fmt in ("nv12", "yuyv", "rgb"):
        with pytest.raises(ValueError, match="format"):
            J.jpeg_encode(raw, 16, 16, fmt)
        with pytest.raises(ValueError, match="format"):
            J.header(fmt, 16, 16, 90)
    for quality in (0, 101, True, 50.0, None):
        with pytest.raises(ValueError, match="quality"):
            J.jpeg_encode(raw, 16, 16, "i420", quality)
    with pytest.raises(ValueError, match="raw"):
        J.jpeg_encode(raw, 16, 18, "i420")
    with pytest.raises(ValueError, match="raw"):
        J.jpeg_encode(raw[0], 16, 16, "i420")
    for H, W in ((0, 16), (16, 0), (16, 4097), (65536, 16)):
        with pytest.raises(ValueError, match="height"):
            J.geometry("i420", H, W)


# ---- the host side: coded frames into an MJPG .avi -------------------------------------------------

def _coded(H=33, W=47, quality=90, seed=0):
    rgb = S.structured_rgb(H, W, seed)
    return rgb, S.stream_bytes(*_ref(S.raw_from_rgb(rgb, "i420"), H, W, "i420", quality))


def test_avi_writer_takes_coded_frames(tmp_path):
    import numpy as np
    from aiko_services_amd.elements.media.avi import AviWriter, _parse, avi_info, jpeg_size, read_avi
    rgb, data = _coded()
    assert jpeg_size(data) == (33, 47) and jpeg_size(S.pillow_encode(rgb, "i444", 50)) == (33, 47)
    path = tmp_path / "a.avi"
    with AviWriter(path, 47, 33, 25) as writer:
        writer.write_jpeg(data)
        writer.write_jpeg(np.frombuffer(data, np.uint8))
        writer.write(rgb.numpy())                           # the host encode still works next to it
        for bad, text in ((data[:-2], "SOI to EOI"), (b"xx" + data, "SOI to EOI"), (_coded(16, 16)[1], "does not match")):
            with pytest.raises(ValueError, match=text):
                writer.write_jpeg(bad)
    info = avi_info(path)
    assert (info["width"], info["height"], info["frames"], info["compression"]) == (47, 33, 3, b"MJPG")
    _, chunks = _parse(path)
    whole = path.read_bytes()
    assert [whole[o:o + n] for o, n, _ in chunks[:2]] == [data, data] and all(c == b"00dc" for _, _, c in chunks)
    back = read_avi(path)
    assert np.array_equal(back[0], S.decode(data)) and np.array_equal(back[1], back[0])
    with AviWriter(tmp_path / "r.avi", 47, 33, 25, codec="raw") as writer:
        with pytest.raises(ValueError, match="MJPG"):
            writer.write_jpeg(data)


def test_video_write_file_takes_coded_frames(tmp_path):
    import queue
    from types import SimpleNamespace
    import numpy as np
    from aiko_services_amd.elements.media.avi import avi_info, read_avi
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    from aiko_services_amd.pipeline.stream import StreamEvent

    def element_for(target, **parameters):
        d = {"version": 0, "name": "p_write", "runtime": "python", "graph": ["(VideoWriteFile)"], "parameters": {},
             "elements": [{"name": "VideoWriteFile", "input": [{"name": "images", "type": "[image]"}], "output": [],
                           "parameters": {"data_targets": f"file://{target}", **parameters},
                           "deploy": {"local": {"module": "aiko_services_amd.elements.media.video_io"}}}]}
        p = PipelineImpl.create_pipeline("<write>", parse_pipeline_definition_dict(d), None, None, "w", [], 0, None, 60,
                                         queue_response=queue.Queue())
        element = p.pipeline_graph.get_node("VideoWriteFile").element
        stream = SimpleNamespace(variables={}, frame_id=0)
        assert element.start_stream(stream, "w")[0] == 0
        return element, stream

    frames = [np.frombuffer(_coded(seed=s)[1], np.uint8) for s in range(3)]
    path = tmp_path / "out.avi"
    element, stream = element_for(path, raw=True, format="jpeg", rate=25)
    assert element.process_frame(stream, images=frames[:2])[0] == StreamEvent.OKAY
    assert element.process_frame(stream, images=frames[2:])[0] == StreamEvent.OKAY
    event, out = element.process_frame(stream, images=[frames[0][:-1]])
    assert event == StreamEvent.ERROR and "SOI to EOI" in out["diagnostic"]
    element.stop_stream(stream, "w")
    info = avi_info(path)
    assert (info["width"], info["height"], info["frames"], info["fps"]) == (47, 33, 3, 25.0)
    assert all(np.array_equal(a, S.decode(f.tobytes())) for a, f in zip(read_avi(path), frames))
    # the size can be given; a file of another kind, or frames that are no JPEG, are errors
    element, stream = element_for(tmp_path / "sized.avi", raw=True, format="jpeg", height=33, width=47)
    assert element.process_frame(stream, images=frames[:1])[0] == StreamEvent.OKAY
    element.stop_stream(stream, "w")
    for target, images, text in ((tmp_path / "out.y4m", frames[:1], ".avi"),
                                 (tmp_path / "junk.avi", [np.zeros(64, np.uint8)], "frame header")):
        element, stream = element_for(target, raw=True, format="jpeg")
        event, out = element.process_frame(stream, images=images)
        assert event == StreamEvent.ERROR and text in out["diagnostic"], out
        assert not target.exists()
