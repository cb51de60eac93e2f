"""Video elements (reference ``elements/media/video_io.py:96-308``, ``webcam_io.py:61-144``).

OpenCV is optional (absent on the MI355X boxes).  Without it, video files are read/written
with in-repo codecs: ``.avi`` (RIFF container, Motion-JPEG through Pillow or uncompressed DIB
frames — ``avi.py``; what cameras and ``cv2.VideoWriter('MJPG')`` produce), animated ``.gif``
(Pillow), raw ``.y4m`` (YUV4MPEG2, 4:2:0 / 4:4:4, converted to RGB with BT.601), ``.npy``
arrays ``[T, H, W, 3]`` uint8, and directories of images.  With OpenCV present any other
container it supports works too.
``VideoShow`` needs a display: without one it logs frame statistics instead.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

from ...pipeline.engine import PipelineElement
from ...pipeline.stream import StreamEvent
from .avi import AviWriter, iter_avi, jpeg_size
from .common_io import DataSource, DataTarget, contains_all

try:  # optional
    import cv2  # type: ignore
    _CV2 = True
except ImportError:
    cv2 = None
    _CV2 = False

__all__ = ["VideoOutput", "VideoReadFile", "VideoSample", "VideoShow", "VideoWriteFile",
           "VideoReadWebcam", "read_y4m", "write_y4m", "iter_video_frames"]


# ---- Y4M codec (YUV4MPEG2) ------------------------------------------------------------------

def _yuv_to_rgb(y, u, v):
    y = y.astype(np.float32)
    u = u.astype(np.float32) - 128.0
    v = v.astype(np.float32) - 128.0
    r = y + 1.402 * v
    g = y - 0.344136 * u - 0.714136 * v
    b = y + 1.772 * u
    return np.clip(np.stack([r, g, b], -1) + 0.5, 0, 255).astype(np.uint8)


def _rgb_to_yuv(rgb):
    f = rgb.astype(np.float32)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    u = -0.168736 * r - 0.331264 * g + 0.5 * b + 128.0
    v = 0.5 * r - 0.418688 * g - 0.081312 * b + 128.0
    c = lambda a: np.clip(a + 0.5, 0, 255).astype(np.uint8)  # noqa: E731
    return c(y), c(u), c(v)


def iter_y4m(path, raw=False):
    """RGB uint8 [H, W, 3] frames of a YUV4MPEG2 file.  ``raw=True``: no conversion — per frame
    ``(fmt, h, w, packed)`` with ``packed`` the frame's planes as one 1-D uint8 array in the layout
    ``ops.yuv`` names ``fmt``: ``i420`` for every ``C420*`` tag, ``i444`` for ``C444``."""
    with open(path, "rb") as f:
        header = f.readline().decode("ascii").split()
        if not header or header[0] != "YUV4MPEG2":
            raise ValueError(f"{path}: not a YUV4MPEG2 file")
        params = {t[0]: t[1:] for t in header[1:]}
        w, h = int(params["W"]), int(params["H"])
        cs = params.get("C", "420jpeg")
        chroma444 = cs.startswith("444")
        cw, ch = (w, h) if chroma444 else ((w + 1) // 2, (h + 1) // 2)
        if raw and cs != "444" and not cs.startswith("420"):
            raise ValueError(f"{path}: chroma C{cs} has no raw format (C420* and C444 do)")
        while True:
            line = f.readline()
            if not line:
                return
            if not line.startswith(b"FRAME"):
                raise ValueError(f"{path}: corrupt frame header")
            if raw:
                packed = np.frombuffer(f.read(w * h + 2 * cw * ch), np.uint8)
                if packed.size != w * h + 2 * cw * ch:
                    raise ValueError(f"{path}: truncated frame")
                yield ("i444" if chroma444 else "i420"), h, w, packed
                continue
            y = np.frombuffer(f.read(w * h), np.uint8).reshape(h, w)
            u = np.frombuffer(f.read(cw * ch), np.uint8).reshape(ch, cw)
            v = np.frombuffer(f.read(cw * ch), np.uint8).reshape(ch, cw)
            if not chroma444:
                u = u.repeat(2, 0).repeat(2, 1)[:h, :w]
                v = v.repeat(2, 0).repeat(2, 1)[:h, :w]
            yield _yuv_to_rgb(y, u, v)


def read_y4m(path) -> np.ndarray:
    return np.stack(list(iter_y4m(path)))


def _rgb_to_yuv420(rgb):
    """(y [H, W], u, v [ceil(H/2), ceil(W/2)]) of an RGB frame, 4:2:0 with centre ("jpeg") siting:
    luma per pixel, each chroma sample from the mean RGB of its 2x2 block's in-frame pixels (2 or 1
    at an odd right or bottom edge) — the integer sum of the bytes times 1/n, as
    ``ops/yuv.py`` defines it for the device (``rgb_to_yuv``, ``i420``, ``jpeg``)."""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    ph, pw = (h + 1) // 2 * 2, (w + 1) // 2 * 2
    s = np.zeros((ph, pw, 3), np.int32)
    s[:h, :w] = rgb
    n = np.zeros((ph, pw), np.int32)
    n[:h, :w] = 1
    s = s.reshape(ph // 2, 2, pw // 2, 2, 3).sum((1, 3))
    n = n.reshape(ph // 2, 2, pw // 2, 2).sum((1, 3))
    mean = s.astype(np.float32) * (np.float32(1.0) / n.astype(np.float32))[..., None]
    y = _rgb_to_yuv(rgb)[0]
    _, u, v = _rgb_to_yuv(mean)
    return y, u, v


class Y4MWriter:
    """``chroma``: ``"444"`` (default) or ``"420jpeg"``, the file's ``C`` tag.  ``write`` converts an
    RGB frame on the host; ``write_raw`` takes a frame's planes as they are: packed ``i444`` /
    ``i420`` bytes (``ops.yuv``), for instance from ``RgbToYuv`` with the ``jpeg`` standard."""

    def __init__(self, path, width, height, fps=30, chroma="444"):
        if chroma not in ("444", "420jpeg"):
            raise ValueError(f"Y4MWriter: chroma {chroma!r} not supported (444 or 420jpeg)")
        self.f = open(path, "wb")
        self.w, self.h, self.chroma = int(width), int(height), chroma
        cw, ch = (self.w, self.h) if chroma == "444" else ((self.w + 1) // 2, (self.h + 1) // 2)
        self.frame_bytes = self.w * self.h + 2 * cw * ch
        self.f.write(f"YUV4MPEG2 W{width} H{height} F{int(fps)}:1 Ip A1:1 C{chroma}\n".encode())

    def write(self, rgb):
        rgb = np.asarray(rgb)[: self.h, : self.w]
        y, u, v = _rgb_to_yuv(rgb) if self.chroma == "444" else _rgb_to_yuv420(rgb)
        self.f.write(b"FRAME\n")
        self.f.write(y.tobytes())
        self.f.write(u.tobytes())
        self.f.write(v.tobytes())

    def write_raw(self, packed):
        packed = np.ascontiguousarray(np.asarray(packed, dtype=np.uint8)).reshape(-1)
        if packed.size != self.frame_bytes:
            raise ValueError(f"Y4MWriter: a C{self.chroma} frame of {self.w} x {self.h} has {self.frame_bytes} "
                             f"bytes, got {packed.size}")
        self.f.write(b"FRAME\n")
        self.f.write(packed.tobytes())

    def close(self):
        self.f.close()


def write_y4m(path, frames, fps=30):
    frames = list(frames)
    h, w = frames[0].shape[:2]
    wr = Y4MWriter(path, w, h, fps)
    for fr in frames:
        wr.write(fr)
    wr.close()


def iter_video_frames(path, raw=False):
    """RGB uint8 frames of a video file / frame directory, whatever backend is available.
    ``raw=True``: each frame as a 1-D uint8 array, unconverted: a Y4M file's packed planes, or the
    coded frames of a Motion-JPEG ``.avi`` (for ``JpegDecode``)."""
    path = Path(path)
    if raw:
        if not path.is_dir() and path.suffix.lower() == ".avi":
            yield from iter_avi(path, raw=True)
            return
        if path.is_dir() or path.suffix.lower() != ".y4m":
            raise ValueError(f"{path}: raw frames need a .y4m file")
        for _fmt, _h, _w, packed in iter_y4m(path, raw=True):
            yield packed
        return
    if path.is_dir():
        from PIL import Image
        for p in sorted(path.iterdir()):
            if p.suffix.lower() in (".png", ".jpg", ".jpeg", ".bmp", ".ppm"):
                yield np.asarray(Image.open(p).convert("RGB"))
        return
    suffix = path.suffix.lower()
    if suffix == ".avi" and not _CV2:
        yield from iter_avi(path)
    elif suffix == ".gif":
        from PIL import Image, ImageSequence
        with Image.open(path) as im:
            for fr in ImageSequence.Iterator(im):
                yield np.asarray(fr.convert("RGB"))
    elif suffix == ".y4m":
        yield from iter_y4m(path)
    elif suffix in (".npy", ".npz"):
        arr = np.load(path, allow_pickle=False)
        if hasattr(arr, "files"):
            arr = arr[arr.files[0]]
        yield from arr
    elif _CV2:
        cap = cv2.VideoCapture(str(path))
        if not cap.isOpened():
            raise ValueError(f"Couldn't open video file: {path}")
        try:
            while True:
                ok, bgr = cap.read()
                if not ok:
                    return
                yield cv2.cvtColor(bgr, cv2.COLOR_BGR2RGB)
        finally:
            cap.release()
    else:
        raise ValueError(f"{path}: unsupported video format without OpenCV "
                         f"(use .avi, .gif, .y4m, .npy or a frame directory)")


# ---- elements -------------------------------------------------------------------------------

class VideoOutput(PipelineElement):
    def __init__(self, context):
        context.set_protocol("video_output:0")
        context.get_implementation("PipelineElement").__init__(self, context)

    def process_frame(self, stream, images):
        return StreamEvent.OKAY, {"images": images}


class VideoReadFile(DataSource):
    """Parameter ``raw: true``: for a Y4M file ``images`` are the frames' packed planes, 1-D uint8
    arrays, for a ``FrameUpload`` with ``format`` i420 / i444; for a Motion-JPEG ``.avi`` they are the
    coded frames as they lie in the file, for a ``JpegDecode``; any other file is an error."""

    def __init__(self, context):
        context.set_protocol("video_read_file:0")
        context.get_implementation("PipelineElement").__init__(self, context)

    def start_stream(self, stream, stream_id):
        stream.variables["video_frame_generator"] = None
        return super().start_stream(stream, stream_id, use_create_frame=False)

    def frame_generator(self, stream, frame_id):
        gen = stream.variables.get("video_frame_generator")
        while True:
            if gen is None:
                try:
                    path, _ = next(stream.variables["source_paths_generator"])
                except StopIteration:
                    return StreamEvent.STOP, {"diagnostic": "End of video file(s)"}
                try:
                    raw = str(self.get_parameter("raw", False)[0]).lower() in ("true", "1", "yes")
                    gen = iter_video_frames(path, raw=raw)
                except ValueError as exc:
                    return StreamEvent.ERROR, {"diagnostic": str(exc)}
                stream.variables["video_frame_generator"] = gen
            try:
                return StreamEvent.OKAY, {"images": [next(gen)]}
            except StopIteration:
                gen = None
                stream.variables["video_frame_generator"] = None
            except ValueError as exc:
                return StreamEvent.ERROR, {"diagnostic": str(exc)}

    def process_frame(self, stream, images):
        return StreamEvent.OKAY, {"images": images}

    def stop_stream(self, stream, stream_id):
        stream.variables["video_frame_generator"] = None
        return StreamEvent.OKAY, {}


class VideoSample(PipelineElement):
    def __init__(self, context):
        context.set_protocol("video_sample:0")
        context.get_implementation("PipelineElement").__init__(self, context)

    def process_frame(self, stream, images):
        rate, _ = self.get_parameter("sample_rate", 1)
        if stream.frame_id % int(rate):
            return StreamEvent.DROP_FRAME, {}
        return StreamEvent.OKAY, {"images": images}


class VideoShow(PipelineElement):
    def __init__(self, context):
        context.set_protocol("video_show:0")
        context.get_implementation("PipelineElement").__init__(self, context)

    def process_frame(self, stream, images):
        title, _ = self.get_parameter("title", "Video")
        for image in images:
            arr = np.asarray(image)
            if _CV2:
                try:
                    bgr = cv2.cvtColor(arr, cv2.COLOR_RGB2BGR) if arr.ndim == 3 else arr
                    cv2.imshow(title, bgr)
                    if cv2.waitKey(1) & 0xFF == ord("x"):
                        return StreamEvent.STOP, {"diagnostic": "VideoShow exit"}
                    continue
                except Exception:
                    pass
            self.logger.debug(f"{title} {self.my_id()}: {arr.shape} mean={float(arr.mean()):.1f}")
        return StreamEvent.OKAY, {}

    def stop_stream(self, stream, stream_id):
        if _CV2:
            try:
                cv2.destroyAllWindows()
            except Exception:
                pass
        return StreamEvent.OKAY, {}


class VideoWriteFile(DataTarget):
    """Writes ``.avi`` (parameters ``codec``: ``MJPG`` (default) | ``raw``, ``quality``),
    ``.gif``, ``.y4m`` or ``.npy``; other suffixes need OpenCV.  ``rate``: frames per second.
    ``raw: true`` (``.y4m`` only) with ``format: i420 | i444``, ``height`` and ``width``: 1-D
    ``images`` are a frame's packed planes (``RgbToYuv`` then ``FrameDownload``) and are written
    unconverted, ``C420jpeg`` or ``C444``; ``raw: true`` with ``format: jpeg`` (``.avi`` only): 1-D
    ``images`` are complete JPEG files (``JpegEncode`` then ``JpegResults``) and become the frames of
    an MJPG video as they are, its size taken from the first (or from ``height`` and ``width``);
    anything else is an error."""

    _RAW_CHROMA = {"i420": "420jpeg", "i444": "444"}

    def _raw_writer(self, path, suffix, first=None):
        """``(writer, None)`` for ``raw: true``, or ``(None, diagnostic)``; ``first``: the first frame."""
        fmt = str(self.get_parameter("format", "")[0]).lower()
        height, width = self.get_parameter("height", None)[0], self.get_parameter("width", None)[0]
        if fmt == "jpeg":
            if suffix != ".avi":
                return None, f"{path}: coded JPEG frames need a .avi file"
            try:
                if height is None or width is None:
                    height, width = jpeg_size(np.asarray(first, np.uint8).tobytes())
            except (ValueError, TypeError) as exc:
                return None, f"{path}: {exc}"
            rate, _ = self.get_parameter("rate", 30)
            return AviWriter(path, int(width), int(height), float(rate), "MJPG"), None
        if suffix != ".y4m":
            return None, f"{path}: raw frames need a .y4m file"
        if fmt not in self._RAW_CHROMA:
            return None, f"{path}: raw format {fmt!r} cannot be written (i420 or i444)"
        if height is None or width is None:
            return None, f"{path}: raw frames need the height and width parameters"
        rate, _ = self.get_parameter("rate", 30)
        return Y4MWriter(path, int(width), int(height), float(rate), self._RAW_CHROMA[fmt]), None

    def __init__(self, context):
        context.set_protocol("video_write_file:0")
        context.get_implementation("PipelineElement").__init__(self, context)

    def start_stream(self, stream, stream_id):
        event, diag = super().start_stream(stream, stream_id)
        if event == StreamEvent.OKAY:
            path = stream.variables["target_path"]
            if contains_all(path, "{}"):
                path = path.format(stream.variables["target_file_id"])
            stream.variables["video_path"] = path
            stream.variables["video_writer"] = None
            stream.variables["video_frames"] = []
        return event, diag

    def process_frame(self, stream, images):
        path = stream.variables["video_path"]
        suffix = Path(path).suffix.lower()
        raw = str(self.get_parameter("raw", False)[0]).lower() in ("true", "1", "yes")
        if raw and stream.variables["video_writer"] is None:
            writer, diagnostic = self._raw_writer(path, suffix, images[0] if len(images) else None)
            if writer is None:
                return StreamEvent.ERROR, {"diagnostic": diagnostic}
            stream.variables["video_writer"] = writer
        for image in images:
            arr = np.asarray(image).astype(np.uint8)
            if raw and arr.ndim == 1:
                try:
                    writer = stream.variables["video_writer"]
                    (writer.write_jpeg if isinstance(writer, AviWriter) else writer.write_raw)(arr)
                except ValueError as exc:
                    return StreamEvent.ERROR, {"diagnostic": str(exc)}
                continue
            if suffix in (".npy", ".gif"):
                stream.variables["video_frames"].append(arr)
                continue
            writer = stream.variables["video_writer"]
            if writer is None:
                rate, _ = self.get_parameter("rate", 30)
                if suffix == ".y4m":
                    writer = Y4MWriter(path, arr.shape[1], arr.shape[0], float(rate))
                elif suffix == ".avi" and not _CV2:
                    codec, _ = self.get_parameter("codec", "MJPG")
                    quality, _ = self.get_parameter("quality", 90)
                    writer = AviWriter(path, arr.shape[1], arr.shape[0], float(rate), str(codec), int(quality))
                elif _CV2:
                    writer = cv2.VideoWriter(path, cv2.VideoWriter_fourcc(*"mp4v"), float(rate),
                                             (arr.shape[1], arr.shape[0]))
                else:
                    return StreamEvent.ERROR, {"diagnostic": f"{path}: unsupported format without OpenCV"}
                stream.variables["video_writer"] = writer
            if isinstance(writer, (Y4MWriter, AviWriter)):
                writer.write(arr)
            else:
                writer.write(cv2.cvtColor(arr, cv2.COLOR_RGB2BGR))
        return StreamEvent.OKAY, {}

    def stop_stream(self, stream, stream_id):
        path = stream.variables.get("video_path")
        frames = stream.variables.get("video_frames")
        suffix = Path(path).suffix.lower() if path else ""
        if path and frames and suffix == ".npy":
            np.save(path, np.stack(frames))
        elif path and frames and suffix == ".gif":
            from PIL import Image
            rate, _ = self.get_parameter("rate", 30)
            ims = [Image.fromarray(f if f.ndim == 3 else np.repeat(f[..., None], 3, 2)) for f in frames]
            ims[0].save(path, save_all=True, append_images=ims[1:], duration=int(round(1000 / float(rate))), loop=0)
        writer = stream.variables.get("video_writer")
        if writer is not None:
            (writer.close if isinstance(writer, (Y4MWriter, AviWriter)) else writer.release)()
        return StreamEvent.OKAY, {}


from .webcam_io import VideoReadWebcam  # noqa: E402,F401  (kept importable from here)
