"""Plain PyTorch references of the native ops — used ONLY by tests / numerics checks.

Every HIP kernel in ``csrc/kernels`` has a counterpart here operating on NCHW tensors (torch's
native layout) so the tests compare two independent implementations.  ``conv_ref`` and
``linear_ref`` follow the dtype of their input: fp32, or fp64 for the per-pixel / per-channel
bounds of the conv tests.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .conv import ACT_GELU, ACT_RELU, ACT_SILU, ConvSpec
from .vision import IMAGENET_MEAN, IMAGENET_STD


def act_ref(x: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_RELU:
        return F.relu(x)
    if act == ACT_SILU:
        return F.silu(x)
    if act == ACT_GELU:
        return F.gelu(x)
    return x


def _conv_taps(x, w, b, stride: int, pad: int) -> torch.Tensor:
    """The convolution as one matmul per filter tap on strided views of the padded input: the
    fp64 form for a device, where only matmul is relied on in fp64."""
    B, _, H, W = x.shape
    R, S = w.shape[2:]
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    xp = F.pad(x, (pad, pad, pad, pad))
    y = torch.zeros(B, w.shape[0], Ho, Wo, dtype=x.dtype, device=x.device)
    for r in range(R):
        for s in range(S):
            tap = xp[:, :, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride]
            y += torch.einsum("bchw,oc->bohw", tap, w[:, :, r, s])
    return y if b is None else y + b.view(1, -1, 1, 1)


def conv_ref(x_nchw: torch.Tensor, spec: ConvSpec, residual_nchw: torch.Tensor | None = None,
             residual_after_act: bool = False) -> torch.Tensor:
    """In the dtype of ``x_nchw``: fp32 as the tests' plain reference, fp64 (``x.double()``) for
    the per-pixel / per-channel bounds.  ``ref_weight`` is the bf16-rounded weight, so kernel
    and reference start from the same operands."""
    w = spec.ref_weight.to(device=x_nchw.device, dtype=x_nchw.dtype)
    b = None if spec.ref_bias is None else spec.ref_bias.to(device=x_nchw.device, dtype=x_nchw.dtype)
    pad = spec.stem_pad if spec.kind == "stem" else spec.pad
    if x_nchw.dtype == torch.float64 and x_nchw.is_cuda:
        y = _conv_taps(x_nchw, w, b, spec.stride, pad)
    else:
        y = F.conv2d(x_nchw, w, b, stride=spec.stride, padding=pad)
    if residual_nchw is not None and residual_after_act:
        return act_ref(y, spec.act) + residual_nchw
    if residual_nchw is not None:
        y = y + residual_nchw
    return act_ref(y, spec.act)


def linear_ref(x: torch.Tensor, spec: ConvSpec) -> torch.Tensor:
    w = spec.ref_weight.to(device=x.device, dtype=x.dtype).reshape(spec.cout, -1)
    b = None if spec.ref_bias is None else spec.ref_bias.to(device=x.device, dtype=x.dtype)
    return act_ref(F.linear(x, w, b), spec.act)


def preprocess_ref(frames_u8: torch.Tensor, size=(224, 224), mean=IMAGENET_MEAN, std=IMAGENET_STD,
                   bgr: bool = False) -> torch.Tensor:
    """uint8 NHWC -> fp32 NCHW normalised (bilinear, half-pixel centres)."""
    x = frames_u8.permute(0, 3, 1, 2).float()
    if bgr:
        x = x.flip(1)
    if tuple(x.shape[-2:]) != tuple(size):
        x = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    m = torch.tensor(mean, device=x.device).view(1, 3, 1, 1)
    s = torch.tensor(std, device=x.device).view(1, 3, 1, 1)
    return (x / 255.0 - m) / s


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2).float()


def nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


# ---- detection ------------------------------------------------------------------------------

def yolo_decode_ref(feats_nchw, strides, nc: int, reg_max: int = 16):
    """Per-level head outputs (fp32 NCHW, 4*reg_max + nc channels) -> boxes [B, A, 4] xyxy,
    max-class sigmoid scores [B, A], class ids [B, A] (levels concatenated, row-major)."""
    boxes, scores, classes = [], [], []
    for f, s in zip(feats_nchw, strides):
        B, _, H, W = f.shape
        f = f.float()
        box = f[:, :4 * reg_max].reshape(B, 4, reg_max, H * W).softmax(2)
        dist = (box * torch.arange(reg_max, device=f.device, dtype=torch.float32).view(1, 1, -1, 1)).sum(2)
        ys, xs = torch.meshgrid(torch.arange(H, device=f.device), torch.arange(W, device=f.device),
                                indexing="ij")
        ax = (xs.reshape(-1).float() + 0.5)
        ay = (ys.reshape(-1).float() + 0.5)
        xyxy = torch.stack([ax - dist[:, 0], ay - dist[:, 1], ax + dist[:, 2], ay + dist[:, 3]], -1) * s
        logit, c = f[:, 4 * reg_max:].reshape(B, nc, H * W).max(1)
        boxes.append(xyxy)
        scores.append(torch.sigmoid(logit))
        classes.append(c.int())
    return torch.cat(boxes, 1), torch.cat(scores, 1), torch.cat(classes, 1)


def box_iou_ref(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    iw = (torch.minimum(a[:, None, 2], b[None, :, 2]) - torch.maximum(a[:, None, 0], b[None, :, 0])).clamp(min=0)
    ih = (torch.minimum(a[:, None, 3], b[None, :, 3]) - torch.maximum(a[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = iw * ih
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / (area_a[:, None] + area_b[None, :] - inter)


def nms_ref(boxes, scores, cls, conf=0.25, iou=0.7, max_candidates=1024, max_det=300,
            max_wh=7680.0):
    """Greedy class-aware NMS for ONE image (Ultralytics ``non_max_suppression`` semantics with
    a candidate cap; ties in score -> lower anchor index first).  Returns kept anchor indices."""
    idx = torch.nonzero(scores > conf).flatten()
    if idx.numel() == 0:
        return idx
    order = torch.sort(scores[idx], descending=True, stable=True).indices
    idx = idx[order][:max_candidates]
    b = boxes[idx] + cls[idx].float()[:, None] * max_wh
    m = box_iou_ref(b, b) > iou
    removed = torch.zeros(idx.numel(), dtype=torch.bool, device=boxes.device)
    keep = []
    m = m.cpu()
    removed = removed.cpu()
    for i in range(idx.numel()):
        if removed[i]:
            continue
        keep.append(i)
        if len(keep) == max_det:
            break
        removed |= m[i] & (torch.arange(idx.numel()) > i)
    return idx[torch.tensor(keep, dtype=torch.long, device=boxes.device)]


# ---- ROI crop -------------------------------------------------------------------------------

def roi_rects_ref(det: torch.Tensor, count: torch.Tensor, k: int, hw, margin: float = 0.0) -> torch.Tensor:
    """Rects of ``ops.roi.roi_crop``: int32 ``[B*k, 4]`` = (X0, Y0, X1, Y1), half-open, zero for a
    slot that is not used.  fp32 throughout, one rounding per operation in the kernel's order
    (``margin`` is a float32 scalar), so the kernel's rects equal these bit for bit.  CPU or GPU."""
    H, W = int(hw[0]), int(hw[1])
    B = det.shape[0]
    d = det[:, :k, :4].to(torch.float32)
    x1, y1, x2, y2 = d.unbind(-1)
    m = torch.tensor(float(margin), dtype=torch.float32, device=det.device)
    bw, bh = x2 - x1, y2 - y1
    ex, ey = m * bw, m * bh
    fx0, fx1 = torch.floor(x1 - ex), torch.ceil(x2 + ex)
    fy0, fy1 = torch.floor(y1 - ey), torch.ceil(y2 + ey)
    X0 = fx0.clamp(0, W - 1)
    X1 = torch.maximum(fx1, X0 + 1).clamp(max=W)
    Y0 = fy0.clamp(0, H - 1)
    Y1 = torch.maximum(fy1, Y0 + 1).clamp(max=H)
    n = count.to(torch.int64).clamp(0, k)
    valid = (torch.arange(k, device=det.device)[None, :] < n[:, None]) & torch.isfinite(d).all(-1)
    rect = torch.stack([X0, Y0, X1, Y1], -1)
    rect = torch.where(valid[..., None], rect, torch.zeros_like(rect))     # drops the NaNs of unused rows
    return rect.to(torch.int32).reshape(B * k, 4)


def roi_crop_ref(frames: torch.Tensor, det: torch.Tensor, count: torch.Tensor, k: int, size=(224, 224),
                 margin: float = 0.0):
    """``ops.roi.roi_crop`` with torch: one bilinear ``F.interpolate`` (half-pixel centres) per
    rect of :func:`roi_rects_ref`, rounded and clamped to uint8; unused slots are zeros.  Returns
    (crops uint8 ``[B*k, Ho, Wo, 3]``, rois int32 ``[B*k, 4]``)."""
    B, H, W, _ = frames.shape
    rois = roi_rects_ref(det, count, k, (H, W), margin)
    crops = torch.zeros(B * k, size[0], size[1], 3, dtype=torch.uint8, device=frames.device)
    for slot, (X0, Y0, X1, Y1) in enumerate(rois.tolist()):
        if X1 <= X0:
            continue
        sub = frames[slot // k, Y0:Y1, X0:X1].permute(2, 0, 1)[None].float()
        out = F.interpolate(sub, size=tuple(size), mode="bilinear", align_corners=False)
        crops[slot] = out.round().clamp(0, 255)[0].permute(1, 2, 0).to(torch.uint8)
    return crops, rois


# ---- detection overlay ----------------------------------------------------------------------

def overlay_text_ref(c: int, p: torch.Tensor, names: torch.Tensor, show_score: bool) -> list[int]:
    """Character codes of one label: the bytes of ``names[c]`` up to the first zero (none if ``c``
    is outside the table), then — if ``show_score`` — a space (only after a name) and the two
    digits of ``min(max(rint(p * 100), 0), 99)``, the product in fp32, NaN counting as 0."""
    text = []
    if 0 <= c < names.shape[0]:
        for ch in names[c].tolist():
            if ch == 0:
                break
            text.append(ch)
    if show_score:
        v = torch.round(p.to(torch.float32) * 100.0)            # fp32 product, round half to even
        pct = 0 if bool(torch.isnan(v)) else int(min(max(float(v), 0.0), 99.0))
        text += ([32] if text else []) + [48 + pct // 10, 48 + pct % 10]
    return text


def draw_detections_ref(frames: torch.Tensor, det: torch.Tensor, count: torch.Tensor, k: int, names: torch.Tensor,
                        font: torch.Tensor, palette: torch.Tensor, *, labels: torch.Tensor | None = None,
                        scores: torch.Tensor | None = None, thickness: int = 2, text_scale: int = 1,
                        margin: float = 0.0, show_score: bool = True, glyph_width: int | None = None) -> torch.Tensor:
    """``ops.overlay.draw_detections`` with torch on the CPU, painter's style: per frame the used
    rows (rects of :func:`roi_rects_ref`) are painted from the highest index down to 0, each as
    four outline strips and then its label block, so the lowest index ends on top and a label
    covers its own outline.  Returns a new uint8 ``[B, H, W, 3]`` tensor."""
    frames, det, count = frames.cpu(), det.cpu().to(torch.float32), count.cpu()
    names, font, palette = names.cpu(), font.cpu(), palette.cpu()
    B, H, W, _ = frames.shape
    G, gh = font.shape
    gw = 6 if glyph_width is None else int(glyph_width)
    s, t = int(text_scale), int(thickness)
    cw, ch = gw * s, gh * s
    out = frames.clone()
    rects = roi_rects_ref(det, count, k, (H, W), margin).view(B, k, 4).tolist()
    # every glyph as a [ch, cw] mask: bit 7 of a row byte is the leftmost pixel
    shifts = 7 - torch.arange(gw)
    masks = ((font.to(torch.int64)[:, :, None] >> shifts[None, None, :]) & 1).bool()
    masks = masks.repeat_interleave(s, 1).repeat_interleave(s, 2)
    for b in range(B):
        for i in reversed(range(k)):
            X0, Y0, X1, Y1 = rects[b][i]
            if X1 <= X0:
                continue
            slot = b * k + i
            if labels is not None:
                c = int(labels[slot])
            else:
                cf = float(det[b, i, 5])
                c = 0 if cf != cf else int(min(max(cf, -2.0 ** 31), 2.0 ** 31 - 1))
            p = scores[slot].cpu() if scores is not None else det[b, i, 4]
            col = palette[c % palette.shape[0] if c >= 0 else 0]
            R, Gc, Bc = (int(v) for v in col)
            ink = 0 if 299 * R + 587 * Gc + 114 * Bc >= 128000 else 255
            frame = out[b]
            frame[Y0:min(Y0 + t, Y1), X0:X1] = col
            frame[max(Y1 - t, Y0):Y1, X0:X1] = col
            frame[Y0:Y1, X0:min(X0 + t, X1)] = col
            frame[Y0:Y1, max(X1 - t, X0):X1] = col
            text = overlay_text_ref(c, p, names, show_score)
            if not text:
                continue
            Lw, Lh = len(text) * cw + 2 * s, ch + 2 * s
            lx = max(min(X0, W - Lw), 0)
            ly = Y0 - Lh if Y0 - Lh >= 0 else Y0
            block = col.expand(Lh, Lw, 3).clone()
            for j, code in enumerate(text):
                if 32 <= code < 32 + G:
                    block[s:s + ch, s + j * cw:s + (j + 1) * cw][masks[code - 32]] = ink
            hh, ww = min(Lh, H - ly), min(Lw, W - lx)
            frame[ly:ly + hh, lx:lx + ww] = block[:hh, :ww]
    return out


# ---- detection redaction --------------------------------------------------------------------

def redact_detections_ref(frames: torch.Tensor, det: torch.Tensor, count: torch.Tensor, k: int, *,
                          mode: str = "pixelate", block: int = 16, fill=(0, 0, 0), margin: float = 0.0,
                          select: torch.Tensor | None = None, labels: torch.Tensor | None = None) -> torch.Tensor:
    """``ops.redact.redact_detections`` with torch on the CPU, from the rule in that module's
    docstring: per frame a boolean coverage mask, the union of the rects (:func:`roi_rects_ref`) of
    the used and selected rows, and — for ``pixelate`` — the frame's ``block`` x ``block`` cell
    means ``(2*S + n) // (2*n)`` in int64, spread back over their cells.  Returns a new uint8
    ``[B, H, W, 3]`` tensor."""
    if mode not in ("pixelate", "fill"):
        raise ValueError(f"redact_detections_ref: unknown mode {mode!r}")
    if int(block) not in (4, 8, 16, 32):
        raise ValueError(f"redact_detections_ref: block in {{4, 8, 16, 32}} required, got {block}")
    frames, det, count = frames.cpu(), det.cpu().to(torch.float32), count.cpu()
    B, H, W, _ = frames.shape
    bs = int(block)
    rects = roi_rects_ref(det, count, k, (H, W), margin).view(B, k, 4).tolist()
    out = frames.clone()
    for b in range(B):
        covered = torch.zeros(H, W, dtype=torch.bool)
        for i in range(k):
            X0, Y0, X1, Y1 = rects[b][i]
            if X1 <= X0:
                continue
            if select is not None:
                if labels is not None:
                    c = int(labels[b * k + i])
                else:
                    cf = float(det[b, i, 5])
                    c = 0 if cf != cf else int(min(max(cf, -2.0 ** 31), 2.0 ** 31 - 1))
                if not (0 <= c < select.shape[0] and int(select[c]) != 0):
                    continue
            covered[Y0:Y1, X0:X1] = True
        if not bool(covered.any()):
            continue
        if mode == "fill":
            colour = torch.tensor([int(c) for c in fill], dtype=torch.uint8).expand(H, W, 3)
        else:
            ch, cw = -(-H // bs), -(-W // bs)
            padded = torch.zeros(ch * bs, cw * bs, 3, dtype=torch.int64)
            padded[:H, :W] = frames[b].to(torch.int64)
            S = padded.view(ch, bs, cw, bs, 3).sum((1, 3))                      # [ch, cw, 3]
            ny = (H - torch.arange(ch) * bs).clamp(max=bs)                     # in-frame rows / columns
            nx = (W - torch.arange(cw) * bs).clamp(max=bs)
            n = (ny[:, None] * nx[None, :])[..., None]
            mean = (2 * S + n) // (2 * n)
            colour = mean.repeat_interleave(bs, 0).repeat_interleave(bs, 1)[:H, :W].to(torch.uint8)
        out[b][covered] = colour[covered]
    return out


# ---- YUV ingest -----------------------------------------------------------------------------

def yuv_planes_ref(raw: torch.Tensor, height: int, width: int, fmt: str):
    """(Y, U, V) uint8 ``[B, H, W]`` of tightly packed raw frames ``[B, frame_bytes]``, the chroma
    replicated to every pixel it serves (nearest: no interpolation)."""
    from .yuv import frame_bytes
    H, W = int(height), int(width)
    raw = raw.cpu()
    if raw.dim() != 2 or raw.dtype != torch.uint8 or raw.shape[1] != frame_bytes(fmt, H, W):
        raise ValueError(f"yuv_planes_ref: uint8 [B, {frame_bytes(fmt, H, W)}] required, got {tuple(raw.shape)}")
    B = raw.shape[0]
    cw, ch = (W + 1) // 2, (H + 1) // 2
    if fmt == "yuyv":
        a = raw.view(B, H, W // 2, 4)
        y = torch.stack([a[..., 0], a[..., 2]], -1).reshape(B, H, W)
        return y, a[..., 1].repeat_interleave(2, 2), a[..., 3].repeat_interleave(2, 2)
    y = raw[:, :H * W].view(B, H, W)
    if fmt == "i444":
        return y, raw[:, H * W:2 * H * W].view(B, H, W), raw[:, 2 * H * W:].view(B, H, W)
    if fmt == "nv12":
        c = raw[:, H * W:].view(B, ch, cw, 2)
        u, v = c[..., 0], c[..., 1]
    else:
        u = raw[:, H * W:H * W + ch * cw].view(B, ch, cw)
        v = raw[:, H * W + ch * cw:].view(B, ch, cw)
    up = lambda p: p.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]  # noqa: E731
    return y, up(u), up(v)


def yuv_to_rgb_ref(raw: torch.Tensor, height: int, width: int, fmt: str, standard: str) -> torch.Tensor:
    """``ops.yuv.yuv_to_rgb`` with torch fp32 on the CPU, the formula of :mod:`~aiko_services_amd.ops.yuv`
    literally: one rounding per operation, the constants as fp32 tensors from the same
    ``STANDARDS`` row the kernel is given.  Returns uint8 ``[B, H, W, 3]``."""
    from .yuv import STANDARDS
    coeffs, rounding = STANDARDS[standard]
    yoff, ygain, rv, gu, gv, bu = (torch.tensor(c, dtype=torch.float32) for c in coeffs)
    Y, U, V = (p.to(torch.float32) for p in yuv_planes_ref(raw, height, width, fmt))
    c = (Y - yoff) * ygain
    u, v = U - 128.0, V - 128.0
    rgb = torch.stack([c + rv * v, (c - gu * u) - gv * v, c + bu * u], -1)
    if rounding == "rint":
        rgb = torch.round(rgb).clamp_(0, 255)               # ties to even
    else:
        rgb = (rgb + 0.5).clamp_(0, 255)                    # the cast truncates
    return rgb.to(torch.uint8)


# ---- YUV egress -----------------------------------------------------------------------------

def _chroma_mean_ref(rgb: torch.Tensor, by: int, bx: int) -> torch.Tensor:
    """fp32 ``[B, ceil(H/by), ceil(W/bx), 3]``: the mean RGB of each ``by`` x ``bx`` block's
    in-frame pixels (``by``, ``bx`` in {1, 2}): the integer sum of the bytes times 1/n."""
    B, H, W, _ = rgb.shape
    ph, pw = -(-H // by) * by, -(-W // bx) * bx
    s = torch.zeros(B, ph, pw, 3, dtype=torch.int32)
    s[:, :H, :W] = rgb.to(torch.int32)
    n = torch.zeros(ph, pw, dtype=torch.int32)
    n[:H, :W] = 1
    s = s.view(B, ph // by, by, pw // bx, bx, 3).sum((2, 4))
    n = n.view(ph // by, by, pw // bx, bx).sum((1, 3))
    inv = (1.0 / n.to(torch.float32))[None, :, :, None]                 # 1, 0.5 or 0.25: exact
    return s.to(torch.float32) * inv


def rgb_to_yuv_ref(rgb: torch.Tensor, fmt: str, standard: str) -> torch.Tensor:
    """``ops.yuv.rgb_to_yuv`` with torch fp32 on the CPU, the formula of :mod:`~aiko_services_amd.ops.yuv`
    literally: one rounding per operation, the constants as fp32 tensors from the same
    ``ENCODE_STANDARDS`` row the kernel is given.  uint8 ``[B, H, W, 3]`` -> uint8 ``[B, frame_bytes]``."""
    from .yuv import ENCODE_STANDARDS, FORMATS, frame_bytes
    if fmt not in FORMATS:
        raise ValueError(f"rgb_to_yuv_ref: unknown format {fmt!r}")
    coeffs, rounding = ENCODE_STANDARDS[standard]
    yoff, yr, yg, yb, ur, ug, ub, vr, vg, vb = (torch.tensor(c, dtype=torch.float32) for c in coeffs)
    rgb = rgb.cpu()
    if rgb.dim() != 4 or rgb.dtype != torch.uint8 or rgb.shape[3] != 3:
        raise ValueError(f"rgb_to_yuv_ref: uint8 [B, H, W, 3] required, got {tuple(rgb.shape)}")
    B, H, W, _ = rgb.shape
    nbytes = frame_bytes(fmt, H, W)                                     # yuyv with an odd width: ValueError

    def level(x):
        if rounding == "rint":
            return torch.round(x).clamp_(0, 255).to(torch.uint8)        # ties to even
        return (x + 0.5).clamp_(0, 255).to(torch.uint8)                 # the cast truncates

    f = rgb.to(torch.float32)
    y = level(((yr * f[..., 0] + yg * f[..., 1]) + yb * f[..., 2]) + yoff)
    by, bx = {"nv12": (2, 2), "i420": (2, 2), "yuyv": (1, 2), "i444": (1, 1)}[fmt]
    m = f if fmt == "i444" else _chroma_mean_ref(rgb, by, bx)
    u = level(((ur * m[..., 0] + ug * m[..., 1]) + ub * m[..., 2]) + 128.0)
    v = level(((vr * m[..., 0] + vg * m[..., 1]) + vb * m[..., 2]) + 128.0)
    if fmt == "yuyv":
        out = torch.stack([y[..., 0::2], u, y[..., 1::2], v], -1).reshape(B, -1)
    elif fmt == "nv12":
        out = torch.cat([y.reshape(B, -1), torch.stack([u, v], -1).reshape(B, -1)], 1)
    else:
        out = torch.cat([y.reshape(B, -1), u.reshape(B, -1), v.reshape(B, -1)], 1)
    assert out.shape[1] == nbytes
    return out.contiguous()


def resample_ref(pcm: torch.Tensor, hist: torch.Tensor, filt: torch.Tensor, L: int, M: int):
    """The definition of :func:`aiko_services_amd.ops.audio.resample` on the CPU: ``(out,
    hist_out)`` for ``pcm`` ``[B, n_in, C]`` (int16 or fp32), ``hist`` fp32 ``[B, T-1]`` and ``filt``
    fp32 ``[L, T]``.  Every step is one fp32 operation on whole tensors — a multiply, then an add,
    per tap — so nothing is fused or reordered; the kernel must match it bit for bit."""
    pcm, hist, filt = pcm.detach().cpu(), hist.detach().cpu().float(), filt.detach().cpu().float()
    L, M = int(L), int(M)
    B, n_in, C = pcm.shape
    T = filt.shape[1]
    if filt.shape[0] != L or hist.shape != (B, T - 1):
        raise ValueError(f"resample_ref: filt [L, T] and hist [B, T-1] required, got {tuple(filt.shape)}, "
                         f"{tuple(hist.shape)}")
    if (n_in * L) % M:
        raise ValueError(f"resample_ref: n_in*L % M != 0 for n_in = {n_in}, L / M = {L} / {M}")
    if pcm.dtype == torch.int16:
        scale = torch.tensor(1.0 / (32768.0 * C), dtype=torch.float64).float()
        mono = pcm.to(torch.int32).sum(dim=2, dtype=torch.int32).float() * scale
    elif pcm.dtype == torch.float32:
        scale = torch.tensor(1.0 / C, dtype=torch.float64).float()
        mono = pcm[:, :, 0]
        for c in range(1, C):
            mono = mono + pcm[:, :, c]
        mono = mono * scale
    else:
        raise ValueError(f"resample_ref: int16 or fp32 pcm required, got {pcm.dtype}")
    s = torch.cat([hist, mono], dim=1)
    n_out = n_in * L // M
    jm = torch.arange(n_out, dtype=torch.int64) * M
    i0, p = jm // L, jm % L
    acc = torch.zeros(B, n_out, dtype=torch.float32)
    for k in range(T):
        prod = filt[p, k][None, :] * s[:, i0 + k]
        acc = acc + prod
    return acc, s[:, n_in:n_in + T - 1].clone()


# ---- tracker --------------------------------------------------------------------------------

def _wrap_i32(v: int) -> int:
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def track_ref(det: torch.Tensor, count: torch.Tensor, state, k: int, *, iou: float = 0.3, max_age: int = 30,
              min_score: float = 0.0, class_aware: bool = True, label_mod: int = 1000):
    """The definition of :func:`aiko_services_amd.ops.track.track_detections` on the CPU, in plain
    loops: ``(ids, hits, labels, state_out)`` for ``det`` ``[B, max_det, 6]``, ``count`` ``[B]`` and a
    ``TrackState``.  The pair geometry is numpy fp32, one rounding per operation; the threshold
    test and the order of two pairs are products of those fp32 values as Python floats (doubles),
    which are exact.  The integer fields wrap like int32.  ``state`` is not modified."""
    import functools

    import numpy as np

    from .track import TrackState
    det = det.detach().cpu().to(torch.float32).numpy()
    count = count.detach().cpu().numpy()
    boxes = state.boxes.detach().cpu().to(torch.float32).numpy().copy()
    meta = state.meta.detach().cpu().numpy().astype(np.int64)
    issued = state.issued.detach().cpu().numpy().astype(np.int64)
    B, T = boxes.shape[:2]
    k = int(k)
    thr, floor = float(np.float32(iou)), np.float32(min_score)
    ids = np.zeros((B, k), np.int64)
    hits = np.zeros((B, k), np.int64)
    labels = np.full((B, k), -1, np.int64)

    def before(p, q):                                   # order of two pairs (t, d, inter, union)
        lhs, rhs = p[2] * q[3], q[2] * p[3]
        if lhs != rhs:
            return -1 if lhs > rhs else 1
        return -1 if p[:2] < q[:2] else 1

    for b in range(B):
        n = min(max(int(count[b]), 0), k)
        rows = det[b, :n]                               # rows at or past count[b] are never read
        valid = [i for i in range(n) if np.isfinite(rows[i, :4]).all()]
        cls = [0 if c != c else int(min(max(float(c), -2.0 ** 31), 2.0 ** 31 - 1)) for c in rows[:, 5]]
        live = [t for t in range(T) if meta[b, t, 0] != 0]
        with np.errstate(all="ignore"):                 # a garbage state may hold inf and NaN
            a, d = boxes[b][:, None, :], rows[None, :, :4]
            aw, ah = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1]
            area_a = aw * ah
            bw, bh = d[..., 2] - d[..., 0], d[..., 3] - d[..., 1]
            area_b = bw * bh
            zero = np.float32(0)
            iw = np.maximum(np.minimum(a[..., 2], d[..., 2]) - np.maximum(a[..., 0], d[..., 0]), zero)
            ih = np.maximum(np.minimum(a[..., 3], d[..., 3]) - np.maximum(a[..., 1], d[..., 1]), zero)
            inter = iw * ih
            union = (area_a + area_b) - inter
        assert inter.dtype == np.float32 and union.dtype == np.float32
        pairs = []
        for t in live:
            for i in valid:
                if class_aware and cls[i] != meta[b, t, 1]:
                    continue
                it, un = float(inter[t, i]), float(union[t, i])
                if it > 0 and un > 0 and it >= thr * un:
                    pairs.append((t, i, it, un))
        pairs.sort(key=functools.cmp_to_key(before))
        of_track, of_det = {}, {}
        for t, i, _, _ in pairs:
            if t not in of_track and i not in of_det:
                of_track[t], of_det[i] = i, t
        for t in live:
            if t in of_track:
                i = of_track[t]
                boxes[b, t] = rows[i, :4]
                if not class_aware:
                    meta[b, t, 1] = cls[i]
                meta[b, t, 2] = _wrap_i32(meta[b, t, 2] + 1)
                meta[b, t, 3] = 0
            else:
                meta[b, t, 3] = _wrap_i32(meta[b, t, 3] + 1)
                if meta[b, t, 3] > int(max_age):
                    meta[b, t] = 0
        for t in range(T):                              # a free slot is all zeros
            if meta[b, t, 0] == 0:
                meta[b, t] = 0
                boxes[b, t] = 0
        for i in valid:
            if i in of_det or not rows[i, 4] >= floor:
                continue
            free = [t for t in range(T) if meta[b, t, 0] == 0]
            if not free:
                break
            t = free[0]
            issued[b] = _wrap_i32(issued[b] + 1)
            boxes[b, t] = rows[i, :4]
            meta[b, t] = (issued[b], cls[i], 1, 0)
            of_det[i] = t
        for i, t in of_det.items():
            ids[b, i], hits[b, i] = meta[b, t, 0], meta[b, t, 2]
            if ids[b, i] > 0:
                labels[b, i] = ids[b, i] % int(label_mod)
    out = [torch.from_numpy(x.astype(np.int32)).reshape(-1) for x in (ids, hits, labels)]
    return (*out, TrackState(torch.from_numpy(boxes), torch.from_numpy(meta.astype(np.int32)),
                             torch.from_numpy(issued.astype(np.int32))))


# ---- motion detection -----------------------------------------------------------------------

def motion_detect_ref(frames: torch.Tensor, state, *, cell: int = 16, threshold: int = 12, learn_shift: int = 4,
                      learn_moving: bool = True, warmup: int = 1, min_cells: int = 2, max_det: int = 16):
    """The definition of :func:`aiko_services_amd.ops.motion.motion_detect` on the CPU, in plain
    loops over cells: ``(det, count, mask, cells, state_out)`` for uint8 ``frames`` ``[B, H, W, 3]``
    and a ``MotionState``.  Integers are Python ints (the per-pixel luma and a cell's sum are numpy
    int64), the components come from a breadth-first walk, the score is a Python float division
    (fp64) rounded to fp32 once.  ``state`` is not modified."""
    from collections import deque

    import numpy as np

    from .motion import MotionState, check_parameters, grid_shape
    check_parameters(cell, threshold, learn_shift, warmup, min_cells, max_det)
    f = frames.detach().cpu().numpy().astype(np.int64)
    B, H, W, _ = f.shape
    gh, gw = grid_shape(H, W, cell)
    bg = state.bg.detach().cpu().numpy().astype(np.int64)
    seen = state.seen.detach().cpu().numpy().astype(np.int64)
    luma = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8
    half = (1 << (learn_shift - 1)) if learn_shift else 0
    bg_out = np.zeros((B, gh, gw), np.int64)
    seen_out = np.zeros(B, np.int64)
    mask = np.zeros((B, gh, gw), np.uint8)
    det = np.zeros((B, max_det, 6), np.float32)
    count = np.zeros(B, np.int32)
    cells = np.zeros(B, np.int32)
    for b in range(B):
        s = max(int(seen[b]), 0)
        for gy in range(gh):
            for gx in range(gw):
                block = luma[b, gy * cell:min((gy + 1) * cell, H), gx * cell:min((gx + 1) * cell, W)]
                S, n = int(block.sum()), block.size
                cur = (32 * S + n) // (2 * n)
                old = int(bg[b, gy, gx])
                moving = s >= warmup and abs(cur - old) > 16 * threshold
                if s == 0:
                    new = cur
                elif moving and not learn_moving:
                    new = old
                else:
                    new = old + ((cur - old + half) >> learn_shift)      # Python's >> floors
                bg_out[b, gy, gx] = new
                mask[b, gy, gx] = 1 if moving else 0
        seen_out[b] = min(s + 1, 2 ** 31 - 1)
        cells[b] = int(mask[b].sum())
        # components in raster order of their first cell: that cell's index is the label
        done = np.zeros((gh, gw), bool)
        found = []                                              # (area, label, cx0, cy0, cx1, cy1)
        for gy in range(gh):
            for gx in range(gw):
                if not mask[b, gy, gx] or done[gy, gx]:
                    continue
                done[gy, gx] = True
                todo, area, box = deque([(gy, gx)]), 0, [gx, gy, gx, gy]
                while todo:
                    y, x = todo.popleft()
                    area += 1
                    box = [min(box[0], x), min(box[1], y), max(box[2], x), max(box[3], y)]
                    for ny in range(max(y - 1, 0), min(y + 2, gh)):
                        for nx in range(max(x - 1, 0), min(x + 2, gw)):
                            if mask[b, ny, nx] and not done[ny, nx]:
                                done[ny, nx] = True
                                todo.append((ny, nx))
                if area >= min_cells:
                    found.append((area, gy * gw + gx, *box))
        found.sort(key=lambda c: (-c[0], c[1]))
        for i, (area, _, cx0, cy0, cx1, cy1) in enumerate(found[:max_det]):
            score = np.float32(area / ((cx1 - cx0 + 1) * (cy1 - cy0 + 1)))
            det[b, i] = (cx0 * cell, cy0 * cell, min((cx1 + 1) * cell, W), min((cy1 + 1) * cell, H), score, 0)
        count[b] = min(len(found), max_det)
    return (torch.from_numpy(det), torch.from_numpy(count), torch.from_numpy(mask), torch.from_numpy(cells),
            MotionState(torch.from_numpy(bg_out.astype(np.int32)), torch.from_numpy(seen_out.astype(np.int32))))


# ---- voice activity ---------------------------------------------------------------------------

def vad_level_ref(E: int) -> int:
    """Step 3 of the rule of ``ops/vad.py``: the level of a frame of energy ``E`` (a Python int)."""
    if E == 0:
        return 0
    p = E.bit_length() - 1
    mant = ((E >> (p - 4)) if p >= 4 else (E << (4 - p))) & 15
    return 16 * (p + 1) + mant


def voice_activity_ref(audio: torch.Tensor, state, *, frame: int = 320, threshold: int = 48, min_level: int = 0,
                       up_shift: int = 6, speech_shift: int = 10, down_shift: int = 1, warmup: int = 10,
                       attack: int = 3, hang: int = 15, max_zc: int = 479, window: int = 1500, max_seg: int = 16):
    """The definition of :func:`aiko_services_amd.ops.vad.voice_activity` on the CPU, in plain loops
    over frames: ``(mask, seg, count, speech, silent, level, zc, state_out)`` for fp32 ``audio`` ``[B,
    n]`` and a ``VadState``.  The samples are scaled in numpy fp32 and rounded by ``np.rint`` (half to
    even); a frame's two sums are numpy int64, everything after them a Python int.  ``state`` is not
    modified."""
    import numpy as np

    from .vad import MAX_FRAMES, VadState, check_parameters
    check_parameters(frame, threshold, min_level, up_shift, speech_shift, down_shift, warmup, attack, hang, max_zc,
                     window, max_seg)
    x = audio.detach().cpu().numpy()
    if x.dtype != np.float32 or x.ndim != 2 or x.shape[0] < 1:
        raise ValueError(f"voice_activity_ref: audio fp32 [B, n] required, got {x.dtype} {x.shape}")
    B, n = x.shape
    if n == 0 or n % frame or n // frame > MAX_FRAMES:
        raise ValueError(f"voice_activity_ref: n = {n} is not 1..{MAX_FRAMES} whole frames of {frame}")
    F = n // frame
    with np.errstate(over="ignore", invalid="ignore"):
        v = x * np.float32(32768.0)
        q = np.where(np.isnan(v), np.float32(0), np.rint(np.clip(v, np.float32(-32768), np.float32(32767))))
    q = q.astype(np.int64).reshape(B, F, frame)
    st = state.v.detach().cpu().numpy().astype(np.int64)
    cap = 2 ** 30
    level = np.zeros((B, F), np.int32)
    zc = np.zeros((B, F), np.int32)
    mask = np.zeros((B, F), np.uint8)
    seg = np.zeros((B, max_seg, 2), np.int32)
    count = np.zeros(B, np.int32)
    speech = np.zeros(B, np.int32)
    silent = np.zeros(B, np.int32)
    out = np.zeros((B, 8), np.int32)
    for b in range(B):
        floor, seen, run, quiet, on, since = (int(c) for c in st[b, :6])
        s = max(seen, 0)
        if s == 0:
            run, quiet, on, since = 0, 0, 0, cap
        else:
            run, quiet, on, since = min(max(run, 0), cap), max(quiet, 0), int(on != 0), min(max(since, 0), cap)
        floor = min(max(floor, 0), 1023 << 8)
        runs = []
        for f in range(F):
            qf = q[b, f]
            E, z = int((qf * qf).sum()), int(((qf[1:] < 0) != (qf[:-1] < 0)).sum())
            lv = vad_level_ref(E)
            cur = lv << 8
            if s == 0:
                floor = cur
            raw = s >= warmup and lv >= min_level and cur - floor > (threshold << 8) and z <= max_zc
            if s > 0:
                k = down_shift if cur < floor else speech_shift if raw else up_shift
                floor += (cur - floor + ((1 << (k - 1)) if k else 0)) >> k      # Python's >> floors
            run = min(run + 1, cap) if raw else 0
            if not on:
                if run >= attack:
                    on, quiet = 1, 0
            else:
                quiet = 0 if raw else quiet + 1
                if quiet > hang:
                    on, quiet = 0, 0
            if on and (f == 0 or not mask[b, f - 1]):
                runs.append([f, f + 1])
            elif on:
                runs[-1][1] = f + 1
            level[b, f], zc[b, f], mask[b, f] = lv, z, on
            since = 0 if on else min(since + 1, cap)
            s = min(s + 1, 2 ** 31 - 1)
        for i, r in enumerate(runs[:max_seg]):
            seg[b, i] = r
        count[b] = min(len(runs), max_seg)
        speech[b] = int(mask[b].sum())
        silent[b] = 1 if since >= window else 0
        out[b] = (floor, s, run, quiet, on, since, 0, 0)
    return (torch.from_numpy(mask), torch.from_numpy(seg), torch.from_numpy(count), torch.from_numpy(speech),
            torch.from_numpy(silent), torch.from_numpy(level), torch.from_numpy(zc), VadState(torch.from_numpy(out)))


# ---- JPEG -------------------------------------------------------------------------------------

def _jpeg_planes_ref(frame: torch.Tensor, fmt: str, H: int, W: int):
    """The three component planes of one packed ``i420`` / ``i444`` frame, int64."""
    ch, cw = ((H + 1) // 2, (W + 1) // 2) if fmt == "i420" else (H, W)
    f = frame.to(torch.int64)
    return [f[:H * W].view(H, W), f[H * W:H * W + ch * cw].view(ch, cw), f[H * W + ch * cw:].view(ch, cw)]


def _jpeg_block_ref(plane: torch.Tensor, by: int, bx: int, M: torch.Tensor, q: torch.Tensor) -> list:
    """The quantised coefficients, natural order, of the 8 x 8 block at (``by``, ``bx``) of ``plane``:
    samples outside the plane are those at the clamped coordinates."""
    ys = torch.arange(by, by + 8).clamp_(max=plane.shape[0] - 1)
    xs = torch.arange(bx, bx + 8).clamp_(max=plane.shape[1] - 1)
    x = plane[ys][:, xs] - 128
    t = (M @ x + 1024) >> 11                                # columns; >> on int64 is arithmetic
    c = (t @ M.T + 16384) >> 15                             # rows
    v = torch.sign(c) * ((c.abs() + (q >> 1)) // q)
    return v.clamp_(-1023, 1023).flatten().tolist()


def jpeg_encode_ref(raw: torch.Tensor, height: int, width: int, fmt: str = "i420", quality: int = 90, *,
                    cap: int | None = None, seg_cap: int | None = None, trace: list | None = None):
    """``ops.jpeg.jpeg_encode`` on the CPU in plain loops, the rule of :mod:`~aiko_services_amd.ops.jpeg`
    literally: uint8 ``[B, frame_bytes]`` -> ``(stream uint8 [B, cap], nbytes int32 [B])``.  An
    overflowed frame has ``nbytes`` -1 and a row of zeros; the bytes past ``nbytes`` are zeros.
    ``trace`` (a list) receives every coded symbol as ``(frame, MCU row, block in the row, "dc" | "ac",
    symbol, value)``, ``value`` the DC difference or the coefficient (0 for ``ZRL`` and ``EOB``)."""
    from . import jpeg as J
    from .yuv import frame_bytes
    mh, mw, nblk, my, mx = J.geometry(fmt, height, width)
    H, W = int(height), int(width)
    raw = raw.cpu()
    if raw.dim() != 2 or raw.dtype != torch.uint8 or raw.shape[1] != frame_bytes(fmt, H, W):
        raise ValueError(f"jpeg_encode_ref: uint8 [B, {frame_bytes(fmt, H, W)}] required, got {tuple(raw.shape)}")
    head = J.header(fmt, H, W, quality)
    dcap, dseg = J.capacities(fmt, H, W)
    cap, seg_cap = dcap if cap is None else int(cap), dseg if seg_cap is None else int(seg_cap)
    M = torch.tensor(J.DCT_MATRIX, dtype=torch.int64)
    quant = [torch.tensor(t, dtype=torch.int64).view(8, 8) for t in J.quant_tables(quality)]
    dc_codes = [J.huffman_codes(0x00), J.huffman_codes(0x01)]
    ac_codes = [J.huffman_codes(0x10), J.huffman_codes(0x11)]
    # (component, block row, block column) of an MCU's blocks, in coding order
    layout = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (2, 0, 0)] if fmt == "i420" else \
        [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
    ysub = 2 if fmt == "i420" else 1                        # luma blocks per MCU side
    B = raw.shape[0]
    stream = torch.zeros(B, cap, dtype=torch.uint8)
    nbytes = torch.empty(B, dtype=torch.int32)
    for b in range(B):
        planes = _jpeg_planes_ref(raw[b], fmt, H, W)
        out, overflow = bytearray(head), False
        for row in range(my):
            acc, nacc, seg = 0, 0, bytearray()              # the bit buffer: nacc bits in acc

            def put(code: int, length: int):
                nonlocal acc, nacc
                acc, nacc = acc << length | code, nacc + length
                while nacc >= 8:
                    byte = acc >> (nacc - 8) & 0xFF
                    seg.append(byte)
                    if byte == 0xFF:
                        seg.append(0)
                    nacc -= 8
                acc &= (1 << nacc) - 1

            def put_value(v: int, size: int):
                if size:
                    put(v if v >= 0 else v + (1 << size) - 1, size)

            pred = [0, 0, 0]
            for m in range(mx):
                for k, (comp, sy, sx) in enumerate(layout):
                    sub = ysub if comp == 0 else 1
                    tq = 0 if comp == 0 else 1
                    v = _jpeg_block_ref(planes[comp], (row * sub + sy) * 8, (m * sub + sx) * 8, M, quant[tq])
                    z = [v[n] for n in J.ZIGZAG]
                    blk = m * nblk + k
                    diff, pred[comp] = z[0] - pred[comp], z[0]
                    size = abs(diff).bit_length()
                    put(*dc_codes[tq][size])
                    put_value(diff, size)
                    if trace is not None:
                        trace.append((b, row, blk, "dc", size, diff))
                    run = 0
                    for i in range(1, 64):
                        if z[i] == 0:
                            run += 1
                            continue
                        while run > 15:
                            put(*ac_codes[tq][0xF0])
                            run -= 16
                            if trace is not None:
                                trace.append((b, row, blk, "ac", 0xF0, 0))
                        size = abs(z[i]).bit_length()
                        put(*ac_codes[tq][run << 4 | size])
                        put_value(z[i], size)
                        if trace is not None:
                            trace.append((b, row, blk, "ac", run << 4 | size, z[i]))
                        run = 0
                    if run:                                 # coefficient 63 is zero
                        put(*ac_codes[tq][0x00])
                        if trace is not None:
                            trace.append((b, row, blk, "ac", 0x00, 0))
            if nacc:
                put((1 << (8 - nacc)) - 1, 8 - nacc)
            overflow = overflow or len(seg) > seg_cap
            out += seg
            out += bytes([0xFF, 0xD0 + row % 8]) if row < my - 1 else b"\xff\xd9"
        if overflow or len(out) > cap:
            nbytes[b] = -1
        else:
            nbytes[b] = len(out)
            stream[b, :len(out)] = torch.frombuffer(out, dtype=torch.uint8)
    return stream, nbytes


class _JpegError(Exception):
    """A status bit of ``ops.jpeg_decode``, raised where an interval stops."""


def _jpeg_interval_ref(d: bytes, start: int, end: int, tables, layout, mcus, coef) -> int:
    """The blocks of the MCUs ``mcus`` from ``d[start:end]`` into ``coef [blocks, 64]`` (zigzag order), bit by
    bit on demand; the interval's status bits.  ``tables[comp]``: ``(dc, ac)``, each ``(maxcode, valoff,
    symbols)``; ``layout``: the component of every block of an MCU."""
    pos, cur, left = start, 0, 0

    def bit() -> int:
        nonlocal pos, cur, left
        if not left:
            if pos >= end:
                raise _JpegError(4)
            cur = d[pos]
            if cur != 0xFF:
                pos += 1
            elif pos + 1 < end and d[pos + 1] == 0:
                pos += 2
            else:
                raise _JpegError(16)
            left = 8
        left -= 1
        return cur >> left & 1

    def symbol(table) -> int:
        maxcode, valoff, symbols = table
        code = 0
        for length in range(16):
            code = code << 1 | bit()
            if code <= maxcode[length]:
                return symbols[(code + valoff[length]) & 255]
        raise _JpegError(2)

    def value(size: int) -> int:
        v = 0
        for _ in range(size):
            v = v << 1 | bit()
        return v if v >= 1 << (size - 1) else v - (1 << size) + 1

    pred = [0, 0, 0]
    try:
        for mcu in mcus:
            for sub, comp in enumerate(layout):
                out = coef[mcu * len(layout) + sub]
                dc, ac = tables[comp]
                size = symbol(dc) & 15
                pred[comp] = min(max(pred[comp] + (value(size) if size else 0), -32768), 32767)
                out[0] = pred[comp]
                k = 1
                while k < 64:
                    rs = symbol(ac)
                    run, size = rs >> 4, rs & 15
                    if size == 0:
                        if run != 15:
                            break                           # EOB
                        if k + 16 > 64:
                            raise _JpegError(8)
                        k += 16
                        continue
                    k += run
                    if k > 63:
                        raise _JpegError(8)
                    out[k] = value(size)
                    k += 1
    except _JpegError as exc:
        return exc.args[0]
    return 0


def jpeg_decode_ref(data: torch.Tensor, nbytes: torch.Tensor, desc: torch.Tensor, height: int, width: int,
                    fmt: str = "i420", *, restart_interval: int | None = None, coefficients: list | None = None):
    """``ops.jpeg_decode.jpeg_decode`` on the CPU in plain loops, the rule of
    :mod:`~aiko_services_amd.ops.jpeg_decode` literally, from the same tensors: ``data`` uint8 ``[B, cap]``,
    ``nbytes`` int32 ``[B]``, ``desc`` uint8 ``[B | 1, PLAN_BYTES]`` -> ``(raw uint8 [B, frame_bytes], status
    int32 [B])``.  What the rule leaves unspecified is fixed here: a frame whose marker scan fails is all
    zero bytes, an interval that stops at an error leaves the rest of its coefficients zero.
    ``coefficients`` (a list) receives per frame the int16 ``[blocks, 64]`` coefficients in zigzag order."""
    import struct

    import numpy as np

    from . import jpeg as J
    from . import jpeg_decode as D
    from .yuv import frame_bytes
    mh, mw, per, my, mx = D.geometry(fmt, height, width)
    H, W = int(height), int(width)
    max_int = D.intervals(fmt, H, W, restart_interval)
    data, nbytes, desc = data.cpu(), nbytes.cpu(), desc.cpu()
    B, cap = data.shape
    if desc.dim() != 2 or desc.shape[0] not in (1, B) or desc.shape[1] != D.PLAN_BYTES:
        raise ValueError(f"jpeg_decode_ref: desc [{B} | 1, {D.PLAN_BYTES}] required, got {tuple(desc.shape)}")
    mcus = my * mx
    layout = {"i420": (0, 0, 0, 0, 1, 2), "yuyv": (0, 0, 1, 2), "i444": (0, 1, 2)}[fmt]
    # (block row, block column) of an MCU's blocks inside the MCU, and the component's blocks per MCU side
    place = {"i420": ((0, 0), (0, 1), (1, 0), (1, 1), (0, 0), (0, 0)), "yuyv": ((0, 0), (0, 1), (0, 0), (0, 0)),
             "i444": ((0, 0),) * 3}[fmt]
    span = {"i420": (2, 2), "yuyv": (1, 2), "i444": (1, 1)}[fmt]       # luma blocks per MCU: rows, columns
    M = np.array(J.DCT_MATRIX, dtype=np.int64)
    unzig = np.empty(64, dtype=np.int64)
    unzig[list(J.ZIGZAG)] = np.arange(64)                               # natural index -> zigzag position
    ch, cw = ((H + 1) // 2, (W + 1) // 2) if fmt == "i420" else ((H, W // 2) if fmt == "yuyv" else (H, W))
    raw = torch.zeros(B, frame_bytes(fmt, H, W), dtype=torch.uint8)
    status = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        plan = bytes(desc[b if desc.shape[0] > 1 else 0].tolist())
        scan, dri = struct.unpack_from("<ii", plan, 0)
        sel = plan[8:14]
        quant = [np.array(list(plan[16 + 64 * c:80 + 64 * c]), dtype=np.int64) for c in range(3)]
        huff = []
        for slot in range(4):
            at = 208 + 384 * slot
            huff.append((struct.unpack_from("<16i", plan, at), struct.unpack_from("<16i", plan, at + 64),
                         plan[at + 128:at + 384]))
        tables = [(huff[sel[c] & 1], huff[2 + (sel[3 + c] & 1)]) for c in range(3)]
        coef = np.zeros((mcus * per, 64), dtype=np.int64)
        n = int(nbytes[b])
        nint = -(-mcus // dri) if dri > 0 else 1
        if n < 1 or n > cap or scan < 2 or scan > n - 2 or dri < 0 or nint > max_int:
            st = 1
        else:
            d = bytes(data[b, :n].tolist())
            st = 0 if d[n - 2:] == b"\xff\xd9" else 1
            marks = [i for i in range(scan, n - 3) if d[i] == 0xFF and 0xD0 <= d[i + 1] <= 0xD7]
            if len(marks) != nint - 1 or any(d[i + 1] & 7 != k & 7 for k, i in enumerate(marks)):
                st = 1
            if st == 0:
                starts = [scan] + [i + 2 for i in marks]
                ends = marks + [n - 2]
                for i in range(nint):
                    span_mcus = range(i * dri, min((i + 1) * dri, mcus)) if dri > 0 else range(mcus)
                    st |= _jpeg_interval_ref(d, starts[i], ends[i], tables, layout, span_mcus, coef)
        status[b] = st
        if coefficients is not None:
            coefficients.append(torch.from_numpy(coef.astype(np.int16)))
        if st & 1:
            continue
        planes = [np.zeros((H, W), np.uint8), np.zeros((ch, cw), np.uint8), np.zeros((ch, cw), np.uint8)]
        for k in range(mcus * per):
            mcu, sub = divmod(k, per)
            comp = layout[sub]
            rows, cols = span if comp == 0 else (1, 1)
            by = (mcu // mx) * rows + place[sub][0]
            bx = (mcu % mx) * cols + place[sub][1]
            c = np.clip(coef[k][unzig] * quant[comp], -2048, 2047).reshape(8, 8)
            t = (M.T @ c + 1024) >> 11                      # columns; >> on int64 is arithmetic
            x = (t @ M + 16384) >> 15                       # rows
            s = np.clip(x + 128, 0, 255).astype(np.uint8)
            plane = planes[comp]
            hh, ww = min(8, plane.shape[0] - 8 * by), min(8, plane.shape[1] - 8 * bx)
            if hh > 0 and ww > 0:
                plane[8 * by:8 * by + hh, 8 * bx:8 * bx + ww] = s[:hh, :ww]
        if fmt == "yuyv":
            packed = np.empty((H, W // 2, 4), np.uint8)
            packed[:, :, 0], packed[:, :, 2] = planes[0][:, 0::2], planes[0][:, 1::2]
            packed[:, :, 1], packed[:, :, 3] = planes[1], planes[2]
            raw[b] = torch.from_numpy(packed.reshape(-1))
        else:
            raw[b] = torch.from_numpy(np.concatenate([p.reshape(-1) for p in planes]))
    return raw, status


# ---- square markers ---------------------------------------------------------------------------

def marker_quad_ref(points) -> list:
    """Rule 6 of ``ops/marker.py``: the quad ``[(x, y)] * 4`` of the dark pixels ``points`` [(x, y),
    ...] (at least one), in Python ints."""
    def extreme(primary):
        return min(points, key=lambda p: (-primary(p), p[1], p[0]))

    def area2(q):
        return abs(sum(q[i][0] * q[(i + 1) % 4][1] - q[(i + 1) % 4][0] * q[i][1] for i in range(4)))

    diagonal = [extreme(lambda p: -(p[0] + p[1])), extreme(lambda p: p[0] - p[1]),
                extreme(lambda p: p[0] + p[1]), extreme(lambda p: -(p[0] - p[1]))]
    axial = [extreme(lambda p: -p[1]), extreme(lambda p: p[0]), extreme(lambda p: p[1]), extreme(lambda p: -p[0])]
    return diagonal if area2(diagonal) >= area2(axial) else axial


def marker_samples_ref(quad, N: int, H: int, W: int):
    """Rule 7 of ``ops/marker.py``: the sample pixel ``(px, py)`` of every module, ``[N][N]`` by row
    and column, of the quad ``[(x, y)] * 4`` in an ``H`` x ``W`` frame, or None if the map is
    degenerate.  Python ints: exact."""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = [(int(x), int(y)) for x, y in quad]
    dx1, dx2, sx = x1 - x2, x3 - x2, x0 - x1 + x2 - x3
    dy1, dy2, sy = y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    den = dx1 * dy2 - dy1 * dx2
    if den == 0:
        return None
    G, Hh = sx * dy2 - sy * dx2, dx1 * sy - dy1 * sx
    A, Bx = den * (x1 - x0) + G * x1, den * (x3 - x0) + Hh * x3
    D, E = den * (y1 - y0) + G * y1, den * (y3 - y0) + Hh * y3
    out = []
    for i in range(N):
        row = []
        for j in range(N):
            a, b = 2 * j + 1, 2 * i + 1
            dd = G * a + Hh * b + 2 * N * den
            nx = A * a + Bx * b + 2 * N * den * x0
            ny = D * a + E * b + 2 * N * den * y0
            if dd == 0:
                return None
            if dd < 0:
                dd, nx, ny = -dd, -nx, -ny
            px, py = (2 * nx + dd) // (2 * dd), (2 * ny + dd) // (2 * dd)      # Python's // floors
            row.append((min(max(px, 0), W - 1), min(max(py, 0), H - 1)))
        out.append(row)
    return out


def detect_markers_ref(frames: torch.Tensor, *, dictionary: str = "original", cell: int = 4, contrast: int = 64,
                       min_side: int = 24, max_cand: int = 32, max_det: int = 16):
    """The definition of :func:`aiko_services_amd.ops.marker.detect_markers` on the CPU, in plain
    loops over blocks, cells and candidates: ``(det, count, corners, ids, cands, mask)`` for uint8
    ``frames`` ``[B, H, W, 3]``.  Integers are Python ints (the per-pixel luma is numpy int64), the
    components come from a breadth-first walk in raster order, the score is a Python float division
    (fp64) rounded to fp32 once."""
    from collections import deque

    import numpy as np

    from ..examples.aruco_marker.aruco import _code, decode_original
    from .marker import BLOCK, DICTIONARIES, MAX_GRID, MAX_SIDE, check_parameters, grid_shape
    check_parameters(dictionary, cell, contrast, min_side, max_cand, max_det)
    f = frames.detach().cpu().numpy().astype(np.int64)
    B, H, W, _ = f.shape
    gh, gw = grid_shape(H, W, cell)
    if H > MAX_SIDE or W > MAX_SIDE or (gh + 2) * (gw + 2) > MAX_GRID:
        raise ValueError(f"detect_markers_ref: {H} x {W} at cell {cell} exceeds the limits")
    N = DICTIONARIES[dictionary]
    luma = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8
    rh, rw = -(-H // BLOCK), -(-W // BLOCK)
    det = np.zeros((B, max_det, 6), np.float32)
    corners = np.zeros((B, max_det, 4, 2), np.int32)
    ids = np.full((B, max_det), -1, np.int32)
    count = np.zeros(B, np.int32)
    cands = np.zeros(B, np.int32)
    mask = np.zeros((B, gh, gw), np.uint8)
    for b in range(B):
        Y = luma[b]
        lo, hi = np.zeros((rh, rw), np.int64), np.zeros((rh, rw), np.int64)
        for ry in range(rh):
            for rx in range(rw):
                block = Y[ry * BLOCK:(ry + 1) * BLOCK, rx * BLOCK:(rx + 1) * BLOCK]
                lo[ry, rx], hi[ry, rx] = block.min(), block.max()
        dark = np.zeros((H, W), bool)
        for ry in range(rh):
            for rx in range(rw):
                near = (slice(max(ry - 1, 0), min(ry + 2, rh)), slice(max(rx - 1, 0), min(rx + 2, rw)))
                m, M = int(lo[near].min()), int(hi[near].max())
                if M - m >= contrast:
                    block = (slice(ry * BLOCK, (ry + 1) * BLOCK), slice(rx * BLOCK, (rx + 1) * BLOCK))
                    dark[block] = 2 * Y[block] < m + M
        for gy in range(gh):
            for gx in range(gw):
                mask[b, gy, gx] = dark[gy * cell:(gy + 1) * cell, gx * cell:(gx + 1) * cell].any()
        # components in raster order of their first cell: that cell's index is the label
        label = np.full((gh, gw), -1, np.int64)
        found = []                                              # (label, cx0, cy0, cx1, cy1), ascending
        for gy in range(gh):
            for gx in range(gw):
                if not mask[b, gy, gx] or label[gy, gx] >= 0:
                    continue
                own = gy * gw + gx
                label[gy, gx] = own
                todo, box = deque([(gy, gx)]), [gx, gy, gx, gy]
                while todo:
                    y, x = todo.popleft()
                    box = [min(box[0], x), min(box[1], y), max(box[2], x), max(box[3], y)]
                    for ny in range(max(y - 1, 0), min(y + 2, gh)):
                        for nx in range(max(x - 1, 0), min(x + 2, gw)):
                            if mask[b, ny, nx] and label[ny, nx] < 0:
                                label[ny, nx] = own
                                todo.append((ny, nx))
                found.append((own, *box))
        accepted = []
        for own, cx0, cy0, cx1, cy1 in found:
            x0, y0, x1, y1 = cx0 * cell, cy0 * cell, min((cx1 + 1) * cell, W), min((cy1 + 1) * cell, H)
            if min(x1 - x0, y1 - y0) < min_side:
                continue
            cands[b] += 1
            if cands[b] > max_cand:
                continue
            points = [(x, y) for y in range(y0, y1) for x in range(x0, x1)
                      if dark[y, x] and label[y // cell, x // cell] == own]
            quad = marker_quad_ref(points)
            samples = marker_samples_ref(quad, N, H, W)
            if samples is None:
                continue
            level = [[int(Y[py, px]) for px, py in row] for row in samples]
            lo_s, hi_s = min(min(row) for row in level), max(max(row) for row in level)
            if hi_s - lo_s < contrast:
                continue
            white = np.array([[1 if 2 * v >= lo_s + hi_s else 0 for v in row] for row in level], np.uint8)
            if white[0].any() or white[-1].any() or white[:, 0].any() or white[:, -1].any():
                continue
            rots = [np.rot90(white[1:-1, 1:-1], -r) for r in range(4)]
            if dictionary == "original":
                decoded = [decode_original(r) for r in rots]
                hits = [r for r in range(4) if decoded[r] is not None]
                if not hits:
                    continue
                r, marker_id = hits[0], decoded[hits[0]]
            else:
                codes = [_code(r) for r in rots]
                marker_id = min(codes)
                r = codes.index(marker_id)
            accepted.append(([quad[(i + (4 - r) % 4) % 4] for i in range(4)], marker_id, hi_s - lo_s))
        for i, (quad, marker_id, spread) in enumerate(accepted[:max_det]):
            xs, ys = [p[0] for p in quad], [p[1] for p in quad]
            corners[b, i] = quad
            ids[b, i] = marker_id
            det[b, i] = (min(xs), min(ys), max(xs) + 1, max(ys) + 1, np.float32(spread / 255.0), marker_id)
        count[b] = min(len(accepted), max_det)
    return tuple(torch.from_numpy(a) for a in (det, count, corners, ids, cands, mask))


# ---- spectrum ---------------------------------------------------------------------------------

def spectrum_power_ref(audio, n_fft: int, hop: int, window):
    """Steps 1 to 4 of :func:`aiko_services_amd.ops.spectrum.spectrum` in numpy: fp32 ``[B, n]`` and the
    fp32 window -> ``(v, power)``, the windowed frames fp32 ``[B, F, n_fft]`` and their power fp32 ``[B,
    F, K]``.  Every operation is an element-wise fp32 numpy operation in the stated order."""
    import numpy as np

    from .spectrum import frame_count, twiddle
    x = np.ascontiguousarray(audio.detach().cpu().numpy() if isinstance(audio, torch.Tensor) else audio, np.float32)
    B, n = x.shape
    N, K = int(n_fft), int(n_fft) // 2 + 1
    F = frame_count(n, N, hop)
    x = np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float32)
    x = np.minimum(np.maximum(x, np.float32(-32768.0)), np.float32(32767.0))
    if n < N:
        x = np.concatenate([x, np.zeros((B, N - n), np.float32)], axis=1)
    idx = np.arange(F)[:, None] * hop + np.arange(N)[None, :]
    v = x[:, idx] * np.asarray(window, np.float32)[None, None, :]            # [B, F, N]
    bits = N.bit_length() - 1
    rev = np.zeros(N, np.int64)
    for i in range(bits):
        rev |= ((np.arange(N) >> i) & 1) << (bits - 1 - i)
    re, im = v[..., rev].copy(), np.zeros_like(v)
    tw = twiddle(N)
    for s in range(1, bits + 1):
        m, h = 1 << s, 1 << (s - 1)
        c, d = tw[np.arange(h) * (N // m), 0], tw[np.arange(h) * (N // m), 1]
        re, im = re.reshape(B, F, N // m, m), im.reshape(B, F, N // m, m)
        a_re, a_im, b_re, b_im = re[..., :h], im[..., :h], re[..., h:], im[..., h:]
        t_re = b_re * c - b_im * d
        t_im = b_re * d + b_im * c
        re = np.concatenate([a_re + t_re, a_re - t_re], axis=-1).reshape(B, F, N)
        im = np.concatenate([a_im + t_im, a_im - t_im], axis=-1).reshape(B, F, N)
    assert re.dtype == np.float32 and im.dtype == np.float32
    power = re[..., :K] * re[..., :K] + im[..., :K] * im[..., :K]
    return v, power


def spectrum_ref(audio, *, sample_rate=16000, n_fft: int = 1024, hop=None, window: str = "hann", band_count: int = 8,
                 frequency_band_maximum=8000.0, amplitude_minimum=0.1, amplitude_maximum=12.0, frequency_minimum=10.0,
                 frequency_maximum=9000.0, max_peaks: int = 100, local: bool = False):
    """The definition of :func:`aiko_services_amd.ops.spectrum.spectrum` in numpy, steps 1 to 7:
    ``(amplitudes, band_amplitudes, peak_bins, peak_amplitudes, peak_counts, power)`` as CPU tensors.
    The tables are those of ``ops.spectrum.tables``, the ones the kernels are given."""
    import numpy as np

    from .spectrum import MAX_FRAMES, check_parameters, frame_count, tables
    check_parameters(sample_rate, n_fft, hop, window, band_count, frequency_band_maximum, amplitude_minimum,
                     amplitude_maximum, frequency_minimum, frequency_maximum, max_peaks, local)
    hop = n_fft // 2 if hop is None else int(hop)
    t = tables(float(sample_rate), int(n_fft), window, int(band_count), float(frequency_band_maximum),
               float(amplitude_minimum), float(amplitude_maximum), float(frequency_minimum), float(frequency_maximum))
    B, n = audio.shape
    F, K = frame_count(n, n_fft, hop), n_fft // 2 + 1
    if F > MAX_FRAMES:
        raise ValueError(f"spectrum_ref: F = {F} frames exceed {MAX_FRAMES} per call")
    _, power = spectrum_power_ref(audio, n_fft, hop, t.window)
    acc = power[:, 0].copy()
    for f in range(1, F):
        acc = acc + power[:, f]
    amp = np.sqrt(acc * np.float32(1.0 / F))
    assert amp.dtype == np.float32
    bands = np.zeros((B, band_count), np.float32)
    for j in range(band_count):
        for k in range(int(t.band_start[j]), int(t.band_start[j + 1])):
            bands[:, j] = bands[:, j] + amp[:, k]
    k = np.arange(K)
    keep = (amp >= np.float32(t.lo)) & (amp <= np.float32(t.hi)) & (k >= t.k_lo)[None] & (k <= t.k_hi)[None]
    if local:
        left = np.concatenate([np.ones((B, 1), bool), amp[:, 1:] > amp[:, :-1]], axis=1)
        right = np.concatenate([amp[:, :-1] >= amp[:, 1:], np.ones((B, 1), bool)], axis=1)
        keep &= left & right
    peak_bins = np.full((B, max_peaks), -1, np.int32)
    peak_amp = np.zeros((B, max_peaks), np.float32)
    counts = np.zeros(B, np.int32)
    for b in range(B):
        keys = sorted(((int(amp[b, i].view(np.uint32)) << 32) | (0xFFFFFFFF - int(i)) for i in np.nonzero(keep[b])[0]),
                      reverse=True)[:max_peaks]
        counts[b] = len(keys)
        for i, key in enumerate(keys):
            peak_bins[b, i] = 0xFFFFFFFF - (key & 0xFFFFFFFF)
            peak_amp[b, i] = np.uint32(key >> 32).view(np.float32)
    return tuple(torch.from_numpy(np.ascontiguousarray(a))
                 for a in (amp, bands, peak_bins, peak_amp, counts, power))


def spectrum_graph_ref(peak_bins, peak_amplitudes, peak_counts, *, n_fft: int = 1024, sample_rate=16000,
                       height: int = 480, width: int = 640, x_max=9000.0, y_max=12.0, color=(0, 255, 0)):
    """Step 8 of the spectrum rule in plain loops: the peaks as a scatter graph, uint8 ``[B, height,
    width, 3]``."""
    import numpy as np

    from .spectrum import bin_pixels, check_graph, frequencies
    check_graph(height, width, x_max, y_max, color)
    bins, amps, counts = (np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)
                          for t in (peak_bins, peak_amplitudes, peak_counts))
    bin_px = bin_pixels(frequencies(n_fft, sample_rate), x_max, width)
    B, H, W = bins.shape[0], int(height), int(width)
    img = np.zeros((B, H, W, 3), np.uint8)
    img[:, H - 1, :] = 128
    img[:, :, 0] = 128
    for b in range(B):
        for i in range(int(counts[b])):
            px = int(bin_px[int(bins[b, i])])
            y = (1.0 - float(amps[b, i]) / float(y_max)) * (H - 1)              # Python floats: fp64
            py = int(min(max(y, 0.0), float(H - 1)))                           # truncation toward zero
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    img[b, min(max(py + dy, 0), H - 1), min(max(px + dx, 0), W - 1)] = color
    return torch.from_numpy(img)


# ---- projective warp --------------------------------------------------------------------------

def warp_coefficients_ref(quad, origin: str = "centre"):
    """Step 2 of ``ops/warp.py`` in Python ints (exact): ``(G, Hh, den, A, Bx, Cx, D, E, Cy)`` of the
    quad ``[(x, y)] * 4`` with ``den > 0``, or None if ``den == 0``."""
    from .warp import ORIGINS
    o = ORIGINS[origin]
    (X0, Y0), (X1, Y1), (X2, Y2), (X3, Y3) = [(2 * int(x) + o, 2 * int(y) + o) for x, y in quad]
    dx1, dx2, sx = X1 - X2, X3 - X2, X0 - X1 + X2 - X3
    dy1, dy2, sy = Y1 - Y2, Y3 - Y2, Y0 - Y1 + Y2 - Y3
    den = dx1 * dy2 - dy1 * dx2
    if den == 0:
        return None
    G, Hh = sx * dy2 - sy * dx2, dx1 * sy - dy1 * sx
    A, Bx, Cx = den * (X1 - X0) + G * X1, den * (X3 - X0) + Hh * X3, den * X0
    D, E, Cy = den * (Y1 - Y0) + G * Y1, den * (Y3 - Y0) + Hh * Y3, den * Y0
    c = (G, Hh, den, A, Bx, Cx, D, E, Cy)
    return tuple(-x for x in c) if den < 0 else c


def warp_quads_ref(frames: torch.Tensor, quads: torch.Tensor, count: torch.Tensor, k: int, size=(224, 224),
                   margin: int = 0, origin: str = "centre"):
    """The definition of :func:`aiko_services_amd.ops.warp.warp_quads` on the CPU: ``(patches,
    valid)``, uint8 ``[B*k, Ho, Wo, 3]`` and int32 ``[B*k]``.  The coefficients are Python ints, the
    per-pixel arithmetic numpy float64 vectorised over the patch (one rounding per operation, numpy
    contracts nothing), the sampling numpy int64.  Any ``Wo`` is taken: the multiple of 4 is the
    kernel's store width, not the rule's."""
    import numpy as np

    from .warp import COORD_MAX, COORD_MIN, MAX_SIDE, check_parameters
    Ho, Wo = int(size[0]), int(size[1])
    check_parameters(k, (Ho, 4), margin, origin)
    if not 1 <= Wo <= MAX_SIDE:
        raise ValueError(f"warp_quads_ref: 1 <= Wo <= {MAX_SIDE} required, got {Wo}")
    f = frames.detach().cpu().numpy().astype(np.int64)
    q = quads.detach().cpu().numpy().astype(np.int64)
    n = count.detach().cpu().numpy().astype(np.int64)
    B, H, W, _ = f.shape
    k, m = int(k), int(margin)
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"warp_quads_ref: H, W <= {MAX_SIDE} required, got {H} x {W}")
    if q.ndim != 4 or q.shape[0] != B or q.shape[1] < k or q.shape[2:] != (4, 2) or n.shape != (B,):
        raise ValueError(f"warp_quads_ref: quads [B, Kq >= k, 4, 2] and count [B] required, got {q.shape}, {n.shape}")
    patches = np.zeros((B * k, Ho, Wo, 3), np.uint8)
    valid = np.zeros(B * k, np.int32)
    f64 = np.float64
    u = ((2 * np.arange(Wo, dtype=np.int64) + 1) * (8 + m) - m * Wo).astype(f64) / f64(16 * Wo)       # [Wo]
    v = (((2 * np.arange(Ho, dtype=np.int64) + 1) * (8 + m) - m * Ho).astype(f64) / f64(16 * Ho))[:, None]
    for b in range(B):
        for i in range(min(max(int(n[b]), 0), k)):
            if q[b, i].min() < COORD_MIN or q[b, i].max() > COORD_MAX:
                continue
            c = warp_coefficients_ref(q[b, i].tolist(), origin)
            if c is None:
                continue
            assert all(abs(x) < 2 ** 53 for x in c)
            G, Hh, den, A, Bx, Cx, D, E, Cy = (f64(x) for x in c)
            w = ((G * u) + (Hh * v)) + den                              # [Ho, Wo]
            X = ((A * u) + (Bx * v)) + Cx
            Y = ((D * u) + (E * v)) + Cy
            ok = w > 0
            with np.errstate(all="ignore"):
                px, py = X / np.where(ok, w, f64(1)), Y / np.where(ok, w, f64(1))
                tx = np.minimum(np.maximum(px * f64(128) - f64(127.5), f64(0)), f64((W - 1) * 256))
                ty = np.minimum(np.maximum(py * f64(128) - f64(127.5), f64(0)), f64((H - 1) * 256))
            Px, Py = np.floor(tx).astype(np.int64), np.floor(ty).astype(np.int64)
            xi, fx, yi, fy = Px >> 8, (Px & 255)[..., None], Py >> 8, (Py & 255)[..., None]
            xj, yj = np.minimum(xi + 1, W - 1), np.minimum(yi + 1, H - 1)
            p = f[b]
            out = ((256 - fx) * (256 - fy) * p[yi, xi] + fx * (256 - fy) * p[yi, xj] + (256 - fx) * fy * p[yj, xi]
                   + fx * fy * p[yj, xj] + 32768) >> 16
            patches[b * k + i] = np.where(ok[..., None], out, 0).astype(np.uint8)
            valid[b * k + i] = 1
    return torch.from_numpy(patches), torch.from_numpy(valid)


# ---- camera wall ----------------------------------------------------------------------------

def wall_weights_ref(full: int, tile: int):
    """int64 ``[tile, full]``: ``w[o, j] = max(0, min((j+1)*tile, (o+1)*full) - max(j*tile, o*full))``,
    the share of source pixel ``j`` in output pixel ``o`` of an axis of ``full`` pixels reduced to
    ``tile``, in units of ``1 / (full*tile)`` of the axis.  Every row sums to ``full``."""
    import numpy as np
    o = np.arange(tile, dtype=np.int64)[:, None]
    j = np.arange(full, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((j + 1) * tile, (o + 1) * full) - np.maximum(j * tile, o * full))


def wall_select_ref(score, batch: int, slots: int, order: str = "index", min_score: int = 1) -> list:
    """The camera of every slot, or -1: ``ops.wall``'s selection rule."""
    if order == "index":
        cams = list(range(batch))
    elif order == "score":
        s = [int(v) for v in score.tolist()]
        cams = sorted((b for b in range(batch) if s[b] >= min_score), key=lambda b: (-s[b], b))
    else:
        raise ValueError(f"wall_select_ref: unknown order {order!r}")
    return [cams[j] if j < len(cams) else -1 for j in range(slots)]


def frame_wall_ref(frames: torch.Tensor, score: torch.Tensor | None = None, *, rows: int, cols: int, tile,
                   gap: int = 0, pages: int = 1, order: str = "index", min_score: int = 1, ring: int = 0,
                   label_scale: int = 0, label_base: int = 0, background=(0, 0, 0), alert=(255, 0, 0),
                   label_fg=(255, 255, 255), label_bg=(0, 0, 0)):
    """``ops.wall.frame_wall`` with numpy int64 on the CPU, from the rule in that module's docstring:
    the selection as a sorted list, each shown tile as ``wy @ frame @ wx^T`` with the weights of
    :func:`wall_weights_ref` and one rounding, then ring and label painted over it.  Returns
    ``(wall, source)``: uint8 ``[pages, Hw, Ww, 3]`` and int32 ``[pages, rows*cols]``."""
    import numpy as np
    from . import overlay_font
    from .wall import check_parameters, wall_shape
    frames = frames.cpu()
    B, H, W, _ = frames.shape
    th, tw = (int(v) for v in tile)
    check_parameters(rows=rows, cols=cols, tile=(th, tw), gap=gap, pages=pages, order=order, min_score=min_score,
                     ring=ring, label_scale=label_scale, label_base=label_base, background=background, alert=alert,
                     label_fg=label_fg, label_bg=label_bg, frame=(H, W))
    if order == "score" and score is None:
        raise ValueError("frame_wall_ref: order 'score' requires a score")
    if score is not None:
        score = score.cpu()
        if tuple(score.shape) != (B,):
            raise ValueError(f"frame_wall_ref: score [{B}] required, got {tuple(score.shape)}")
    N, g, q, s = rows * cols, int(gap), int(ring), int(label_scale)
    Hw, Ww = wall_shape(rows, cols, (th, tw), g)
    source = wall_select_ref(score, B, pages * N, order, int(min_score))
    wall = np.empty((pages, Hw, Ww, 3), np.uint8)
    wall[:] = np.asarray(background, np.uint8)
    wy, wx = wall_weights_ref(H, th), wall_weights_ref(W, tw)               # [th, H], [tw, W]
    f = frames.numpy()
    for slot, cam in enumerate(source):
        if cam < 0:
            continue
        p, t = divmod(slot, N)
        oy, ox = g + (t // cols) * (th + g), g + (t % cols) * (tw + g)
        S = np.tensordot(wy, f[cam].astype(np.int64), axes=(1, 0))          # rows: int64 [th, W, 3]
        S = np.tensordot(S, wx, axes=(1, 1)).transpose(0, 2, 1)             # columns: [th, tw, 3]
        tile_px = ((2 * S + W * H) // (2 * W * H)).astype(np.uint8)
        if q > 0 and score is not None and int(score[cam]) >= int(min_score):
            i, j = np.arange(th)[:, None], np.arange(tw)[None, :]
            edge = np.minimum(np.minimum(i, j), np.minimum(th - 1 - i, tw - 1 - j)) < q
            tile_px[edge] = np.asarray(alert, np.uint8)
        if s > 0:
            text = str(int(label_base) + cam)
            box = np.empty((s + 8 * s, s + len(text) * 6 * s, 3), np.uint8)
            box[:] = np.asarray(label_bg, np.uint8)
            for n, ch in enumerate(text):
                for gy, bits in enumerate(overlay_font.glyph_rows(ch)):
                    for gx in range(overlay_font.CELL_W):
                        if bits & (0x80 >> gx):
                            y0, x0 = s + gy * s, s + (n * 6 + gx) * s
                            box[y0:y0 + s, x0:x0 + s] = np.asarray(label_fg, np.uint8)
            hh, ww = min(box.shape[0], th - q), min(box.shape[1], tw - q)      # clipped to the tile
            if hh > 0 and ww > 0:
                tile_px[q:q + hh, q:q + ww] = box[:hh, :ww]
        wall[p, oy:oy + th, ox:ox + tw] = tile_px
    return torch.from_numpy(wall), torch.tensor(source, dtype=torch.int32).view(pages, N)


# ---- antialiased resize ---------------------------------------------------------------------

def scale_pass_sums_ref(pixels, bounds, k, axis: int):
    """One pass of ``ops.scale``'s rule before the clamp: int64 ``(2**21 + sum_x k[x] * p[first + x])
    >> 22`` along ``axis`` of the integer array ``pixels``, one output position at a time."""
    import numpy as np
    p = np.moveaxis(np.asarray(pixels).astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + p.shape[1:], np.int64)
    for xx in range(bounds.shape[0]):
        first, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.full(p.shape[1:], 1 << 21, np.int64)
        for x in range(n):
            acc += int(k[xx, x]) * p[first + x]
        out[xx] = acc >> 22
    return np.moveaxis(out, 0, axis)


def scale_frames_ref(frames: torch.Tensor, size, filter: str = "bicubic", box=None) -> torch.Tensor:
    """``ops.scale.scale_frames`` with numpy int64 on the CPU, from the rule in that module's
    docstring and with its :func:`~aiko_services_amd.ops.scale.axis_plan`: the horizontal pass over
    every source row, clamped to uint8, then the vertical pass on that; a pass the rule leaves out is
    left out.  ``box`` = (left, top, right, bottom) in sixteenths.  Returns a new uint8
    ``[B, Ho, Wo, 3]`` tensor."""
    import numpy as np
    from .scale import axis_plans
    frames = frames.cpu()
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8:
        raise ValueError("scale_frames_ref: frames uint8 [B, H, W, 3] required")
    horizontal, vertical = axis_plans(int(frames.shape[1]), int(frames.shape[2]), size, filter, box)
    p = frames.numpy()
    if horizontal is not None:
        p = np.clip(scale_pass_sums_ref(p, *horizontal, axis=2), 0, 255).astype(np.uint8)
    if vertical is not None:
        p = np.clip(scale_pass_sums_ref(p, *vertical, axis=1), 0, 255).astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(p).copy())
