"""ROI crop (``csrc/kernels/roi_ops.hip``): the detector's fixed-size NMS rows select K sub-images
per frame, each resized to the classifier's uint8 input — detect-then-classify without the
detections visiting the host, so the whole cascade is hipGraph-capturable."""
from __future__ import annotations

import torch

__all__ = ["roi_crop"]


def roi_crop(frames: torch.Tensor, det: torch.Tensor, count: torch.Tensor, k: int = 8,
             size: tuple[int, int] = (224, 224), margin: float = 0.0,
             crops: torch.Tensor | None = None, rois: torch.Tensor | None = None):
    """uint8 ``[B, H, W, 3]`` frames + ``det`` ``[B, max_det, 6]`` / ``count`` ``[B]`` (the outputs
    of :func:`~aiko_services_amd.ops.detect.topk_nms`) -> ``crops`` uint8 ``[B*k, Ho, Wo, 3]`` and
    ``rois`` int32 ``[B*k, 4]`` = (X0, Y0, X1, Y1), half-open; slot ``b*k + i`` belongs to row ``i``
    of frame ``b``.

    Row ``i`` is used iff ``i < min(count[b], k)`` and its coordinates are finite; every other
    slot is zero in both outputs (a used rect has X1 > X0).  The box grows by ``margin`` x its
    width / height on each side, is rounded outwards and clamped to the frame (at least 1 x 1);
    the crop is the bilinear resize (half-pixel centres) of that rect to ``size``, ``Wo % 4 == 0``.
    ``count`` is read on the device: no host synchronisation."""
    B = frames.shape[0]
    Ho, Wo = size
    if crops is None:
        crops = torch.empty(B * k, Ho, Wo, 3, dtype=torch.uint8, device=frames.device)
    if rois is None:
        rois = torch.empty(B * k, 4, dtype=torch.int32, device=frames.device)
    torch.ops.aiko.roi_crop_out(frames, det, count, int(k), float(margin), crops, rois)
    return crops, rois
