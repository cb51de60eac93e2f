"""Detect-then-classify example (``yolo_cascade_gpu.json``): YOLOv8 finds boxes, ``RoiCrop`` cuts
and resizes them on the device, ResNet-50 classifies every crop.  ``DetectionLabeler`` is the host
end of it: it joins the detection rows, the crop rects and the classifier's top-k into the
reference's overlay dictionary (``examples/yolo/yolo.py``)

    {"objects": [{"name", "confidence", ...}], "rectangles": [{"x", "y", "w", "h"}]}

one entry per used ROI slot, in frame order then score order.  ``name`` is ``class_<index>`` of the
classifier's best class and ``confidence`` its probability (the weights are random-init, so the
labels are structural); ``detector_class`` / ``detector_confidence`` are the detector's row.  The
element waits only on the two :class:`DeviceResult` objects it is given — their pinned host
copies complete by event, the device is never synchronised.
"""
from __future__ import annotations

from aiko_services_amd.pipeline.engine import PipelineElement
from aiko_services_amd.pipeline.stream import StreamEvent

__all__ = ["DetectionLabeler"]


class DetectionLabeler(PipelineElement):
    def __init__(self, context):
        context.set_protocol("detection_labeler:0")
        context.get_implementation("PipelineElement").__init__(self, context)

    def process_frame(self, stream, regions, topk):
        regions, topk = regions.wait(), topk.wait()
        det, rois = regions["det"], regions["rois"].tolist()
        prob, index = topk["top_prob"][:, 0].tolist(), topk["top_index"][:, 0].tolist()
        k = len(rois) // det.shape[0]
        overlay = {"objects": [], "rectangles": []}
        for slot, (x0, y0, x1, y1) in enumerate(rois):
            if x1 <= x0:                                  # unused slot
                continue
            row = det[slot // k, slot % k].tolist()
            overlay["objects"].append({"name": f"class_{index[slot]}", "confidence": round(prob[slot], 2),
                                       "detector_class": int(row[5]), "detector_confidence": round(row[4], 2)})
            overlay["rectangles"].append({"x": x0, "y": y0, "w": x1 - x0, "h": y1 - y0})
        return StreamEvent.OKAY, {"overlay": overlay}
