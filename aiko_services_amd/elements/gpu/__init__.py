"""GPU-resident elements (MI355X): synthetic decode, raw YUV ingest and egress, preprocess, ResNet-50, top-k."""
from .egress import FrameDownload, RgbToYuv  # noqa: F401
from .ingest import YuvToRgb  # noqa: F401
