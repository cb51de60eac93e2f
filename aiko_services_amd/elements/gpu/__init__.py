"""GPU-resident elements (MI355X): synthetic decode, raw YUV ingest, preprocess, ResNet-50, top-k."""
from .ingest import YuvToRgb  # noqa: F401
