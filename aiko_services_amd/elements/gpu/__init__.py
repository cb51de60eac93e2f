"""GPU-resident elements (MI355X): synthetic decode, raw YUV ingest and egress, raw PCM ingest, preprocess,
ResNet-50, top-k."""
from .audio_ingest import AudioResample  # noqa: F401
from .egress import FrameDownload, RgbToYuv  # noqa: F401
from .ingest import YuvToRgb  # noqa: F401
from .marker import MarkerDetector, MarkerResults  # noqa: F401
from .scale import FrameScale  # noqa: F401
from .spectrum import AudioSpectrum, SpectrumResults  # noqa: F401
from .warp import FrameWarp, QuadRectify  # noqa: F401
