"""Scratch budget of the voice-activity kernels (vad_ops.hip), read from the metadata comments of the
cross-compiled gfx950 assembly (CPU only: no GPU needed).  The frame pass keeps a lane's samples and
its 64-bit sum in registers, the stream pass keeps its rows in LDS and its one serial lane's state
in registers: a spill in either would go to scratch memory."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parents[1] / "aiko_services_amd" / "csrc" / "kernels"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_vad_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "vad_ops.s"
    cmd = [HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-I", str(KERNELS),
           "--cuda-device-only", "-S", "-o", str(out), str(KERNELS / "vad_ops.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    fns = {m.group(1): int(m.group(2))
           for m in re.finditer(r"^(_Z[^:\s]+):.*?^; ScratchSize: (\d+)", asm, re.S | re.M)}
    fns = {k: v for k, v in fns.items() if "vad_" in k}
    frames = [k for k in fns if "vad_frames_kernel" in k]
    stream = [k for k in fns if "vad_stream_kernel" in k]
    assert len(frames) == 2 and len(stream) == 1 and len(fns) == 3, \
        f"expected the vector and the scalar frame pass and one stream pass, found {sorted(fns)}"
    for name, scratch in fns.items():
        assert scratch == 0, f"{name}: {scratch} B of scratch"
