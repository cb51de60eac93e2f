"""Scratch budget of the JPEG decode kernels (jpeg_decode_ops.hip), read from the metadata comments of
the cross-compiled gfx950 assembly (CPU only: no GPU needed).  The entropy kernel runs the serial decoder
of jpeg_decode_core.h with its bit buffer, three predictors and table pointers in registers, and the
IDCT kernel keeps two 8-vectors per thread in arrays it indexes from unrolled loops: an index the
compiler cannot resolve, or a spill, would go to scratch memory."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parents[1] / "aiko_services_amd" / "csrc" / "kernels"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_jpeg_decode_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "jpeg_decode_ops.s"
    cmd = [HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-I", str(KERNELS),
           "--cuda-device-only", "-S", "-o", str(out), str(KERNELS / "jpeg_decode_ops.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    fns = {m.group(1): int(m.group(2))
           for m in re.finditer(r"^(_Z[^:\s]+):.*?^; ScratchSize: (\d+)", asm, re.S | re.M)}
    fns = {k: v for k, v in fns.items() if "jpeg_" in k}
    for kernel in ("jpeg_scan_kernel", "jpeg_entropy_kernel", "jpeg_idct_kernel"):
        assert len([k for k in fns if kernel in k]) == 1, f"expected one {kernel}, found {sorted(fns)}"
    assert len(fns) == 3, f"expected the scan, entropy and IDCT kernels, found {sorted(fns)}"
    for name, scratch in fns.items():
        assert scratch == 0, f"{name}: {scratch} B of scratch"
