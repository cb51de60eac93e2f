"""Scratch budget of the marker kernels (marker_ops.hip), read from the metadata comments of the
cross-compiled gfx950 assembly (CPU only: no GPU needed).  The mask pass keeps a wave's 16 loads in
registers and the region pass runs 1024 threads per workgroup, which caps its registers at 128,
with eight 64-bit extremes and the sampling's 64-bit divisions live in them: a spill in either
would go to scratch memory."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parents[1] / "aiko_services_amd" / "csrc" / "kernels"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_marker_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "marker_ops.s"
    cmd = [HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-I", str(KERNELS),
           "--cuda-device-only", "-S", "-o", str(out), str(KERNELS / "marker_ops.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    fns = {m.group(1): int(m.group(2))
           for m in re.finditer(r"^(_Z[^:\s]+):.*?^; ScratchSize: (\d+)", asm, re.S | re.M)}
    fns = {k: v for k, v in fns.items() if "marker_" in k}
    ranges = [k for k in fns if "marker_range_kernel" in k]
    masks = [k for k in fns if "marker_mask_kernel" in k]
    regions = [k for k in fns if "marker_regions_kernel" in k]
    assert len(ranges) == 2 and len(masks) == 2 and len(regions) == 1 and len(fns) == 5, \
        f"expected the vector and the byte form of the range and the mask pass and one region pass, found {sorted(fns)}"
    for name, scratch in fns.items():
        assert scratch == 0, f"{name}: {scratch} B of scratch"
