"""Scratch budget of the warp kernel (warp_ops.hip), read from the metadata comments of the
cross-compiled gfx950 assembly (CPU only: no GPU needed).  A lane keeps the fp64 u products of its four
pixels over a band's rows beside the nine coefficients and the four taps of a pixel: a spill would go
to scratch memory."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parents[1] / "aiko_services_amd" / "csrc" / "kernels"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_warp_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "warp_ops.s"
    cmd = [HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-I", str(KERNELS),
           "--cuda-device-only", "-S", "-o", str(out), str(KERNELS / "warp_ops.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    fns = {m.group(1): int(m.group(2))
           for m in re.finditer(r"^(_Z[^:\s]+):.*?^; ScratchSize: (\d+)", asm, re.S | re.M)}
    assert len(fns) == 1 and "quad_warp_u8_kernel" in next(iter(fns)), f"expected the one warp kernel, found {sorted(fns)}"
    for name, scratch in fns.items():
        assert scratch == 0, f"{name}: {scratch} B of scratch"
    # the kernel has no LDS, and no atomics
    assert re.search(r"^\s*\.amdhsa_group_segment_fixed_size 0\s*$", asm, re.M) and "atomic" not in asm
