"""Scratch budget of the camera-wall kernels (wall_ops.hip), read from the metadata comments of the
cross-compiled gfx950 assembly (CPU only: no GPU needed).  A thread of ``wall_compose`` keeps the
16 column sums of a source piece and its output bytes' sums and footprints in registers; an index
the compiler cannot resolve would move them to scratch memory."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parents[1] / "aiko_services_amd" / "csrc" / "kernels"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_wall_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "wall_ops.s"
    cmd = [HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-I", str(KERNELS),
           "--cuda-device-only", "-S", "-o", str(out), str(KERNELS / "wall_ops.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    fns = {m.group(1): int(m.group(2))
           for m in re.finditer(r"^(_Z[^:\s]+):.*?^; ScratchSize: (\d+)", asm, re.S | re.M)}
    compose = [k for k in fns if "wall_compose_kernel" in k]
    select = [k for k in fns if "wall_select_kernel" in k]
    assert len(compose) == 2, f"expected the vector and the byte instantiation, found {sorted(fns)}"
    assert len(select) == 1, f"expected one selection kernel, found {sorted(fns)}"
    assert len(fns) == 3, f"a kernel this test does not know: {sorted(fns)}"
    for name, scratch in fns.items():
        assert scratch == 0, f"{name}: {scratch} B of scratch"
