"""Scratch budget of the antialiased-resize kernels (scale_ops.hip), read from the metadata comments
of the cross-compiled gfx950 assembly (CPU only: no GPU needed).  A thread of the horizontal pass
keeps twelve sums (four source rows x three channels) and its four row pointers in registers, one of
the vertical pass four sums; an index the compiler cannot resolve would move them to scratch
memory.  The set of kernels is the one named here: both passes, the horizontal pass alone, and the
vertical pass alone with dword and with byte loads."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parents[1] / "aiko_services_amd" / "csrc" / "kernels"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_scale_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "scale_ops.s"
    cmd = [HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-I", str(KERNELS),
           "--cuda-device-only", "-S", "-o", str(out), str(KERNELS / "scale_ops.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    fns = {m.group(1): int(m.group(2))
           for m in re.finditer(r"^(_Z[^:\s]+):.*?^; ScratchSize: (\d+)", asm, re.S | re.M)}
    both = [k for k in fns if "scale_both_kernel" in k]
    horizontal = [k for k in fns if "scale_h_kernel" in k]
    vertical = [k for k in fns if "scale_v_kernel" in k]
    assert len(both) == 1 and len(horizontal) == 1, f"expected one kernel each, found {sorted(fns)}"
    assert len(vertical) == 2, f"expected the dword and the byte instantiation, found {sorted(fns)}"
    assert len(fns) == 4, f"a kernel this test does not know: {sorted(fns)}"
    for name, scratch in fns.items():
        assert scratch == 0, f"{name}: {scratch} B of scratch"
