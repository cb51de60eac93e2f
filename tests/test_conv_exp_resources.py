"""Register / scratch budget of the fused 3x3 + expansion kernel (conv_exp.hip), read from the
metadata comments of its cross-compiled gfx950 assembly (CPU only: no GPU needed).  Its phase 1
waits on counted `vmcnt(N)`; a scratch access is a VMEM op those counts do not include, and the
kernel runs one 512-thread workgroup per CU, which leaves each wave 256 VGPRs."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parents[1] / "aiko_services_amd" / "csrc" / "kernels"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_conv_exp_kernel_fits_registers_without_scratch(tmp_path):
    out = tmp_path / "conv_exp.s"
    cmd = [HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-I", str(KERNELS),
           "--cuda-device-only", "-S", "-o", str(out), str(KERNELS / "conv_exp.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    fns = {}
    for m in re.finditer(r"^(_Z[^:\s]+):(.*?)^; ScratchSize: (\d+)", asm, re.S | re.M):
        v = re.search(r"^; NumVgprs: (\d+)", m.group(2), re.M)
        fns[m.group(1)] = (int(m.group(3)), int(v.group(1)) if v else -1)
    fns = {k: v for k, v in fns.items() if "conv3x3_exp_kernel" in k}
    assert len(fns) >= 1, "no instantiation of conv3x3_exp_kernel found"
    for name, (scratch, vgprs) in fns.items():
        assert scratch == 0, f"{name}: {scratch} B of scratch"
        assert 0 < vgprs <= 256, (name, vgprs)
