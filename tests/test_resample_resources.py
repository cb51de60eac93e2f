"""Resource budget of the resample kernels (resample_ops.hip), read from the metadata comments of
the cross-compiled gfx950 assembly (CPU only: no GPU needed).  A thread keeps four accumulators and
their LDS offsets in registers, indexed by unrolled constants, and the vector loads unpack their
frames by name; an index the compiler cannot resolve would move them to scratch memory."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parents[1] / "aiko_services_amd" / "csrc" / "kernels"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_resample_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "resample_ops.s"
    cmd = [HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-I", str(KERNELS),
           "--cuda-device-only", "-S", "-o", str(out), str(KERNELS / "resample_ops.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    fns = {m.group(1): (int(m.group(2)), int(m.group(3)))
           for m in re.finditer(r"^(_Z[^:\s]+):.*?^; NumVgprs: (\d+).*?^; ScratchSize: (\d+)", asm, re.S | re.M)}
    # template arguments in the mangled name: I<s: int16, f: fp32>Lb<vector>EE
    found = {}
    for name, (vgprs, scratch) in fns.items():
        m = re.search(r"resample_kernelI([sf])Lb([01])EE", name)
        if m:
            found[(m.group(1), bool(int(m.group(2))))] = (vgprs, scratch)
    want = {(sample, vec) for sample in "sf" for vec in (False, True)}
    assert set(found) == want, f"expected the vector and the scalar instantiation of int16 and fp32, found {sorted(found)}"
    for key, (vgprs, scratch) in sorted(found.items()):
        print(f"sample {key[0]} vector {key[1]}: {vgprs} VGPRs, {scratch} B scratch")
        assert scratch == 0, f"{key}: {scratch} B of scratch"
        assert vgprs <= 128, f"{key}: {vgprs} VGPRs leave fewer than 4 waves per SIMD"
