"""Scratch budget of the spectrum kernels (spectrum_ops.hip), read from the metadata comments of the
cross-compiled gfx950 assembly (CPU only: no GPU needed).  The frame pass keeps a frame in LDS and a
butterfly in registers, the reduce pass its amplitudes and sort keys in LDS, the graph pass a strip's
dots in LDS: a spill in any of them would go to scratch memory."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parents[1] / "aiko_services_amd" / "csrc" / "kernels"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_spectrum_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "spectrum_ops.s"
    cmd = [HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-I", str(KERNELS),
           "--cuda-device-only", "-S", "-o", str(out), str(KERNELS / "spectrum_ops.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    fns = {m.group(1): int(m.group(2))
           for m in re.finditer(r"^(_Z[^:\s]+):.*?^; ScratchSize: (\d+)", asm, re.S | re.M)}
    fns = {k: v for k, v in fns.items() if "spectrum_" in k}
    frames = [k for k in fns if "spectrum_frames_kernel" in k]
    reduce = [k for k in fns if "spectrum_reduce_kernel" in k]
    graph = [k for k in fns if "spectrum_graph_kernel" in k]
    assert len(frames) == 12 and len(reduce) == 1 and len(graph) == 1 and len(fns) == 14, \
        f"expected the vector and the scalar frame pass at six sizes, one reduce and one graph pass, found {sorted(fns)}"
    for name, scratch in fns.items():
        assert scratch == 0, f"{name}: {scratch} B of scratch"
    lds = [int(m.group(1)) for m in re.finditer(r"^; LDSByteSize: (\d+)", asm, re.M)]
    assert len(lds) == 14 and max(lds) == 65536              # the 8192-point frame: 64 KB, the static limit
