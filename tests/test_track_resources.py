"""Resource budget of the tracker kernel (track_ops.hip), read from the metadata comments of the
cross-compiled gfx950 assembly (CPU only: no GPU needed).  A lane keeps its track, its best pair and
its 64-bit masks in registers; the row's detections sit in a few hundred bytes of LDS.  Per-pair
tables indexed by a detection number would move to scratch memory, which this rules out."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parents[1] / "aiko_services_amd" / "csrc" / "kernels"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_track_kernel_uses_no_scratch_and_little_lds(tmp_path):
    out = tmp_path / "track_ops.s"
    cmd = [HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-I", str(KERNELS),
           "--cuda-device-only", "-S", "-o", str(out), str(KERNELS / "track_ops.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    fns = {m.group(1): tuple(int(g) for g in m.groups()[1:])
           for m in re.finditer(r"^(_Z[^:\s]+):.*?^; NumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)",
                                asm, re.S | re.M)}
    found = {name: v for name, v in fns.items() if "track_detections_kernel" in name}
    assert len(found) == 1, f"expected one track_detections_kernel, found {sorted(fns)}"
    (vgprs, scratch, lds), = found.values()
    # occupancy does not bound a one-wave-per-row kernel: the VGPR count is printed, not pinned
    print(f"track_detections_kernel: {vgprs} VGPRs, {scratch} B scratch, {lds} B LDS")
    assert scratch == 0, f"{scratch} B of scratch"
    assert lds <= 64 * 1024, f"{lds} B of static LDS"
