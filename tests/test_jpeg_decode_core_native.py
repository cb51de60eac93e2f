"""The serial decoder of ``csrc/kernels/jpeg_decode_core.h`` — the text a lane of the entropy kernel runs —
on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer, before it sees a GPU.
``tests/native/jpeg_decode_core_main.cpp`` is built with the host compiler into a program of its own and
run as a process; it decodes every stream from an allocation of exactly the stream's length into one of
exactly the frame's coefficients.  Its coefficients and statuses must equal ``jpeg_decode_ref``'s, and
the sanitizers must stay silent."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import jpeg_decode_scenes as DS
from aiko_services_amd.ops import jpeg_decode as D
from aiko_services_amd.ops.reference import jpeg_decode_ref

ROOT = Path(__file__).resolve().parents[1]
SOURCE = ROOT / "tests" / "native" / "jpeg_decode_core_main.cpp"
KERNELS = ROOT / "aiko_services_amd" / "csrc" / "kernels"
CXX = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
FMT = {"i420": 1, "i444": 2, "yuyv": 3}

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("jpeg_decode_core") / "jpeg_decode_core_main"
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I", str(KERNELS), str(SOURCE), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return out


def _run(program, tmp_path, data, nbytes, desc, H, W, fmt):
    """``(coef int16 [N, blocks, 64], status int32 [N])`` of the program; fails on any sanitizer report."""
    N, cap = data.shape
    (tmp_path / "data.bin").write_bytes(data.numpy().tobytes())
    (tmp_path / "nbytes.bin").write_bytes(nbytes.numpy().astype("<i4").tobytes())
    (tmp_path / "desc.bin").write_bytes(desc.numpy().tobytes())
    res = subprocess.run([str(program), str(tmp_path), str(N), str(cap), str(H), str(W), str(FMT[fmt])],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and not res.stderr, f"exit {res.returncode}\n{res.stderr[-4000:]}"
    nblocks = D.blocks(fmt, H, W)
    coef = np.frombuffer((tmp_path / "coef.bin").read_bytes(), "<i2").reshape(N, nblocks, 64)
    status = np.frombuffer((tmp_path / "status.bin").read_bytes(), "<i4")
    return torch.from_numpy(coef.copy()), torch.from_numpy(status.copy())


def _compare(program, tmp_path, data, nbytes, desc, H, W, fmt):
    coefficients = []
    _, want = jpeg_decode_ref(data, nbytes, desc, H, W, fmt, coefficients=coefficients)
    coef, status = _run(program, tmp_path, data, nbytes, desc, H, W, fmt)
    assert torch.equal(status, want), (status.tolist(), want.tolist())
    assert torch.equal(coef, torch.stack(coefficients))
    return want


@pytest.mark.parametrize("fmt", DS.FORMATS)
def test_valid_streams(program, tmp_path, fmt):
    for H, W in ((17, DS.width(fmt, 23)), (152, 24), (16, 720)):
        for kind in DS.KINDS:
            if not DS.streams(fmt, H, W, kind):
                continue
            data, nbytes, desc, _ = DS.packed(fmt, H, W, kind)
            want = _compare(program, tmp_path, data, nbytes, desc, H, W, fmt)
            assert not want.any()


def test_the_corrupt_handful(program, tmp_path):
    fmt, H, W = DS.CORRUPT_SHAPE
    hand = DS.corrupt_handful()
    plan = D.parse(hand["valid"][0])
    data, nbytes, desc = DS.pack_raw([f for f, _ in hand.values()], [n for _, n in hand.values()], plan)
    want = _compare(program, tmp_path, data, nbytes, desc, H, W, fmt)
    assert want[0] == 0 and bool((want[1:] != 0).all())


def test_every_truncation_and_every_bit_flip(program, tmp_path):
    """One small stream (16 x 16, i420, with optimised tables so that not every bit pattern is a code): cut
    at every length, cut at every length with an EOI put behind, and with every single bit of its
    entropy-coded bytes flipped."""
    fmt, H, W = "i420", 16, 16
    good = DS.streams(fmt, H, W, "pillow_opt")[0]
    plan = D.parse(good)
    scan = plan.scan_offset
    frames = [good] + [good[:n] for n in range(len(good))] + \
        [good[:n] + b"\xff\xd9" for n in range(scan, len(good) - 2)] + \
        [DS.flip(good, bit) for bit in range(8 * scan, 8 * (len(good) - 2))]
    data, nbytes, desc = DS.pack_raw(frames, [len(f) for f in frames], plan)
    want = _compare(program, tmp_path, data, nbytes, desc, H, W, fmt)
    seen = sorted(set(want.tolist()))
    print(f"{len(frames)} streams of at most {len(good)} bytes; statuses seen: {seen}")
    assert want[0] == 0 and {0, 1, 4}.issubset(seen)
