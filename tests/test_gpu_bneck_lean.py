"""bneck_fused's lean production instance (the default launch) against the generic instance of
the same build (AIKO_BN_LEAN=0, schedule mode 1024): the two share tile geometry, MFMA order and
rounding, so the outputs must be bit-identical.  Shapes: the smallest at which the lean loop nest
(image prologue / interior rows / boundary rows) and its immediate `s_waitcnt vmcnt(N)` counts
can go wrong."""
import pytest
import torch

import conv_parity_cases as P
import kernel_guard

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16

LEAN_CASES = [
    (4, 1, 1), (3, 2, 2),      # an image boundary every row or two
    (2, 13, 4),                # an uneven split
    (2, 20, 1),                # one workgroup across two images
    (1, 56, 1),                # a pure interior run
    (3, 56, 7),                # ranges that start and end mid-image
    (2, 3, 0),                 # more CUs than rows
    (24, 56, 0),               # several rows per CU: the steady-state counted waits carry the load
]


def _operands(B, H, dual, grid):
    from aiko_services_amd.ops import conv as C
    pc = P.bneck_case(B, H, dual, grid, DEV)
    c1, c2, c3, down = pc.specs["c1"], pc.specs["c2"], pc.specs["c3"], pc.specs.get("down")
    conv3 = C.fuse_shortcut(c3, down) if dual else c3
    x = pc.ops["x"].permute(0, 2, 3, 1).contiguous().to(DEV)
    return x, c1, c2, conv3


def _run(x, c1, c2, conv3, grid, out=None):
    from aiko_services_amd.ops import conv as C
    B, H = x.shape[:2]
    if out is None:
        out = torch.full((B, H, 56, 256), float("nan"), dtype=BF16, device=DEV)
    y = C.bneck_fused(x, c1, c2, conv3, out=out, grid=grid)
    torch.cuda.synchronize()
    return y


def _generic(monkeypatch, *args):
    with monkeypatch.context() as mp:
        mp.setenv("AIKO_BN_LEAN", "0")
        mp.setenv("AIKO_BN_MODE", "1024")
        return _run(*args)


@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("B,H,grid", LEAN_CASES)
def test_lean_equals_generic(native, monkeypatch, B, H, grid, dual):
    monkeypatch.delenv("AIKO_BN_LEAN", raising=False)
    monkeypatch.delenv("AIKO_BN_MODE", raising=False)
    x, c1, c2, conv3 = _operands(B, H, dual, grid)
    lean = _run(x, c1, c2, conv3, grid)
    gen = _generic(monkeypatch, x, c1, c2, conv3, grid)
    assert torch.isfinite(lean.float()).all(), "unwritten / non-finite output pixels"
    assert torch.equal(lean, gen)


@pytest.mark.parametrize("dual", [False, True])
def test_lean_between_guard_bands(native, monkeypatch, dual):
    """(3, 56, 7): seven ranges of 24 rows, starting and ending mid-image; y sits between poison
    guards, which the kernel must leave as they are while writing every element of y."""
    monkeypatch.delenv("AIKO_BN_LEAN", raising=False)
    monkeypatch.delenv("AIKO_BN_MODE", raising=False)
    B, H, grid = 3, 56, 7
    x, c1, c2, conv3 = _operands(B, H, dual, grid)
    xg, check_x = kernel_guard.guarded(x.shape, BF16, DEV, values=x, name="x")
    yg, check_y = kernel_guard.guarded((B, H, 56, 256), BF16, DEV, name="y")
    y = _run(xg, c1, c2, conv3, grid, out=yg)
    check_y()
    check_x()
    assert torch.isfinite(y.float()).all(), "unwritten / non-finite output pixels"
    assert torch.equal(y, _generic(monkeypatch, x, c1, c2, conv3, grid))


@pytest.mark.parametrize("dual", [False, True])
def test_lean_graph_replay(native, monkeypatch, dual):
    """The lean instance replayed from a captured graph is bit-equal to its eager run."""
    monkeypatch.delenv("AIKO_BN_LEAN", raising=False)
    monkeypatch.delenv("AIKO_BN_MODE", raising=False)
    from aiko_services_amd.ops import conv as C
    B, H, grid = 2, 20, 3
    x, c1, c2, conv3 = _operands(B, H, dual, grid)
    eager = _run(x, c1, c2, conv3, grid)
    out = torch.full((B, H, 56, 256), float("nan"), dtype=BF16, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        C.bneck_fused(x, c1, c2, conv3, out=out, grid=grid)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    out.fill_(float("nan"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        C.bneck_fused(x, c1, c2, conv3, out=out, grid=grid)
    torch.cuda.synchronize()
    for _ in range(2):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
