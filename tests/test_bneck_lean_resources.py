"""bneck_fused.hip builds four kernels under one name: a generic and a lean instance per CIN.  All
four keep the counted-wait budget of tests/test_kernel_resources.py (no scratch, at most 256
VGPRs), and each lean instance carries strictly less control flow and scalar arithmetic than the
generic instance of the same CIN in the same build (CPU: hipcc cross-compiles gfx950 assembly)."""
import re

import pytest

from test_kernel_resources import HIPCC, _device_asm, _functions

NOT_SALU = ("s_cbranch", "s_branch", "s_waitcnt", "s_barrier", "s_nop", "s_load", "s_buffer_load", "s_endpgm",
            "s_memtime", "s_sleep", "s_setprio")


def _mnemonics(body: str) -> list:
    out = []
    for line in body.splitlines():
        m = re.match(r"^\t([a-z][a-z0-9_]+)\b", line)
        if m:
            out.append(m.group(1))
    return out


def _counts(body: str):
    ins = _mnemonics(body)
    branches = sum(1 for i in ins if i.startswith("s_cbranch") or i == "s_branch")
    salu = sum(1 for i in ins if i.startswith("s_") and not i.startswith(NOT_SALU))
    return branches, salu


@pytest.fixture(scope="module")
def instances(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not available")
    asm = _device_asm("bneck_fused.hip", tmp_path_factory.mktemp("bneck_lean"))
    return {k: v for k, v in _functions(asm).items() if "bneck_fused_kernel" in k}


def _pick(instances, cin, lean):
    # the template arguments as the Itanium mangling spells them: <int CIN, bool LEAN>
    tag = f"ILi{cin}ELb{int(lean)}E"
    hit = [k for k in instances if tag in k]
    assert len(hit) == 1, (tag, sorted(instances))
    return instances[hit[0]]


def test_four_instances_within_the_counted_wait_budget(instances):
    assert len(instances) == 4, sorted(instances)
    for name, (scratch, vgprs, body) in instances.items():
        assert scratch == 0, f"{name}: {scratch} B of scratch"
        assert "scratch_load" not in body and "scratch_store" not in body, name
        assert 0 < vgprs <= 256, (name, vgprs)


@pytest.mark.parametrize("cin", [256, 64])
def test_lean_has_fewer_branches_and_scalar_ops(instances, cin):
    gb, gs = _counts(_pick(instances, cin, False)[2])
    lb, ls = _counts(_pick(instances, cin, True)[2])
    print(f"CIN {cin}: branches generic {gb} lean {lb}; scalar ALU generic {gs} lean {ls}")
    assert gb > 0 and gs > 0 and lb > 0 and ls > 0
    assert lb < gb, (lb, gb)
    assert ls < gs, (ls, gs)
