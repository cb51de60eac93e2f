"""Which kernels the tuners may time for a layer: ``ops.conv.conv_candidates`` and
``ops.transformer.fp8_candidates`` against ``tests/golden/conv_candidates.json``.

The golden lists were recorded from the commit BEFORE the candidate lists were split out of the
tuners (``_tune`` / ``_tune_fp8`` driven with a recording ``launch`` and a stubbed
``torch.cuda.Event``), for exactly the cases built here — so they pin the order as well as the
membership: the first of equal times wins.  No GPU: every tensor is a CPU or meta tensor."""
import json
import os

import pytest
import torch

from aiko_services_amd.ops import conv as C
from aiko_services_amd.ops import transformer as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_candidates.json")
SWITCHES = ("AIKO_CONV_EXTRA", "AIKO_PW_AB", "AIKO_PW_DUAL", "AIKO_CONV_SKIP", "AIKO_CONV_SKIP_TILES",
            "AIKO_FP8_SKIP")
ALL_VARIANTS = ",".join(str(v) for v in range(21))


def _spec(cin, cout, k, stride=1, pad=None, act="relu"):
    return C.make_conv_spec(torch.zeros(cout, cin, k, k), torch.zeros(cout), stride=stride,
                            pad=k // 2 if pad is None else pad, act=act)


def _x(*shape, device="cpu"):
    return torch.zeros(*shape, dtype=torch.bfloat16, device=device)


def conv_cases():
    """name -> (kwargs of conv_candidates, environment).  One entry per branch of the tuner's list."""
    cases = {}

    def add(name, spec, x, env=None, **kw):
        cases[name] = (dict(spec=spec, x=x, **kw), env or {})

    add("narrow_3x3_16_32_s2", _spec(16, 32, 3, stride=2), _x(1, 8, 8, 16))
    buf = _x(2, 5, 80, 128)
    add("rows_3x3_32_32_slice_res_after", _spec(32, 32, 3, act="silu"), buf[..., :32],
        residual=buf[..., 32:64], residual_after_act=True)
    add("pw_64_32_narrow_tiles_only", _spec(64, 32, 1), _x(1, 8, 8, 64))
    hp, wp = C.stem_geometry(32, 32)
    add("stem_7x7", C.make_stem_spec(torch.zeros(64, 3, 7, 7), torch.zeros(64)), _x(1, hp, wp, 4))
    add("glds_exact_n_3x3_80_80", _spec(80, 80, 3), _x(1, 8, 8, 80))
    add("exact_n_3x3_64_80", _spec(64, 80, 3), _x(1, 8, 8, 64))
    add("exact_n_3x3_64_144", _spec(64, 144, 3), _x(1, 8, 8, 64))
    s64 = _spec(64, 64, 3)
    add("patch_3x3_64_64_w56", s64, _x(2, 56, 56, 64))
    add("patch_off_w55", s64, _x(2, 56, 55, 64))
    add("patch_off_res_after", s64, _x(2, 56, 56, 64), residual=_x(2, 56, 56, 64), residual_after_act=True)
    add("patchw_3x3_128_128_w28", _spec(128, 128, 3), _x(2, 28, 28, 128))
    add("pw_128_512_res", _spec(128, 512, 1), _x(1, 4, 4, 128), residual=_x(1, 4, 4, 512))
    s256 = _spec(256, 1024, 1)
    pw256 = dict(x=_x(1, 4, 4, 256), residual=_x(1, 4, 4, 1024))
    add("pw_256_1024_res", s256, **pw256)
    add("pw_512_2048_res", _spec(512, 2048, 1), _x(1, 4, 4, 512), residual=_x(1, 4, 4, 2048))
    add("pw_1024_256", _spec(1024, 256, 1), _x(1, 4, 4, 1024))
    add("pw_256_4096", _spec(256, 4096, 1), _x(1, 4, 4, 256))
    dual = C.fuse_shortcut(_spec(128, 512, 1), _spec(256, 512, 1, stride=2, act=None))
    add("dual_projection", dual, _x(1, 4, 4, 128), x2=_x(1, 8, 8, 256))
    add("dual_projection_pw_dual", dual, _x(1, 4, 4, 128), x2=_x(1, 8, 8, 256), env={"AIKO_PW_DUAL": "1"})
    add("meta_3x3_256_256_over_2gib", _spec(256, 256, 3), _x(1400, 56, 56, 256, device="meta"))
    for name, env in (("extra_5", {"AIKO_CONV_EXTRA": "5"}), ("extra_6", {"AIKO_CONV_EXTRA": "6"}),
                      ("extra_11", {"AIKO_CONV_EXTRA": "11"}), ("extra_19", {"AIKO_CONV_EXTRA": "19"}),
                      ("pw_ab", {"AIKO_PW_AB": "1"}), ("skip_8_20", {"AIKO_CONV_SKIP": "8,20"}),
                      ("skip_tile_256x256x8", {"AIKO_CONV_SKIP_TILES": "256x256x8"}),
                      ("skip_all", {"AIKO_CONV_SKIP": ALL_VARIANTS})):
        add("pw_256_1024_res_" + name, s256, env=env, **pw256)
    return cases


def fp8_cases():
    """name -> (key, mx, environment); key = (M, N, K, lda, residual, act, MX in, MX out), one per
    arm of the fp8 tuner's list."""
    return {
        "mx": ((256, 768, 768, 768, False, 0, True, False), True, {}),
        "n_192": ((256, 192, 768, 768, False, 0, False, False), False, {}),
        "n_768": ((256, 768, 768, 768, False, 0, False, False), False, {}),
        "n_768_mx_in_res": ((256, 768, 3072, 3072, True, 0, True, False), True, {}),
        "n_4096": ((256, 4096, 768, 768, False, 3, False, False), False, {}),
        "n_768_skip": ((256, 768, 768, 768, False, 0, False, False), False, {"AIKO_FP8_SKIP": "256x256x4"}),
    }


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture
def switches(monkeypatch):
    def apply(env):
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
    return apply


def _tuples(rows):
    return [tuple(r) for r in rows]


def test_golden_covers_the_cases(golden):
    assert set(golden["conv"]) == set(conv_cases())
    assert set(golden["fp8"]) == set(fp8_cases())


@pytest.mark.parametrize("name", list(conv_cases()))
def test_conv_candidates_match_parent(name, golden, switches):
    kw, env = conv_cases()[name]
    switches(env)
    got = C.conv_candidates(**kw)
    assert got == _tuples(golden["conv"][name])
    for bm, bn, v in got:
        assert (bm, bn) in C.VARIANTS[C.Variant(v)].tiles


@pytest.mark.parametrize("name", list(fp8_cases()))
def test_fp8_candidates_match_parent(name, golden, switches):
    key, mx, env = fp8_cases()[name]
    switches(env)
    assert T.fp8_candidates(key, mx) == _tuples(golden["fp8"][name])


def test_branches_are_reached(golden):
    """The golden lists themselves show each case's branch (so a case that drifted off its branch
    is noticed when the file is re-recorded)."""
    g = {k: _tuples(v) for k, v in golden["conv"].items()}
    variants = lambda name: {t[2] for t in g[name]}   # noqa: E731
    assert variants("narrow_3x3_16_32_s2") == {0, 7}
    assert variants("rows_3x3_32_32_slice_res_after") == {0, 7, 17}
    assert variants("pw_64_32_narrow_tiles_only") == {0}
    assert variants("stem_7x7") == {0, 1}
    assert (256, 80, 1) in g["glds_exact_n_3x3_80_80"] and variants("glds_exact_n_3x3_80_80") == {0, 1}
    assert (256, 80, 18) in g["exact_n_3x3_64_80"] and (128, 144, 18) in g["exact_n_3x3_64_144"]
    assert 10 in variants("patch_3x3_64_64_w56")
    assert 10 not in variants("patch_off_w55") and 10 not in variants("patch_off_res_after")
    assert 16 in variants("patchw_3x3_128_128_w28")
    assert 13 in variants("pw_128_512_res") and {12, 20}.isdisjoint(variants("pw_128_512_res"))
    assert {12, 13, 20} <= variants("pw_256_1024_res") and (256, 256, 20) not in g["pw_256_1024_res"]
    assert {12, 13, 20} <= variants("pw_512_2048_res")
    assert (256, 256, 20) in g["pw_1024_256"] and 12 in variants("pw_1024_256") and 13 not in variants("pw_1024_256")
    assert 20 not in variants("pw_256_4096")
    assert 13 not in variants("dual_projection") and 13 in variants("dual_projection_pw_dual")
    assert variants("meta_3x3_256_256_over_2gib") == {0, 1}
    for v in (5, 6, 11, 19):
        assert v not in variants("pw_256_1024_res") and v in variants(f"pw_256_1024_res_extra_{v}")
    assert 14 in variants("pw_256_1024_res_pw_ab")
    assert {8, 20}.isdisjoint(variants("pw_256_1024_res_skip_8_20"))
    assert (256, 256, 8) not in g["pw_256_1024_res_skip_tile_256x256x8"]
    assert g["pw_256_1024_res_skip_all"] == g["pw_256_1024_res"]


def test_candidates_survive_the_tile_cache_file(tmp_path, monkeypatch, switches):
    """Tuples from the tuner serialise as plain ints and load back equal (the ids are a persisted
    format: tile-cache files, profiles, ``tile=`` arguments)."""
    switches({"AIKO_CONV_EXTRA": "5,6,11,19", "AIKO_PW_AB": "1"})
    cache = {}
    for i, (kw, _) in enumerate(conv_cases().values()):
        for j, t in enumerate(C.conv_candidates(**kw)):
            assert C.Variant(t[2]) in C.VARIANTS
            cache[(i, j, 64, 1, 1, 1, 64, None, False, 64)] = t
    monkeypatch.setattr(C, "_tile_cache", dict(cache))
    path = tmp_path / "tiles.json"
    C.save_tile_cache(str(path))
    assert json.loads(json.dumps(json.load(open(path)))) == [[list(k), list(v)] for k, v in cache.items()]
    monkeypatch.setattr(C, "_tile_cache", {})
    assert C.load_tile_cache(str(path)) == len(cache)
    assert C._tile_cache == cache
    assert all(type(v) is int for t in C._tile_cache.values() for v in t)
