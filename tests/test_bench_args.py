"""bench.py's per-model defaults (the driver runs it with only --gpus/--steps/--warmup): the
batch sizes chosen for tile quantisation on 256 CUs and the configs' frame sizes."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402


def test_resnet_default_batch_fills_the_chip():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.model == "resnet50" and a.batch == 640 and (a.height, a.width) == (224, 224)
    # stage 3 (14 x 14 outputs) at 256-row tiles: whole rounds over 256 CUs, >= 95 % busy
    tiles = -(-a.batch * 196 // 256)
    rounds = -(-tiles // 256)
    assert tiles / (256 * rounds) >= 0.95


def test_model_defaults_and_explicit_overrides():
    assert bench.parse_args(["--model", "yolov8n"]).batch == 192
    y = bench.parse_args(["--model", "yolov8n"])
    assert (y.height, y.width) == (480, 640)
    assert bench.parse_args(["--model", "whisper-small"]).batch == 28
    assert bench.parse_args(["--batch", "256"]).batch == 256
    p = bench.parse_args(["--parallel", "pp", "--height", "224", "--width", "224"])
    assert (p.height, p.width) == (224, 224) and p.batch == 640
    assert (bench.parse_args(["--parallel", "pp"]).height, bench.parse_args([]).height) == (480, 224)


def test_dump_and_full_options_leave_the_plain_run_as_it_was():
    plain = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert plain.dump_outputs is None and plain.full is False and (plain.steps, plain.warmup) == (7, 3)
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3", "--dump-outputs", "out", "--full"])
    assert a.dump_outputs == "out" and a.full is True
    for k, v in vars(plain).items():           # the two options change nothing else about the run
        if k not in ("dump_outputs", "full"):
            assert getattr(a, k) == v, k


def test_dump_outputs_writes_float_arrays_within_the_size_limit(tmp_path, monkeypatch):
    import numpy as np
    import torch
    g = torch.Generator().manual_seed(0)
    result = {"top_prob": torch.rand(6, 5, generator=g), "top_index": torch.arange(30, dtype=torch.int32).view(6, 5),
              "stamp": torch.tensor([2 ** 40 + 1]), "text": "not an array"}
    written = bench.dump_outputs(str(tmp_path / "a"), result)
    assert written == {"top_prob": [6, 5], "top_index": [6, 5], "stamp": [1]}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["stamp.npy", "top_index.npy", "top_prob.npy"]
    prob, index, stamp = (np.load(tmp_path / "a" / f"{n}.npy") for n in ("top_prob", "top_index", "stamp"))
    assert prob.dtype == np.float32 and np.array_equal(prob, result["top_prob"].numpy())
    assert index.dtype == np.float32 and np.array_equal(index, np.arange(30).reshape(6, 5))
    assert stamp.dtype == np.float64 and stamp[0] == 2 ** 40 + 1      # int64 goes to float64: exact up to 2^53
    # past the limit every array is cut to its share: a fixed sample, the same in every run
    monkeypatch.setattr(bench, "DUMP_LIMIT", 400)
    big = {"x": torch.arange(1000, dtype=torch.float32), "y": torch.arange(200, dtype=torch.float32)}
    w1 = bench.dump_outputs(str(tmp_path / "b"), big)
    w2 = bench.dump_outputs(str(tmp_path / "c"), big)
    assert w1 == w2
    total = 0
    for n in ("x", "y"):
        s1, s2 = np.load(tmp_path / "b" / f"{n}.npy"), np.load(tmp_path / "c" / f"{n}.npy")
        assert np.array_equal(s1, s2) and 0 < s1.size < big[n].numel()
        assert np.all(np.diff(s1) > 0)                                 # sorted flat indices, no repeats
        total += s1.nbytes
    assert total <= 400
