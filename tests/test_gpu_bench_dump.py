"""``bench.py --dump-outputs``: a plain one-GPU run writes what its last timed step returned to
the caller (the top-5 of every frame of the batch), equal arguments give equal dumps, and the
dump is the result of the last timed frame and of no other.

The runs here switch the tile tuner off (``AIKO_GPU_AUTOTUNE=false``: tiles come from the
geometry alone), so two runs launch the same kernels and equal inputs must give equal bits; with
the tuner on, a timing tie may pick another tile and move the last bits of a bf16 sum."""
import json
import os
import queue
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
BATCH, STEPS, WARMUP = 24, 3, 1


def _bench(out_dir):
    env = dict(os.environ, AIKO_GPU_AUTOTUNE="false")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--batch", str(BATCH), "--dump-outputs", str(out_dir)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """One bench run shared by the tests below: (result line, directory of its dump)."""
    out_dir = tmp_path_factory.mktemp("bench") / "outputs"
    return _bench(out_dir), out_dir


def test_bench_dumps_the_last_timed_steps_outputs(dumped):
    res, out_dir = dumped
    assert res["steps"] == STEPS and res["warmup"] == WARMUP and res["unit"] == "frames/s" and res["dtype"] == "bf16"
    assert res["ms_per_step"] > 0 and res["higher_is_better"] is True
    # value and ms_per_step describe the same timed region (both rounded in the result line)
    assert res["value"] == pytest.approx(BATCH / (res["ms_per_step"] * 1e-3), rel=1e-2)
    assert res["outputs"] == {"top_index": [BATCH, 5], "top_prob": [BATCH, 5]}
    assert sorted(p.name for p in out_dir.iterdir()) == ["top_index.npy", "top_prob.npy"]
    prob, index = np.load(out_dir / "top_prob.npy"), np.load(out_dir / "top_index.npy")
    assert prob.dtype == np.float32 and index.dtype == np.float32
    assert prob.shape == index.shape == (BATCH, 5)
    assert np.isfinite(prob).all() and (prob > 0).all() and (prob.sum(1) <= 1 + 1e-3).all()
    assert (np.diff(prob, axis=1) <= 0).all()                          # best class first
    assert np.array_equal(index, np.round(index)) and index.min() >= 0 and index.max() < 1000
    assert all(len(set(row)) == 5 for row in index.tolist())           # five different classes


def test_equal_arguments_give_equal_dumps(dumped, tmp_path):
    _, first = dumped
    _bench(tmp_path / "again")
    for name in ("top_prob.npy", "top_index.npy"):
        assert np.array_equal(np.load(first / name), np.load(tmp_path / "again" / name)), name


def test_dump_is_the_last_timed_frame(dumped, native):
    """The bench pipeline run directly, frame by frame: the dump equals the result of frame
    SETUP_FRAMES + W + K - 1 (frames count from 0), and differs from the frame before it, which
    was served from another pool slot (other pixels)."""
    import bench
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    _, out_dir = dumped
    a = bench.parse_args(["--gpus", "1", "--batch", str(BATCH)])
    d = bench.definition(a.batch, not a.no_graph, a.height, a.width, a.lanes)
    d["elements"][1]["parameters"]["autotune"] = False
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<dump>", parse_pipeline_definition_dict(d), None, None, "dump", [], 0, None,
                                     600, queue_response=q)
    last = bench.SETUP_FRAMES + WARMUP + STEPS - 1
    results = {}
    for fid in range(last + 1):
        p.process_frame({"stream_id": "dump", "frame_id": fid}, {})
        info, out = q.get_nowait()
        assert info["state"] == 0, (info, out)
        t = out["topk"].wait()
        if fid >= last - 1:
            results[fid] = (t["top_prob"].clone().numpy(), t["top_index"].float().numpy())
    torch.cuda.synchronize()
    prob, index = np.load(out_dir / "top_prob.npy"), np.load(out_dir / "top_index.npy")
    assert np.array_equal(prob, results[last][0]) and np.array_equal(index, results[last][1])
    assert not np.array_equal(prob, results[last - 1][0])
