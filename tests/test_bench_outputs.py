"""bench.py's plain run and ``--dump-outputs``: a plain run times the C2 headline alone and can write
what its last timed step returned; the other legs belong to ``--full``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "LOCAL_RANK", "RANK", "MASTER_ADDR", "MASTER_PORT", "GR_BENCH_DEVICE"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env,
                          capture_output=True, text=True, timeout=240)


def test_dump_outputs_float64_and_seeded_sample(tmp_path):
    import torch

    import bench
    idx = torch.arange(3000, dtype=torch.int64).reshape(1000, 3)
    bench.dump_outputs(str(tmp_path / "all"), {"idx": idx}, 0)
    v = np.load(tmp_path / "all" / "idx.npy")
    assert v.dtype == np.float64 and np.array_equal(v, idx.numpy())
    # over the budget: the same sorted sample of whole rows on every call, within the budget
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"idx": idx, "vec": idx[:, 0]}, 1, budget=4800)
    s1 = np.load(tmp_path / "s1" / "idx.rank1.npy")
    assert s1.shape == (100, 3) and np.array_equal(s1, np.load(tmp_path / "s2" / "idx.rank1.npy"))
    assert np.all(np.diff(s1[:, 0]) > 0) and np.array_equal(s1[:, 1], s1[:, 0] + 1)
    assert np.load(tmp_path / "s1" / "vec.rank1.npy").shape == (300, 1)
    assert sum(os.path.getsize(tmp_path / "s1" / f) - 128 for f in os.listdir(tmp_path / "s1")) <= 4800


def test_legs_need_full():
    p = _bench("--legs", "sasrec")
    assert p.returncode != 0 and "--full" in p.stderr and not p.stdout.strip()


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_its_last_step(dev, tmp_path):
    import torch
    from gr_amd import synth
    n = 5000   # small, and no multiple of the encoder's row tile
    p = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--rq-items", str(n), "--spinup-s", "0",
               "--dump-outputs", str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = lines[0]
    assert line["steps"] == 3 and line["unit"] == "items/s" and line["higher_is_better"] and line["dtype"] == "f32"
    assert line["value"] == pytest.approx(n / (line["ms_per_step"] * 1e-3), rel=1e-9)
    # no other leg, no CPU baseline, no per-kernel figures
    assert not {"sasrec", "rq_c4", "sasrec_c5", "calls", "ref_eval", "roofline", "cpu_baseline"} & set(line)
    assert os.listdir(tmp_path) == ["rq_c2_indices.npy"]
    got = np.load(tmp_path / "rq_c2_indices.npy")
    ref = synth.rqvae_model(3, 256, dev).get_indices(synth.items(n, 1000, dev))
    assert got.dtype == np.float64 and np.array_equal(got, ref.cpu().numpy())
    assert ref.dtype == torch.int64
