"""evaluate_pose.py end to end on the CPU: an h36m checkpoint saved in-process,
the CLI run as a subprocess on the synthetic fallback poses, the JSON it
writes."""
import json
import math
import os
import subprocess
import sys

import torch

from p2pvg_amd.core import Config
from p2pvg_amd.models import P2PModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMING = ("seconds_generate", "seconds_score")
CURVES = ("mpjpe_best", "mpjpe_mean", "mse_best", "mse_mean", "spread")
SCALARS = ("end_pose_mpjpe_best", "end_pose_mpjpe_mean", "end_pose_spread")
META = ("unit", "pose_scale", "dataset", "data_synthetic", "nsample",
        "sample_chunk", "n_past", "seq_len", "n_sequences", "seed", "dtype",
        "device", "kernel_backend") + TIMING
SEQ_LEN = 30  # load_dataset fixes the h36m sequence length


def _run(script, ckpt, out, *extra):
    env = os.environ.copy()
    env["PYTHONPATH"] = ROOT
    return subprocess.run(
        [sys.executable, os.path.join(ROOT, script), "--ckpt", str(ckpt),
         "--device", "cpu", "--nsample", "5", "--n_batches", "1",
         "--out", str(out), *extra],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
    )


def test_evaluate_pose_cli_json_and_determinism(tmp_path):
    cfg = Config(dataset="h36m", backbone="mlp", batch_size=2, max_seq_len=30,
                 delta_len=1, n_past=2, g_dim=32, z_dim=4, rnn_size=32,
                 device="cpu", num_workers=0, data_root="/nonexistent")
    torch.manual_seed(0)
    ckpt = tmp_path / "pose.pth"
    P2PModel(cfg).save(str(ckpt), 0)

    out1, out2 = tmp_path / "a.json", tmp_path / "b.json"
    args = ("--sample_chunk", "2", "--batch_size", "3", "--seed", "7")
    r = _run("evaluate_pose.py", ckpt, out1, *args)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(out1.read_text())

    for k in CURVES + SCALARS + META:
        assert k in res, k
    for k in CURVES:
        assert len(res[k]) == SEQ_LEN - cfg.n_past, k
        assert all(math.isfinite(v) and v >= 0 for v in res[k]), k
    for k in SCALARS:
        assert math.isfinite(res[k]) and res[k] >= 0, k
    assert res["end_pose_mpjpe_best"] <= res["end_pose_mpjpe_mean"]
    # the best sample is picked by its mean over the frames, not per frame
    assert sum(res["mpjpe_best"]) <= sum(res["mpjpe_mean"])
    assert sum(res["mse_best"]) <= sum(res["mse_mean"])
    assert res["dataset"] == "h36m" and res["data_synthetic"] is True
    assert res["unit"] == "standardized" and res["pose_scale"] == [1.0, 1.0, 1.0]
    assert res["nsample"] == 5 and res["sample_chunk"] == 2
    assert res["n_past"] == cfg.n_past and res["seq_len"] == SEQ_LEN
    assert res["n_sequences"] == 3  # --batch_size really sets it
    assert res["seed"] == 7 and res["dtype"] == "fp32" and res["device"] == "cpu"
    assert res["kernel_backend"] == "torch"
    for k in CURVES + SCALARS:  # one line per metric on stdout
        assert f"{k}: " in r.stdout, k

    # same seed -> the same file, apart from the timing fields
    r2 = _run("evaluate_pose.py", ckpt, out2, *args)
    assert r2.returncode == 0, r2.stderr[-3000:]
    res2 = json.loads(out2.read_text())
    strip = lambda d: {k: v for k, v in d.items() if k not in TIMING}  # noqa: E731
    assert strip(res) == strip(res2)

    # evaluate.py points an h36m checkpoint here
    out3 = tmp_path / "c.json"
    r3 = _run("evaluate.py", ckpt, out3)
    assert r3.returncode != 0 and "evaluate_pose.py" in r3.stderr
    assert not out3.exists()


def test_evaluate_pose_cli_rejects_image_checkpoint(tiny_cfg, tmp_path):
    torch.manual_seed(0)
    ckpt = tmp_path / "mnist.pth"
    P2PModel(tiny_cfg).save(str(ckpt), 0)
    out = tmp_path / "d.json"
    r = _run("evaluate_pose.py", ckpt, out)
    assert r.returncode == 2
    assert "evaluate.py" in r.stderr and "mnist" in r.stderr
    assert not out.exists()
