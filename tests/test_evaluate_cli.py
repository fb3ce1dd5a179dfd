"""evaluate.py end to end on the CPU: a checkpoint saved in-process, the CLI
run as a subprocess, the JSON it writes."""
import json
import math
import os
import subprocess
import sys

import torch

from p2pvg_amd.models import P2PModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMING = ("seconds_generate", "seconds_score")
CURVES = ("ssim_best", "ssim_mean", "psnr_best", "psnr_mean")
SCALARS = ("end_frame_ssim_best", "end_frame_ssim_mean",
           "end_frame_psnr_best", "end_frame_psnr_mean")
META = ("dataset", "ckpt", "model_mode", "nsample", "n_past", "seq_len",
        "kernel_backend", "data_synthetic", "n_sequences") + TIMING


def _run(ckpt, out, *extra):
    env = os.environ.copy()
    env["PYTHONPATH"] = ROOT
    return subprocess.run(
        [sys.executable, os.path.join(ROOT, "evaluate.py"), "--ckpt", str(ckpt),
         "--device", "cpu", "--nsample", "3", "--n_batches", "1",
         "--out", str(out), *extra],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
    )


def test_evaluate_cli_json_and_determinism(tiny_cfg, tmp_path):
    tiny_cfg.num_workers = 0
    torch.manual_seed(0)
    ckpt = tmp_path / "model.pth"
    P2PModel(tiny_cfg).save(str(ckpt), 0)

    out1, out2 = tmp_path / "a.json", tmp_path / "b.json"
    r = _run(ckpt, out1, "--seed", "7")
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(out1.read_text())

    for k in CURVES + SCALARS + META:
        assert k in res, k
    T, n_past = tiny_cfg.max_seq_len, tiny_cfg.n_past
    for k in CURVES:
        assert len(res[k]) == T - n_past, k
        assert all(math.isfinite(v) for v in res[k]), k
    for k in SCALARS:
        assert math.isfinite(res[k]), k
    for k in ("ssim_best", "ssim_mean"):
        assert all(-1.0 <= v <= 1.0 for v in res[k]), k
    assert -1.0 <= res["end_frame_ssim_mean"] <= res["end_frame_ssim_best"] <= 1.0
    assert res["dataset"] == "mnist" and res["ckpt"] == str(ckpt)
    assert res["model_mode"] == "full" and res["nsample"] == 3
    assert res["n_past"] == n_past and res["seq_len"] == T
    assert res["n_sequences"] == tiny_cfg.batch_size
    assert res["kernel_backend"] == "torch"  # --device cpu
    assert res["data_synthetic"] is True     # data_root does not exist
    # one line per metric on stdout
    for k in CURVES + SCALARS:
        assert f"{k}: " in r.stdout, k

    # same seed -> the same file, apart from the timing fields
    r2 = _run(ckpt, out2, "--seed", "7")
    assert r2.returncode == 0, r2.stderr[-3000:]
    res2 = json.loads(out2.read_text())
    strip = lambda d: {k: v for k, v in d.items() if k not in TIMING}  # noqa: E731
    assert strip(res) == strip(res2)


def test_evaluate_cli_rejects_h36m(tiny_cfg, tmp_path):
    torch.manual_seed(0)
    states = P2PModel(tiny_cfg).state_for_checkpoint(0)
    states["opt"]["dataset"] = "h36m"
    ckpt = tmp_path / "h36m.pth"
    torch.save(states, str(ckpt))
    out = tmp_path / "c.json"
    r = _run(ckpt, out)
    assert r.returncode != 0
    assert "h36m" in r.stderr and "poses" in r.stderr
    assert not out.exists()
