"""Best-of-N evaluation protocol (utils/evaluation.py) and the CPU path of
ops.frame_metrics.

`best_of_n` is checked on hand-made (S=3, T=5, B=2) scores built from exact
binary fractions, so every expected value below is worked out by hand and a
tie is a tie in fp32 too.
"""
import dataclasses
import random

import numpy as np
import pytest
import torch

from p2pvg_amd import data as data_utils
from p2pvg_amd import ops
from p2pvg_amd.models import P2PModel
from p2pvg_amd.utils import metrics
from p2pvg_amd.utils.evaluation import best_of_n, evaluate_model, score_samples

N_PAST = 2


def _hand_scores():
    """(S=3, T=5, B=2). Rows below are frames 2..4 per (sample, sequence)."""
    ssim = torch.zeros(3, 5, 2)
    psnr = torch.zeros(3, 5, 2)
    # sequence 0: SSIM picks sample 1 (mean .75), PSNR picks sample 2
    ssim[0, 2:, 0] = torch.tensor([0.5, 0.5, 0.5])
    ssim[1, 2:, 0] = torch.tensor([0.875, 0.625, 0.75])
    ssim[2, 2:, 0] = torch.tensor([0.125, 0.25, 0.875])
    psnr[0, 2:, 0] = torch.tensor([20.0, 20.0, 20.0])
    psnr[1, 2:, 0] = torch.tensor([10.0, 10.0, 10.0])
    psnr[2, 2:, 0] = torch.tensor([30.0, 32.0, 34.0])
    # sequence 1: SSIM samples 0 and 2 tie (sum 1.5) -> sample 0; PSNR picks 1
    ssim[0, 2:, 1] = torch.tensor([0.5, 0.5, 0.5])
    ssim[1, 2:, 1] = torch.tensor([0.25, 0.25, 0.25])
    ssim[2, 2:, 1] = torch.tensor([0.25, 0.5, 0.75])
    psnr[0, 2:, 1] = torch.tensor([16.0, 16.0, 16.0])
    psnr[1, 2:, 1] = torch.tensor([24.0, 26.0, 28.0])
    psnr[2, 2:, 1] = torch.tensor([20.0, 20.0, 20.0])
    # frames before n_past: extreme values that would flip every choice
    ssim[2, :2] = 100.0
    ssim[0, :2] = -100.0
    ssim[1, :2] = -100.0
    psnr[0, :2] = 1000.0
    psnr[1, :2, 1] = -1000.0
    return ssim, psnr


def test_best_of_n_by_hand():
    ssim, psnr = _hand_scores()
    r = best_of_n(ssim, psnr, N_PAST)
    close = lambda a, b: torch.testing.assert_close(  # noqa: E731
        a, torch.tensor(b, dtype=torch.float32), rtol=0, atol=1e-6)
    # each metric picks its own best sample per sequence
    close(r["ssim_best"], [(0.875 + 0.5) / 2, (0.625 + 0.5) / 2, (0.75 + 0.5) / 2])
    close(r["psnr_best"], [(30 + 24) / 2, (32 + 26) / 2, (34 + 28) / 2])
    close(r["ssim_mean"], [2.5 / 6, 2.625 / 6, 3.625 / 6])
    close(r["psnr_mean"], [120 / 6, 124 / 6, 128 / 6])
    # end frame (t = 4): max / mean over samples, then mean over sequences
    close(r["end_frame_ssim_best"], (0.875 + 0.75) / 2)
    close(r["end_frame_ssim_mean"], 3.625 / 6)
    close(r["end_frame_psnr_best"], (34 + 28) / 2)
    close(r["end_frame_psnr_mean"], 128 / 6)
    for k in ("ssim_best", "ssim_mean", "psnr_best", "psnr_mean"):
        assert r[k].shape == (5 - N_PAST,)


def test_best_of_n_tie_goes_to_lowest_index():
    ssim, psnr = _hand_scores()
    r = best_of_n(ssim, psnr, N_PAST)
    # sequence 1 alone: the tie between samples 0 and 2 resolves to sample 0,
    # whose curve is flat .5 (sample 2's is .25 .5 .75)
    one = best_of_n(ssim[:, :, 1:], psnr[:, :, 1:], N_PAST)
    assert torch.equal(one["ssim_best"], torch.tensor([0.5, 0.5, 0.5]))
    # and it stays sample 0 whatever the order of the other samples
    perm = [0, 2, 1]
    two = best_of_n(ssim[perm][:, :, 1:], psnr[perm][:, :, 1:], N_PAST)
    assert torch.equal(two["ssim_best"], torch.tensor([0.5, 0.5, 0.5]))
    # put the tying sample first and it wins instead
    perm = [2, 0, 1]
    three = best_of_n(ssim[perm][:, :, 1:], psnr[perm][:, :, 1:], N_PAST)
    assert torch.equal(three["ssim_best"], torch.tensor([0.25, 0.5, 0.75]))
    assert r["ssim_best"].shape == (3,)


def test_best_of_n_ignores_frames_before_n_past():
    ssim, psnr = _hand_scores()
    r = best_of_n(ssim, psnr, N_PAST)
    ssim0, psnr0 = ssim.clone(), psnr.clone()
    ssim0[:, :N_PAST] = 0
    psnr0[:, :N_PAST] = 0
    r0 = best_of_n(ssim0, psnr0, N_PAST)
    for k in r:
        assert torch.equal(r[k], r0[k]), k


def test_best_of_n_rejects_bad_arguments():
    ssim, psnr = _hand_scores()
    with pytest.raises(ValueError):
        best_of_n(ssim, psnr[:2], N_PAST)
    with pytest.raises(ValueError):
        best_of_n(ssim, psnr, 5)
    with pytest.raises(ValueError):
        best_of_n(ssim[0], psnr[0], 1)


def test_frame_metrics_cpu_is_utils_metrics():
    g = torch.Generator().manual_seed(3)
    a = torch.rand(3, 2, 3, 20, 24, generator=g)
    b = (a + 0.05 * torch.randn(a.shape, generator=g)).clamp(0, 1)
    ssim, mse = ops.frame_metrics(a, b)
    assert ssim.shape == mse.shape == (3, 2)
    assert ssim.dtype == mse.dtype == torch.float32
    a4, b4 = a.reshape(-1, 3, 20, 24), b.reshape(-1, 3, 20, 24)
    assert torch.equal(ssim.reshape(-1), metrics.ssim(a4, b4))
    assert torch.equal(mse.reshape(-1), metrics.mse(a4, b4))
    # data_range reaches the constants
    s255, m255 = ops.frame_metrics(a[0] * 255, b[0] * 255, data_range=255.0)
    assert torch.equal(s255, metrics.ssim(a[0] * 255, b[0] * 255, 255.0))
    assert s255.shape == (2,)
    # channels_last views and half inputs take the same path
    s_cl, _ = ops.frame_metrics(a[0].contiguous(memory_format=torch.channels_last), b[0])
    assert torch.equal(s_cl, metrics.ssim(a[0], b[0]))
    s_bf, m_bf = ops.frame_metrics(a[0].bfloat16(), b[0])
    assert s_bf.dtype == m_bf.dtype == torch.float32
    assert torch.equal(s_bf, metrics.ssim(a[0].bfloat16(), b[0]))


def test_frame_metrics_validation_and_no_autograd():
    a = torch.rand(2, 1, 8, 8)
    for bad in (
        lambda: ops.frame_metrics(a, a[:1]),
        lambda: ops.frame_metrics(a[0], a[0]),
        lambda: ops.frame_metrics(a.double(), a.double()),
        lambda: ops.frame_metrics(a, (a * 255).to(torch.uint8)),
        lambda: ops.frame_metrics(a, a, data_range=0.0),
        lambda: ops.frame_metrics(a, a, data_range=-1.0),
        lambda: ops.frame_metrics(a, a, data_range=float("nan")),
    ):
        with pytest.raises(ValueError):
            bad()
    w = a.clone().requires_grad_()
    with pytest.raises(RuntimeError):
        ops.frame_metrics(w, a)
    with torch.no_grad():
        ssim, mse = ops.frame_metrics(w, a)
    assert float(mse.max()) == 0.0 and not ssim.requires_grad


def test_frame_metrics_scores_outside_autocast():
    """Scores are fp32 whatever the caller's autocast state: under autocast the
    convolutions of utils.metrics.ssim would round to bf16 (3 digits)."""
    g = torch.Generator().manual_seed(8)
    a = torch.rand(4, 3, 24, 24, generator=g)
    b = (a + 0.05 * torch.randn(a.shape, generator=g)).clamp(0, 1)
    want_s, want_m = ops.frame_metrics(a, b)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        lossy = metrics.ssim(a, b).float()
        got_s, got_m = ops.frame_metrics(a, b)
    assert got_s.dtype == got_m.dtype == torch.float32
    assert torch.equal(got_s, want_s) and torch.equal(got_m, want_m)
    # the hazard is real on this build: the bare metric does lose digits
    assert float((lossy - want_s).abs().max()) > 1e-5


def test_frame_metrics_empty_leading_dimension():
    a = torch.rand(0, 3, 8, 8)
    ssim, mse = ops.frame_metrics(a, a)
    assert ssim.shape == mse.shape == (0,) and ssim.dtype == torch.float32
    ssim, mse = ops.frame_metrics(torch.rand(2, 0, 1, 8, 8), torch.rand(2, 0, 1, 8, 8))
    assert ssim.shape == mse.shape == (2, 0)


def test_frame_metrics_backend_on_cpu(monkeypatch):
    assert ops.frame_metrics_backend("cpu") == "torch"
    assert ops.frame_metrics_backend(torch.zeros(1)) == "torch"
    monkeypatch.setenv("P2PVG_KERNELS", "torch")
    assert ops.frame_metrics_backend(torch.device("cpu")) == "torch"


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _evaluate(cfg, seed, n_batches=2, nsample=2):
    _seed(seed)
    model = P2PModel(cfg)
    model.eval()
    _, test = data_utils.load_dataset(cfg)
    gen = data_utils.get_data_generator(test, train=False, dynamic_length=False, opt=cfg)
    return evaluate_model(model, gen, n_batches, nsample, "full")


def test_evaluate_model_two_batches(tiny_cfg):
    cfg = dataclasses.replace(tiny_cfg, num_workers=0)
    r1 = _evaluate(cfg, 5)
    assert r1["n_sequences"] == 2 * cfg.batch_size
    for k in ("ssim_best", "ssim_mean", "psnr_best", "psnr_mean"):
        assert len(r1[k]) == cfg.max_seq_len - cfg.n_past
        assert all(np.isfinite(v) for v in r1[k])
    for k in ("end_frame_ssim_best", "end_frame_ssim_mean",
              "end_frame_psnr_best", "end_frame_psnr_mean"):
        assert isinstance(r1[k], float) and np.isfinite(r1[k])
    # best-of-N can only improve on the mean, and the end frame closes the curve
    assert all(b >= m - 1e-6 for b, m in zip(r1["ssim_best"], r1["ssim_mean"]))
    assert r1["end_frame_ssim_best"] >= r1["end_frame_ssim_mean"] - 1e-6
    assert r1["end_frame_ssim_mean"] == pytest.approx(r1["ssim_mean"][-1], abs=1e-6)
    assert r1["seconds_generate"] > 0 and r1["seconds_score"] > 0
    # the same seed gives identical numbers
    r2 = _evaluate(cfg, 5)
    timing = ("seconds_generate", "seconds_score")
    assert {k: v for k, v in r1.items() if k not in timing} == \
        {k: v for k, v in r2.items() if k not in timing}


def test_score_samples_shapes_and_gt_frames(tiny_cfg):
    _seed(2)
    model = P2PModel(tiny_cfg)
    model.eval()
    x = torch.rand(tiny_cfg.max_seq_len, tiny_cfg.batch_size, 1, 64, 64)
    ssim, psnr = score_samples(model, x, 3)
    assert ssim.shape == psnr.shape == (3, tiny_cfg.max_seq_len, tiny_cfg.batch_size)
    assert ssim.dtype == psnr.dtype == torch.float32
    # frame 0 is a ground-truth copy: mse 0 -> SSIM 1, PSNR at the clamp (120 dB)
    torch.testing.assert_close(ssim[:, 0], torch.ones(3, 2), rtol=0, atol=1e-5)
    torch.testing.assert_close(psnr[:, 0], torch.full((3, 2), 120.0), rtol=0, atol=1e-3)
    with pytest.raises(ValueError):
        score_samples(model, x, 0)
