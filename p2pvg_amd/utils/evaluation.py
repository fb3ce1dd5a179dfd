"""Best-of-N SSIM/PSNR evaluation (the stochastic video prediction protocol).

For every test sequence draw N samples, score every generated frame against
the ground truth, keep the best sample per sequence and report per-timestep
curves (SVG, Denton & Fergus 2018; the reference descends from it). Point to
point generation adds the end-frame score at the control point.

- `score_samples`  : N x `p2p_generate`, each scored by ONE ops.frame_metrics
                     call (fused HIP SSIM+MSE on GPU) -> (S, T, B) tensors
- `best_of_n`      : pure tensor function, (S, T, B) -> per-timestep curves
- `evaluate_model` : accumulates `best_of_n` over batches of a generator
"""
from __future__ import annotations

import contextlib
import time
from typing import Dict, Optional, Tuple

import torch


def _psnr_from_mse(mse: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    # the formula of utils.metrics.psnr
    return 10.0 * torch.log10(data_range**2 / mse.clamp_min(1e-12))


def _clock(device) -> float:
    if getattr(device, "type", str(device)).startswith("cuda"):
        torch.cuda.synchronize(device)
    return time.perf_counter()


def _generation_autocast(device, amp_dtype):
    if amp_dtype is None or not getattr(device, "type", str(device)).startswith("cuda"):
        return contextlib.nullcontext()
    return torch.autocast("cuda", dtype=amp_dtype)


@torch.no_grad()
def _score(model, x, nsample, model_mode, data_range, seconds=None,
           amp_dtype=None):
    """The sampling loop; `seconds` = [generate, score] is advanced when given
    (the clock is read behind a device synchronise). `amp_dtype` puts
    GENERATION under autocast on a GPU; scoring is always outside it."""
    from ..ops import frame_metrics

    if nsample < 1:
        raise ValueError(f"nsample must be >= 1, got {nsample}")
    T = len(x)
    ssim = torch.empty((nsample, T, x.shape[1]), dtype=torch.float32,
                       device=x.device)
    psnr = torch.empty_like(ssim)
    for s in range(nsample):
        t0 = _clock(x.device) if seconds is not None else 0.0
        with _generation_autocast(x.device, amp_dtype):
            gen = torch.stack(model.p2p_generate(
                x, T, T - 1, model_mode=model_mode, skip_frame=False))
        t1 = _clock(x.device) if seconds is not None else 0.0
        ssim[s], mse = frame_metrics(gen, x, data_range)
        psnr[s] = _psnr_from_mse(mse, data_range)
        if seconds is not None:
            seconds[0] += t1 - t0
            seconds[1] += _clock(x.device) - t1
    return ssim, psnr


def score_samples(model, x: torch.Tensor, nsample: int,
                  model_mode: str = "full", data_range: float = 1.0,
                  amp_dtype: Optional[torch.dtype] = None,
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """x (T, B, C, H, W) -> (ssim, psnr), each (S, T, B) fp32 on x.device.

    Each sample is `torch.stack(model.p2p_generate(x, T, T - 1, ...))` scored
    against x by ONE ops.frame_metrics call. Samples are generated and scored
    one at a time: memory does not grow with `nsample`. `amp_dtype`
    (torch.bfloat16) wraps generation, and only generation, in autocast on a
    GPU; the scores are fp32 either way."""
    return _score(model, x, nsample, model_mode, data_range, None, amp_dtype)


def _pick_best(metric: torch.Tensor, n_past: int) -> torch.Tensor:
    """(S, T, B) -> (T, B): per sequence, the sample with the highest mean
    over frames n_past..T-1 (a tie goes to the lowest sample index)."""
    S, T, B = metric.shape
    score = metric[:, n_past:].mean(dim=1)                      # (S, B)
    top = score.max(dim=0, keepdim=True).values
    first = torch.arange(S, device=metric.device).unsqueeze(1).expand(S, B)
    first = first.masked_fill(score != top, S).min(dim=0).values  # (B,)
    first = first.clamp_max(S - 1)  # all-NaN column: keep it, do not index out
    return metric.gather(0, first.view(1, 1, B).expand(1, T, B))[0]


def best_of_n(ssim: torch.Tensor, psnr: torch.Tensor, n_past: int) -> Dict[str, torch.Tensor]:
    """Per-timestep curves over frames t in [n_past, T-1] from (S, T, B) scores.

    Frames t < n_past are ground-truth copies in `p2p_generate` and excluded.
    `*_best[t]`: each metric picks its own best sample per sequence, mean over
    sequences; `*_mean[t]`: mean over samples and sequences;
    `end_frame_*`: frame T-1 against the control point, max / mean over
    samples, then mean over sequences (0-d tensors)."""
    if ssim.shape != psnr.shape or ssim.dim() != 3:
        raise ValueError(
            f"ssim and psnr must be equal (S, T, B), got {tuple(ssim.shape)} "
            f"and {tuple(psnr.shape)}")
    T = ssim.shape[1]
    if not 0 <= n_past < T:
        raise ValueError(f"0 <= n_past < T={T} required, got {n_past}")
    out = {}
    for name, m in (("ssim", ssim.float()), ("psnr", psnr.float())):
        out[f"{name}_best"] = _pick_best(m, n_past)[n_past:].mean(dim=1)
        out[f"{name}_mean"] = m[:, n_past:].mean(dim=(0, 2))
        out[f"end_frame_{name}_best"] = m[:, T - 1].max(dim=0).values.mean()
        out[f"end_frame_{name}_mean"] = m[:, T - 1].mean()
    return out


_KEYS = tuple(f"{m}_{k}" for m in ("ssim", "psnr") for k in ("best", "mean")) + tuple(
    f"end_frame_{m}_{k}" for m in ("ssim", "psnr") for k in ("best", "mean"))


@torch.no_grad()
def evaluate_model(model, generator, n_batches: int, nsample: int,
                   model_mode: str = "full",
                   amp_dtype: Optional[torch.dtype] = None) -> dict:
    """Best-of-N curves over `n_batches` batches of `generator`, every batch
    weighted by its sequence count: lists of floats for the curves, floats for
    the end-frame values, plus n_sequences / seconds_generate / seconds_score.
    One DtoH copy per batch. `amp_dtype` (torch.bfloat16) wraps generation,
    and only generation, in autocast on a GPU; scores are fp32 either way."""
    if n_batches < 1:
        raise ValueError(f"n_batches must be >= 1, got {n_batches}")
    n_past = model.cfg.n_past
    sums, sizes, n_seq = None, None, 0
    seconds = [0.0, 0.0]
    for _ in range(n_batches):
        x = next(generator)
        B = x.shape[1]
        ssim, psnr = _score(model, x, nsample, model_mode, 1.0, seconds,
                            amp_dtype)
        res = best_of_n(ssim, psnr, n_past)
        flat = torch.cat([res[k].reshape(-1) for k in _KEYS]).double().cpu()
        if sums is None:
            sums = torch.zeros_like(flat)
            sizes = [res[k].numel() for k in _KEYS]
        elif flat.numel() != sums.numel():
            raise ValueError("the batches of one evaluation must have one length")
        sums += flat * B
        n_seq += B
    out = {}
    for k, v in zip(_KEYS, (sums / n_seq).split(sizes)):
        out[k] = float(v[0]) if k.startswith("end_frame") else v.tolist()
    out["n_sequences"] = n_seq
    out["seconds_generate"], out["seconds_score"] = seconds
    return out
