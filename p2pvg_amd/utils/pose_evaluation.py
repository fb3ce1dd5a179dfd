"""Best-of-N evaluation of skeleton sequences (Human3.6M).

The three axes of point-to-point generation, stated for poses: quality is the
best-of-N mean per-joint position error (MPJPE), consistency the error of the
end pose at the control point, diversity the mean pairwise distance between
the N samples of a timestep (which a point-to-point model drives towards zero
as the control point nears).

- `sample_poses`        : N samples of a batch in ceil(N / sample_chunk)
                          rollouts, the samples folded into the batch axis
                          -> (T, S, B, J, 3)
- `best_of_n_pose`      : pure tensor function, (S, T, B) scores and (T, B)
                          spread -> per-timestep curves
- `evaluate_pose_model` : accumulates `best_of_n_pose` over batches of an h36m
                          generator; scoring is ops.pose_metrics and
                          ops.pose_spread (HIP kernels on GPU)
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from .evaluation import _clock, _generation_autocast

DEFAULT_SAMPLE_CHUNK = 100


def _check_x3(x3) -> None:
    if not isinstance(x3, torch.Tensor) or x3.dim() != 4 or x3.shape[-1] != 3:
        shape = tuple(x3.shape) if isinstance(x3, torch.Tensor) else type(x3).__name__
        raise ValueError(f"x3 must be (T, B, J, 3) poses, got {shape}")
    if not x3.is_floating_point():
        raise ValueError(f"x3 must be floating point poses, got {x3.dtype}")
    if min(x3.shape) < 1:
        raise ValueError(f"x3 must not be empty, got {tuple(x3.shape)}")


@torch.no_grad()
def sample_poses(model, x3: torch.Tensor, nsample: int,
                 model_mode: str = "full",
                 sample_chunk: int = DEFAULT_SAMPLE_CHUNK,
                 amp_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """x3 (T, B, J, 3) -> nsample generated sequences, (T, S, B, J, 3) fp32.

    Samples are folded into the batch axis: per chunk of k <= sample_chunk
    samples x3 is expanded to (T, k * B, J, 3), row r = s * B + b, and ONE
    `model.p2p_generate(xk, T, T - 1, model_mode, skip_frame=False)` rollout
    generates them all; the chunk is then copied into the result. A last chunk
    smaller than sample_chunk is fine.

    Folding rests on the skeleton model being row-wise: its backbone is
    Linear + ReLU + LayerNorm (no batch statistic) and its recurrent stacks are
    per-row LSTMs, and every row draws its own noise. A folded rollout
    therefore draws from the same distribution as S separate rollouts. It does
    NOT make the same draws: the random stream is consumed in another order.
    A backbone with batch statistics (the image backbones in training mode)
    must not be folded.

    The result takes S*T*B*J*12 bytes (627 MB at S=100, T=30, B=1024, J=17).
    `amp_dtype` (torch.bfloat16) wraps generation in autocast on a GPU; the
    result is fp32 either way."""
    _check_x3(x3)
    if nsample < 1:
        raise ValueError(f"nsample must be >= 1, got {nsample}")
    if sample_chunk < 1:
        raise ValueError(f"sample_chunk must be >= 1, got {sample_chunk}")
    T, B, J, _ = x3.shape
    out = torch.empty((T, nsample, B, J, 3), dtype=torch.float32, device=x3.device)
    for s0 in range(0, nsample, sample_chunk):
        k = min(sample_chunk, nsample - s0)
        xk = x3.unsqueeze(1).expand(T, k, B, J, 3).reshape(T, k * B, J, 3)
        with _generation_autocast(x3.device, amp_dtype):
            frames = model.p2p_generate(xk, T, T - 1, model_mode=model_mode,
                                        skip_frame=False)
        for t, frame in enumerate(frames):
            out[t, s0:s0 + k] = frame.reshape(k, B, J, 3)
    return out


def _pick_lowest(metric: torch.Tensor, n_past: int) -> torch.Tensor:
    """(S, T, B) -> (T, B): per sequence, the sample with the lowest mean over
    frames n_past..T-1 (a tie goes to the lowest sample index)."""
    S, T, B = metric.shape
    score = metric[:, n_past:].mean(dim=1)                       # (S, B)
    low = score.min(dim=0, keepdim=True).values
    first = torch.arange(S, device=metric.device).unsqueeze(1).expand(S, B)
    first = first.masked_fill(score != low, S).min(dim=0).values  # (B,)
    first = first.clamp_max(S - 1)  # all-NaN column: keep it, do not index out
    return metric.gather(0, first.view(1, 1, B).expand(1, T, B))[0]


def best_of_n_pose(mpjpe: torch.Tensor, mse: torch.Tensor,
                   spread: torch.Tensor, n_past: int) -> Dict[str, torch.Tensor]:
    """Per-timestep curves over frames t in [n_past, T-1] from (S, T, B)
    errors and the (T, B) spread.

    Frames t < n_past are ground-truth copies in `p2p_generate` and excluded.
    `*_best[t]`: each error picks its own best (lowest mean) sample per
    sequence, mean over sequences; `*_mean[t]`: mean over samples and
    sequences; `spread[t]`: mean over sequences; `end_pose_mpjpe_*`: frame
    T-1 against the control point, min / mean over samples, then mean over
    sequences; `end_pose_spread`: the spread at frame T-1 (0-d tensors)."""
    if mpjpe.shape != mse.shape or mpjpe.dim() != 3:
        raise ValueError(
            f"mpjpe and mse must be equal (S, T, B), got {tuple(mpjpe.shape)} "
            f"and {tuple(mse.shape)}")
    S, T, B = mpjpe.shape
    if tuple(spread.shape) != (T, B):
        raise ValueError(
            f"spread must be (T, B) = {(T, B)}, got {tuple(spread.shape)}")
    if S < 1 or B < 1:
        raise ValueError(f"S and B must be >= 1, got S={S}, B={B}")
    if not 0 <= n_past < T:
        raise ValueError(f"0 <= n_past < T={T} required, got {n_past}")
    out = {}
    for name, m in (("mpjpe", mpjpe.float()), ("mse", mse.float())):
        out[f"{name}_best"] = _pick_lowest(m, n_past)[n_past:].mean(dim=1)
        out[f"{name}_mean"] = m[:, n_past:].mean(dim=(0, 2))
    spread = spread.float()
    out["spread"] = spread[n_past:].mean(dim=1)
    m = mpjpe.float()
    out["end_pose_mpjpe_best"] = m[:, T - 1].min(dim=0).values.mean()
    out["end_pose_mpjpe_mean"] = m[:, T - 1].mean()
    out["end_pose_spread"] = spread[T - 1].mean()
    return out


CURVE_KEYS = ("mpjpe_best", "mpjpe_mean", "mse_best", "mse_mean", "spread")
SCALAR_KEYS = ("end_pose_mpjpe_best", "end_pose_mpjpe_mean", "end_pose_spread")
_KEYS = CURVE_KEYS + SCALAR_KEYS


@torch.no_grad()
def evaluate_pose_model(model, generator, n_batches: int, nsample: int,
                        model_mode: str = "full",
                        sample_chunk: int = DEFAULT_SAMPLE_CHUNK,
                        axis_scale: Optional[Sequence[float]] = None,
                        amp_dtype: Optional[torch.dtype] = None) -> dict:
    """Best-of-N pose curves over `n_batches` batches of an h36m `generator`
    (which yields (pose_2d, pose_3d, camera_view); a bare (T, B, J, 3) tensor
    is taken as pose_3d), every batch weighted by its sequence count: lists of
    floats for the curves, floats for the end-pose values, plus n_sequences /
    seconds_generate / seconds_score (read behind a device synchronise). One
    DtoH copy per batch. `axis_scale` puts the errors into other units (the
    dataset's `pose_scale_3d`); `nsample` >= 2, the spread needs a pair."""
    from ..ops import pose_metrics, pose_spread

    if n_batches < 1:
        raise ValueError(f"n_batches must be >= 1, got {n_batches}")
    if nsample < 2:
        raise ValueError(f"nsample must be >= 2 (the spread needs a pair), got {nsample}")
    n_past = model.cfg.n_past
    sums, sizes, n_seq = None, None, 0
    seconds = [0.0, 0.0]
    for _ in range(n_batches):
        batch = next(generator)
        x3 = batch[1] if isinstance(batch, (tuple, list)) else batch
        _check_x3(x3)
        B = x3.shape[1]
        t0 = _clock(x3.device)
        gen = sample_poses(model, x3, nsample, model_mode, sample_chunk, amp_dtype)
        t1 = _clock(x3.device)
        mpjpe, mse = pose_metrics(gen, x3, axis_scale)
        spread = pose_spread(gen, axis_scale)
        res = best_of_n_pose(mpjpe, mse, spread, n_past)
        flat = torch.cat([res[k].reshape(-1) for k in _KEYS]).double().cpu()
        seconds[0] += t1 - t0
        seconds[1] += _clock(x3.device) - t1
        del gen
        if sums is None:
            sums = torch.zeros_like(flat)
            sizes = [res[k].numel() for k in _KEYS]
        elif flat.numel() != sums.numel():
            raise ValueError("the batches of one evaluation must have one length")
        sums += flat * B
        n_seq += B
    out = {}
    for k, v in zip(_KEYS, (sums / n_seq).split(sizes)):
        out[k] = float(v[0]) if k in SCALAR_KEYS else v.tolist()
    out["n_sequences"] = n_seq
    out["seconds_generate"], out["seconds_score"] = seconds
    return out
