"""Pose scores for best-of-N evaluation of skeleton sequences (K20).

`gen` (T, S, B, J, 3) holds S generated samples per sequence, `ref`
(T, B, J, 3) the ground truth, `axis_scale` = (w0, w1, w2) positive per-axis
scales (None: ones). Operands are converted to fp32 exactly; a difference is
formed first, in fp32, and scaled afterwards:

    d             = f32(gen[t,s,b,j,:]) - f32(ref[t,b,j,:])
    mpjpe[s,t,b]  = (1/J)  sum_j sqrt(sum_a (w_a * d_a)^2)
    mse[s,t,b]    = (1/3J) sum_{j,a} d_a^2        (unscaled: the training loss)
    spread[t,b]   = 2/(S(S-1)J) sum_{i<j} sum_joint
                    sqrt(sum_a (w_a * (gen_i - gen_j)_a)^2)

`pose_metrics(gen, ref, axis_scale)` returns (mpjpe, mse), both (S, T, B) fp32;
`pose_spread(gen, axis_scale)` returns (T, B) fp32 and needs S >= 2.

Arguments are validated BEFORE anything is launched (ValueError on any
violation). On a GPU the HIP kernels (csrc/pose_metrics.hip) read the operands
once, fp32 / bf16 / fp16 per operand; non-contiguous operands are made
contiguous first. `pose_spread` stages the S samples of a frame in LDS, which
bounds S * J by SPREAD_MAX_SJ on that path. On CPU - and on any device under
P2PVG_KERNELS=torch - plain torch ops compute the same definitions, one sample
(for spread: one sample against the later ones) at a time so that memory stays
bounded; that path has no S limit and is what the kernels are tested against.

Evaluation ops: there is no backward.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

SPREAD_MAX_SJ = 4096  # csrc/pose_metrics.hip: the S * J its LDS budget holds
_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _axis_scale(axis_scale) -> Tuple[float, float, float]:
    if axis_scale is None:
        return (1.0, 1.0, 1.0)
    if isinstance(axis_scale, torch.Tensor):
        raise ValueError(
            "axis_scale must be three host floats, not a tensor (it is passed "
            "to the kernel by value)")
    try:
        w = tuple(float(v) for v in axis_scale)
    except (TypeError, ValueError):
        w = ()
    if len(w) != 3 or not all(math.isfinite(v) and v > 0 for v in w):
        raise ValueError(
            f"axis_scale must be None or three finite numbers > 0, got {axis_scale!r}")
    return w


def _check_poses(name: str, t, rank: int, layout: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if t.dtype not in _DTYPES:
        raise ValueError(f"{name} must be fp32, bf16 or fp16, got {t.dtype}")
    if t.dim() != rank or t.shape[-1] != 3:
        raise ValueError(f"{name} must be {layout}, got {tuple(t.shape)}")
    if t.shape[-2] < 1:
        raise ValueError(f"{name} needs at least one joint, got {tuple(t.shape)}")


def _no_grad_needed(op: str, *tensors) -> None:
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError(
            f"{op} is an evaluation op without a backward: call it under "
            "torch.no_grad() or detach its inputs")


def _lengths(d: torch.Tensor, w: Tuple[float, float, float]) -> torch.Tensor:
    """(..., 3) fp32 differences -> (...) scaled lengths."""
    s = d * d.new_tensor(w)
    return (s * s).sum(dim=-1).sqrt()


def _torch_metrics(gen, ref, w):
    T, S, B, J, _ = gen.shape
    mpjpe = torch.empty((S, T, B), dtype=torch.float32, device=gen.device)
    mse = torch.empty_like(mpjpe)
    with torch.autocast(gen.device.type, enabled=False):
        r = ref.float()
        for s in range(S):
            d = gen[:, s].float() - r                       # (T, B, J, 3)
            mpjpe[s] = _lengths(d, w).sum(dim=-1) / J
            mse[s] = (d * d).sum(dim=(-2, -1)) / (3 * J)
    return mpjpe, mse


def _torch_spread(gen, w):
    T, S, B, J, _ = gen.shape
    total = torch.zeros((T, B), dtype=torch.float32, device=gen.device)
    with torch.autocast(gen.device.type, enabled=False):
        for i in range(S - 1):
            # sample i against samples i+1 .. S-1: every unordered pair once
            d = gen[:, i + 1:].float() - gen[:, i:i + 1].float()
            total += _lengths(d, w).sum(dim=(1, 3))
    return total / (S * (S - 1) // 2 * J)


def pose_metrics_backend(where) -> str:
    """The path `pose_metrics` and `pose_spread` take for a tensor, or for
    tensors on a device: "hip" (the kernels) or "torch". The ops dispatch on
    this very answer; like them, this raises on a GPU whose extension is
    missing."""
    from . import _want_hip

    t = where if isinstance(where, torch.Tensor) else torch.empty(0, device=where)
    return "hip" if _want_hip(t) else "torch"


def pose_metrics(gen: torch.Tensor, ref: torch.Tensor,
                 axis_scale: Optional[Sequence[float]] = None,
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """gen (T, S, B, J, 3), ref (T, B, J, 3) -> (mpjpe, mse), (S, T, B) fp32."""
    from . import _load_hip_ext

    _check_poses("gen", gen, 5, "(T, S, B, J, 3)")
    _check_poses("ref", ref, 4, "(T, B, J, 3)")
    T, S, B, J, _ = gen.shape
    if tuple(ref.shape) != (T, B, J, 3):
        raise ValueError(
            f"gen {tuple(gen.shape)} and ref {tuple(ref.shape)} must agree in "
            "T, B and J")
    if gen.device != ref.device:
        raise ValueError(
            f"gen and ref must be on one device, got {gen.device} and {ref.device}")
    w = _axis_scale(axis_scale)
    _no_grad_needed("pose_metrics", gen, ref)
    if T * S * B == 0:  # an empty leading dimension: nothing to score
        empty = torch.empty((S, T, B), dtype=torch.float32, device=gen.device)
        return empty, empty.clone()
    gen, ref = gen.detach().contiguous(), ref.detach().contiguous()
    if pose_metrics_backend(gen) == "torch":
        return _torch_metrics(gen, ref, w)
    mpjpe, mse = _load_hip_ext().pose_metrics(gen, ref, *w)
    return mpjpe, mse


def pose_spread(gen: torch.Tensor,
                axis_scale: Optional[Sequence[float]] = None) -> torch.Tensor:
    """gen (T, S, B, J, 3), S >= 2 -> spread (T, B) fp32."""
    from . import _load_hip_ext

    _check_poses("gen", gen, 5, "(T, S, B, J, 3)")
    T, S, B, J, _ = gen.shape
    if S < 2:
        raise ValueError(f"pose_spread needs S >= 2 samples, got S={S}")
    w = _axis_scale(axis_scale)
    _no_grad_needed("pose_spread", gen)
    if T * B == 0:
        return torch.empty((T, B), dtype=torch.float32, device=gen.device)
    backend = pose_metrics_backend(gen)
    if backend == "hip" and S * J > SPREAD_MAX_SJ:
        raise ValueError(
            f"pose_spread stages the S samples of a frame in LDS: S * J = "
            f"{S * J} exceeds {SPREAD_MAX_SJ} (P2PVG_KERNELS=torch has no limit)")
    gen = gen.detach().contiguous()
    if backend == "torch":
        return _torch_spread(gen, w)
    return _load_hip_ext().pose_spread(gen, *w)
