"""Per-frame SSIM and MSE in one pass, for evaluation.

`frame_metrics(a, b, data_range)` scores image pairs of shape (..., C, H, W)
and returns two fp32 tensors with the shape of the leading dimensions:
the mean SSIM (the definition of utils.metrics.ssim: 11x11 gaussian window,
sigma 1.5, zero padding) and the mean squared difference.

Arguments are validated BEFORE anything is launched (ValueError on any
violation). On a GPU the HIP kernel (csrc/frame_metrics.hip) reads both
operands once, in place: dense NCHW or dense channels_last images at any image
stride, fp32 / bf16 / fp16 per operand; any other stride pattern is made
contiguous here first. On CPU - and on any device under P2PVG_KERNELS=torch -
the result is utils.metrics.ssim / utils.metrics.mse on the flattened images,
which is also what the kernel is tested against.

An evaluation op: there is no backward.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch

WINDOW = 11
SIGMA = 1.5
_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def window_1d() -> torch.Tensor:
    """The eleven fp32 weights g with utils.metrics._gaussian_window == g (x) g,
    computed the way that function computes its 1-D factor."""
    coords = torch.arange(WINDOW, dtype=torch.float32) - (WINDOW - 1) / 2.0
    g = torch.exp(-(coords**2) / (2 * SIGMA**2))
    return (g / g.sum()).contiguous()


def _validate(a, b, data_range) -> None:
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype not in _DTYPES:
            raise ValueError(f"{name} must be fp32, bf16 or fp16, got {t.dtype}")
        if t.dim() < 4:
            raise ValueError(
                f"{name} must be (..., C, H, W) with at least one leading "
                f"dimension, got {tuple(t.shape)}")
    if a.shape != b.shape:
        raise ValueError(
            f"a and b must have equal shapes, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.device != b.device:
        raise ValueError(f"a and b must be on one device, got {a.device} and {b.device}")
    if min(a.shape[-3:]) < 1:
        raise ValueError(f"C, H, W must be >= 1, got {tuple(a.shape[-3:])}")
    try:
        ok = math.isfinite(float(data_range)) and float(data_range) > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"data_range must be a finite number > 0, got {data_range!r}")


def _as_images(t: torch.Tensor, M: int) -> torch.Tensor:
    """(..., C, H, W) -> a (M, C, H, W) view the kernel reads in place: inner
    strides dense NCHW or dense channels_last, image stride >= C*H*W. Anything
    else is copied to contiguous NCHW."""
    C, H, W = t.shape[-3:]
    try:
        v = t.view(M, C, H, W)
    except RuntimeError:  # leading dimensions do not merge into one stride
        return t.contiguous().view(M, C, H, W)

    def matches(want):  # the stride of a size-1 dimension is never used
        return all(n == 1 or s == w
                   for n, s, w in zip((C, H, W), v.stride()[1:], want))

    dense = matches((H * W, W, 1)) or matches((1, W * C, C))
    if dense and (v.shape[0] <= 1 or v.stride(0) >= C * H * W):
        return v
    return v.contiguous()


def _torch_path(a4: torch.Tensor, b4: torch.Tensor, data_range: float):
    from ..utils import metrics

    # scores are fp32 whatever the caller's autocast state: under autocast the
    # five convolutions of utils.metrics.ssim would run, and round, in bf16
    with torch.autocast(a4.device.type, enabled=False):
        return (metrics.ssim(a4, b4, data_range).float(),
                metrics.mse(a4, b4).float())


def frame_metrics_backend(where) -> str:
    """The path `frame_metrics` takes for a tensor, or for tensors on a device:
    "hip" (the kernel) or "torch" (utils.metrics). The op dispatches on this
    very answer; like it, this raises on a GPU whose extension is missing."""
    from . import _want_hip

    t = where if isinstance(where, torch.Tensor) else torch.empty(0, device=where)
    return "hip" if _want_hip(t) else "torch"


def frame_metrics(a: torch.Tensor, b: torch.Tensor,
                  data_range: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """a, b (..., C, H, W) -> (ssim, mse), fp32, shape = the leading dimensions."""
    from . import _load_hip_ext

    _validate(a, b, data_range)
    if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
        raise RuntimeError(
            "frame_metrics is an evaluation op without a backward: call it "
            "under torch.no_grad() or detach its inputs")
    data_range = float(data_range)
    lead = a.shape[:-3]
    C, H, W = a.shape[-3:]
    M = math.prod(lead)
    if M == 0:  # an empty leading dimension: nothing to score on either path
        empty = torch.empty(lead, dtype=torch.float32, device=a.device)
        return empty, empty.clone()
    if frame_metrics_backend(a) == "torch":
        ssim, mse = _torch_path(a.reshape(M, C, H, W), b.reshape(M, C, H, W),
                                data_range)
    else:
        ssim, mse = _load_hip_ext().frame_metrics(
            _as_images(a, M), _as_images(b, M), window_1d(), data_range)
    return ssim.view(lead), mse.view(lead)
