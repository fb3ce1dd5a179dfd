"""MovingMNIST frame synthesis from a host trajectory plan.

`moving_mnist_render(digits, idx, pos, image_size)` renders the plan that
`DynamicLengthMovingMNIST.plan_batch` draws: `idx` (B, D) picks sprites of the
`digits` (N, 32, 32) bank and `pos` (L, B, D, 2) holds their (sy, sx) per
frame. Each output pixel is the fp32 sum, over d = 0..D-1 in that order, of
the sprites whose 32x32 window covers it, clamped with min(., 1).

The plan is validated on the host BEFORE anything is launched (ValueError on
any violation), so the HIP kernel (csrc/mnist_synth.hip) never sees a window
that leaves the canvas or a sprite index outside the bank. On CPU — and on any
device under P2PVG_KERNELS=torch — the frames come from `_render_torch`, the
dataset's own slice-adds; it is the oracle the kernel is tested against
(tests/test_mnist_synth_gpu.py, every comparison torch.equal).
"""
from __future__ import annotations

import torch

SPRITE = 32
MAX_DIGITS = 8
MIN_SIZE = 36


def _validate(digits: torch.Tensor, idx: torch.Tensor, pos: torch.Tensor,
              S: int) -> None:
    if S < MIN_SIZE or S % 4 != 0:
        raise ValueError(
            f"image_size must be >= {MIN_SIZE} and a multiple of 4, got {S}")
    if (digits.dtype != torch.float32 or digits.dim() != 3
            or digits.shape[0] < 1 or tuple(digits.shape[1:]) != (SPRITE, SPRITE)):
        raise ValueError(
            "digits must be a (N, 32, 32) float32 tensor, got "
            f"{tuple(digits.shape)} {digits.dtype}")
    if not digits.is_contiguous():
        raise ValueError("digits must be contiguous")
    for name, t in (("idx", idx), ("pos", pos)):
        if t.device.type != "cpu":
            raise ValueError(f"{name} is the host plan: it must be a CPU tensor")
        if t.dtype != torch.int32:
            raise ValueError(f"{name} must be int32, got {t.dtype}")
    if idx.dim() != 2:
        raise ValueError(f"idx must be (B, D), got {tuple(idx.shape)}")
    B, D = idx.shape
    if not 1 <= D <= MAX_DIGITS:
        raise ValueError(f"1 <= num_digits <= {MAX_DIGITS} required, got {D}")
    if pos.dim() != 4 or tuple(pos.shape[1:]) != (B, D, 2):
        raise ValueError(
            f"pos must be (L, {B}, {D}, 2) to match idx, got {tuple(pos.shape)}")
    N = digits.shape[0]
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= N):
        raise ValueError(f"idx out of range [0, {N})")
    if pos.numel() and (int(pos.min()) < 0 or int(pos.max()) > S - SPRITE):
        raise ValueError(
            f"positions out of range [0, {S - SPRITE}]: a window leaves the canvas")


def _render_torch(digits: torch.Tensor, idx: torch.Tensor, pos: torch.Tensor,
                  S: int) -> torch.Tensor:
    """The dataset's slice-adds (moving_mnist.py __getitem__), from a plan."""
    L, B, D = pos.shape[:3]
    out = torch.zeros(L, B, 1, S, S, dtype=torch.float32, device=digits.device)
    sprite = idx.tolist()
    for l, frame in enumerate(pos.tolist()):
        for b, image in enumerate(frame):
            for d, (sy, sx) in enumerate(image):
                out[l, b, 0, sy:sy + SPRITE, sx:sx + SPRITE] += digits[sprite[b][d]]
    return out.clamp_(max=1.0)


def moving_mnist_render(digits: torch.Tensor, idx: torch.Tensor,
                        pos: torch.Tensor, image_size: int) -> torch.Tensor:
    """digits (N,32,32) f32 on the target device; idx (B,D), pos (L,B,D,2)
    int32 on the CPU -> (L, B, 1, S, S) f32 on digits.device."""
    from . import _load_hip_ext, _want_hip

    image_size = int(image_size)
    _validate(digits, idx, pos, image_size)
    if not _want_hip(digits):
        return _render_torch(digits, idx, pos, image_size)
    # the plan is ~120 KB per batch: pinned staging + async HtoD on the
    # current stream, the kernel is ordered behind both copies
    idx_d = idx.contiguous().pin_memory().to(digits.device, non_blocking=True)
    pos_d = pos.contiguous().pin_memory().to(digits.device, non_blocking=True)
    return _load_hip_ext().moving_mnist_render(digits, idx_d, pos_d, image_size)
