"""Batch gather from a device-resident uint8 frame bank.

`clip_gather(bank, idx, L)` builds a training batch from decoded frames kept
as `bank` (N, T, H, W, C) uint8 (`BairRobotPush.load_pack`, uploaded once):
`idx` (B,) picks the clips (`BairRobotPush.plan_batch`), the first L frames of
each are converted and laid out as the generator yields them,

    out[l, b] = float(bank[idx[b], l]) / 255        fp32, correctly rounded

stored (L, B, H, W, C) and returned as the view (L, B, C, H, W): the strides of
the CUDA branch of `data.get_generator`, each out[l] a channels_last frame.

Arguments are validated on the host BEFORE anything is launched (ValueError on
any violation), so the HIP kernel (csrc/clip_gather.hip) never reads outside
the bank. On CPU - and on any device under P2PVG_KERNELS=torch - the result is
`bank[idx.long(), :L].float().div(255)` permuted to the same layout; it is the
oracle the kernel is tested against (tests/test_bair_cache_gpu.py, every
comparison torch.equal).
"""
from __future__ import annotations

import torch


def _validate(bank, idx, L) -> None:
    for name, t in (("bank", bank), ("idx", idx)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if bank.dtype != torch.uint8 or bank.dim() != 5:
        raise ValueError(
            "bank must be a (N, T, H, W, C) uint8 tensor, got "
            f"{tuple(bank.shape)} {bank.dtype}")
    if not bank.is_contiguous():
        raise ValueError("bank must be contiguous")
    N, T, H, W, C = bank.shape
    if N < 1 or H * W * C < 16 or (H * W * C) % 16 != 0:
        raise ValueError(
            "bank needs N >= 1 and H*W*C a positive multiple of 16, got "
            f"{tuple(bank.shape)}")
    if bank.data_ptr() % 16 != 0:
        raise ValueError("bank must be 16-byte aligned")
    if idx.device.type != "cpu":
        raise ValueError("idx is the host plan: it must be a CPU tensor")
    if idx.dtype != torch.int32:
        raise ValueError(f"idx must be int32, got {idx.dtype}")
    if idx.dim() != 1:
        raise ValueError(f"idx must be (B,), got {tuple(idx.shape)}")
    if isinstance(L, bool) or not isinstance(L, int):
        raise ValueError(f"L must be an int, got {L!r}")
    if not 1 <= L <= T:
        raise ValueError(f"1 <= L <= T = {T} required, got {L}")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= N):
        raise ValueError(f"idx out of range [0, {N})")


def _gather_torch(bank: torch.Tensor, idx: torch.Tensor, L: int) -> torch.Tensor:
    sel = bank[idx.long().to(bank.device), :L]  # (B, L, H, W, C) u8
    if bank.is_cuda:
        # ATen's GPU division by a Python scalar multiplies by its reciprocal,
        # which is not the correctly rounded quotient: look the 256 quotients
        # up in a table divided on the host instead
        table = (torch.arange(256, dtype=torch.float32) / 255.0).to(bank.device)
        x = table[sel.long()]
    else:
        x = sel.float().div(255)
    # a fresh (L, B, H, W, C) buffer: .contiguous() would keep the strides of
    # the (B, L) order whenever B or L is 1
    out = torch.empty((L,) + tuple(sel.shape[:1]) + tuple(sel.shape[2:]),
                      dtype=torch.float32, device=bank.device)
    return out.copy_(x.permute(1, 0, 2, 3, 4))


def clip_gather(bank: torch.Tensor, idx: torch.Tensor, L: int) -> torch.Tensor:
    """bank (N,T,H,W,C) u8 on the target device, idx (B,) int32 on the CPU ->
    (L, B, C, H, W) f32 on bank.device, stored (L, B, H, W, C)."""
    from . import _load_hip_ext, _want_hip

    _validate(bank, idx, L)
    if not _want_hip(bank):
        out = _gather_torch(bank, idx, L)
    else:
        # the plan is ~2 KB per batch: pinned staging + async HtoD on the
        # current stream, the kernel is ordered behind the copy
        idx_d = idx.contiguous().pin_memory().to(bank.device, non_blocking=True)
        out = _load_hip_ext().clip_gather(bank, idx_d, L)
    return out.permute(0, 1, 4, 2, 3)
