"""MovingMNIST render kernel (csrc/mnist_synth.hip) against the CPU op.

A random fp32 sprite bank in [0, 1), N = 5, and hand-made plans; the CPU
implementation of ops.moving_mnist_render (the dataset's slice-adds) is the
oracle and every comparison is torch.equal: the kernel adds the same fp32
values in the same digit order and clamps with the same min(., 1).

No test feeds the kernel an out-of-range plan: the validation tests assert
that such a plan raises before the extension is reached.
"""
import dataclasses

import numpy as np
import pytest
import torch

from p2pvg_amd import data as data_utils
from p2pvg_amd import ops
from p2pvg_amd.data.moving_mnist import DynamicLengthMovingMNIST
from p2pvg_amd.ops import moving_mnist_render

pytestmark = pytest.mark.gpu

N = 5


@pytest.fixture(scope="module")
def bank():
    cpu = torch.rand(N, 32, 32, generator=torch.Generator().manual_seed(11))
    assert float(cpu.min()) >= 0.0 and float(cpu.max()) < 1.0
    return cpu, cpu.cuda()


def _i32(x):
    return torch.tensor(x, dtype=torch.int32)


def plan_corners():
    """L3 B2 D2 S64: the four corners, full overlap, one-row/one-column overlap."""
    idx = _i32([[0, 1], [2, 3]])
    pos = _i32([
        [[[0, 0], [32, 32]], [[0, 32], [32, 0]]],
        [[[10, 20], [10, 20]], [[0, 0], [31, 31]]],
        [[[32, 32], [32, 32]], [[1, 0], [32, 31]]],
    ])
    return idx, pos, 64


def plan_three_digits():
    """L2 B3 D3 S128: three distinct sprites on one spot (fp32 sum order),
    far corners and an almost-corner."""
    idx = _i32([[0, 1, 2], [3, 4, 0], [2, 2, 1]])
    pos = _i32([
        [[[40, 50]] * 3, [[0, 0], [96, 96], [95, 1]], [[10, 10], [20, 20], [30, 30]]],
        [[[96, 96]] * 3, [[95, 1], [0, 0], [96, 96]], [[0, 96], [16, 80], [1, 95]]],
    ])
    return idx, pos, 128


def plan_single_digit_odd_sx():
    """L5 B3 D1 S64: odd image counts, odd sx (unaligned sprite reads)."""
    g = torch.Generator().manual_seed(3)
    L, B = 5, 3
    idx = torch.randint(0, N, (B, 1), generator=g, dtype=torch.int32)
    sy = torch.randint(0, 33, (L, B, 1), generator=g, dtype=torch.int32)
    sx = torch.randint(0, 16, (L, B, 1), generator=g, dtype=torch.int32) * 2 + 1
    assert int(sx.max()) <= 31 and bool((sx % 2 == 1).all())
    return idx, torch.stack([sy, sx], dim=-1).contiguous(), 64


def plan_smallest_canvas():
    """L1 B1 D8 S36: smallest canvas, most digits, every position in 0..4."""
    idx = _i32([[0, 1, 2, 3, 4, 0, 1, 2]])
    pos = _i32([[[[0, 1], [1, 2], [2, 3], [3, 4], [4, 0], [0, 4], [2, 2], [4, 4]]]])
    return idx, pos, 36


def plan_bank_indexing():
    """Two images share their idx row; the third uses the bank's last sprite."""
    idx = _i32([[4, 1], [4, 1], [N - 1, N - 1]])
    pos = _i32([
        [[[3, 5], [20, 9]], [[30, 2], [0, 31]], [[0, 0], [32, 32]]],
        [[[4, 6], [19, 10]], [[29, 3], [1, 30]], [[16, 16], [17, 15]]],
    ])
    return idx, pos, 64


PLANS = {
    "corners": (plan_corners, (3, 2, 2, 64)),
    "three_digits": (plan_three_digits, (2, 3, 3, 128)),
    "single_digit_odd_sx": (plan_single_digit_odd_sx, (5, 3, 1, 64)),
    "smallest_canvas": (plan_smallest_canvas, (1, 1, 8, 36)),
    "bank_indexing": (plan_bank_indexing, (2, 3, 2, 64)),
}


@pytest.mark.parametrize("name", list(PLANS))
def test_render_matches_cpu_op(bank, name):
    cpu_bank, gpu_bank = bank
    make, (L, B, D, S) = PLANS[name]
    idx, pos, S_ = make()
    assert S_ == S and idx.shape == (B, D) and pos.shape == (L, B, D, 2)
    want = moving_mnist_render(cpu_bank, idx, pos, S)
    got = moving_mnist_render(gpu_bank, idx, pos, S)
    assert got.is_cuda and got.shape == (L, B, 1, S, S)
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    if D >= 2:
        # the plan overlaps digits: the clamp is exercised, not just present
        assert float(want.max()) == 1.0


def test_dataset_parity_on_device():
    S, D, T, B, seed = 64, 2, 30, 6, 1234
    ds = DynamicLengthMovingMNIST(
        data_root="/nonexistent", train=True, max_seq_len=T, delta_len=1,
        image_size=S, num_digits=D, deterministic=False)
    ds.seed_is_set = True
    np.random.seed(seed)
    want = torch.stack([ds[i] for i in range(B)]).permute(1, 0, 2, 3, 4)
    idx, pos = ds.plan_batch(B, np.random.RandomState(seed))
    got = moving_mnist_render(ds.digits.cuda(), idx, pos, S)
    assert torch.equal(got.cpu(), want)


def test_render_on_ambient_stream(bank):
    cpu_bank, gpu_bank = bank
    idx, pos, S = plan_corners()
    want = moving_mnist_render(cpu_bank, idx, pos, S)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = moving_mnist_render(gpu_bank, idx, pos, S)
        host = got.cpu()       # DtoH on s, ordered behind the kernel on s
    s.synchronize()
    assert torch.equal(host, want)


def _good_plan(D=2, S=64, L=2, B=2):
    g = torch.Generator().manual_seed(7)
    idx = torch.randint(0, N, (B, D), generator=g, dtype=torch.int32)
    pos = torch.randint(0, S - 31, (L, B, D, 2), generator=g, dtype=torch.int32)
    return idx, pos, S


def _bad_plans():
    cases = {}
    i, p, S = _good_plan()
    j = i.clone(); j[1, 0] = N
    cases["idx==N"] = (j, p, S)
    j = i.clone(); j[0, 1] = -1
    cases["idx==-1"] = (j, p, S)
    q = p.clone(); q[1, 0, 1, 0] = S - 31
    cases["sy==S-31"] = (i, q, S)
    q = p.clone(); q[0, 1, 0, 1] = -1
    cases["sx==-1"] = (i, q, S)
    cases["int64 idx"] = (i.long(), p, S)
    cases["pos trailing dim"] = (i, torch.zeros(2, 2, 2, 3, dtype=torch.int32), S)
    i9, p9, _ = _good_plan(D=9)
    cases["D==9"] = (i9, p9, S)
    cases["S==66"] = (i, p, 66)
    return cases


class _RecordingExt:
    """Stands in for the extension and counts render launches."""

    def __init__(self, real):
        self._real = real
        self.calls = 0

    def moving_mnist_render(self, *a):
        self.calls += 1
        return self._real.moving_mnist_render(*a)

    def __getattr__(self, name):
        return getattr(self._real, name)


def test_validation_raises_before_launch(bank, monkeypatch):
    _, gpu_bank = bank
    rec = _RecordingExt(ops._load_hip_ext())
    monkeypatch.setattr(ops, "_load_hip_ext", lambda: rec)
    for name, (idx, pos, S) in _bad_plans().items():
        with pytest.raises(ValueError):
            moving_mnist_render(gpu_bank, idx, pos, S)
        assert rec.calls == 0, f"{name}: reached the extension"
    idx, pos, S = _good_plan()
    moving_mnist_render(gpu_bank, idx, pos, S)
    assert rec.calls == 1  # the probe does see a valid plan's launch


def test_training_step_on_device_generator(tiny_cfg):
    from p2pvg_amd.models import P2PModel

    cfg = dataclasses.replace(tiny_cfg, device="cuda", dtype="bf16",
                              num_digits=2, skip_prob=0.0,
                              mnist_synth="device")
    torch.manual_seed(0)
    np.random.seed(0)
    train, test = data_utils.load_dataset(cfg)
    for data, flag in ((train, True), (test, False)):
        x = next(data_utils.get_data_generator(data, train=flag, opt=cfg))
        assert x.is_cuda and x.shape[1:] == (2, 1, 64, 64) and 6 <= len(x) <= 8
        assert x[0].is_contiguous(memory_format=torch.channels_last)
    model = P2PModel(cfg).to("cuda").to(memory_format=torch.channels_last)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        losses = model(x, 0, len(x) - 1)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v) for v in losses), losses
