"""Device-side MovingMNIST synthesis, host half: trajectory planner, plan
validation, the torch render (the oracle of tests/test_mnist_synth_gpu.py),
the DataLoader-free generator and its configuration.

Every comparison is exact (torch.equal): the planner performs the dataset's
own random draws in the dataset's order and the render performs its
slice-adds in its digit order, so nothing here needs a tolerance.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from p2pvg_amd import data as data_utils
from p2pvg_amd.core import Config
from p2pvg_amd.data.moving_mnist import DynamicLengthMovingMNIST
from p2pvg_amd.ops import moving_mnist_render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (image_size, num_digits, deterministic bounce, max_seq_len)
PARITY_CONFIGS = [
    (64, 2, False, 30),
    (64, 3, False, 12),
    (64, 2, True, 12),
    (128, 2, False, 12),
    (64, 1, False, 8),
]


def _dataset(S, D, det, T, delta=1):
    return DynamicLengthMovingMNIST(
        data_root="/nonexistent", train=True, max_seq_len=T, delta_len=delta,
        image_size=S, num_digits=D, deterministic=det)


def dataset_batch(ds, B, seed):
    """(T, B, 1, S, S) from B consecutive ds[i] on the global numpy stream
    seeded with `seed`, plus the next draw of that stream."""
    ds.seed_is_set = True
    np.random.seed(seed)
    x = torch.stack([ds[i] for i in range(B)]).permute(1, 0, 2, 3, 4)
    return x, int(np.random.randint(1 << 30))


@pytest.mark.parametrize("S,D,det,T", PARITY_CONFIGS)
def test_planner_parity_with_dataset(S, D, det, T):
    B, seed = 6, 1000 + S + 10 * D + T
    ds = _dataset(S, D, det, T)
    want, want_next = dataset_batch(ds, B, seed)

    rng = np.random.RandomState(seed)
    idx, pos = ds.plan_batch(B, rng)
    assert idx.shape == (B, D) and idx.dtype == torch.int32
    assert pos.shape == (T, B, D, 2) and pos.dtype == torch.int32
    assert not idx.is_cuda and not pos.is_cuda
    assert int(pos.min()) >= 0 and int(pos.max()) <= S - 33
    got = moving_mnist_render(ds.digits, idx, pos, S)
    assert got.shape == (T, B, 1, S, S) and got.dtype == torch.float32
    assert torch.equal(got, want)
    # the planner leaves its RandomState where the dataset leaves the global one
    assert int(rng.randint(1 << 30)) == want_next


def test_partial_length_renders_leading_frames():
    ds = _dataset(64, 2, False, 10)
    idx, pos = ds.plan_batch(3, np.random.RandomState(3))
    full = moving_mnist_render(ds.digits, idx, pos, 64)
    part = moving_mnist_render(ds.digits, idx, pos[:4], 64)
    assert part.shape == (4, 3, 1, 64, 64)
    assert torch.equal(part, full[:4])


def test_overlap_clamps_to_one():
    ds = _dataset(64, 2, False, 4)
    k = int(ds.digits.flatten(1).max(dim=1).values.argmax())
    assert float(ds.digits[k].max()) > 0.5
    idx = torch.tensor([[k, k]], dtype=torch.int32)
    pos = torch.tensor([[[[7, 9], [7, 9]]], [[[7, 9], [20, 30]]]],
                       dtype=torch.int32)           # (L=2, B=1, D=2, 2)
    raw = torch.zeros(2, 1, 1, 64, 64)
    for l in range(2):
        for d in range(2):
            sy, sx = pos[l, 0, d].tolist()
            raw[l, 0, 0, sy:sy + 32, sx:sx + 32] += ds.digits[k]
    over = raw > 1.0
    assert over[0].any(), "the plan must push some pixel above 1"
    got = moving_mnist_render(ds.digits, idx, pos, 64)
    assert (got[over] == 1.0).all()
    assert torch.equal(got, raw.clamp(max=1.0))
    assert float(got.max()) == 1.0 and float(got.min()) == 0.0


def _good_plan(N=5, L=2, B=2, D=2, S=64):
    g = torch.Generator().manual_seed(7)
    digits = torch.rand(N, 32, 32, generator=g)
    idx = torch.randint(0, N, (B, D), generator=g, dtype=torch.int32)
    pos = torch.randint(0, S - 31, (L, B, D, 2), generator=g, dtype=torch.int32)
    return digits, idx, pos, S


def bad_plans():
    """name -> (digits, idx, pos, S), each violating one rule of the contract."""
    cases = {}
    d, i, p, S = _good_plan()
    j = i.clone(); j[1, 0] = 5
    cases["idx==N"] = (d, j, p, S)
    j = i.clone(); j[0, 1] = -1
    cases["idx==-1"] = (d, j, p, S)
    q = p.clone(); q[1, 0, 1, 0] = S - 31
    cases["sy==S-31"] = (d, i, q, S)
    q = p.clone(); q[0, 1, 0, 1] = -1
    cases["sx==-1"] = (d, i, q, S)
    cases["int64 idx"] = (d, i.long(), p, S)
    cases["pos trailing dim"] = (d, i, torch.zeros(2, 2, 2, 3, dtype=torch.int32), S)
    d9, i9, p9, _ = _good_plan(D=9)
    cases["D==9"] = (d9, i9, p9, S)
    d66, i66, p66, _ = _good_plan(S=64)
    cases["S==66"] = (d66, i66, p66, 66)
    return cases


@pytest.mark.parametrize("name", list(bad_plans()))
def test_validation_raises(name):
    digits, idx, pos, S = bad_plans()[name]
    with pytest.raises(ValueError):
        moving_mnist_render(digits, idx, pos, S)


def test_good_plan_passes_validation():
    digits, idx, pos, S = _good_plan()
    assert moving_mnist_render(digits, idx, pos, S).shape == (2, 2, 1, 64, 64)


def _gen_cfg(**kw):
    base = dict(dataset="mnist", num_digits=2, batch_size=3, max_seq_len=8,
                delta_len=1, data_root="/nonexistent", device="cpu",
                num_workers=0, mnist_synth="device")
    base.update(kw)
    return Config(**base)


def test_generator_output():
    cfg = _gen_cfg()
    train, _ = data_utils.load_dataset(cfg)
    torch.manual_seed(5)
    gen = data_utils.get_data_generator(train, train=True, opt=cfg)
    lengths = set()
    for _ in range(20):
        x = next(gen)
        t, b, c, h, w = x.shape
        assert (b, c, h, w) == (3, 1, 64, 64) and 6 <= t <= 8
        assert x.dtype == torch.float32 and x.device.type == "cpu"
        assert x[0].is_contiguous(memory_format=torch.channels_last)
        assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0
        assert float(x.sum()) > 0
        lengths.add(t)
    assert len(lengths) > 1

    torch.manual_seed(5)
    fixed = data_utils.get_data_generator(train, train=True,
                                          dynamic_length=False, opt=cfg)
    assert all(next(fixed).shape[0] == 8 for _ in range(3))


def test_generator_seeding():
    cfg = _gen_cfg()
    train, _ = data_utils.load_dataset(cfg)

    def batches(train_flag, rank, n=3):
        torch.manual_seed(5)
        g = data_utils.get_data_generator(train, train=train_flag, opt=cfg,
                                          rank=rank)
        return [next(g) for _ in range(n)]

    def same(a, b):
        return all(x.shape == y.shape and torch.equal(x, y)
                   for x, y in zip(a, b))

    ref = batches(True, 0)
    assert same(ref, batches(True, 0))
    assert not same(ref, batches(True, 1))
    assert not same(ref, batches(False, 0))


def test_generator_matches_dataset_stream():
    """The generator is plan_batch + one seq_len draw per batch on its own
    RandomState: replaying that stream through the dataset gives its frames."""
    cfg = _gen_cfg()
    train, _ = data_utils.load_dataset(cfg)
    torch.manual_seed(9)
    gen = data_utils.get_data_generator(train, train=True, opt=cfg)
    got = [next(gen) for _ in range(2)]

    train.seed_is_set = True
    np.random.seed(9 % 2**31)
    for x in got:
        want = torch.stack([train[i] for i in range(3)]).permute(1, 0, 2, 3, 4)
        seq_len = int(np.random.randint(8 - 2, 8 + 1))
        assert torch.equal(x, want[:seq_len])


def test_dispatch_and_config(monkeypatch):
    made = []
    real = data_utils.DataLoader

    def recording_loader(*a, **kw):
        made.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(data_utils, "DataLoader", recording_loader)

    cfg = _gen_cfg(mnist_synth="loader")
    train, test = data_utils.load_dataset(cfg)
    x = next(data_utils.get_data_generator(train, train=True, opt=cfg))
    assert len(made) == 1 and x.shape[1:] == (3, 1, 64, 64)

    cfg = _gen_cfg(mnist_synth="device")
    for data, flag in ((train, True), (test, False)):
        x = next(data_utils.get_data_generator(data, train=flag, opt=cfg))
        assert x.shape[1:] == (3, 1, 64, 64)
    assert len(made) == 1, "the device path must not build a DataLoader"

    with pytest.raises(ValueError):
        data_utils.get_data_generator(train, opt=_gen_cfg(mnist_synth="gpu"))
    with pytest.raises(ValueError):
        data_utils.get_data_generator(
            train, opt=_gen_cfg(dataset="bair", channels=3))

    assert Config().mnist_synth == "loader"
    assert Config.from_dict(Config().to_dict()).to_dict() == Config().to_dict()
    cfg2 = Config.from_dict(_gen_cfg().to_dict())
    assert cfg2.mnist_synth == "device"
    old = Config().to_dict()
    del old["mnist_synth"]
    assert Config.from_dict(old).mnist_synth == "loader"


def test_train_cli_device_synth_cpu(tmp_path):
    env = os.environ.copy()
    env["PYTHONPATH"] = ROOT
    log_dir = tmp_path / "logs" / "run"
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "train.py"),
         "--dataset", "mnist", "--mnist_synth", "device", "--num_digits", "2",
         "--backbone", "dcgan", "--batch_size", "2", "--max_seq_len", "6",
         "--delta_len", "1", "--g_dim", "32", "--z_dim", "4",
         "--rnn_size", "32", "--nepochs", "1", "--epoch_size", "2",
         "--nsample", "2", "--device", "cpu", "--qual_iter", "100",
         "--data_root", "/nonexistent", "--num_workers", "0",
         "--log_dir", str(log_dir)],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
    )
    assert r.returncode == 0, r.stderr[-3000:]
    run = [d for d in (tmp_path / "logs").iterdir() if d.is_dir()][0]
    assert (run / "model_0.pth").exists()
    assert (run / "model.pth").exists()
