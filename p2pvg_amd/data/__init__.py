"""Dataset factory and infinite batch generators.

Capability parity with reference data/data_utils.py:6-140: `load_dataset(cfg)`
dispatches on cfg.dataset; `get_data_generator` yields (t, b, ...) batches on
the target device, truncated to a per-batch dynamic length drawn by the
dataset. MI355X-native differences: pinned host memory + non_blocking HtoD
(the reference does a blocking `.cuda()` per batch, data_utils.py:100,116),
device is configurable (CPU works), and under DDP each rank seeds its workers
with a rank offset so shards differ. `mnist_synth="device"` swaps the
MovingMNIST DataLoader for a host trajectory planner plus an on-device render
(`get_device_mnist_generator`); the frames are bit-identical to the dataset's.
`frame_cache="device"` does the same for BAIR with the decoded frames kept on
the device as uint8 and one gather kernel per batch
(`get_device_bair_generator`).
"""
from __future__ import annotations

import os
from typing import Iterator, Tuple

import torch
from torch.utils.data import DataLoader

from .bair import BairRobotPush
from .human36m import Human36mDataset
from .moving_mnist import DynamicLengthMovingMNIST
from .weizmann import WeizmannDataset


def load_dataset(cfg, eval=False, eval_len=None):
    if cfg.dataset == "mnist":
        mk = lambda train: DynamicLengthMovingMNIST(  # noqa: E731
            train=train,
            data_root=cfg.data_root,
            max_seq_len=cfg.max_seq_len,
            delta_len=cfg.delta_len,
            image_size=cfg.image_width,
            deterministic=False,
            num_digits=cfg.num_digits,
        )
        return mk(True), mk(False)

    if cfg.dataset == "weizmann":
        assert cfg.channels == 3, f"weizmann has 3 channels, got {cfg.channels}"
        mk = lambda train, msl: WeizmannDataset(  # noqa: E731
            data_root=cfg.data_root,
            train=train,
            max_seq_len=msl,
            n_past=cfg.n_past,
            delta_len=cfg.delta_len,
            image_size=cfg.image_width,
        )
        return mk(True, 18), mk(False, 10)

    if cfg.dataset == "h36m":
        data_root = os.path.join(cfg.data_root, "processed/h36m-fetch/processed")
        mk = lambda mode, spd: Human36mDataset(  # noqa: E731
            data_root=data_root,
            max_seq_len=30,
            delta_len=cfg.delta_len,
            speed_range=spd,
            n_breakpoints=0,
            acc_range=[0, 0],
            mode=mode,
        )
        return mk("train", [6, 6]), mk("test", [1, 1])

    if cfg.dataset == "bair":
        assert cfg.channels == 3, f"bair has 3 channels, got {cfg.channels}"
        mk = lambda train: BairRobotPush(  # noqa: E731
            data_root=cfg.data_root,
            train=train,
            max_seq_len=cfg.max_seq_len,
            delta_len=cfg.delta_len,
            image_size=cfg.image_width,
        )
        return mk(True), mk(False)

    raise ValueError(f"Unknown dataset {cfg.dataset!r}")


def _worker_seed_fn(rank: int):
    def _init(worker_id: int):
        import numpy as np

        seed = (torch.initial_seed() + rank * 7919 + worker_id) % (2**31)
        np.random.seed(seed)

    return _init


def _make_loader(data, batch_size: int, cfg, rank: int = 0, sampler=None) -> DataLoader:
    pin = torch.cuda.is_available()
    return DataLoader(
        data,
        batch_size=batch_size,
        shuffle=sampler is None,
        sampler=sampler,
        drop_last=True,
        num_workers=getattr(cfg, "num_workers", 1),
        pin_memory=pin,
        worker_init_fn=_worker_seed_fn(rank),
        persistent_workers=getattr(cfg, "num_workers", 1) > 0,
    )


def get_generator(loader: DataLoader, device, dynamic_length: bool = True) -> Iterator:
    cuda = getattr(device, "type", str(device)).startswith("cuda")
    while True:
        for data in loader:
            if cuda:
                # transfer the PINNED collated batch as-is (a host-side
                # permute().contiguous() would allocate an unpinned
                # intermediate and silently degrade the copy to synchronous),
                # then do the (b,t)->(t,b) transpose on device where it costs
                # one ~30us pass at HBM bandwidth. Store the clip NHWC so
                # each x[i] is a channels_last (B,C,H,W) frame — the NHWC
                # conv path then never re-lays frames out per encoder call.
                data = data.to(device, non_blocking=True)
                data = (data.permute(1, 0, 3, 4, 2).contiguous()
                        .permute(0, 1, 4, 2, 3))
            else:
                data = data.permute(1, 0, 2, 3, 4).contiguous().to(device)
            if dynamic_length:
                data = data[: loader.dataset.get_seq_len()]
            yield data


def get_h36m_generator(loader: DataLoader, device, dynamic_length: bool = True) -> Iterator:
    cuda = getattr(device, "type", str(device)).startswith("cuda")
    while True:
        for data in loader:
            seq_len = loader.dataset.get_seq_len()
            if cuda:
                # pinned batch HtoD first, permute/cast on device (see above)
                pose_2d = data["pose_2d"].to(device, non_blocking=True).permute(1, 0, 2, 3).float()
                pose_3d = data["pose_3d"].to(device, non_blocking=True).permute(1, 0, 2, 3).float()
            else:
                pose_2d = data["pose_2d"].permute(1, 0, 2, 3).float().to(device)
                pose_3d = data["pose_3d"].permute(1, 0, 2, 3).float().to(device)
            camera_view = data["camera_view"]
            if dynamic_length:
                pose_2d = pose_2d[:seq_len]
                pose_3d = pose_3d[:seq_len]
            yield (pose_2d, pose_3d, camera_view)


def get_h36m_test_generator(data, cfg, batch_size: int,
                            dynamic_length: bool = False, rank: int = 0) -> Iterator:
    """The h36m test generator at `batch_size` sequences per batch, for
    evaluation. `get_data_generator(train=False)` keeps its fixed 10.

    A batch larger than the split (the loader drops incomplete batches, so it
    would never yield) draws sequences with replacement; every draw still
    crops its own random window."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    if len(data) < 1:
        raise ValueError("the h36m test split is empty")
    device = torch.device(cfg.resolved_device() if hasattr(cfg, "resolved_device") else "cpu")
    sampler = None
    if batch_size > len(data):
        sampler = torch.utils.data.RandomSampler(
            data, replacement=True, num_samples=batch_size)
    loader = _make_loader(data, batch_size, cfg, rank, sampler)
    return get_h36m_generator(loader, device, dynamic_length)


def get_device_mnist_generator(data, cfg, device, train: bool = True,
                               dynamic_length: bool = True, rank: int = 0) -> Iterator:
    """MovingMNIST batches without a DataLoader (`--mnist_synth device`).

    Per batch the host only plans trajectories (`data.plan_batch`, the
    dataset's own random draws from a generator-owned RandomState) and ships
    the ~120 KB plan; the frames are rendered on `device` from the 32px sprite
    bank kept there (ops.moving_mnist_render: HIP kernel on GPU, slice-adds on
    CPU). Yields (seq_len, B, 1, S, S) fp32 with the strides of the CUDA
    branch of `get_generator`: each x[i] is a channels_last frame.
    """
    import numpy as np

    from ..ops import moving_mnist_render

    digits = data.digits.contiguous().to(device)
    rng = np.random.RandomState(
        (torch.initial_seed() + rank * 7919 + (0 if train else 1)) % (2**31))
    B, S, T = cfg.batch_size, data.image_size, data.max_seq_len

    def _gen():
        while True:
            idx, pos = data.plan_batch(B, rng)
            seq_len = T
            if dynamic_length:
                seq_len = int(rng.randint(T - 2 * data.delta_len, T + 1))
            x = moving_mnist_render(digits, idx, pos[:seq_len], S)
            yield x.view(seq_len, B, S, S, 1).permute(0, 1, 4, 2, 3)

    return _gen()


UPLOAD_STAGE_BYTES = 64 << 20  # pinned staging buffer of the frame-bank upload


def upload_frame_bank(pack, device) -> torch.Tensor:
    """A `BairRobotPush.load_pack` array (memory-mapped or not) as a uint8
    tensor on `device`. On a GPU the pack goes up once, in slices through one
    pinned staging buffer of UPLOAD_STAGE_BYTES, after a check that it fits."""
    import numpy as np

    device = torch.device(device)
    if device.type != "cuda":
        return torch.from_numpy(np.array(pack))  # an in-memory, writable copy
    free, _total = torch.cuda.mem_get_info(device)
    if pack.nbytes > free:
        raise ValueError(
            f"the frame pack is {pack.nbytes / 2**30:.2f} GiB but only "
            f"{free / 2**30:.2f} GiB of device memory is free on {device}: "
            "frame_cache='device' keeps every decoded frame on the device")
    bank = torch.empty(pack.shape, dtype=torch.uint8, device=device)
    flat_dst = bank.view(-1)
    flat_src = pack.reshape(-1)  # a view: load_pack arrays are C-contiguous
    stage = torch.empty(min(UPLOAD_STAGE_BYTES, pack.nbytes), dtype=torch.uint8,
                        pin_memory=True)
    stage_np = stage.numpy()
    for a in range(0, pack.nbytes, stage.numel()):
        n = min(stage.numel(), pack.nbytes - a)
        stage_np[:n] = flat_src[a:a + n]
        flat_dst[a:a + n].copy_(stage[:n], non_blocking=True)
        torch.cuda.current_stream(device).synchronize()  # stage is reused
    return bank


def get_device_bair_generator(data, cfg, device, train: bool = True,
                              dynamic_length: bool = True, rank: int = 0) -> Iterator:
    """BAIR batches without a DataLoader (`--frame_cache device`).

    The split is decoded once (`data.load_pack`, cached on disk) and kept on
    `device` as uint8; under DDP each rank holds the whole bank. Per batch the
    host only draws the clip indices (`data.plan_batch`, the dataset's own
    draws from a generator-owned RandomState) and ships those ~2 KB;
    ops.clip_gather converts and lays out the frames (HIP kernel on GPU,
    indexing on CPU), bit-identical to the dataset's. Yields (seq_len, B, 3,
    S, S) fp32 with the strides of the CUDA branch of `get_generator`: each
    x[i] is a channels_last frame.
    """
    import numpy as np

    from ..ops import clip_gather

    bank = upload_frame_bank(data.load_pack(), device)
    rng = np.random.RandomState(
        (torch.initial_seed() + rank * 7919 + (0 if train else 1)) % (2**31))
    B, T = cfg.batch_size, data.max_seq_len

    def _gen():
        while True:
            idx = data.plan_batch(B, rng)
            seq_len = T
            if dynamic_length:
                seq_len = int(rng.randint(T - 2 * data.delta_len, T + 1))
            yield clip_gather(bank, idx, seq_len)

    return _gen()


def get_data_generator(data, train: bool = True, dynamic_length: bool = True, opt=None, rank: int = 0):
    cfg = opt
    device = torch.device(cfg.resolved_device() if hasattr(cfg, "resolved_device") else "cpu")
    cache = getattr(cfg, "frame_cache", "loader")
    if cache not in ("loader", "device"):
        raise ValueError(f"frame_cache must be 'loader' or 'device', got {cache!r}")
    if cache == "device":
        if cfg.dataset != "bair":
            raise ValueError(
                f"frame_cache='device' needs dataset='bair', got {cfg.dataset!r}")
        return get_device_bair_generator(data, cfg, device, train, dynamic_length, rank)
    synth = getattr(cfg, "mnist_synth", "loader")
    if synth not in ("loader", "device"):
        raise ValueError(f"mnist_synth must be 'loader' or 'device', got {synth!r}")
    if synth == "device":
        if cfg.dataset != "mnist":
            raise ValueError(
                f"mnist_synth='device' needs dataset='mnist', got {cfg.dataset!r}")
        return get_device_mnist_generator(data, cfg, device, train, dynamic_length, rank)
    if cfg.dataset == "h36m":
        bs = cfg.batch_size if train else 10
        loader = _make_loader(data, bs, cfg, rank)
        return get_h36m_generator(loader, device, dynamic_length)
    loader = _make_loader(data, cfg.batch_size, cfg, rank)
    return get_generator(loader, device, dynamic_length)
