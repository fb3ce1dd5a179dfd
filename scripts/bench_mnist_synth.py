#!/usr/bin/env python
"""MovingMNIST input pipeline: DataLoader path vs on-device synthesis.

Run on a GPU box: python scripts/bench_mnist_synth.py [--batches 100 256]

For each batch size, max_seq_len 30, 2 digits, 64x64, fixed length, all in
this one process (at most 16 CPU threads):

  (a) loader     frames/s of the default path (Dataset.__getitem__ in
                 DataLoader workers, pinned HtoD, device permute),
                 num_workers 1 and 8
  (b) device     frames/s of the --mnist_synth device generator, and its host
                 time per batch (plan + validate + enqueue, no device wait)
  (c) planner    DynamicLengthMovingMNIST.plan_batch alone, ms per batch
  (d) kernel     moving_mnist_render kernel alone on a resident plan, us per
                 call and GB/s of output written, from device events

One JSON line per figure. `--device cpu` is a dry run of the script's own
logic (it skips (d)); its figures say nothing about the GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2pvg_amd import data as data_utils  # noqa: E402
from p2pvg_amd.core import Config  # noqa: E402

T, D, S = 30, 2, 64


def emit(**kw):
    print(json.dumps(kw), flush=True)


def sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize()


def make_cfg(batch, device, **kw):
    return Config(dataset="mnist", num_digits=D, max_seq_len=T, delta_len=5,
                  image_width=S, batch_size=batch, data_root="/nonexistent",
                  device=str(device), **kw)


def time_generator(gen, device, n, warmup):
    """(seconds per batch incl. device completion, host seconds per batch)."""
    for _ in range(warmup):
        x = next(gen)
    sync(device)
    t0 = time.perf_counter()
    for _ in range(n):
        x = next(gen)
    t_host = time.perf_counter() - t0
    sync(device)
    t_all = time.perf_counter() - t0
    assert x.shape == (T, x.shape[1], 1, S, S)
    return t_all / n, t_host / n


def bench_loader(batch, device, workers, n):
    cfg = make_cfg(batch, device, num_workers=workers)
    train, _ = data_utils.load_dataset(cfg)
    loader = data_utils._make_loader(train, batch, cfg)
    gen = data_utils.get_generator(loader, device, dynamic_length=False)
    per_batch, _ = time_generator(gen, device, n, warmup=2)
    gen.close()
    del gen, loader  # shuts the persistent workers down
    emit(section="a_loader", batch=batch, num_workers=workers, batches=n,
         ms_per_batch=round(per_batch * 1e3, 2),
         frames_per_s=round(batch * T / per_batch, 1), device=str(device))


def bench_device_generator(batch, device, n):
    cfg = make_cfg(batch, device, mnist_synth="device")
    train, _ = data_utils.load_dataset(cfg)
    gen = data_utils.get_data_generator(train, train=True,
                                        dynamic_length=False, opt=cfg)
    per_batch, host = time_generator(gen, device, n, warmup=3)
    emit(section="b_device_generator", batch=batch, batches=n,
         ms_per_batch=round(per_batch * 1e3, 2),
         host_ms_per_batch=round(host * 1e3, 2),
         frames_per_s=round(batch * T / per_batch, 1), device=str(device))
    return train


def bench_planner(train, batch, n):
    rng = np.random.RandomState(0)
    train.plan_batch(batch, rng)
    t0 = time.perf_counter()
    for _ in range(n):
        train.plan_batch(batch, rng)
    emit(section="c_planner", batch=batch, batches=n,
         ms_per_batch=round((time.perf_counter() - t0) / n * 1e3, 2))


def bench_kernel(train, batch, device, n):
    from p2pvg_amd.ops import _hip_ext_loader, moving_mnist_render

    ext = _hip_ext_loader.load()
    digits = train.digits.contiguous().to(device)
    idx, pos = train.plan_batch(batch, np.random.RandomState(1))
    moving_mnist_render(digits, idx, pos, S)  # validates this very plan
    idx_d, pos_d = idx.to(device), pos.to(device)
    for _ in range(5):
        out = ext.moving_mnist_render(digits, idx_d, pos_d, S)
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    start.record()
    for _ in range(n):
        out = ext.moving_mnist_render(digits, idx_d, pos_d, S)
    end.record()
    enqueue_us = (time.perf_counter() - t0) / n * 1e6
    torch.cuda.synchronize()
    us = start.elapsed_time(end) / n * 1e3
    nbytes = out.numel() * out.element_size()
    # enqueue_us close to us_per_call means the loop was launch-bound and
    # us_per_call is only an upper bound of the kernel's time
    emit(section="d_render_kernel", batch=batch, calls=n,
         us_per_call=round(us, 1), host_enqueue_us=round(enqueue_us, 1),
         out_mb=round(nbytes / 1e6, 1),
         out_gb_per_s=round(nbytes / us / 1e3, 1),
         frames_per_s=round(batch * T / us * 1e6, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[100, 256])
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--loader_iters", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()

    device = torch.device(args.device)
    if device.type == "cuda" and not torch.cuda.is_available():
        sys.exit("bench_mnist_synth: no GPU; these figures are only meaningful on one")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    torch.manual_seed(0)

    for batch in args.batches:
        for workers in (1, 8):
            bench_loader(batch, device, workers, args.loader_iters)
        train = bench_device_generator(batch, device, args.iters)
        bench_planner(train, batch, max(3, args.iters // 2))
        if device.type == "cuda":
            bench_kernel(train, batch, device, 2000)
        else:
            emit(section="d_render_kernel", batch=batch, note="not measured (no GPU)")


if __name__ == "__main__":
    main()
