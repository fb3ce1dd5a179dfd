#!/usr/bin/env python
"""BAIR input pipeline: DataLoader path vs the device-resident frame cache.

Run on a GPU box: python scripts/bench_bair_cache.py [--sections a b c d]

The driver writes a PNG tree into a temporary directory (512 train clips x 30
frames, 64x64 RGB, smooth content plus mild noise; NOT BAIR's own frames, so
the decode figures are an order of magnitude, not BAIR's) and then runs every
measurement as a child process under its own `timeout`, stopping at the first
failure. Nothing is sized by os.cpu_count(): worker counts are given
explicitly and never exceed 16.

  (a) loader     frames/s of the default path at batch 512 (PIL decode in
                 DataLoader workers, collate, pinned HtoD, device permute),
                 num_workers 1, 8 and 16, GPU otherwise idle
  (b) device     frames/s of the --frame_cache device generator and its host
                 time per batch (plan + validate + enqueue, no device wait)
  (c) kernel     clip_gather alone at (30, 512, 3, 64, 64), us per call and
                 output GB/s from device events, next to moving_mnist_render
                 writing the same number of output bytes in the same process
  (d) train      short train.py runs (bair, vgg, batch 512, bf16,
                 --use_graphs, fixed length, 3 epochs x 20 iterations) under
                 loader with 1 and 16 workers and under device, frames/s per
                 epoch, next to one bench.py headline run

One JSON line per figure.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, S, C = 30, 64, 3
CLIPS, TEST_CLIPS = 512, 16
BATCH = 512
MAX_WORKERS = 16


def emit(**kw):
    print(json.dumps(kw), flush=True)


# -- the PNG tree --------------------------------------------------------------

def _write_clip(task):
    import numpy as np
    from PIL import Image

    d, seed = task
    rng = np.random.RandomState(seed)
    os.makedirs(d)
    # a smooth field (8x8 control points, bilinear to 64x64) that drifts from
    # frame to frame, plus +-4 levels of noise: PNG-compressible like a photo
    ctrl = rng.rand(8, 8, C)
    drift = rng.randn(8, 8, C) * 0.01
    for i in range(T):
        field = np.asarray(Image.fromarray(
            np.uint8(np.clip(ctrl + i * drift, 0, 1) * 255), "RGB").resize(
                (S, S), Image.BILINEAR), dtype=np.int16)
        px = np.clip(field + rng.randint(-4, 5, field.shape), 0, 255)
        Image.fromarray(px.astype(np.uint8), "RGB").save(os.path.join(d, f"{i}.png"))


def write_tree(root, workers):
    import multiprocessing as mp

    tasks = []
    for split, n in (("train", CLIPS), ("test", TEST_CLIPS)):
        for k in range(n):
            d = os.path.join(root, "bair", "processed_data", split,
                             f"traj_{k // 256}", str(k % 256))
            tasks.append((d, len(tasks)))
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(workers) as pool:
        pool.map(_write_clip, tasks, chunksize=8)
    emit(section="tree", clips=CLIPS, test_clips=TEST_CLIPS, frames_per_clip=T,
         size=S, workers=workers, seconds=round(time.perf_counter() - t0, 1))


# -- children ------------------------------------------------------------------

def make_cfg(root, **kw):
    from p2pvg_amd.core import Config

    return Config(dataset="bair", channels=C, image_width=S, max_seq_len=T,
                  delta_len=5, batch_size=BATCH, data_root=root, device="cuda",
                  **kw)


def time_generator(gen, n, warmup):
    """(seconds per batch incl. device completion, host seconds per batch)."""
    import torch

    for _ in range(warmup):
        x = next(gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        x = next(gen)
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    assert x.shape == (T, BATCH, C, S, S)
    return t_all / n, t_host / n


def child_loader(args):
    import torch

    from p2pvg_amd import data as data_utils

    cfg = make_cfg(args.root, num_workers=args.workers)
    train, _ = data_utils.load_dataset(cfg)
    assert not train.synthetic
    loader = data_utils._make_loader(train, BATCH, cfg)
    gen = data_utils.get_generator(loader, torch.device("cuda"), dynamic_length=False)
    # every worker builds whole batches and the loader keeps two per worker
    # in flight: drain those first, so that the timed batches arrive at the
    # rate the workers produce them
    per_batch, _ = time_generator(gen, args.iters, warmup=2 * max(1, args.workers))
    gen.close()
    del gen, loader  # shuts the persistent workers down
    emit(section="a_loader", batch=BATCH, num_workers=args.workers,
         batches=args.iters, ms_per_batch=round(per_batch * 1e3, 1),
         frames_per_s=round(BATCH * T / per_batch, 1))


def child_device(args):
    import torch

    from p2pvg_amd import data as data_utils

    cfg = make_cfg(args.root, frame_cache="device")
    train, _ = data_utils.load_dataset(cfg)
    t0 = time.perf_counter()
    gen = data_utils.get_data_generator(train, train=True, dynamic_length=False,
                                        opt=cfg)
    torch.cuda.synchronize()
    setup = time.perf_counter() - t0
    per_batch, host = time_generator(gen, args.iters, warmup=3)
    emit(section="b_device_generator", batch=BATCH, batches=args.iters,
         setup_seconds=round(setup, 2), ms_per_batch=round(per_batch * 1e3, 3),
         host_ms_per_batch=round(host * 1e3, 3),
         frames_per_s=round(BATCH * T / per_batch, 1))


def _time_calls(fn, n):
    import torch

    for _ in range(5):
        out = fn()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    start.record()
    for _ in range(n):
        out = fn()
    end.record()
    enqueue_us = (time.perf_counter() - t0) / n * 1e6
    torch.cuda.synchronize()
    us = start.elapsed_time(end) / n * 1e3
    nbytes = out.numel() * out.element_size()
    # host_enqueue_us close to us_per_call means the loop was launch-bound and
    # us_per_call is only an upper bound of the kernel's time
    return dict(calls=n, us_per_call=round(us, 1),
                host_enqueue_us=round(enqueue_us, 1),
                out_mb=round(nbytes / 1e6, 1),
                out_gb_per_s=round(nbytes / us / 1e3, 1))


def child_kernel(args):
    import numpy as np
    import torch

    from p2pvg_amd import data as data_utils
    from p2pvg_amd.data.moving_mnist import DynamicLengthMovingMNIST
    from p2pvg_amd.ops import _hip_ext_loader, clip_gather, moving_mnist_render

    ext = _hip_ext_loader.load()
    cfg = make_cfg(args.root)
    train, _ = data_utils.load_dataset(cfg)
    bank = data_utils.upload_frame_bank(train.load_pack(), "cuda")
    idx = train.plan_batch(BATCH, np.random.RandomState(1))
    got = clip_gather(bank, idx, T)  # validates this very call
    idx_d = idx.cuda()
    emit(section="c_clip_gather", shape=list(got.shape),
         **_time_calls(lambda: ext.clip_gather(bank, idx_d, T), args.iters))

    # the render kernel writing the same number of bytes: 30 x 1536 images of
    # 64x64 fp32 = 30 x 512 x 3 x 64 x 64 floats
    mnist = DynamicLengthMovingMNIST(train=True, data_root="/nonexistent",
                                     max_seq_len=T, delta_len=5, image_size=S,
                                     deterministic=False, num_digits=2)
    digits = mnist.digits.contiguous().cuda()
    midx, mpos = mnist.plan_batch(BATCH * C, np.random.RandomState(1))
    moving_mnist_render(digits, midx, mpos, S)  # validates this very plan
    midx_d, mpos_d = midx.cuda(), mpos.cuda()
    emit(section="c_render_yardstick", images=T * BATCH * C,
         **_time_calls(lambda: ext.moving_mnist_render(digits, midx_d, mpos_d, S),
                       args.iters))


def child_train(args):
    """train.py as a grandchild (it owns its GPU context); per-epoch frames/s
    come from its own log lines."""
    log_dir = os.path.join(args.root, "logs", f"{args.mode}_{args.workers}")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"),
           "--dataset", "bair", "--channels", str(C), "--backbone", "vgg",
           "--batch_size", str(BATCH), "--dtype", "bf16", "--use_graphs",
           "--max_seq_len", str(T), "--delta_len", "0",
           # bench.py's settings: every step does full work
           "--skip_prob", "0", "--weight_align", "0.5", "--weight_cpc", "100",
           "--nepochs", str(args.epochs), "--epoch_size", str(args.epoch_size),
           "--qual_iter", "100000", "--quan_iter", "100000",
           "--frame_cache", args.mode, "--num_workers", str(args.workers),
           "--data_root", args.root, "--log_dir", log_dir, "--device", "cuda"]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(r.returncode)
    rates = [float(m) for m in re.findall(r"([0-9.]+) frames/s", r.stdout + r.stderr)]
    assert len(rates) == args.epochs, (rates, r.stdout[-2000:], r.stderr[-2000:])
    emit(section="d_train", frame_cache=args.mode, num_workers=args.workers,
         epochs=args.epochs, epoch_size=args.epoch_size,
         frames_per_s_by_epoch=rates, wall_seconds=round(time.perf_counter() - t0, 1))


def child_headline(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", str(args.iters), "--warmup", "5"],
                       cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(r.returncode)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    emit(section="d_headline", bench=json.loads(line))


CHILDREN = {"loader": child_loader, "device": child_device, "kernel": child_kernel,
            "train": child_train, "headline": child_headline}


# -- driver --------------------------------------------------------------------

def run_child(limit, *argv):
    """One measurement in a fresh process under `timeout`; False stops the run."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable,
           os.path.abspath(__file__)] + [str(a) for a in argv]
    rc = subprocess.run(cmd, cwd=ROOT).returncode
    if rc != 0:
        emit(section="failed", argv=[str(a) for a in argv], exit_code=rc)
    return rc == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", nargs="+", default=["a", "b", "c", "d"],
                    choices=["a", "b", "c", "d"])
    ap.add_argument("--loader_workers", type=int, nargs="+", default=[1, 8, 16])
    ap.add_argument("--train_loader_workers", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--loader_iters", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--epoch_size", type=int, default=20)
    ap.add_argument("--headline_steps", type=int, default=20)
    ap.add_argument("--tree_workers", type=int, default=8)
    # child mode
    ap.add_argument("--child", choices=list(CHILDREN))
    ap.add_argument("--root")
    ap.add_argument("--workers", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--mode", default="loader")
    args = ap.parse_args()
    for w in args.loader_workers + args.train_loader_workers + [args.workers, args.tree_workers]:
        if not 0 <= w <= MAX_WORKERS:
            sys.exit(f"bench_bair_cache: at most {MAX_WORKERS} workers, got {w}")

    if args.child:
        import torch

        if not torch.cuda.is_available():
            sys.exit("bench_bair_cache: no GPU; these figures are only meaningful on one")
        torch.set_num_threads(min(MAX_WORKERS, torch.get_num_threads()))
        torch.manual_seed(0)
        CHILDREN[args.child](args)
        return 0

    with tempfile.TemporaryDirectory(prefix="bair_cache_bench_") as root:
        write_tree(root, max(1, args.tree_workers))
        steps = []
        if "a" in args.sections:
            for w in args.loader_workers:
                # 4 batches of 15360 PNG decodes per worker: 2 to drain the
                # prefetch queue, 2 timed (3 at the least)
                steps.append((240, "--child", "loader", "--workers", w,
                              "--iters", max(args.loader_iters, 2 * w)))
        if "b" in args.sections:
            steps.append((180, "--child", "device", "--iters", 50))
        if "c" in args.sections:
            steps.append((180, "--child", "kernel", "--iters", 200))
        if "d" in args.sections:
            per_run = 120 + args.epochs * args.epoch_size * 10
            steps.append((per_run, "--child", "train", "--mode", "device"))
            steps.append((300, "--child", "headline", "--iters", args.headline_steps))
            for w in args.train_loader_workers:
                steps.append((per_run, "--child", "train", "--mode", "loader",
                              "--workers", w))
        for limit, *argv in steps:
            common = ["--root", root, "--epochs", args.epochs,
                      "--epoch_size", args.epoch_size]
            if not run_child(limit, *argv, *common):
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
