#!/usr/bin/env python
"""Benchmark harness — the driver contract.

Measures the BASELINE.json headline metric: train frames/sec (whole node) on
the BAIR 64x64 / vgg_64 / seq_len=30 config, bf16 compute, synthetic data
(random-init weights; no network for datasets). A "step" is one full training
iteration: forward over the 30-step recurrence, both backward phases, all five
Adam steps — nothing is skipped inside the timed region.

Launch: python bench.py --gpus N --steps K --warmup W
  N>1 is launched by the driver via torch.distributed.run (one rank per GPU,
  RCCL over xGMI); this script reads RANK/LOCAL_RANK/WORLD_SIZE from the env.

A plain run does only what the headline figure needs: set up, warm up, time
the K steps, print the result line. Anything further the benchmark grows
(baselines, other configs, per-kernel figures) belongs behind --full.

--dump-outputs DIR writes what the last timed step produced, from rank 0:
  DIR/losses.npy         float32 (4,): the step's return value — per-frame
                         mean mse, kld, cpc, align losses
  DIR/params_sample.npy  float32 (<=2^20,): the model parameters the step
                         left behind, a fixed seeded sample of the flattened
                         parameter vector
Inputs, weights and the sampling noise are seeded, so the same arguments give
the same inputs run after run and two builds can be compared file for file.

Prints ONE JSON line from rank 0.
"""
from __future__ import annotations

import os
os.environ.setdefault("PYTORCH_ALLOC_CONF", "expandable_segments:True")
os.environ.setdefault("PYTORCH_HIP_ALLOC_CONF", "expandable_segments:True")

import argparse
import json
import os
import time

import numpy as np
import torch

from p2pvg_amd.core import Config
from p2pvg_amd.models import P2PModel


def make_synthetic_batch(cfg, device, seed: int):
    """Synthetic clip batch: (T, B, C, H, W) frames in [0,1] smooth in t, or
    (T, B, 17, 3) standardized skeletons for the h36m config."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    t, b = cfg.max_seq_len, cfg.batch_size
    if cfg.dataset == "h36m":
        base = torch.randn(1, b, 17, 3, generator=g)
        steps = torch.randn(t, b, 17, 3, generator=g) * 0.08
        return (base + steps.cumsum(0)).to(device)
    c, s = cfg.channels, cfg.image_width
    base = torch.rand(1, b, c, s, s, generator=g)
    drift = torch.randn(t, b, c, 1, 1, generator=g) * 0.05
    x = (base + drift.cumsum(0)).clamp_(0, 1)
    return x.to(device)


DUMP_PARAM_SAMPLE = 1 << 20   # elements; 4 MB as float32
DUMP_SAMPLE_SEED = 20240


def dump_outputs(out_dir: str, losses, model) -> None:
    """Write the last timed step's results as float32 .npy files."""
    os.makedirs(out_dir, exist_ok=True)
    vals = torch.stack([v.detach().float().reshape(()) for v in losses])
    np.save(os.path.join(out_dir, "losses.npy"), vals.cpu().numpy())
    flat = torch.cat([p.detach().reshape(-1).float() for p in model.parameters()])
    if flat.numel() > DUMP_PARAM_SAMPLE:
        g = torch.Generator(device="cpu").manual_seed(DUMP_SAMPLE_SEED)
        idx = torch.randint(0, flat.numel(), (DUMP_PARAM_SAMPLE,), generator=g)
        flat = flat[idx.sort().values.to(flat.device)]
    np.save(os.path.join(out_dir, "params_sample.npy"), flat.cpu().numpy())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch", type=int, default=512, help="per-GPU batch size "
               "(512: 13.4k f/s with ~90 GB headroom after the round-2 "
               "memory work; 640 measured within noise of 512)")
    p.add_argument("--seq_len", type=int, default=30)
    p.add_argument("--g_dim", type=int, default=128)
    p.add_argument("--backbone", type=str, default="vgg")
    p.add_argument("--image_width", type=int, default=64)
    p.add_argument("--dataset", type=str, default="bair")
    p.add_argument("--dtype", type=str, default="bf16")
    p.add_argument("--kernels", type=str, default="auto")
    p.add_argument("--channels_last", type=int, default=1,
                   help="NHWC activations/weights (MIOpen igemm is NHWC-native)")
    p.add_argument("--use_graphs", type=int, default=-1,
                   help="-1: auto (on for single-GPU CUDA)")
    p.add_argument("--dump-outputs", dest="dump_outputs", metavar="DIR",
                   default=None,
                   help="after the timed steps, write the last step's losses "
                        "and a seeded sample of the updated parameters to "
                        "DIR/*.npy (float32)")
    p.add_argument("--full", action="store_true",
                   help="also run every secondary measurement or check; the "
                        "benchmark has none yet, so this equals a plain run")
    args = p.parse_args()
    if args.dump_outputs is not None and args.steps < 1:
        p.error("--dump-outputs needs at least one timed step")

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", rank))

    use_cuda = torch.cuda.is_available()
    if args.kernels != "auto":
        os.environ["P2PVG_KERNELS"] = args.kernels

    dist = None
    if world > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        backend = "nccl" if use_cuda else "gloo"
        dist.init_process_group(backend=backend)
    if use_cuda:
        # oversubscription probe: N ranks on fewer GPUs (e.g. 2-rank RCCL on
        # one MI355X to exercise real collectives within a 1-GPU lease)
        dev_idx = local_rank % torch.cuda.device_count()
        torch.cuda.set_device(dev_idx)
        device = torch.device(f"cuda:{dev_idx}")
    else:
        device = torch.device("cpu")

    cfg = Config(
        g_dim=args.g_dim,
        dataset=args.dataset,
        backbone=args.backbone,
        image_width=args.image_width,
        channels=3 if args.dataset in ("bair", "weizmann") else 1,
        batch_size=args.batch,
        max_seq_len=args.seq_len,
        skip_prob=0.0,       # fixed-length timing: every step does full work
        weight_align=0.5,
        weight_cpc=100.0,
        dtype=args.dtype if use_cuda else "fp32",
        device=str(device),
        ddp=world > 1,
        use_graphs=(args.use_graphs == 1 or (args.use_graphs == -1 and world == 1))
        and use_cuda,
    )
    if args.dataset == "h36m":
        cfg.backbone = "mlp"

    torch.manual_seed(1234 + rank)
    np.random.seed(1234 + rank)

    model = P2PModel(cfg).to(device)
    if args.channels_last and use_cuda and args.dataset != "h36m":
        model = model.to(memory_format=torch.channels_last)
    if world > 1:
        from p2pvg_amd.parallel import DDPGradSync

        sync = DDPGradSync(model, bucket_mb=cfg.bucket_mb)
        sync.broadcast_parameters()

    x = make_synthetic_batch(cfg, device, seed=1234 + rank)
    if args.channels_last and use_cuda and args.dataset != "h36m":
        # store the clip NHWC so each x[i] is a channels_last (B,C,H,W) view
        t, b, c, h, w = x.shape
        nhwc = torch.empty(t, b, h, w, c, device=device, dtype=x.dtype)
        nhwc.copy_(x.permute(0, 1, 3, 4, 2))
        x = nhwc.permute(0, 1, 4, 2, 3)
    amp = cfg.dtype == "bf16" and use_cuda

    if cfg.use_graphs:
        from p2pvg_amd.runtime import GraphedTrainStep

        stepper = GraphedTrainStep(
            model, amp_dtype=torch.bfloat16 if amp else None
        )

        def one_step():
            return stepper.step(x)

    else:

        def one_step():
            model.zero_grad(set_to_none=False)
            if amp:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return model(x, 0, len(x) - 1)
            return model(x, 0, len(x) - 1)

    # warmup
    for _ in range(args.warmup):
        one_step()

    if world > 1:
        dist.barrier()
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for _ in range(args.steps):
        last = one_step()
    if use_cuda:
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0

    # max over ranks
    if world > 1:
        t = torch.tensor([elapsed], device=device if use_cuda else None)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if args.dump_outputs is not None and rank == 0:
        dump_outputs(args.dump_outputs, last, model)

    global_batch = args.batch * world
    frames = global_batch * args.seq_len * args.steps
    fps = frames / elapsed

    if use_cuda:
        import sys

        if cfg.use_graphs:
            print(f"[bench] rank {rank} graphs: {len(stepper.graphs)} captured, "
                  f"{len(stepper.eager_keys)} eager keys", file=sys.stderr)
        print(
            f"[bench] rank {rank} peak GB: "
            f"allocated {torch.cuda.max_memory_allocated() / 2**30:.1f} "
            f"reserved {torch.cuda.max_memory_reserved() / 2**30:.1f}",
            file=sys.stderr,
        )
    if rank == 0:
        result = {
            "metric": "train_frames_per_sec",
            "value": fps,
            "unit": "frames/s",
            "n_gpus": world if use_cuda else 0,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": cfg.dtype,
            "data": "synthetic",
            "config": {
                "model": ("p2pvg_h36m_mlp" if args.dataset == "h36m" else f"p2pvg_{args.backbone}_{args.image_width}"),
                "dataset": args.dataset,
                "global_batch": global_batch,
                "seq_len": args.seq_len,
                "parallelism": f"dp{world}",
            },
        }
        print(json.dumps(result))

    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
