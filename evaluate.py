#!/usr/bin/env python
"""Evaluation CLI: best-of-N SSIM/PSNR curves for a checkpoint.

The standard stochastic video prediction protocol: draw --nsample samples per
test sequence, score every generated frame against the ground truth (SSIM and
PSNR, one fused HIP pass per sample on GPU), keep the best sample per sequence
and report the per-timestep curves plus the end-frame score at the control
point. Rebuilds the model from the checkpoint's own config, as generate.py
does, and writes everything to --out as JSON.

    python evaluate.py --ckpt logs/.../model.pth --nsample 100 --out eval.json
"""
from __future__ import annotations

import argparse
import json
import random
import sys

import numpy as np
import torch

from p2pvg_amd import data as data_utils
from p2pvg_amd import ops
from p2pvg_amd.models import P2PModel
from p2pvg_amd.utils import config_from_states, load_checkpoint
from p2pvg_amd.utils.evaluation import evaluate_model


def main(argv=None) -> int:
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--ckpt", type=str, required=True, help="model .pth file")
    parser.add_argument("--data_root", type=str, default=None,
                        help="dataset root (default: the checkpoint's)")
    parser.add_argument("--nsample", type=int, default=100,
                        help="samples drawn per test sequence")
    parser.add_argument("--n_batches", type=int, default=1)
    parser.add_argument("--batch_size", type=int, default=None,
                        help="sequences per batch (default: the checkpoint's)")
    parser.add_argument("--model_mode", type=str, default="full",
                        choices=["full", "posterior", "prior"])
    parser.add_argument("--seed", type=int, default=1)
    parser.add_argument("--device", type=str, default="auto")
    parser.add_argument("--dtype", type=str, default="fp32", choices=["fp32", "bf16"],
                        help="bf16 wraps generation in autocast (GPU only)")
    parser.add_argument("--frame_cache", type=str, default="loader",
                        choices=["loader", "device"],
                        help="device: keep the decoded test frames on the device "
                             "(bair only); always overrides the checkpoint's value")
    parser.add_argument("--out", type=str, default="eval.json")
    args = parser.parse_args(argv)

    states = load_checkpoint(args.ckpt)
    cfg = config_from_states(states)
    if cfg.dataset == "h36m":
        print("evaluate.py scores images (SSIM/PSNR); dataset 'h36m' holds "
              "poses, not images, and cannot be evaluated this way",
              file=sys.stderr)
        return 2
    cfg.device = args.device
    cfg.frame_cache = args.frame_cache
    if args.data_root is not None:
        cfg.data_root = args.data_root
    if args.batch_size is not None:
        cfg.batch_size = args.batch_size

    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(args.seed)

    device = torch.device(cfg.resolved_device())
    model = P2PModel(cfg).to(device)
    if device.type == "cuda":
        model = model.to(memory_format=torch.channels_last)
    model.load(states=states)
    model.eval()

    _, test_data = data_utils.load_dataset(cfg)
    generator = data_utils.get_data_generator(
        test_data, train=False, dynamic_length=False, opt=cfg)

    # bf16: autocast around generation only; frames are scored in fp32
    bf16 = args.dtype == "bf16" and device.type == "cuda"
    result = evaluate_model(model, generator, args.n_batches, args.nsample,
                            args.model_mode,
                            amp_dtype=torch.bfloat16 if bf16 else None)

    n_curve = len(result["ssim_best"])
    result.update(
        dataset=cfg.dataset,
        data_synthetic=bool(getattr(test_data, "synthetic", False)),
        ckpt=args.ckpt,
        model_mode=args.model_mode,
        nsample=args.nsample,
        n_past=cfg.n_past,
        seq_len=cfg.n_past + n_curve,
        seed=args.seed,
        dtype=args.dtype if device.type == "cuda" else "fp32",
        device=str(device),
        kernel_backend=ops.frame_metrics_backend(device),
    )

    def fmt(v):
        return (" ".join(f"{u:.4f}" for u in v) if isinstance(v, list) else f"{v:.4f}")

    print(f"[eval] {cfg.dataset}{' (synthetic data)' if result['data_synthetic'] else ''}: "
          f"{result['n_sequences']} sequences x {args.nsample} samples, "
          f"frames {cfg.n_past}..{result['seq_len'] - 1}, mode {args.model_mode}, "
          f"backend {result['kernel_backend']}")
    for key in ("ssim_best", "ssim_mean", "psnr_best", "psnr_mean",
                "end_frame_ssim_best", "end_frame_ssim_mean",
                "end_frame_psnr_best", "end_frame_psnr_mean"):
        print(f"{key}: {fmt(result[key])}")
    print(f"seconds_generate: {result['seconds_generate']:.3f}  "
          f"seconds_score: {result['seconds_score']:.3f}")
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"[eval] wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
