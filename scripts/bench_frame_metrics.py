#!/usr/bin/env python
"""ops.frame_metrics (fused HIP SSIM+MSE) against the torch path.

Run on a GPU box:  python scripts/bench_frame_metrics.py [--sections ...]

Every section runs in child processes of its own, each under a time limit; a
child that fails or runs out of time ends the whole script (nothing more is
started on the GPU). One JSON line per figure.

  percall    ops.frame_metrics on (30*256, 3, 64, 64) and (30*128, 3, 128, 128),
             channels_last bf16 against channels_last fp32 (a generated clip
             against the data generator's), kernel path and P2PVG_KERNELS=torch
             path alternating, three runs each after a warm-up, device-event
             time per call, min/median/max over the runs, and the kernel's
             share of the read-bandwidth floor (bytes of both operands over the
             measured 6.29 TB/s streaming-read rate of an MI355X)
  e2e        evaluate.py --nsample 10 on a fresh vgg_64 BAIR (synthetic data)
             checkpoint under both backends: seconds_generate / seconds_score
  noregress  python bench.py --gpus 1 --steps 20 --warmup 5 in this tree and in
             --parent_tree (a built checkout of the parent commit), three
             alternating runs each

`--device cpu` is a dry run of the script's own logic at toy sizes; its
figures say nothing about the GPU.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_READ_BYTES_PER_S = 6.29e12  # measured float4 streaming rate, not the 8 TB/s spec
SHAPES = [(30 * 256, 3, 64, 64), (30 * 128, 3, 128, 128)]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def spread(vals):
    return {"min": round(min(vals), 3), "median": round(statistics.median(vals), 3),
            "max": round(max(vals), 3)}


# ---------------------------------------------------------------------------
# percall (child)
# ---------------------------------------------------------------------------

def child_percall(device, shapes, runs):
    import torch

    from p2pvg_amd.ops import frame_metrics

    dev = torch.device(device)
    cuda = dev.type == "cuda"

    def timed(fn, n):
        if cuda:
            start = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(n):
                out = fn()
            end.record()
            torch.cuda.synchronize()
            return start.elapsed_time(end) / n, out
        import time

        t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        return (time.perf_counter() - t0) * 1e3 / n, out

    for shape in shapes:
        M, C, H, W = shape
        g = torch.Generator().manual_seed(0)
        # built like get_generator's CUDA branch: NHWC storage, NCHW view
        b = torch.rand(M, H, W, C, generator=g).to(dev).permute(0, 3, 1, 2)
        a = (b + 0.05 * torch.randn(M, C, H, W, generator=g).to(dev)).clamp(0, 1)
        a = a.bfloat16().contiguous(memory_format=torch.channels_last)
        nbytes = a.numel() * a.element_size() + b.numel() * b.element_size()
        floor_ms = nbytes / HBM_READ_BYTES_PER_S * 1e3

        def call(backend):
            os.environ["P2PVG_KERNELS"] = backend
            return frame_metrics(a, b)

        calls = {"auto": 100 if cuda else 1, "torch": 5 if cuda else 1}
        for backend in ("auto", "torch"):  # warm-up, both paths
            timed(lambda: call(backend), 3 if cuda else 1)
        ms = {"auto": [], "torch": []}
        outs = {}
        for _ in range(runs):
            for backend in ("auto", "torch"):  # alternating
                t, outs[backend] = timed(lambda: call(backend), calls[backend])
                ms[backend].append(t)
        d_ssim = float((outs["auto"][0] - outs["torch"][0]).abs().max())
        rel_mse = float(((outs["auto"][1] - outs["torch"][1]).abs()
                         / outs["torch"][1]).max())
        emit(section="percall", shape=list(shape), pairing="channels_last bf16 / fp32",
             device=device, runs=runs, calls_per_run=calls,
             kernel_ms=spread(ms["auto"]), torch_ms=spread(ms["torch"]),
             speedup_median=round(statistics.median(ms["torch"])
                                  / statistics.median(ms["auto"]), 2),
             worst_case_speedup=round(min(ms["torch"]) / max(ms["auto"]), 2),
             operand_mb=round(nbytes / 1e6, 1),
             read_floor_ms=round(floor_ms, 4),
             kernel_share_of_read_floor=round(floor_ms / statistics.median(ms["auto"]), 3),
             max_abs_ssim_diff=d_ssim, max_rel_mse_diff=rel_mse)


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------

def run(cmd, limit, env=None, cwd=ROOT):
    """One child under its own time limit; anything but a clean exit ends the
    script, so nothing further starts on a GPU that may be in trouble."""
    full_env = os.environ.copy()
    full_env["PYTHONPATH"] = cwd
    full_env.update(env or {})
    try:
        r = subprocess.run(cmd, cwd=cwd, env=full_env, capture_output=True,
                           text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_frame_metrics: time limit of {limit}s hit by {cmd}")
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"bench_frame_metrics: exit {r.returncode} from {cmd}")
    return r.stdout


def section_percall(args):
    out = run([sys.executable, os.path.abspath(__file__), "--child", "percall",
               "--device", args.device, "--runs", str(args.runs)], args.limit)
    sys.stdout.write(out)
    sys.stdout.flush()


def section_e2e(args):
    import torch

    from p2pvg_amd.core import Config
    from p2pvg_amd.models import P2PModel

    toy = args.device == "cpu"
    cfg = Config(dataset="bair", backbone="vgg", image_width=64, channels=3,
                 batch_size=2 if toy else 256, max_seq_len=6 if toy else 30,
                 g_dim=128, skip_prob=0.0, data_root="/nonexistent",
                 num_workers=0 if toy else 1)
    with tempfile.TemporaryDirectory() as tmp:
        ckpt = os.path.join(tmp, "vgg64_bair.pth")
        torch.manual_seed(0)
        P2PModel(cfg).save(ckpt, 0)
        for rep in range(args.e2e_runs):
            for backend in ("auto", "torch"):  # alternating
                out_json = os.path.join(tmp, f"eval_{backend}_{rep}.json")
                run([sys.executable, os.path.join(ROOT, "evaluate.py"),
                     "--ckpt", ckpt, "--nsample", "2" if toy else "10",
                     "--n_batches", "1", "--device", args.device,
                     "--dtype", args.e2e_dtype, "--seed", "1", "--out", out_json],
                    args.limit, env={"P2PVG_KERNELS": backend})
                with open(out_json) as f:
                    res = json.load(f)
                emit(section="e2e", run=rep, P2PVG_KERNELS=backend,
                     kernel_backend=res["kernel_backend"], dtype=res["dtype"],
                     nsample=res["nsample"], n_sequences=res["n_sequences"],
                     seq_len=res["seq_len"], data_synthetic=res["data_synthetic"],
                     seconds_generate=round(res["seconds_generate"], 3),
                     seconds_score=round(res["seconds_score"], 3),
                     end_frame_ssim_best=res["end_frame_ssim_best"])


def section_noregress(args):
    trees = [("this", ROOT)]
    if args.parent_tree:
        trees.insert(0, ("parent", os.path.abspath(args.parent_tree)))
    else:
        emit(section="noregress", note="no --parent_tree: this tree only")
    values = {name: [] for name, _ in trees}
    for rep in range(args.runs):
        for name, tree in trees:  # alternating
            out = run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1",
                       "--steps", "20", "--warmup", "5"], args.limit, cwd=tree)
            line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
            res = json.loads(line)
            values[name].append(res["value"])
            emit(section="noregress", tree=name, run=rep, metric=res["metric"],
                 value=round(res["value"], 1), ms_per_step=round(res["ms_per_step"], 2))
    for name, vals in values.items():
        emit(section="noregress_summary", tree=name, frames_per_s=spread(vals),
             spread_pct=round(100 * (max(vals) - min(vals)) / statistics.median(vals), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", nargs="+", default=["percall", "e2e", "noregress"],
                    choices=["percall", "e2e", "noregress"])
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--e2e_runs", type=int, default=1)
    ap.add_argument("--e2e_dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--parent_tree", default="",
                    help="built checkout of the parent commit (noregress)")
    ap.add_argument("--limit", type=int, default=420,
                    help="time limit of every child process, seconds")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()

    if args.child == "percall":
        shapes = SHAPES if args.device != "cpu" else [(4, 3, 64, 64), (2, 3, 128, 128)]
        child_percall(args.device, shapes, args.runs)
        return
    if args.device != "cpu":
        import torch

        if not torch.cuda.is_available():
            sys.exit("bench_frame_metrics: no GPU; these figures are only "
                     "meaningful on one")
    for s in args.sections:
        {"percall": section_percall, "e2e": section_e2e,
         "noregress": section_noregress}[s](args)


if __name__ == "__main__":
    main()
