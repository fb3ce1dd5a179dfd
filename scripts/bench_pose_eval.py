#!/usr/bin/env python
"""Pose evaluation: ops.pose_metrics / ops.pose_spread (HIP) against the torch
path, and the cost of generating N samples at several fold widths.

Run on a GPU box:  python scripts/bench_pose_eval.py [--sections ...]

Every figure comes from a child process of its own, each under a time limit; a
child that fails or runs out of time ends the whole script (nothing more is
started on the GPU). One JSON line per figure.

  percall    pose_metrics and pose_spread on (T,S,B,J) = (30,100,1024,17) and
             (30,100,10,17), fp32 poses, one child per shape: kernel path and
             P2PVG_KERNELS=torch path alternating, three runs each after a
             warm-up of both, device-event time per call, min/median/max over
             the runs, and pose_metrics' share of the read-bandwidth floor
             (bytes of both operands over the measured 6.29 TB/s
             streaming-read rate of an MI355X)
  fold       evaluate_pose.py on a fresh h36m checkpoint (synthetic poses),
             --nsample 100, --sample_chunk 1 / 4 / 16 / 100 alternating, for
             batch sizes 10 and 256, fp32 and bf16: seconds_generate
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
SHAPES = [(30, 100, 1024, 17), (30, 100, 10, 17)]
TOY_SHAPES = [(4, 5, 6, 17), (4, 5, 2, 17)]
AXIS_SCALE = (0.5, 1.25, 3.0)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def spread(vals):
    return {"min": round(min(vals), 4), "median": round(statistics.median(vals), 4),
            "max": round(max(vals), 4)}


# ---------------------------------------------------------------------------
# percall (child): one shape
# ---------------------------------------------------------------------------

def child_percall(device, shape, runs):
    import torch

    from p2pvg_amd.ops import pose_metrics, pose_spread

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

    T, S, B, J = shape
    g = torch.Generator().manual_seed(0)
    ref = (3.0 * torch.randn(T, B, J, 3, generator=g)).to(dev)
    gen = ref.unsqueeze(1) + 0.3 * torch.randn(T, S, B, J, 3, generator=g).to(dev)
    nbytes = gen.numel() * gen.element_size() + ref.numel() * ref.element_size()
    floor_ms = nbytes / HBM_READ_BYTES_PER_S * 1e3

    ops = {"pose_metrics": lambda: pose_metrics(gen, ref, AXIS_SCALE),
           "pose_spread": lambda: (pose_spread(gen, AXIS_SCALE),)}
    for op, fn in ops.items():
        def call(backend):
            os.environ["P2PVG_KERNELS"] = backend
            return fn()

        calls = {"auto": 20 if cuda else 1, "torch": 2 if cuda else 1}
        for backend in ("auto", "torch"):  # warm-up, both paths
            timed(lambda: call(backend), 2 if cuda else 1)
        ms = {"auto": [], "torch": []}
        outs = {}
        for _ in range(runs):
            for backend in ("auto", "torch"):  # alternating
                t, outs[backend] = timed(lambda: call(backend), calls[backend])
                ms[backend].append(t)
        rel = max(float(((k - t).abs() / t).max())
                  for k, t in zip(outs["auto"], outs["torch"]))
        extra = {}
        if op == "pose_metrics":
            extra = dict(operand_mb=round(nbytes / 1e6, 1),
                         read_floor_ms=round(floor_ms, 4),
                         kernel_share_of_read_floor=round(
                             floor_ms / statistics.median(ms["auto"]), 3))
        emit(section="percall", op=op, shape=list(shape), dtype="fp32",
             device=device, runs=runs, calls_per_run=calls,
             kernel_ms=spread(ms["auto"]), torch_ms=spread(ms["torch"]),
             speedup_median=round(statistics.median(ms["torch"])
                                  / statistics.median(ms["auto"]), 2),
             worst_case_speedup=round(min(ms["torch"]) / max(ms["auto"]), 2),
             max_rel_diff=rel, **extra)


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
        sys.exit(f"bench_pose_eval: time limit of {limit}s hit by {cmd}")
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"bench_pose_eval: exit {r.returncode} from {cmd}")
    return r.stdout


def section_percall(args):
    shapes = TOY_SHAPES if args.device == "cpu" else SHAPES
    for shape in shapes:
        out = run([sys.executable, os.path.abspath(__file__), "--child", "percall",
                   "--shape", *map(str, shape), "--device", args.device,
                   "--runs", str(args.runs)], args.limit)
        sys.stdout.write(out)
        sys.stdout.flush()


def section_fold(args):
    import torch

    from p2pvg_amd.core import Config
    from p2pvg_amd.models import P2PModel

    toy = args.device == "cpu"
    nsample = 6 if toy else 100
    chunks = [1, 4, nsample] if toy else [1, 4, 16, nsample]
    cfg = Config(dataset="h36m", backbone="mlp", batch_size=64, max_seq_len=30,
                 skip_prob=0.0, data_root="/nonexistent", num_workers=0,
                 **(dict(g_dim=32, z_dim=4, rnn_size=32) if toy else {}))
    with tempfile.TemporaryDirectory() as tmp:
        ckpt = os.path.join(tmp, "h36m_mlp.pth")
        torch.manual_seed(0)
        P2PModel(cfg).save(ckpt, 0)
        for dtype in (["fp32"] if toy else ["fp32", "bf16"]):
            for bs in ([3] if toy else [10, 256]):
                secs = {c: [] for c in chunks}
                for rep in range(args.runs):
                    for c in chunks:  # alternating
                        out_json = os.path.join(tmp, "eval.json")
                        run([sys.executable, os.path.join(ROOT, "evaluate_pose.py"),
                             "--ckpt", ckpt, "--nsample", str(nsample),
                             "--sample_chunk", str(c), "--batch_size", str(bs),
                             "--n_batches", "1", "--device", args.device,
                             "--dtype", dtype, "--seed", "1", "--out", out_json],
                            args.limit)
                        with open(out_json) as f:
                            res = json.load(f)
                        secs[c].append(res["seconds_generate"])
                        emit(section="fold", run=rep, dtype=res["dtype"],
                             batch_size=res["n_sequences"], nsample=res["nsample"],
                             sample_chunk=res["sample_chunk"],
                             kernel_backend=res["kernel_backend"],
                             seconds_generate=round(res["seconds_generate"], 4),
                             seconds_score=round(res["seconds_score"], 4))
                emit(section="fold_summary", dtype=dtype, batch_size=bs,
                     nsample=nsample,
                     seconds_generate={str(c): spread(v) for c, v in secs.items()})


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
    ap.add_argument("--sections", nargs="+", default=["percall", "fold", "noregress"],
                    choices=["percall", "fold", "noregress"])
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent_tree", default="",
                    help="built checkout of the parent commit (noregress)")
    ap.add_argument("--limit", type=int, default=420,
                    help="time limit of every child process, seconds")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--shape", type=int, nargs=4, help=argparse.SUPPRESS)
    args = ap.parse_args()

    if args.child == "percall":
        child_percall(args.device, tuple(args.shape), args.runs)
        return
    if args.device != "cpu":
        import torch

        if not torch.cuda.is_available():
            sys.exit("bench_pose_eval: no GPU; these figures are only "
                     "meaningful on one")
    for s in args.sections:
        {"percall": section_percall, "fold": section_fold,
         "noregress": section_noregress}[s](args)


if __name__ == "__main__":
    main()
