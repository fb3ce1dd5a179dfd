"""End-to-end CLI tests: train.py one tiny epoch on CPU, then generate.py
consumes the written checkpoint (the §3.4 round-trip through both CLIs)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.slow
def test_train_then_generate(tmp_path):
    env = os.environ.copy()
    env["PYTHONPATH"] = ROOT
    log_dir = tmp_path / "logs" / "run"
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "train.py"),
         "--dataset", "mnist", "--backbone", "dcgan", "--batch_size", "2",
         "--max_seq_len", "6", "--delta_len", "1", "--g_dim", "32",
         "--z_dim", "4", "--rnn_size", "32", "--nepochs", "1",
         "--epoch_size", "3", "--nsample", "2", "--device", "cpu",
         "--data_root", "/nonexistent", "--num_workers", "0",
         "--log_dir", str(log_dir)],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
    )
    assert r.returncode == 0, r.stderr[-3000:]

    # locate the run dir (train.py appends the hyperparam suffix)
    runs = [d for d in (tmp_path / "logs").iterdir() if d.is_dir()]
    assert runs, "no log dir created"
    run = runs[0]
    ckpt = run / "model.pth"
    assert ckpt.exists(), f"missing latest checkpoint in {run}"
    assert (run / "model_0.pth").exists()
    assert (run / "cmd.txt").exists()
    assert (run / "scalars.jsonl").exists()
    vis = list((run / "gen_vis").glob("*.png"))
    assert vis, "no qualitative eval images written"
    gifs = list((run / "gen_vis").glob("*.gif"))
    assert gifs, "no GIFs written"

    # generate.py consumes the checkpoint with a frame-dir input
    frames_dir = tmp_path / "frames"
    frames_dir.mkdir()
    import numpy as np
    from PIL import Image

    for i in range(6):
        arr = (np.random.rand(64, 64, 3) * 255).astype("uint8")
        Image.fromarray(arr).save(frames_dir / f"{i:02d}.png")

    out_dir = tmp_path / "gen_out"
    r2 = subprocess.run(
        [sys.executable, os.path.join(ROOT, "generate.py"),
         "--ckpt", str(ckpt), "--video", str(frames_dir),
         "--output_root", str(out_dir), "--device", "cpu"],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
    )
    assert r2.returncode == 0, r2.stderr[-3000:]
    for length in (10, 20, 30):
        assert (out_dir / f"len_{length}-gt.png").exists()
        assert (out_dir / f"len_{length}-gen_full.gif").exists()

    # --start_img/--end_img pair input, off-size frames (auto-resized)
    import numpy as np
    from PIL import Image

    pair_dir = tmp_path / "pair"
    pair_dir.mkdir()
    for name in ("s.png", "e.png"):
        arr = (np.random.rand(32, 32, 3) * 255).astype("uint8")
        Image.fromarray(arr).save(pair_dir / name)
    pair_out = tmp_path / "gen_pair"
    rp = subprocess.run(
        [sys.executable, os.path.join(ROOT, "generate.py"),
         "--ckpt", str(ckpt), "--start_img", str(pair_dir / "s.png"),
         "--end_img", str(pair_dir / "e.png"),
         "--output_root", str(pair_out), "--device", "cpu"],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
    )
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert list(pair_out.glob("*.gif")), "no pair-input outputs"

    # --multi_cp and --loop modes (reference README demo flows)
    for flag, stem in (("--multi_cp", "multicpgen"), ("--loop", "loopgen")):
        mode_dir = tmp_path / f"gen_out_{stem}"
        r3 = subprocess.run(
            [sys.executable, os.path.join(ROOT, "generate.py"),
             "--ckpt", str(ckpt), "--video", str(frames_dir),
             "--output_root", str(mode_dir), "--device", "cpu", flag,
             "--segment_len", "4"],
            cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
        )
        assert r3.returncode == 0, r3.stderr[-3000:]
        pngs = list(mode_dir.glob("*.png"))
        gifs = list(mode_dir.glob("*.gif"))
        assert pngs and gifs, f"{flag}: no outputs in {mode_dir}"


@pytest.mark.slow
def test_bench_contract_cpu(tmp_path):
    env = os.environ.copy()
    env["PYTHONPATH"] = ROOT
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"),
         "--steps", "2", "--warmup", "1", "--batch", "2", "--seq_len", "6"],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
    )
    assert r.returncode == 0, r.stderr[-3000:]
    line = r.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in d, f"bench JSON missing {key}"
    assert d["data"] == "synthetic"
    assert d["config"]["global_batch"] == 2


def test_bench_dump_outputs_reproducible_cpu(tmp_path):
    """--dump-outputs writes the last timed step's losses and a sample of the
    updated parameters as float32 .npy; the same arguments give the same
    inputs, so two runs agree file for file. --steps is the number of timed
    steps, and --full is accepted. Pinned to the CPU path so the comparison
    is exact on every machine."""
    import numpy as np

    env = os.environ.copy()
    env["PYTHONPATH"] = ROOT
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    dumps = []
    for sub, extra in (("a", []), ("b", ["--full"])):
        out = tmp_path / sub / "dump"
        r = subprocess.run(
            [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
             "--steps", "2", "--warmup", "0", "--batch", "2", "--seq_len", "4",
             "--dump-outputs", str(out), *extra],
            cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
        )
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.strip().splitlines()
                 if ln.startswith("{")]
        assert len(lines) == 1, f"expected exactly one JSON line: {r.stdout}"
        d = json.loads(lines[0])
        assert d["steps"] == 2 and d["warmup"] == 0
        assert d["n_gpus"] == 0 and d["dtype"] == "fp32"
        assert d["ms_per_step"] > 0
        frames = d["config"]["global_batch"] * d["config"]["seq_len"] * 2
        assert d["value"] == pytest.approx(
            frames / (d["ms_per_step"] * 2 / 1000.0), rel=1e-6)
        assert sorted(p.name for p in out.iterdir()) == [
            "losses.npy", "params_sample.npy"]
        arrs = {p.name: np.load(p) for p in out.iterdir()}
        assert arrs["losses.npy"].shape == (4,)
        assert 0 < arrs["params_sample.npy"].size <= 1 << 20
        for a in arrs.values():
            assert a.dtype == np.float32 and np.isfinite(a).all()
        assert sum(a.nbytes for a in arrs.values()) <= 64 * 2**20
        dumps.append(arrs)
    for name in dumps[0]:
        np.testing.assert_allclose(dumps[0][name], dumps[1][name],
                                   rtol=1e-5, atol=1e-6, err_msg=name)


def test_phase_timing_harness_cpu():
    """SURVEY §5.1 per-phase timing harness runs on CPU and covers all six
    phases."""
    import numpy as np
    import torch

    from p2pvg_amd.core import Config
    from p2pvg_amd.models import P2PModel
    from p2pvg_amd.utils.phases import measure_phase_times

    cfg = Config(dataset="mnist", backbone="dcgan", channels=1, batch_size=2,
                 max_seq_len=6, g_dim=16, z_dim=4, rnn_size=32, device="cpu")
    torch.manual_seed(0)
    np.random.seed(0)
    model = P2PModel(cfg)
    x = torch.rand(6, 2, 1, 64, 64)
    times = measure_phase_times(model, x, iters=1, warmup=1)
    assert set(times) == {"htod", "forward", "bwd_nonprior", "bwd_prior",
                          "step_nonprior", "step_prior"}
    assert all(v >= 0 for v in times.values())


def test_read_video_mp4_dispatch(tmp_path):
    """.mp4 paths route to the mp4 decoder chain; with no backend installed
    the error names the optional dependencies (imageio / PyAV / ffmpeg)."""
    sys.path.insert(0, ROOT)
    try:
        import generate as gen_cli
    finally:
        sys.path.pop(0)
    p = tmp_path / "clip.mp4"
    p.write_bytes(b"\x00\x00\x00\x18ftypmp42")  # not a decodable file
    try:
        gen_cli.read_video(str(p))
    except RuntimeError as e:
        assert "mp4 backend" in str(e) or "imageio" in str(e)
    except Exception:
        # a real backend IS installed and rejected the bogus bytes — fine
        pass
    else:
        raise AssertionError("bogus mp4 should not decode")


def test_read_video_gif_roundtrip(tmp_path):
    import numpy as np
    from PIL import Image

    sys.path.insert(0, ROOT)
    try:
        import generate as gen_cli
    finally:
        sys.path.pop(0)
    frames = [Image.fromarray(np.full((8, 8, 3), v, dtype=np.uint8)) for v in (0, 128, 255)]
    p = tmp_path / "clip.gif"
    frames[0].save(p, save_all=True, append_images=frames[1:], duration=100)
    t = gen_cli.read_video(str(p))
    assert t.shape[0] == 3 and t.shape[1] == 1 and t.shape[2] == 3
    assert 0.0 <= float(t.min()) and float(t.max()) <= 1.0


def test_train_resume_from_checkpoint(tmp_path):
    """train.py --ckpt resumes into the SAME log dir at the next epoch
    (reference train.py resume contract: log dir and epoch both come from
    the checkpoint)."""
    env = os.environ.copy()
    env["PYTHONPATH"] = ROOT
    log_dir = tmp_path / "logs" / "run"
    flags = ["--dataset", "mnist", "--backbone", "dcgan", "--batch_size", "2",
             "--max_seq_len", "6", "--delta_len", "1", "--g_dim", "32",
             "--z_dim", "4", "--rnn_size", "32", "--epoch_size", "2",
             "--nsample", "2", "--device", "cpu", "--qual_iter", "100",
             "--data_root", "/nonexistent", "--num_workers", "0",
             "--log_dir", str(log_dir)]
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "train.py"), "--nepochs", "1",
         *flags],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
    )
    assert r.returncode == 0, r.stderr[-3000:]
    run = [d for d in (tmp_path / "logs").iterdir() if d.is_dir()][0]
    assert (run / "model_0.pth").exists()
    assert not (run / "model_1.pth").exists()

    r2 = subprocess.run(
        [sys.executable, os.path.join(ROOT, "train.py"), "--nepochs", "2",
         "--ckpt", str(run / "model.pth"), *flags],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
    )
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert "continuing at epoch 1" in (r2.stdout + r2.stderr)
    assert (run / "model_1.pth").exists(), "resume did not write epoch-1 ckpt"
    # resumed run landed in the original log dir, no second dir created
    assert len([d for d in (tmp_path / "logs").iterdir() if d.is_dir()]) == 1


def test_train_deterministic_cpu_bitwise(tmp_path):
    """Two identical --deterministic --seed runs produce bitwise-identical
    weights (the GPU counterpart over the native kernels:
    tests/test_managed_grads_gpu.py)."""
    import torch

    env = os.environ.copy()
    env["PYTHONPATH"] = ROOT
    outs = []
    for sub in ("a", "b"):
        log_dir = tmp_path / sub / "run"
        r = subprocess.run(
            [sys.executable, os.path.join(ROOT, "train.py"),
             "--dataset", "mnist", "--backbone", "dcgan", "--batch_size", "2",
             "--max_seq_len", "6", "--delta_len", "1", "--g_dim", "32",
             "--z_dim", "4", "--rnn_size", "32", "--nepochs", "1",
             "--epoch_size", "2", "--nsample", "2", "--device", "cpu",
             "--qual_iter", "100", "--deterministic", "--seed", "11",
             "--data_root", "/nonexistent", "--num_workers", "0",
             "--log_dir", str(log_dir)],
            cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
        )
        assert r.returncode == 0, r.stderr[-3000:]
        run = [d for d in (tmp_path / sub).iterdir() if d.is_dir()][0]
        outs.append(torch.load(run / "model.pth", map_location="cpu",
                               weights_only=False))
    sd_a = outs[0]["frame_predictor"], outs[0]["encoder"]
    sd_b = outs[1]["frame_predictor"], outs[1]["encoder"]
    for a, b in zip(sd_a, sd_b):
        for k in a:
            va, vb = a[k], b[k]
            if isinstance(va, torch.Tensor) and va.is_floating_point():
                assert torch.equal(va, vb), f"weights diverged at {k}"


def test_bench_distributed_2rank_gloo_cpu():
    """The exact multi-rank path the driver launches for SCALE runs:
    torch.distributed.run -> bench.py with world=2 (gloo on CPU here, RCCL
    on GPU boxes) — init, DDPGradSync, barriers, MAX-over-ranks timing,
    one JSON line from rank 0 with parallelism dp2. The ranks are pinned to
    the CPU/gloo path so the test also runs on a machine with fewer GPUs than
    ranks."""
    env = os.environ.copy()
    env["PYTHONPATH"] = ROOT
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29771", os.path.join(ROOT, "bench.py"),
         "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "2",
         "--seq_len", "6"],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=900,
    )
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines()
             if ln.startswith("{")]
    assert len(lines) == 1, f"expected exactly one JSON line: {r.stdout}"
    d = json.loads(lines[0])
    assert d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 4  # 2 ranks x per-rank batch 2
    assert d["value"] > 0 and d["ms_per_step"] > 0


def test_train_ddp_2rank_gloo_cpu(tmp_path):
    """train.py under torch.distributed.run with 2 CPU ranks (gloo): real
    setup_distributed + per-rank data seeds + DDPGradSync in the epoch loop;
    rank 0 owns logging/checkpoints. The ranks are pinned to the CPU/gloo
    path so the test also runs on a machine with fewer GPUs than ranks."""
    env = os.environ.copy()
    env["PYTHONPATH"] = ROOT
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    log_dir = tmp_path / "logs" / "run"
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29772", os.path.join(ROOT, "train.py"),
         "--dataset", "mnist", "--backbone", "dcgan", "--batch_size", "2",
         "--max_seq_len", "6", "--delta_len", "1", "--g_dim", "32",
         "--z_dim", "4", "--rnn_size", "32", "--nepochs", "1",
         "--epoch_size", "2", "--nsample", "2", "--device", "cpu",
         "--qual_iter", "100", "--ddp", "--data_root", "/nonexistent",
         "--num_workers", "0", "--log_dir", str(log_dir)],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=900,
    )
    assert r.returncode == 0, r.stderr[-3000:]
    run = [d for d in (tmp_path / "logs").iterdir() if d.is_dir()][0]
    assert (run / "model_0.pth").exists()
    # exactly one rank wrote the checkpoint/log set
    assert (run / "cmd.txt").exists() and (run / "scalars.jsonl").exists()


def test_train_h36m_cli_cpu(tmp_path):
    """h36m branch of the training CLI: skeleton modality (tuple batches),
    mlp backbone, 3D-visualizer qualitative eval — synthetic fallback data."""
    env = os.environ.copy()
    env["PYTHONPATH"] = ROOT
    log_dir = tmp_path / "logs" / "run"
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "train.py"),
         "--dataset", "h36m", "--backbone", "mlp", "--batch_size", "2",
         "--max_seq_len", "6", "--delta_len", "1", "--g_dim", "32",
         "--z_dim", "4", "--rnn_size", "32", "--nepochs", "1",
         "--epoch_size", "2", "--nsample", "2", "--device", "cpu",
         "--qual_iter", "1", "--data_root", "/nonexistent",
         "--num_workers", "0", "--log_dir", str(log_dir)],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
    )
    assert r.returncode == 0, r.stderr[-3000:]
    run = [d for d in (tmp_path / "logs").iterdir() if d.is_dir()][0]
    assert (run / "model_0.pth").exists()
    vis = list((run / "gen_vis").glob("*"))
    assert vis, "no h36m qualitative outputs written"
