"""Pose evaluation on the CPU: the torch path of ops.pose_metrics / pose_spread
against fp64 loops written out from the definitions, exact integer cases,
best_of_n_pose against a python-loop reference, sample folding, dataset units.

Tolerance (derived, not measured): every output is a sum of N non-negative
terms, each the square root of a sum of three squares of correctly rounded fp32
differences of exactly converted operands, so its relative error against fp64
is at most about (N + 8) * 2^-24, with N = J for mpjpe, 3J for mse and
J * S(S-1)/2 for spread. The tests allow twice that, relative, and no
absolute slack.
"""
import dataclasses
import math

import numpy as np
import pytest
import torch

from p2pvg_amd import ops
from p2pvg_amd.core import Config
from p2pvg_amd.data.human36m import STD_SCALE, Human36mDataset, standardize_dataset
from p2pvg_amd.models import P2PModel
from p2pvg_amd.ops import pose_metrics, pose_spread
from p2pvg_amd.utils.pose_evaluation import (
    best_of_n_pose,
    evaluate_pose_model,
    sample_poses,
)

U = 2.0 ** -24
SCALE = (0.5, 1.25, 3.0)
QUADS = [(1, 2, 2), (2, 3, 6), (4, 4, 7), (1, 4, 8), (2, 6, 9)]  # |q| = 3 7 9 9 11


def tol(n_terms):
    return 2 * (n_terms + 8) * U


def make_poses(T, S, B, J, noise, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * T + 100 * S + 10 * B + J)
    ref = 3.0 * torch.randn(T, B, J, 3, generator=g)
    gen = ref.unsqueeze(1) + noise * torch.randn(T, S, B, J, 3, generator=g)
    return gen, ref


def loops64(gen, ref, w):
    """mpjpe, mse (S,T,B) and spread (T,B; None if S < 2) in python floats
    (fp64), straight from the definitions."""
    T, S, B, J, _ = gen.shape
    g, r = gen.double().tolist(), ref.double().tolist()
    mpjpe = torch.zeros(S, T, B, dtype=torch.float64)
    mse = torch.zeros(S, T, B, dtype=torch.float64)
    spread = torch.zeros(T, B, dtype=torch.float64) if S >= 2 else None
    for t in range(T):
        for b in range(B):
            for s in range(S):
                e = q = 0.0
                for j in range(J):
                    d = [g[t][s][b][j][a] - r[t][b][j][a] for a in range(3)]
                    e += math.sqrt(sum((w[a] * d[a]) ** 2 for a in range(3)))
                    q += sum(d[a] ** 2 for a in range(3))
                mpjpe[s, t, b] = e / J
                mse[s, t, b] = q / (3 * J)
            if S >= 2:
                acc = 0.0
                for i in range(S):
                    for k in range(i + 1, S):
                        for j in range(J):
                            acc += math.sqrt(sum(
                                (w[a] * (g[t][i][b][j][a] - g[t][k][b][j][a])) ** 2
                                for a in range(3)))
                spread[t, b] = 2.0 * acc / (S * (S - 1) * J)
    return mpjpe, mse, spread


def rel_err(got, want):
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert bool((want > 0).all())
    return float(((got.double() - want).abs() / want).max())


@pytest.mark.parametrize("noise", [1e-3, 1.0])
@pytest.mark.parametrize("shape", [(3, 5, 7, 17), (1, 2, 1, 1)],
                         ids=lambda s: "x".join(map(str, s)))
def test_torch_path_against_fp64_loops(shape, noise):
    T, S, B, J = shape
    gen, ref = make_poses(T, S, B, J, noise)
    assert ops.pose_metrics_backend(gen) == "torch"
    m64, q64, s64 = loops64(gen, ref, SCALE)
    mpjpe, mse = pose_metrics(gen, ref, SCALE)
    spread = pose_spread(gen, SCALE)
    assert mpjpe.shape == mse.shape == (S, T, B) and spread.shape == (T, B)
    errs = (rel_err(mpjpe, m64), rel_err(mse, q64), rel_err(spread, s64))
    print(f"{shape} noise {noise}: mpjpe {errs[0]:.2e} mse {errs[1]:.2e} "
          f"spread {errs[2]:.2e}")
    assert errs[0] <= tol(J)
    assert errs[1] <= tol(3 * J)
    assert errs[2] <= tol(J * S * (S - 1) // 2)
    # mse ignores axis_scale; unit scale is the default
    assert torch.equal(pose_metrics(gen, ref)[1], mse)
    assert torch.equal(pose_metrics(gen, ref, (1, 1, 1))[0], pose_metrics(gen, ref)[0])


def exact_case(dtype):
    """J = 16, small integer ref, every joint of gen displaced by a multiple
    of a Pythagorean quadruple: all lengths are integers, all sums exact."""
    T, S, B, J = 2, 3, 5, 16
    g = torch.Generator().manual_seed(5)
    ref = torch.randint(-8, 9, (T, B, J, 3), generator=g).float()
    quad = torch.tensor(QUADS, dtype=torch.float32)[
        torch.randint(0, len(QUADS), (T, S, B, J), generator=g)]
    mult = torch.randint(-3, 4, (T, S, B, J, 1), generator=g).float()
    sign = torch.randint(0, 2, (T, S, B, J, 3), generator=g).float() * 2 - 1
    gen = ref.unsqueeze(1) + mult * quad * sign
    gen, ref = gen.to(dtype), ref.to(dtype)
    d = gen.double() - ref.double().unsqueeze(1)
    want = d.pow(2).sum(-1).sqrt().mean(-1).permute(1, 0, 2)
    assert bool((want * J == (want * J).round()).all())  # integer lengths
    assert float(want.max()) > 0
    return gen, ref, want


def exact_spread_case(dtype):
    """S = 2, J = 16: every joint of sample 1 is sample 0 shifted along one
    axis by an integer."""
    T, B, J = 2, 5, 16
    g = torch.Generator().manual_seed(6)
    s0 = torch.randint(-8, 9, (T, B, J, 3), generator=g).float()
    shift = torch.randint(-5, 6, (T, B, J), generator=g).float()
    axis = torch.randint(0, 3, (T, B, J), generator=g)
    s1 = s0 + shift.unsqueeze(-1) * torch.nn.functional.one_hot(axis, 3).float()
    gen = torch.stack([s0, s1], dim=1).to(dtype)
    want = shift.abs().double().mean(-1)
    return gen, want


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_exact_cases(dtype):
    gen, ref, want = exact_case(dtype)
    mpjpe, _ = pose_metrics(gen, ref)
    assert torch.equal(mpjpe.double(), want)
    gen2, want2 = exact_spread_case(dtype)
    assert torch.equal(pose_spread(gen2).double(), want2)


def test_op_validation_and_edges():
    gen, ref = make_poses(2, 3, 4, 5, 0.1)
    bad = [
        lambda: pose_metrics(gen[0], ref),                    # rank
        lambda: pose_metrics(gen, ref[0]),
        lambda: pose_metrics(gen[..., :2], ref[..., :2]),     # trailing 3
        lambda: pose_metrics(gen, ref[:1]),                   # T
        lambda: pose_metrics(gen, ref[:, :3]),                # B
        lambda: pose_metrics(gen, ref[:, :, :4]),             # J
        lambda: pose_metrics(gen.double(), ref.double()),     # dtype
        lambda: pose_metrics(gen, ref.long()),
        lambda: pose_metrics(gen, ref, (1.0, 2.0)),           # axis_scale
        lambda: pose_metrics(gen, ref, (1.0, 0.0, 1.0)),
        lambda: pose_metrics(gen, ref, (1.0, -1.0, 1.0)),
        lambda: pose_metrics(gen, ref, (1.0, float("nan"), 1.0)),
        lambda: pose_metrics(gen, ref, (1.0, float("inf"), 1.0)),
        lambda: pose_metrics(gen, ref, torch.ones(3)),
        lambda: pose_metrics(gen, ref, 2.0),
        lambda: pose_metrics(gen.tolist(), ref),
        lambda: pose_spread(gen[:, :1]),                      # S >= 2
        lambda: pose_spread(gen[0]),
        lambda: pose_spread(gen.double()),
        lambda: pose_spread(gen, (0.0, 1.0, 1.0)),
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    w = gen.clone().requires_grad_()
    with pytest.raises(RuntimeError):
        pose_metrics(w, ref)
    with pytest.raises(RuntimeError):
        pose_spread(w)
    with torch.no_grad():
        pose_metrics(w, ref)
        pose_spread(w)
    # empty leading dimensions
    m, q = pose_metrics(gen[:, :, :0], ref[:, :0])
    assert m.shape == q.shape == (3, 2, 0) and m.dtype == torch.float32
    assert pose_spread(gen[:0]).shape == (0, 4)
    # non-contiguous operands: same values as their contiguous copies
    gt, rt = gen.transpose(2, 3), ref.transpose(1, 2)          # (T,S,J,B,3)
    gen_nc = gt.contiguous().transpose(2, 3)
    ref_nc = rt.contiguous().transpose(1, 2)
    assert not gen_nc.is_contiguous() and not ref_nc.is_contiguous()
    for a, b in zip(pose_metrics(gen_nc, ref_nc, SCALE), pose_metrics(gen, ref, SCALE)):
        assert torch.equal(a, b)
    assert torch.equal(pose_spread(gen_nc, SCALE), pose_spread(gen, SCALE))


# --------------------------------------------------------------------------
# best_of_n_pose
# --------------------------------------------------------------------------

def best_of_n_loops(mpjpe, mse, spread, n_past):
    S, T, B = mpjpe.shape
    out = {}
    for name, m in (("mpjpe", mpjpe.double()), ("mse", mse.double())):
        best = torch.zeros(T - n_past, dtype=torch.float64)
        for b in range(B):
            means = [float(m[s, n_past:, b].mean()) for s in range(S)]
            pick = min(range(S), key=lambda s: (means[s], s))
            best += m[pick, n_past:, b]
        out[f"{name}_best"] = best / B
        out[f"{name}_mean"] = torch.stack(
            [m[:, t].mean() for t in range(n_past, T)])
    out["spread"] = torch.stack([spread[t].double().mean() for t in range(n_past, T)])
    m = mpjpe.double()
    out["end_pose_mpjpe_best"] = torch.stack(
        [min(m[s, T - 1, b] for s in range(S)) for b in range(B)]).mean()
    out["end_pose_mpjpe_mean"] = m[:, T - 1].mean()
    out["end_pose_spread"] = spread[T - 1].double().mean()
    return out


@pytest.mark.parametrize("n_past", [0, 1, 5])
def test_best_of_n_pose_against_loops(n_past):
    S, T, B = 4, 6, 3
    g = torch.Generator().manual_seed(11)
    mpjpe = torch.rand(S, T, B, generator=g) + 0.1
    mse = torch.rand(S, T, B, generator=g) + 0.1
    spread = torch.rand(T, B, generator=g)
    res = best_of_n_pose(mpjpe, mse, spread, n_past)
    want = best_of_n_loops(mpjpe, mse, spread, n_past)
    assert set(res) == set(want)
    for k in want:
        assert res[k].shape == want[k].shape, k
        assert torch.allclose(res[k].double(), want[k], rtol=1e-6, atol=0), k
    assert res["mpjpe_best"].shape == (T - n_past,)
    assert res["end_pose_mpjpe_best"].dim() == 0
    assert float(res["end_pose_mpjpe_best"]) <= float(res["end_pose_mpjpe_mean"])


def test_best_of_n_pose_tie_and_errors():
    S, T, B = 3, 4, 2
    mpjpe = torch.ones(S, T, B)
    # sequence 0: samples 1 and 2 tie on the mean over frames 1.. (both 0.5)
    # but differ per frame; the lowest index (1) must be picked
    mpjpe[1, 1:, 0] = torch.tensor([0.25, 0.5, 0.75])
    mpjpe[2, 1:, 0] = torch.tensor([0.75, 0.5, 0.25])
    mpjpe[2, 0, 0] = 0.0  # frame 0 < n_past must not decide
    mse = mpjpe.clone()
    spread = torch.zeros(T, B)
    res = best_of_n_pose(mpjpe, mse, spread, 1)
    want = (torch.tensor([0.25, 0.5, 0.75]) + 1.0) / 2  # sequence 1: all ones
    assert torch.equal(res["mpjpe_best"], want)
    assert torch.equal(res["mse_best"], want)
    assert float(res["end_pose_mpjpe_best"]) == (0.25 + 1.0) / 2
    for call in (
        lambda: best_of_n_pose(mpjpe, mse[:2], spread, 1),
        lambda: best_of_n_pose(mpjpe[0], mse[0], spread, 1),
        lambda: best_of_n_pose(mpjpe, mse, spread[:3], 1),
        lambda: best_of_n_pose(mpjpe, mse, spread.t(), 1),
        lambda: best_of_n_pose(mpjpe, mse, spread, T),
        lambda: best_of_n_pose(mpjpe, mse, spread, -1),
    ):
        with pytest.raises(ValueError):
            call()


def test_spread_zero_for_equal_samples():
    _, ref = make_poses(3, 1, 4, 17, 0.1)
    gen = ref.unsqueeze(1).expand(3, 5, 4, 17, 3)
    spread = pose_spread(gen, SCALE)
    assert torch.equal(spread, torch.zeros(3, 4))
    mpjpe, mse = pose_metrics(gen, ref, SCALE)
    res = best_of_n_pose(mpjpe, mse, spread, 1)
    assert float(res["spread"].abs().max()) == 0.0 and float(res["end_pose_spread"]) == 0.0


# --------------------------------------------------------------------------
# sample_poses
# --------------------------------------------------------------------------

class _StubModel:
    """p2p_generate returns x + row index: the output says which folded row
    produced it."""

    def __init__(self):
        self.calls = []

    def p2p_generate(self, x, len_output, eval_cp_ix, model_mode="full",
                     skip_frame=False):
        assert len_output == len(x) and eval_cp_ix == len(x) - 1
        assert skip_frame is False
        self.calls.append((x.shape[1], model_mode))
        rows = torch.arange(x.shape[1], dtype=x.dtype).view(-1, 1, 1)
        return [x[t] + rows for t in range(len(x))]


@pytest.mark.parametrize("nsample,chunk,rollouts", [
    (5, 2, [2, 2, 1]), (4, 7, [4]), (6, 3, [3, 3]), (3, 1, [1, 1, 1])])
def test_sample_poses_row_mapping(nsample, chunk, rollouts):
    T, B, J = 4, 3, 2
    x3 = torch.arange(T * B * J * 3, dtype=torch.float32).view(T, B, J, 3) / 64
    stub = _StubModel()
    out = sample_poses(stub, x3, nsample, model_mode="prior", sample_chunk=chunk)
    assert out.shape == (T, nsample, B, J, 3) and out.dtype == torch.float32
    assert out.is_contiguous()
    assert stub.calls == [(k * B, "prior") for k in rollouts]
    # sample s of a chunk starting at s0 was row (s - s0) * B + b
    s_in_chunk = torch.arange(nsample) % chunk
    want = x3.unsqueeze(1) + (s_in_chunk.view(1, -1, 1, 1, 1) * B
                              + torch.arange(B).view(1, 1, -1, 1, 1)).float()
    assert torch.equal(out, want)


def test_sample_poses_rejects_non_poses():
    stub = _StubModel()
    for bad in (torch.zeros(4, 3, 17, 2), torch.zeros(4, 3, 1, 64, 64),
                torch.zeros(3, 17, 3), torch.zeros(4, 3, 17, 3).long(), [1, 2]):
        with pytest.raises(ValueError):
            sample_poses(stub, bad, 2)
    x3 = torch.zeros(4, 3, 17, 3)
    with pytest.raises(ValueError):
        sample_poses(stub, x3, 0)
    with pytest.raises(ValueError):
        sample_poses(stub, x3, 2, sample_chunk=0)
    assert not stub.calls


@pytest.fixture
def tiny_pose_cfg():
    return Config(dataset="h36m", backbone="mlp", batch_size=2, max_seq_len=8,
                  delta_len=1, n_past=2, g_dim=32, z_dim=4, rnn_size=32,
                  device="cpu", num_workers=0, data_root="/nonexistent")


def test_sample_poses_tiny_mlp_model(tiny_pose_cfg):
    cfg = tiny_pose_cfg
    torch.manual_seed(0)
    np.random.seed(0)
    model = P2PModel(cfg)
    model.eval()
    T, B, S = 8, 3, 5
    x3 = torch.randn(T, B, 17, 3, generator=torch.Generator().manual_seed(2))
    out = sample_poses(model, x3, S, sample_chunk=2)
    assert out.shape == (T, S, B, 17, 3)
    assert bool(torch.isfinite(out).all())
    for s in range(S):
        assert torch.equal(out[:cfg.n_past, s], x3[:cfg.n_past])
        for s2 in range(s):
            for t in range(cfg.n_past, T):
                assert not torch.equal(out[t, s], out[t, s2]), (t, s, s2)


def test_evaluate_pose_model_weights_batches(tiny_pose_cfg):
    """Two batches of different size: the result is the sequence-weighted mean
    of the per-batch curves, computed here from the same poses."""
    cfg = tiny_pose_cfg
    torch.manual_seed(0)
    model = P2PModel(cfg)
    model.eval()
    g = torch.Generator().manual_seed(3)
    x_a = torch.randn(8, 2, 17, 3, generator=g)
    x_b = torch.randn(8, 4, 17, 3, generator=g)
    batches = [(x_a[..., :2], x_a, [0, 1]), x_b]  # the h36m tuple, and bare poses

    def run():
        torch.manual_seed(9)
        np.random.seed(9)
        return evaluate_pose_model(model, iter(batches), 2, 3, sample_chunk=2,
                                   axis_scale=SCALE)

    res = run()
    assert res["n_sequences"] == 6
    assert len(res["mpjpe_best"]) == 8 - cfg.n_past
    assert res["seconds_generate"] > 0 and res["seconds_score"] > 0
    torch.manual_seed(9)
    np.random.seed(9)
    parts = []
    for x3 in (x_a, x_b):
        gen = sample_poses(model, x3, 3, sample_chunk=2)
        parts.append(best_of_n_pose(*pose_metrics(gen, x3, SCALE),
                                    pose_spread(gen, SCALE), cfg.n_past))
    for k in ("mpjpe_best", "mse_mean", "spread", "end_pose_mpjpe_best"):
        want = (2 * parts[0][k].double() + 4 * parts[1][k].double()) / 6
        got = torch.tensor(res[k], dtype=torch.float64)
        assert torch.allclose(got, want, rtol=1e-12, atol=0), k
    with pytest.raises(ValueError):
        evaluate_pose_model(model, iter(batches), 1, 1)
    with pytest.raises(ValueError):
        evaluate_pose_model(model, iter(batches), 0, 3)


# --------------------------------------------------------------------------
# dataset units
# --------------------------------------------------------------------------

def test_synthetic_dataset_units():
    ds = Human36mDataset(data_root="/nonexistent", max_seq_len=10, delta_len=2,
                         mode="test")
    assert ds.synthetic
    assert ds.pose_unit == "standardized"
    assert ds.pose_scale_3d.dtype == np.float32
    assert np.array_equal(ds.pose_scale_3d, np.ones(3, dtype=np.float32))


def test_standardize_dataset_returns_statistics():
    rng = np.random.RandomState(0)
    axis_std = np.array([2.0, 50.0, 700.0])
    seqs3 = [rng.randn(n, 17, 3) * axis_std + 5.0 for n in (12, 20)]
    raw3 = [s.copy() for s in seqs3]
    data = {"pose": {"2d": [s[:, :, :2].copy() for s in seqs3], "3d": seqs3}}
    stats = standardize_dataset(data)
    allp = np.concatenate([s.reshape(-1, 3) for s in raw3])
    assert np.allclose(stats["std3"], allp.std(axis=0), rtol=1e-12)
    assert np.allclose(stats["mean3"], allp.mean(axis=0), rtol=1e-12)
    assert stats["std2"].shape == (2,) and stats["mean2"].shape == (2,)
    # std3 / STD_SCALE de-standardises a difference back to the original
    diff_std = data["pose"]["3d"][0][3] - data["pose"]["3d"][1][7]
    diff_raw = raw3[0][3] - raw3[1][7]
    assert np.allclose(diff_std * (stats["std3"] / STD_SCALE), diff_raw,
                       rtol=1e-9, atol=1e-9)
    assert standardize_dataset({"pose": {"2d": [], "3d": []}}) is None


def test_h36m_test_generator_batch_size(tiny_pose_cfg):
    from p2pvg_amd import data as data_utils

    cfg = dataclasses.replace(tiny_pose_cfg)
    _, test = data_utils.load_dataset(cfg)
    for bs in (3, len(test) + 5):  # the second exceeds the split: replacement
        gen = data_utils.get_h36m_test_generator(test, cfg, bs)
        p2, p3, cam = next(gen)
        assert p3.shape == (30, bs, 17, 3) and p2.shape == (30, bs, 17, 2)
        assert len(cam) == bs
    with pytest.raises(ValueError):
        data_utils.get_h36m_test_generator(test, cfg, 0)
    # get_data_generator keeps its fixed 10
    _, p3, _ = next(data_utils.get_data_generator(test, train=False,
                                                  dynamic_length=False, opt=cfg))
    assert p3.shape[1] == 10
