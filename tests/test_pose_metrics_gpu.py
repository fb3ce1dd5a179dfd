"""Pose scoring kernels (csrc/pose_metrics.hip) against the fp64 definition.

Oracle: the definitions of ops/pose_metrics.py evaluated in fp64 on the CPU,
on the values the kernel sees (operands rounded to their dtype first).

Tolerance (derived, not measured): every output is a sum of N non-negative
terms, each the square root of a sum of three squares of correctly rounded fp32
differences of exactly converted operands, so its relative error against fp64
is at most about (N + 8) * 2^-24, with N = J for mpjpe, 3J for mse and
J * S(S-1)/2 for spread. The tests allow twice that, relative, and no
absolute slack. Every figure is printed before it is asserted.
"""
import dataclasses

import numpy as np
import pytest
import torch

from p2pvg_amd import ops
from p2pvg_amd.core import Config
from p2pvg_amd.ops import pose_metrics, pose_spread
from p2pvg_amd.ops.pose_metrics import SPREAD_MAX_SJ
from p2pvg_amd.utils.pose_evaluation import best_of_n_pose, sample_poses

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SCALE = (0.5, 1.25, 3.0)
QUADS = [(1, 2, 2), (2, 3, 6), (4, 4, 7), (1, 4, 8), (2, 6, 9)]

SHAPES = [
    (1, 1, 1, 1),
    (3, 5, 7, 17),     # frames are 204 B, only 4-byte aligned
    (1, 2, 1, 16),
    (2, 3, 300, 17),   # B crosses the block's frame tile
    (2, 100, 3, 17),   # the default S
]
DTYPES = {"fp32_fp32": (torch.float32, torch.float32),
          "bf16_fp32": (torch.bfloat16, torch.float32),
          "fp16_bf16": (torch.float16, torch.bfloat16)}
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def tol(n_terms):
    return 2 * (n_terms + 8) * U


def make_poses(shape, pair, noise=0.05, seed=0):
    T, S, B, J = shape
    g = torch.Generator().manual_seed(seed + 1000 * T + 100 * S + 10 * B + J)
    ref = 3.0 * torch.randn(T, B, J, 3, generator=g)
    gen = ref.unsqueeze(1) + noise * torch.randn(T, S, B, J, 3, generator=g)
    dg, dr = DTYPES[pair]
    return gen.to(dg), ref.to(dr)


def metrics64(gen, ref, w):
    d = gen.double() - ref.double().unsqueeze(1)                 # (T,S,B,J,3)
    w = torch.tensor(w, dtype=torch.float64)
    mpjpe = (d * w).pow(2).sum(-1).sqrt().mean(-1)
    mse = d.pow(2).mean(dim=(-2, -1))
    return mpjpe.permute(1, 0, 2), mse.permute(1, 0, 2)


def spread64(gen, w):
    T, S, B, J, _ = gen.shape
    g = gen.double() * torch.tensor(w, dtype=torch.float64)
    total = torch.zeros(T, B, dtype=torch.float64)
    for i in range(S - 1):
        total += (g[:, i + 1:] - g[:, i:i + 1]).pow(2).sum(-1).sqrt().sum(dim=(1, 3))
    return 2.0 * total / (S * (S - 1) * J)


def rel_err(got, want):
    assert got.dtype == torch.float32 and got.is_cuda
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool((want > 0).all())
    return float(((got.double().cpu() - want).abs() / want).max())


_REF = {}


def cached(shape, pair):
    key = (shape, pair)
    if key not in _REF:
        gen, ref = make_poses(shape, pair)
        want = {}
        for name, w in (("unit", None), ("scaled", SCALE)):
            w3 = w or (1.0, 1.0, 1.0)
            want[name] = metrics64(gen, ref, w3) + (
                (spread64(gen, w3),) if shape[1] >= 2 else (None,))
        _REF[key] = (gen, ref, want)
    return _REF[key]


@pytest.mark.parametrize("scale", ["unit", "scaled"])
@pytest.mark.parametrize("pair", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_kernels_against_fp64(shape, pair, scale):
    T, S, B, J = shape
    gen, ref, want = cached(shape, pair)
    m64, q64, s64 = want[scale]
    w = None if scale == "unit" else SCALE
    gg, rg = gen.cuda(), ref.cuda()
    assert ops.pose_metrics_backend(gg) == "hip"
    mpjpe, mse = pose_metrics(gg, rg, w)
    assert mpjpe.shape == mse.shape == (S, T, B)
    e_m, e_q = rel_err(mpjpe, m64), rel_err(mse, q64)
    print(f"{shape} {pair} {scale}: mpjpe {e_m:.2e} (tol {tol(J):.2e})  "
          f"mse {e_q:.2e} (tol {tol(3 * J):.2e})")
    assert e_m <= tol(J)
    assert e_q <= tol(3 * J)
    if S >= 2:
        spread = pose_spread(gg, w)
        n = J * S * (S - 1) // 2
        e_s = rel_err(spread, s64)
        print(f"{shape} {pair} {scale}: spread {e_s:.2e} (tol {tol(n):.2e})")
        assert e_s <= tol(n)
    else:
        with pytest.raises(ValueError):
            pose_spread(gg, w)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_exact_cases(dtype):
    """J = 16, small integer ref, every joint of gen displaced by a multiple
    of a Pythagorean quadruple: integer lengths, exact sums. Spread: S = 2,
    every joint of sample 1 shifted along one axis by an integer."""
    T, S, B, J = 2, 3, 5, 16
    g = torch.Generator().manual_seed(5)
    ref = torch.randint(-8, 9, (T, B, J, 3), generator=g).float()
    quad = torch.tensor(QUADS, dtype=torch.float32)[
        torch.randint(0, len(QUADS), (T, S, B, J), generator=g)]
    mult = torch.randint(-3, 4, (T, S, B, J, 1), generator=g).float()
    sign = torch.randint(0, 2, (T, S, B, J, 3), generator=g).float() * 2 - 1
    gen = (ref.unsqueeze(1) + mult * quad * sign).to(dtype)
    ref = ref.to(dtype)
    want, _ = metrics64(gen, ref, (1.0, 1.0, 1.0))
    assert float(want.max()) > 0
    mpjpe, _ = pose_metrics(gen.cuda(), ref.cuda())
    assert torch.equal(mpjpe.double().cpu(), want)

    s0 = torch.randint(-8, 9, (T, B, J, 3), generator=g).float()
    shift = torch.randint(-5, 6, (T, B, J), generator=g).float()
    axis = torch.randint(0, 3, (T, B, J), generator=g)
    s1 = s0 + shift.unsqueeze(-1) * torch.nn.functional.one_hot(axis, 3).float()
    gen2 = torch.stack([s0, s1], dim=1).to(dtype)
    assert torch.equal(pose_spread(gen2.cuda()).double().cpu(),
                       shift.abs().double().mean(-1))


def test_spread_at_its_s_limit(monkeypatch):
    J = 17
    S = SPREAD_MAX_SJ // J  # 240
    assert ops._load_hip_ext().pose_spread_max_sj() == SPREAD_MAX_SJ
    assert S * J <= SPREAD_MAX_SJ < (S + 1) * J
    gen, _ = make_poses((1, S + 1, 2, J), "fp32_fp32", seed=7)
    at_limit = gen[:, :S].contiguous()
    spread = pose_spread(at_limit.cuda(), SCALE)
    n = J * S * (S - 1) // 2
    err = rel_err(spread, spread64(at_limit, SCALE))
    print(f"S limit {S} x J {J}: spread {err:.2e} (tol {tol(n):.2e})")
    assert err <= tol(n)
    # the other corner of the limit: one joint, the most samples
    g1, _ = make_poses((1, SPREAD_MAX_SJ, 1, 1), "fp32_fp32", seed=8)
    n1 = SPREAD_MAX_SJ * (SPREAD_MAX_SJ - 1) // 2
    err1 = rel_err(pose_spread(g1.cuda()), spread64(g1, (1.0, 1.0, 1.0)))
    print(f"S limit {SPREAD_MAX_SJ} x J 1: spread {err1:.2e} (tol {tol(n1):.2e})")
    assert err1 <= tol(n1)

    rec = _RecordingExt(ops._load_hip_ext())
    monkeypatch.setattr(ops, "_load_hip_ext", lambda: rec)
    with pytest.raises(ValueError):
        pose_spread(gen.cuda(), SCALE)
    assert not rec.calls
    # the torch path has no limit
    monkeypatch.setenv("P2PVG_KERNELS", "torch")
    over = pose_spread(gen.cuda(), SCALE)
    assert rel_err(over, spread64(gen, SCALE)) <= tol(J * (S + 1) * S // 2)


def test_guards_nan_around_the_operands():
    """The operands as contiguous slices of larger NaN-filled buffers, NaN
    directly before and after: a read outside them would poison a result."""
    for shape in [(3, 5, 7, 17), (2, 3, 300, 17), (1, 2, 1, 1)]:
        for pair in ("fp32_fp32", "fp16_bf16"):
            gen, ref = make_poses(shape, pair, seed=3)
            gg, rg = gen.cuda(), ref.cuda()
            pad = 5  # odd: the slices start off every alignment but their own
            bg = torch.full((gen.numel() + 2 * pad,), float("nan"),
                            dtype=gen.dtype, device="cuda")
            br = torch.full((ref.numel() + 2 * pad,), float("nan"),
                            dtype=ref.dtype, device="cuda")
            bg[pad:-pad] = gg.reshape(-1)
            br[pad:-pad] = rg.reshape(-1)
            gs, rs = bg[pad:-pad].view(gen.shape), br[pad:-pad].view(ref.shape)
            assert gs.is_contiguous() and gs.data_ptr() != bg.data_ptr()
            m1, q1 = pose_metrics(gs, rs, SCALE)
            m0, q0 = pose_metrics(gg, rg, SCALE)
            assert torch.equal(m1, m0) and torch.equal(q1, q0)
            assert bool(torch.isfinite(m1).all()) and bool(torch.isfinite(q1).all())
            s1, s0 = pose_spread(gs, SCALE), pose_spread(gg, SCALE)
            assert torch.equal(s1, s0) and bool(torch.isfinite(s1).all())


def test_determinism_and_backends(monkeypatch):
    shape = (3, 5, 7, 17)
    T, S, B, J = shape
    gen, ref = make_poses(shape, "bf16_fp32", seed=4)
    gg, rg = gen.cuda(), ref.cuda()
    first = pose_metrics(gg, rg, SCALE) + (pose_spread(gg, SCALE),)
    again = pose_metrics(gg, rg, SCALE) + (pose_spread(gg, SCALE),)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    # a frame's spread does not depend on its neighbours in the batch
    assert torch.equal(pose_spread(gg[:, :, 2:3].contiguous(), SCALE), first[2][:, 2:3])
    # non-contiguous operands are made contiguous
    g_nc = gg.transpose(2, 3).contiguous().transpose(2, 3)
    assert not g_nc.is_contiguous()
    assert torch.equal(pose_metrics(g_nc, rg, SCALE)[0], first[0])
    assert torch.equal(pose_spread(g_nc, SCALE), first[2])
    # both backends stay within the tolerance of the fp64 definition
    monkeypatch.setenv("P2PVG_KERNELS", "torch")
    assert ops.pose_metrics_backend(gg) == "torch"
    other = pose_metrics(gg, rg, SCALE) + (pose_spread(gg, SCALE),)
    want = metrics64(gen, ref, SCALE) + (spread64(gen, SCALE),)
    for name, n, k, t, w in zip(("mpjpe", "mse", "spread"),
                                (J, 3 * J, J * S * (S - 1) // 2),
                                first, other, want):
        e_k, e_t = rel_err(k, w), rel_err(t, w)
        print(f"{name}: kernel {e_k:.2e} torch {e_t:.2e} (tol {tol(n):.2e})")
        assert e_k <= tol(n) and e_t <= tol(n)
    # the scores do not depend on a caller's autocast state
    monkeypatch.setenv("P2PVG_KERNELS", "auto")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        inside = pose_metrics(gg, rg, SCALE) + (pose_spread(gg, SCALE),)
    for a, b in zip(first, inside):
        assert a.dtype == torch.float32 and torch.equal(a, b)


class _RecordingExt:
    def __init__(self, real):
        self._real = real
        self.calls = []

    def pose_metrics(self, *args):
        self.calls.append(args)
        return self._real.pose_metrics(*args)

    def pose_spread(self, *args):
        self.calls.append(args)
        return self._real.pose_spread(*args)

    def __getattr__(self, name):
        return getattr(self._real, name)


def test_validation_raises_before_launch(monkeypatch):
    rec = _RecordingExt(ops._load_hip_ext())
    monkeypatch.setattr(ops, "_load_hip_ext", lambda: rec)
    gen, ref = make_poses((2, 3, 4, 5), "fp32_fp32")
    gen, ref = gen.cuda(), ref.cuda()
    bad = {
        "rank gen": lambda: pose_metrics(gen[0], ref),
        "rank ref": lambda: pose_metrics(gen, ref[0]),
        "trailing 3": lambda: pose_metrics(gen[..., :2], ref[..., :2]),
        "T": lambda: pose_metrics(gen, ref[:1]),
        "B": lambda: pose_metrics(gen, ref[:, :3]),
        "J": lambda: pose_metrics(gen, ref[:, :, :4]),
        "device": lambda: pose_metrics(gen, ref.cpu()),
        "dtype f64": lambda: pose_metrics(gen.double(), ref.double()),
        "dtype i64": lambda: pose_metrics(gen, ref.long()),
        "scale len": lambda: pose_metrics(gen, ref, (1.0, 2.0)),
        "scale 0": lambda: pose_metrics(gen, ref, (1.0, 0.0, 1.0)),
        "scale nan": lambda: pose_metrics(gen, ref, (1.0, float("nan"), 1.0)),
        "scale tensor": lambda: pose_metrics(gen, ref, torch.ones(3, device="cuda")),
        "spread S=1": lambda: pose_spread(gen[:, :1]),
        "spread rank": lambda: pose_spread(gen[0]),
        "spread dtype": lambda: pose_spread(gen.double()),
        "spread scale": lambda: pose_spread(gen, (1.0, -1.0, 1.0)),
    }
    for name, call in bad.items():
        with pytest.raises(ValueError):
            call()
        assert not rec.calls, f"{name}: reached the extension"
    w = gen.clone().requires_grad_()
    with pytest.raises(RuntimeError):
        pose_metrics(w, ref)
    with pytest.raises(RuntimeError):
        pose_spread(w)
    assert not rec.calls
    # empty leading dimensions: empty results, nothing launched
    m, q = pose_metrics(gen[:, :, :0], ref[:, :0])
    assert m.shape == q.shape == (3, 2, 0) and m.is_cuda and m.dtype == torch.float32
    assert pose_spread(gen[:0]).shape == (0, 4)
    assert not rec.calls
    pose_metrics(gen, ref)
    pose_spread(gen)
    assert len(rec.calls) == 2  # the probe does see valid calls


def test_joints_beyond_one_tile():
    """J > 1024: one frame per block, its joints in chunks."""
    shape = (1, 2, 3, 1500)
    gen, ref = make_poses(shape, "fp32_fp32", seed=6)
    m64, q64 = metrics64(gen, ref, SCALE)
    mpjpe, mse = pose_metrics(gen.cuda(), ref.cuda(), SCALE)
    e_m, e_q = rel_err(mpjpe, m64), rel_err(mse, q64)
    print(f"{shape}: mpjpe {e_m:.2e} (tol {tol(1500):.2e})  mse {e_q:.2e}")
    assert e_m <= tol(1500) and e_q <= tol(4500)


@pytest.mark.parametrize("amp", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_end_to_end_backends_agree(monkeypatch, amp):
    from p2pvg_amd.models import P2PModel

    cfg = Config(dataset="h36m", backbone="mlp", batch_size=4, max_seq_len=8,
                 delta_len=1, n_past=2, g_dim=32, z_dim=4, rnn_size=32,
                 device="cuda", num_workers=0, data_root="/nonexistent")
    torch.manual_seed(0)
    np.random.seed(0)
    model = P2PModel(cfg).to("cuda")
    model.eval()
    T, S, B, J = 8, 6, 4, 17
    x3 = torch.randn(T, B, J, 3, generator=torch.Generator().manual_seed(2)).cuda()
    gen = sample_poses(model, x3, S, sample_chunk=4, amp_dtype=amp)
    assert gen.shape == (T, S, B, J, 3) and gen.dtype == torch.float32
    assert bool(torch.isfinite(gen).all())
    assert torch.equal(gen[:cfg.n_past], x3[:cfg.n_past].unsqueeze(1).expand(-1, S, -1, -1, -1))
    assert not torch.equal(gen[T - 1, 0], gen[T - 1, 1])

    # The same poses are scored under both backends: two generations, even
    # reseeded, need not agree in the last bits.
    def score(backend):
        monkeypatch.setenv("P2PVG_KERNELS", backend)
        name = ops.pose_metrics_backend(gen)
        mpjpe, mse = pose_metrics(gen, x3, SCALE)
        return name, best_of_n_pose(mpjpe, mse, pose_spread(gen, SCALE), cfg.n_past)

    name_k, res_k = score("auto")
    name_t, res_t = score("torch")
    assert name_k == "hip" and name_t == "torch"
    # every output is a mean of scores, each within tol(N) of fp64 on either path
    bound = {"mpjpe": 2 * tol(J), "mse": 2 * tol(3 * J),
             "spread": 2 * tol(J * S * (S - 1) // 2)}
    for k in res_k:
        a, b = res_k[k].double().cpu(), res_t[k].double().cpu()
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), k
        kind = "spread" if "spread" in k else ("mse" if "mse" in k else "mpjpe")
        err = float(((a - b).abs() / b).max())
        print(f"{k} ({amp}): backends differ by {err:.2e} (bound {bound[kind]:.2e})")
        assert err <= bound[kind], k
