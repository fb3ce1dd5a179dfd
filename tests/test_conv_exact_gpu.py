"""Exact integer-valued tests of the conv forward, dgrad and ConvT kernels.

Inputs are small integers: activations and gradients from {-2..2}, weights
from {-1,0,1} thinned by a per-case density, biases from {-4..4}. Every value
is bf16-exact and every product and partial sum is an integer far below 2^24,
so fp32 accumulation is exact in any order, with any tiling and any split:
the kernel's pre-rounding value IS the mathematically exact integer. Where
that integer is at most 256 in magnitude it is bf16-exact as well, and the
kernel output must be bit-identical to a CPU fp64 reference: no tolerance.

Assertion rules (derived, not measured):
- act 0: torch.equal(got, ref.bfloat16()), after asserting on the reference
  alone that max|ref| <= 256 (<= 128 where statistics are checked, so that a
  bucket's sum of squares, at most 128 rows x 128^2, stays below 2^22).
- act 1 (leaky 0.2): equal where the exact value v >= 0; where v < 0,
  |got - 0.2 v| <= 2^-8 |0.2 v| (1 + 2^-10): one fp32 rounding of the product
  followed by one round-to-nearest to bf16.
- act 2/3: |got - ref64| <= 2^-8 |ref64| + 1e-5 (the bf16 half-ulp).
- stats, act 0: bucket rows summed over dim 0 in fp64 equal the fp64 sums of
  v and v^2 exactly; the bucket shape is asserted too.
- stats, act 1: |S - S_ref| <= 2^-16 sum|v| (second row: 2^-16 sum v^2), which
  covers the at most 128 fp32 additions behind one bucket entry.
- dW through the autograd Functions is fp32 and must be exactly equal.

Section 0 runs without a GPU: it checks every case's reference against an
independent formulation (unfold + matmul for conv, zero-dilate + flipped conv
for ConvT) and asserts the magnitude caps, so a GPU mismatch is a kernel bug
and not a convention of the reference.

docs/KERNELS.md ("Conv test matrix") lists which case reaches which template
instantiation; extend both together.
"""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

CL = torch.channels_last
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from p2pvg_amd.ops import _hip_ext_loader

    return _hip_ext_loader.load()


# --------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------

def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _ints(seed, shape, lo, hi, density=1.0):
    """Integers from [lo, hi], each kept with probability `density` (else 0).
    4-D: bf16 channels_last. 1-D (bias): fp32."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, shape, generator=g).float()
    if density < 1.0:
        t = t * (torch.rand(shape, generator=g) < density)
    if len(shape) == 4:
        return t.to(torch.bfloat16).contiguous(memory_format=CL)
    return t


def _ring(t, r, value=0.0):
    """Zero-ring padder (channels_last)."""
    if r == 0:
        return t.contiguous(memory_format=CL)
    return F.pad(t, (r,) * 4, value=value).contiguous(memory_format=CL)


def _density(terms):
    """Weight density for a reduction of `terms` products. An activation has
    mean square 2, so the sum has variance 2*terms*density; 200 terms kept
    give sigma = 20 and the caps sit at 6 (128) and 12 (256) sigma."""
    return min(1.0, 200.0 / terms)


def _ref_conv(x, w, b, st, pad):
    return F.conv2d(x.double(), w.double(),
                    None if b is None else b.double(), st, pad)


def _ref_convt(x, w, b, st, pad):
    """w is the ConvTranspose layout (Ci, Co, k, k)."""
    return F.conv_transpose2d(x.double(), w.double(),
                              None if b is None else b.double(), st, pad)


def _ref_grads(fn, x, w, g):
    """fp64 (dx, dw) of y = fn(x, w) for the incoming gradient g."""
    xd = x.double().requires_grad_()
    wd = w.double().requires_grad_()
    dx, dw = torch.autograd.grad(fn(xd, wd), [xd, wd], g.double())
    return dx, dw


def _conv_unfold(x, w, b, st, pad):
    """Independent conv: im2col (F.unfold) + one fp64 matmul per batch slab."""
    x, w = x.double(), w.double()
    n, _, h, wd = x.shape
    k_out, _, k, _ = w.shape
    ho = (h + 2 * pad - k) // st + 1
    wo = (wd + 2 * pad - k) // st + 1
    wm = w.reshape(k_out, -1)
    outs = []
    for i in range(0, n, 8):
        cols = F.unfold(x[i:i + 8], k, padding=pad, stride=st)
        outs.append((wm @ cols).view(-1, k_out, ho, wo))
    y = torch.cat(outs)
    if b is not None:
        y = y + b.double().view(1, -1, 1, 1)
    return y


def _convt_dilate(x, w, b, st, pad):
    """Independent ConvT: zero-dilate the input, then a stride-1 conv with
    the flipped, transposed weight and padding k-1-pad (via _conv_unfold)."""
    n, c, h, wd = x.shape
    k = w.shape[2]
    xd = torch.zeros(n, c, (h - 1) * st + 1, (wd - 1) * st + 1,
                     dtype=torch.float64)
    xd[:, :, ::st, ::st] = x.double()
    return _conv_unfold(xd, w.double().flip(2, 3).transpose(0, 1), b, 1,
                        k - 1 - pad)


def _assert_caps(v, cap):
    """The reference alone: integer-valued, within the cap, bf16-exact."""
    m = v.abs().max().item()
    assert m <= cap, f"reference magnitude {m} exceeds the cap {cap}"
    assert torch.equal(v, v.round())
    assert torch.equal(v.to(torch.bfloat16).double(), v)


def _assert_exact(got, v, cap=256, what="y"):
    _assert_caps(v, cap)
    got = got.detach().cpu()
    assert got.dtype == torch.bfloat16 and got.shape == v.shape, \
        (got.dtype, tuple(got.shape), tuple(v.shape))
    want = v.to(torch.bfloat16)
    if not torch.equal(got, want):
        d = (got.double() - v).abs()
        bad = int((d != 0).sum()) if torch.isfinite(d).all() else -1
        raise AssertionError(
            f"{what}: {bad} of {v.numel()} elements differ, max |err| "
            f"{d.max().item()} (max |ref| {v.abs().max().item()})")


def _assert_leaky(got, v, cap=256):
    _assert_caps(v, cap)
    got = got.detach().cpu()
    assert got.dtype == torch.bfloat16 and got.shape == v.shape
    pos = v >= 0
    gd = got.double()
    npos = int((gd[pos] != v[pos]).sum())
    assert npos == 0, f"leaky: {npos} non-negative outputs differ"
    want = 0.2 * v[~pos]
    err = (gd[~pos] - want).abs()
    bound = 2.0 ** -8 * want.abs() * (1 + 2.0 ** -10)
    nbad = int((err > bound).sum())
    assert nbad == 0, (f"leaky: {nbad} negative outputs outside the bf16 "
                       f"rounding bound, worst ratio "
                       f"{(err / bound).max().item():.3f}")


def _assert_smooth(got, v, act):
    """tanh / sigmoid epilogues against fp64, bf16 half-ulp bound."""
    ref = torch.tanh(v) if act == 2 else torch.sigmoid(v)
    gd = got.detach().cpu().double()
    assert gd.shape == ref.shape
    err = (gd - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-5
    nbad = int((err > bound).sum())
    assert nbad == 0, f"act {act}: {nbad} outputs outside the bound, " \
                      f"worst ratio {(err / bound).max().item():.3f}"


def _assert_stats(stats, v, act, rows):
    """Bucket shape (rows, 2, K) and the two per-channel rows."""
    _assert_caps(v, 128)
    k = v.shape[1]
    assert tuple(stats.shape) == (rows, 2, k), (tuple(stats.shape), rows, k)
    assert stats.dtype == torch.float32
    s = stats.detach().cpu().double().sum(0)
    a = v if act == 0 else torch.where(v >= 0, v, 0.2 * v)
    s1, s2 = a.sum((0, 2, 3)), (a * a).sum((0, 2, 3))
    if act == 0:
        assert torch.equal(s[0], s1), \
            f"sum row: max |err| {(s[0] - s1).abs().max().item()}"
        assert torch.equal(s[1], s2), \
            f"sumsq row: max |err| {(s[1] - s2).abs().max().item()}"
    else:
        t1 = 2.0 ** -16 * v.abs().sum((0, 2, 3))
        t2 = 2.0 ** -16 * (v * v).sum((0, 2, 3))
        assert ((s[0] - s1).abs() <= t1).all(), \
            f"sum row: worst ratio {((s[0] - s1).abs() / t1).max().item()}"
        assert ((s[1] - s2).abs() <= t2).all(), \
            f"sumsq row: worst ratio {((s[1] - s2).abs() / t2).max().item()}"


def _cdiv(a, b):
    return -(-a // b)


def _reg_tile(m, c, k_out, k, frac=False):
    """(BM, BN) of the register kernel (dispatch_tile in conv2d_nhwc.hip)."""
    if not frac and c < 32 and k > 1:
        return (128, 64) if k_out <= 64 else (128, 128)
    if _cdiv(m, 128) * _cdiv(k_out, 128) < 160:
        return (64, 64)
    return (128, 64) if k_out <= 64 else (128, 128)


def _out_hw(h, w, k, st, pad):
    return (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1


# --------------------------------------------------------------------------
# case matrices: (N, C, H, W, K, k, stride, pad)
# --------------------------------------------------------------------------

REG_CASES = [
    (2, 3, 9, 11, 24, 3, 1, 1),      # RSCLIN <128,64>, K column mask, M tail
    (2, 1, 10, 14, 64, 4, 2, 1),     # RSCLIN, RSC=16 in one partial chunk
    (2, 20, 7, 9, 72, 4, 1, 0),      # RSCLIN <128,128>, 5 chunks, masked half
    (2, 3, 9, 11, 136, 3, 1, 1),     # RSCLIN wide, two column blocks
    (3, 36, 5, 7, 40, 3, 1, 1),      # dense <64,64>, C%8 != 0 scalar path
    (3, 72, 6, 10, 80, 3, 1, 1),     # dense, vector path, partial 2nd chunk
    (2, 64, 8, 12, 64, 1, 1, 0),     # k1
    (2, 64, 7, 9, 64, 2, 1, 0),      # k2
    (2, 64, 7, 9, 64, 4, 1, 0),      # k4s1
    (3, 64, 10, 14, 96, 4, 2, 1),    # k4s2, odd output 5x7
    (2, 64, 3, 5, 64, 4, 1, 3),      # pad = k-1 (full correlation, dgrad form)
    (5, 40, 64, 66, 64, 3, 1, 1),    # <128,64> non-small, mblocks=165 (rem 5)
    (3, 72, 64, 66, 192, 3, 1, 1),   # <128,128> non-small, K=192 mask, block 2
]
REG_SMALL = (3, 36, 5, 7, 40, 3, 1, 1)
REG_STATS = [REG_SMALL, (5, 40, 64, 66, 64, 3, 1, 1), (2, 3, 9, 11, 24, 3, 1, 1)]
REG_SMOOTH = (3, 72, 6, 10, 80, 3, 1, 1)

# logical shapes; the glds kernel is handed the input zero-ringed by `pad`
GLDS_CASES = [
    (3, 64, 9, 13, 64, 3, 1, 1),     # BN=64, M=351 (partial tile)
    (3, 128, 9, 13, 128, 3, 1, 1),   # BN=128
    (2, 64, 36, 38, 128, 3, 1, 1),   # 11 M-blocks (remap remainder 3)
    (2, 64, 9, 13, 192, 3, 1, 1),    # BN=64, three column blocks
    (3, 64, 18, 22, 64, 4, 2, 1),    # <64,4,2>
    (3, 64, 18, 22, 128, 4, 2, 1),   # <128,4,2>
    (2, 64, 7, 9, 64, 4, 1, 0),      # <64,4,1>, no ring
    (2, 64, 7, 9, 128, 2, 1, 0),     # <128,2,1>
]
GLDS_M351 = GLDS_CASES[0]
GLDS_11BLK = GLDS_CASES[2]
GLDS_ACT = [GLDS_M351, (3, 64, 18, 22, 128, 4, 2, 1)]

DUAL_SRC = [(64, 128), (128, 64), (64, 64)]            # (c1, c2), 6x10 map
DUAL_DST = [(192, 64), (192, 128), (256, 64), (256, 192)]   # (K, K1)

# dispatch threshold of conv2d_nhwc_fwd: (M/256)*(K/BN) >= 200 -> glds
THRESH_N = [50, 49]

# conv2d_nhwc_fracstride, k4 s2 p1: (N, Ci, H, W, Co)
FRAC_CASES = [
    (2, 64, 3, 5, 64),
    (3, 128, 4, 6, 1),
    (2, 8, 5, 3, 64),
    (2, 36, 4, 6, 40),
    (5, 64, 64, 66, 64),             # one non-small tile case, <128,64>
]
FRAC_RINGS = [(0, 0), (1, 0), (0, 1), (1, 1)]

# Function level (section 4): the ring combinations the fused path issues.
#   "bn"  = fused_conv_bn_act (p2pvg_amd/ops/fused_norm.py:116-132): bias
#           None, act 0, want_stats (training), in_ring = the input's
#           `_pvg_pad`, out_ring = 1 if pad_out else 0. ConvT k4s2p1 is not a
#           ring consumer (_consumes_ring, fused_norm.py:197-206) and is only
#           ever followed by one, so it runs with (0, 0) or (0, 1).
#   "act" = fused_conv_act (fused_norm.py:168-176) and the module forwards
#           (ops/conv.py Conv2d / ConvTranspose2d): conv.bias, in_ring,
#           out_ring = 0. Run here with act 0 (the module form) so that the
#           gradient entering the dgrad stays integer-valued.
# (kind, form, N, Ci, H, W, Co, k, stride, pad, in_ring, out_ring). The
# non-square ones pin that the Functions size a ringed output from the height
# AND the width (they once used the height for both).
FN_CASES = [
    ("conv", "bn", 3, 64, 12, 12, 128, 3, 1, 1, 1, 1),
    ("conv", "bn", 3, 64, 12, 12, 128, 3, 1, 1, 1, 0),
    ("conv", "act", 3, 64, 12, 12, 128, 3, 1, 1, 1, 0),
    ("conv", "bn", 2, 64, 6, 10, 64, 3, 1, 1, 1, 1),
    ("conv", "bn", 3, 64, 12, 12, 128, 4, 2, 1, 1, 0),
    ("conv", "bn", 2, 64, 8, 12, 64, 4, 2, 1, 1, 1),
    ("conv", "act", 2, 3, 8, 8, 64, 3, 1, 1, 0, 0),
    ("convt", "act", 2, 64, 8, 8, 3, 3, 1, 1, 1, 0),
    ("convt", "bn", 2, 64, 6, 10, 64, 3, 1, 1, 1, 1),
    ("convt", "bn", 3, 64, 6, 6, 128, 4, 2, 1, 0, 0),
    ("convt", "bn", 2, 64, 4, 6, 64, 4, 2, 1, 0, 1),
    ("convt", "act", 3, 64, 6, 6, 128, 4, 2, 1, 0, 0),
    ("cat", "bn", 3, (64, 128), 8, 8, 128, 3, 1, 1, 1, 1),
    ("cat", "bn", 2, (64, 64), 8, 16, 64, 3, 1, 1, 1, 1),
]


# --------------------------------------------------------------------------
# cached inputs + references (built on first use, shared, never modified)
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _conv_case(case, density=None, tag=""):
    """x, w, b and the exact fp64 pre-activation value v = conv(x, w) + b."""
    n, c, h, wd, k_out, k, st, pad = case
    d = _density(c * k * k) if density is None else density
    x = _ints(_seed("x", case, tag), (n, c, h, wd), -2, 2)
    w = _ints(_seed("w", case, tag), (k_out, c, k, k), -1, 1, d)
    b = _ints(_seed("b", case, tag), (k_out,), -4, 4)
    return x, w, b, _ref_conv(x, w, b, st, pad)


@functools.lru_cache(maxsize=None)
def _thresh_case():
    """N=50 pre-padded 34x34 input; the N=49 case is its first 49 images."""
    x = _ring(_ints(_seed("thr-x"), (50, 64, 32, 32), -2, 2), 1)
    w = _ints(_seed("thr-w"), (64, 64, 3, 3), -1, 1, _density(576))
    b = _ints(_seed("thr-b"), (64,), -4, 4)
    return x, w, b, _ref_conv(x, w, b, 1, 0)


@functools.lru_cache(maxsize=None)
def _frac_case(case):
    """x, ConvT-layout weight wt (Ci, Co, 4, 4), b and v = convT(x, wt) + b.
    An output element sums 2x2 taps of Ci channels."""
    n, ci, h, wd, co = case
    x = _ints(_seed("fx", case), (n, ci, h, wd), -2, 2)
    wt = _ints(_seed("fw", case), (ci, co, 4, 4), -1, 1, _density(4 * ci))
    b = _ints(_seed("fb", case), (co,), -4, 4)
    return x, wt, b, _ref_convt(x, wt, b, 2, 1)


@functools.lru_cache(maxsize=None)
def _dual_dst_case(k_out):
    """Dgrad-shaped call: logical (2, 64, 6, 10) -> K, 3x3 pad 1."""
    return _conv_case((2, 64, 6, 10, k_out, 3, 1, 1))


@functools.lru_cache(maxsize=None)
def _fn_case(case):
    """Module-layout weight, inputs, incoming gradient and fp64 y/dx/dw/db."""
    kind, form, n, ci, h, wd, co, k, st, pad, in_ring, out_ring = case
    cin = sum(ci) if kind == "cat" else ci
    if kind == "convt":
        wshape = (cin, co, k, k)
        taps = k * k if st == 1 else (k // st) ** 2
        d = _density(max(cin * taps, co * k * k))
        fn = lambda xx, ww: F.conv_transpose2d(xx, ww, None, st, pad)  # noqa
    else:
        wshape = (co, cin, k, k)
        taps = k * k if st == 1 else (k // st) ** 2
        d = _density(max(cin * k * k, co * taps))
        fn = lambda xx, ww: F.conv2d(xx, ww, None, st, pad)  # noqa: E731
    key = case[:1] + case[2:10]          # inputs shared across forms / rings
    x = _ints(_seed("nx", key), (n, cin, h, wd), -2, 2)
    w = _ints(_seed("nw", key), wshape, -1, 1, d)
    b = _ints(_seed("nb", key), (co,), -4, 4) if form == "act" else None
    y = fn(x.double(), w.double())
    g = _ints(_seed("ng", key), tuple(y.shape), -2, 2)
    dx, dw = _ref_grads(fn, x, w, g)
    db = g.double().sum((0, 2, 3))
    if b is not None:
        y = y + b.double().view(1, -1, 1, 1)
    return dict(x=x, w=w, b=b, g=g, y=y, dx=dx, dw=dw, db=db)


# --------------------------------------------------------------------------
# 0. CPU: the references themselves
# --------------------------------------------------------------------------

def _id(case):
    return "-".join("x".join(map(str, c)) if isinstance(c, tuple) else str(c)
                    for c in case)


@pytest.mark.parametrize("case", REG_CASES + GLDS_CASES, ids=_id)
def test_cpu_reference_conv(case):
    x, w, b, v = _conv_case(case)
    n, c, h, wd, k_out, k, st, pad = case
    stats_case = case in REG_STATS or case in (GLDS_M351, GLDS_11BLK) \
        or case in GLDS_ACT
    _assert_caps(v, 128 if stats_case else 256)
    assert tuple(v.shape) == (n, k_out) + _out_hw(h, wd, k, st, pad)
    assert torch.equal(v, _conv_unfold(x, w, b, st, pad))
    # the ring convention: a conv with pad 0 over the zero-ringed input
    assert torch.equal(v, _ref_conv(_ring(x, pad), w, b, st, 0))
    # fp32 accumulation is exact on these inputs
    assert torch.equal(v.float(), F.conv2d(x.float(), w.float(), b, st, pad))


def test_cpu_reference_conv_smooth_and_dual():
    for case in (REG_SMOOTH, GLDS_M351):
        x, w, b, v = _conv_case(case, 4.0 / (case[1] * case[5] ** 2), "smooth")
        _assert_caps(v, 256)
        assert torch.equal(v, _conv_unfold(x, w, b, case[6], case[7]))
        assert v.abs().median() <= 4     # the activations are not saturated
    for c1, c2 in DUAL_SRC:
        x, w, b, v = _conv_case((2, c1 + c2, 6, 10, 64, 3, 1, 1))
        _assert_caps(v, 256)
        assert torch.equal(v, _conv_unfold(x, w, b, 1, 1))
    for k_out in (192, 256):
        x, w, b, v = _dual_dst_case(k_out)
        _assert_caps(v, 256)
        assert torch.equal(v, _conv_unfold(x, w, b, 1, 1))


def test_cpu_reference_threshold():
    x, w, b, v = _thresh_case()
    _assert_caps(v, 128)
    assert tuple(v.shape) == (50, 64, 32, 32)
    assert torch.equal(v, _conv_unfold(x, w, b, 1, 0))
    # the two batch sizes lie either side of the dispatch rule
    assert (50 * 32 * 32 // 256) * (64 // 64) >= 200
    assert (49 * 32 * 32 // 256) * (64 // 64) < 200


@pytest.mark.parametrize("case", FRAC_CASES, ids=_id)
def test_cpu_reference_fracstride(case):
    x, wt, b, v = _frac_case(case)
    n, ci, h, wd, co = case
    _assert_caps(v, 128)
    assert tuple(v.shape) == (n, co, 2 * h, 2 * wd)
    assert torch.equal(v, _convt_dilate(x, wt, b, 2, 1))
    # the ring convention: the interior of the ConvT of the ringed input
    vr = _ref_convt(_ring(x, 1), wt, b, 2, 1)
    assert torch.equal(v, vr[:, :, 2:-2, 2:-2])


@pytest.mark.parametrize("case", FN_CASES, ids=_id)
def test_cpu_reference_functions(case):
    kind, form, n, ci, h, wd, co, k, st, pad, in_ring, out_ring = case
    r = _fn_case(case)
    x, w, b, g = r["x"], r["w"], r["b"], r["g"]
    _assert_caps(r["y"], 128 if form == "bn" else 256)
    _assert_caps(r["dx"], 256)
    assert r["dw"].abs().max() < 2 ** 24 and r["db"].abs().max() < 2 ** 24
    assert torch.equal(r["dw"], r["dw"].round())
    if kind == "convt":
        assert torch.equal(r["y"], _convt_dilate(x, w, b, st, pad))
        # dgrad of a ConvT is the plain conv with the untransposed weight
        assert torch.equal(r["dx"], _conv_unfold(g, w, None, st, pad))
        dw = torch.nn.grad.conv2d_weight(g.double(), tuple(w.shape),
                                         x.double(), stride=st, padding=pad)
    else:
        assert torch.equal(r["y"], _conv_unfold(x, w, b, st, pad))
        # dgrad of a conv is the ConvT of the gradient with the same weight
        assert torch.equal(r["dx"], _convt_dilate(g, w, None, st, pad))
        dw = torch.nn.grad.conv2d_weight(x.double(), tuple(w.shape),
                                         g.double(), stride=st, padding=pad)
    assert torch.equal(r["dw"], dw)


# --------------------------------------------------------------------------
# 1. register kernel, direct ext.conv2d_nhwc_fwd (pad given, no rings)
# --------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("case", REG_CASES, ids=_id)
def test_reg_conv_exact(ext, case, act):
    x, w, b, v = _conv_case(case)
    st, pad = case[6], case[7]
    got = ext.conv2d_nhwc_fwd(x.cuda(), w.cuda(), b.cuda(), st, pad, act)[0]
    (_assert_exact if act == 0 else _assert_leaky)(got, v)


@gpu
@pytest.mark.parametrize("act", [2, 3])
def test_reg_conv_tanh_sigmoid(ext, act):
    case = REG_SMOOTH
    x, w, b, v = _conv_case(case, 4.0 / (case[1] * case[5] ** 2), "smooth")
    got = ext.conv2d_nhwc_fwd(x.cuda(), w.cuda(), b.cuda(), case[6], case[7],
                              act)[0]
    _assert_smooth(got, v, act)


@gpu
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("case", REG_STATS, ids=_id)
def test_reg_conv_stats(ext, case, act):
    x, w, b, v = _conv_case(case)
    n, c, h, wd, k_out, k, st, pad = case
    got, stats = ext.conv2d_nhwc_fwd(x.cuda(), w.cuda(), b.cuda(), st, pad,
                                     act, True)
    (_assert_exact if act == 0 else _assert_leaky)(got, v, 128)
    ho, wo = _out_hw(h, wd, k, st, pad)
    bm, _ = _reg_tile(n * ho * wo, c, k_out, k)
    _assert_stats(stats, v, act, _cdiv(n * ho * wo, bm) * 2)


@gpu
def test_reg_conv_placement(ext):
    """oh/ow/oy0/ox0 all distinct: a swapped pair moves the interior."""
    case = REG_SMALL
    x, w, b, v = _conv_case(case)
    n, c, h, wd, k_out, k, st, pad = case
    ho, wo = _out_hw(h, wd, k, st, pad)
    got = ext.conv2d_nhwc_fwd(x.cuda(), w.cuda(), b.cuda(), st, pad, 0, False,
                              ho + 3, wo + 2, 2, 1)[0]
    assert tuple(got.shape) == (n, k_out, ho + 3, wo + 2)
    _assert_exact(got[:, :, 2:2 + ho, 1:1 + wo], v)


# --------------------------------------------------------------------------
# 2. glds kernel, direct ext.conv2d_glds_fwd on zero-ringed inputs
# --------------------------------------------------------------------------

def _glds(ext, case, x, w, b, act=0, stats=False, place=(0, 0, 0, 0),
          in2=None, out2=None):
    return ext.conv2d_glds_fwd(_ring(x, case[7]).cuda(), w.cuda(),
                               None if b is None else b.cuda(), case[6], act,
                               stats, *place, in2, out2)


@gpu
@pytest.mark.parametrize("case", GLDS_CASES, ids=_id)
def test_glds_conv_exact(ext, case):
    x, w, b, v = _conv_case(case)
    _assert_exact(_glds(ext, case, x, w, b)[0], v)
    # no bias: the null-pointer branch of the epilogue
    _assert_exact(_glds(ext, case, x, w, None)[0],
                  v - b.double().view(1, -1, 1, 1))


@gpu
@pytest.mark.parametrize("case", GLDS_ACT, ids=_id)
def test_glds_conv_leaky_bias(ext, case):
    x, w, b, v = _conv_case(case)
    n, c, h, wd, k_out, k, st, pad = case
    got, stats = _glds(ext, case, x, w, b, 1, True)
    _assert_leaky(got, v, 128)
    ho, wo = _out_hw(h, wd, k, st, pad)
    _assert_stats(stats, v, 1, _cdiv(n * ho * wo, 256) * 2)


@gpu
@pytest.mark.parametrize("act", [2, 3])
def test_glds_conv_tanh_sigmoid(ext, act):
    case = GLDS_M351
    x, w, b, v = _conv_case(case, 4.0 / (case[1] * case[5] ** 2), "smooth")
    _assert_smooth(_glds(ext, case, x, w, b, act)[0], v, act)


@gpu
@pytest.mark.parametrize("case", [GLDS_M351, GLDS_11BLK], ids=_id)
def test_glds_conv_stats(ext, case):
    """Both rows, with a partly empty last tile (M % 256 != 0)."""
    x, w, b, v = _conv_case(case)
    n, c, h, wd, k_out, k, st, pad = case
    got, stats = _glds(ext, case, x, w, b, 0, True)
    _assert_exact(got, v, 128)
    ho, wo = _out_hw(h, wd, k, st, pad)
    assert (n * ho * wo) % 256 != 0
    _assert_stats(stats, v, 0, _cdiv(n * ho * wo, 256) * 2)


@gpu
def test_glds_conv_placement(ext):
    case = GLDS_M351
    x, w, b, v = _conv_case(case)
    n, c, h, wd, k_out, k, st, pad = case
    ho, wo = _out_hw(h, wd, k, st, pad)
    got = _glds(ext, case, x, w, b, place=(ho + 3, wo + 2, 2, 1))[0]
    assert tuple(got.shape) == (n, k_out, ho + 3, wo + 2)
    _assert_exact(got[:, :, 2:2 + ho, 1:1 + wo], v)


@gpu
@pytest.mark.parametrize("c1,c2", DUAL_SRC)
def test_glds_dual_source(ext, c1, c2):
    case = (2, c1 + c2, 6, 10, 64, 3, 1, 1)
    x, w, b, v = _conv_case(case)
    x1 = x[:, :c1].contiguous(memory_format=CL)
    x2 = _ring(x[:, c1:], 1).cuda()
    got = _glds(ext, case, x1, w, b, in2=x2)[0]
    _assert_exact(got, v)


@gpu
@pytest.mark.parametrize("k_out,k1", DUAL_DST)
def test_glds_dual_destination(ext, k_out, k1):
    """Columns [0, K1) go to the returned tensor, [K1, K) to the caller's
    out2, both as the interior of a ringed map (the dgrad of a cat conv).
    out2's ring must be left alone."""
    case = (2, 64, 6, 10, k_out, 3, 1, 1)
    x, w, b, v = _dual_dst_case(k_out)
    n, h, wd = 2, 6, 10
    sentinel = 7.0
    out2 = torch.full((n, k_out - k1, h + 2, wd + 2), sentinel,
                      dtype=torch.bfloat16).contiguous(memory_format=CL).cuda()
    out1 = _glds(ext, case, x, w, b, place=(h + 2, wd + 2, 1, 1),
                 out2=out2)[0]
    assert tuple(out1.shape) == (n, k1, h + 2, wd + 2)
    _assert_exact(out1[:, :, 1:-1, 1:-1], v[:, :k1])
    _assert_exact(out2[:, :, 1:-1, 1:-1], v[:, k1:])
    ring = out2.cpu().float().clone()
    ring[:, :, 1:-1, 1:-1] = sentinel
    assert (ring == sentinel).all(), "out2's ring cells were written"


@gpu
@pytest.mark.parametrize("n", THRESH_N)
def test_dispatch_threshold_exact(ext, n):
    """conv2d_nhwc_fwd hands C=K=64 3x3 pad 0 to the glds kernel from
    (M/256)*(K/BN) >= 200 on: N=50 runs it, N=49 the register <128,64> tile.
    The bucket count tells which kernel ran; both are exact."""
    x, w, b, v = _thresh_case()
    x, v = x[:n], v[:n]
    got, stats = ext.conv2d_nhwc_fwd(x.cuda(), w.cuda(), b.cuda(), 1, 0, 0,
                                     True)
    _assert_exact(got, v, 128)
    m = n * 32 * 32
    _assert_stats(stats, v, 0, _cdiv(m, 256 if n == 50 else 128) * 2)


# --------------------------------------------------------------------------
# 3. ext.conv2d_nhwc_fracstride direct (k4, stride 2, pad 1)
# --------------------------------------------------------------------------

def _frac(ext, case, act=0, stats=False, in_ring=0, out_ring=0, bias=True):
    x, wt, b, v = _frac_case(case)
    n, ci, h, wd, co = case
    # the kernel takes the weight with dim 0 = output channels
    wk = wt.transpose(0, 1).contiguous(memory_format=CL)
    got, st = ext.conv2d_nhwc_fracstride(
        _ring(x, in_ring).cuda(), wk.cuda(), b.cuda() if bias else None, 2, 1,
        2 * h, 2 * wd, act, stats, in_ring, out_ring)
    assert tuple(got.shape) == (n, co, 2 * h + 2 * out_ring,
                                2 * wd + 2 * out_ring)
    if out_ring:
        got = got[:, :, out_ring:-out_ring, out_ring:-out_ring]
    return got, st, (v if bias else v - b.double().view(1, -1, 1, 1))


@gpu
@pytest.mark.parametrize("case", FRAC_CASES, ids=_id)
def test_fracstride_exact(ext, case):
    got, _, v = _frac(ext, case)
    _assert_exact(got, v)


@gpu
@pytest.mark.parametrize("in_ring,out_ring", FRAC_RINGS)
def test_fracstride_rings(ext, in_ring, out_ring):
    got, _, v = _frac(ext, FRAC_CASES[0], 0, False, in_ring, out_ring, False)
    _assert_exact(got, v)


@gpu
def test_fracstride_rings_odd_channels(ext):
    got, _, v = _frac(ext, FRAC_CASES[3], 0, False, 1, 1)
    _assert_exact(got, v)


@gpu
def test_fracstride_leaky_bias(ext):
    got, _, v = _frac(ext, FRAC_CASES[3], 1)
    _assert_leaky(got, v)


@gpu
@pytest.mark.parametrize("case", [FRAC_CASES[0], FRAC_CASES[4]], ids=_id)
def test_fracstride_stats(ext, case):
    """Four parity sub-convolutions, each with its own bucket rows."""
    n, ci, h, wd, co = case
    got, stats, v = _frac(ext, case, 0, True)
    _assert_exact(got, v, 128)
    m = n * h * wd                      # compact grid of one parity
    bm, _ = _reg_tile(m, ci, co, 2, frac=True)
    _assert_stats(stats, v, 0, _cdiv(m, bm) * 4 * 2)


# --------------------------------------------------------------------------
# 4. Function level, with rings and shadows
# --------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("case", FN_CASES, ids=_id)
def test_functions_exact(case):
    from p2pvg_amd.ops.conv import (CatConv2dFn, Conv2d, Conv2dNHWCFn,
                                    ConvT2dNHWCFn, ConvTranspose2d,
                                    _conv_shadows)

    kind, form, n, ci, h, wd, co, k, st, pad, in_ring, out_ring = case
    r = _fn_case(case)
    cin = sum(ci) if kind == "cat" else ci
    mod = (ConvTranspose2d if kind == "convt" else Conv2d)(
        cin, co, k, st, pad).cuda()
    mod.weight.data.copy_(r["w"].float())
    if form == "act":
        mod.bias.data.copy_(r["b"])
    sh = _conv_shadows(mod)             # the layouts under test
    bias = mod.bias if form == "act" else None
    stats_wanted = form == "bn"

    x = _ring(r["x"], in_ring).cuda()
    if kind == "cat":
        c1 = ci[0]
        x1 = x[:, :c1].contiguous(memory_format=CL).requires_grad_()
        x2 = x[:, c1:].contiguous(memory_format=CL).requires_grad_()
        y, stats = CatConv2dFn.apply(x1, x2, mod.weight, st, pad, 0,
                                     stats_wanted, sh["f"], sh["b"], in_ring,
                                     out_ring)
    else:
        x.requires_grad_()
        fn = ConvT2dNHWCFn if kind == "convt" else Conv2dNHWCFn
        y, stats = fn.apply(x, mod.weight, bias, st, pad, 0, stats_wanted,
                            sh["f"], sh["b"], in_ring, out_ring)

    def inner(t, ring):
        return t[:, :, ring:-ring, ring:-ring] if ring else t

    cap = 128 if stats_wanted else 256
    assert tuple(y.shape[2:]) == tuple(d + 2 * out_ring
                                       for d in r["y"].shape[2:])
    _assert_exact(inner(y, out_ring), r["y"], cap)
    if stats_wanted:
        if kind == "cat":               # glds kernel
            rows = _cdiv(n * h * wd, 256) * 2
        elif kind == "convt" and st == 2:   # four parities of the h x w grid
            m = n * h * wd
            rows = _cdiv(m, _reg_tile(m, cin, co, 2, True)[0]) * 4 * 2
        else:
            m = n * r["y"].shape[2] * r["y"].shape[3]
            rows = _cdiv(m, _reg_tile(m, cin, co, k)[0]) * 2
        _assert_stats(stats, r["y"], 0, rows)

    # the protocol: a gradient entering a ringed output carries a zero ring
    y.backward(_ring(r["g"], out_ring).cuda())
    if kind == "cat":
        assert x1.grad.shape == x1.shape and x2.grad.shape == x2.shape
        dx = torch.cat([inner(x1.grad, in_ring), inner(x2.grad, in_ring)], 1)
    else:
        assert x.grad.shape == x.shape
        dx = inner(x.grad, in_ring)
    _assert_exact(dx, r["dx"], 256, "dx")
    dw = mod.weight.grad
    assert dw.dtype == torch.float32 and dw.shape == r["dw"].shape
    assert torch.equal(dw.cpu().double(), r["dw"]), \
        f"dW: {int((dw.cpu().double() != r['dw']).sum())} elements differ"
    if form == "act":
        db = mod.bias.grad
        assert db.dtype == torch.float32
        assert torch.equal(db.cpu().double(), r["db"])
