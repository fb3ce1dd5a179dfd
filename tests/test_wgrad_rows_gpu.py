"""GPU tests: row-order all-taps 3x3 wgrad for 64-wide maps.

`conv2d_nhwc_wgrad(..., taps=2)` requires the row-order kernel (3 and 4 the
same with the 64x64 and the 32x64 tile forced, where 2 picks by CU fill),
`taps=0` forces the per-tap path. The acceptance property is bitwise equality
with the per-tap path: same slabs, same K-steps in the same order, one
accumulator chain per element. Operands are the training form: X zero-ringed
with pad=0, Y carrying a ring of width yr.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
ROWS = [2, 3, 4]        # auto tile, 64x64 tiles, 32x64 tiles


@pytest.fixture(scope="module")
def ext():
    from p2pvg_amd.ops import _hip_ext_loader

    return _hip_ext_loader.load()


@functools.lru_cache(maxsize=None)
def _operands(n, a, b, h, ks=3, st=1, seed=0):
    """Dense bf16 operands of a pad-1 conv. Computed once per shape and
    shared; callers must not modify them."""
    torch.manual_seed(seed)
    x = torch.randn(n, a, h, h, device="cuda").bfloat16()
    ho = (h + 2 - ks) // st + 1
    g = torch.randn(n, b, ho, ho, device="cuda").bfloat16()
    return x, g


@functools.lru_cache(maxsize=None)
def _int_operands(n, a, b, h):
    """Integer-valued operands in [-2, 2] and the float64 weight gradient.
    A product is at most 4 and an element sums n*h*h <= 12288 of them, so
    every fp32 partial sum is an integer below 2^24: exact in any order."""
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randint(-2, 3, (n, a, h, h), device="cuda", generator=gen)
    g = torch.randint(-2, 3, (n, b, h, h), device="cuda", generator=gen)
    xp = F.pad(x.double(), (1,) * 4)
    gd = g.double()
    ref = torch.empty(b, a, 3, 3, device="cuda", dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            ref[:, :, r, s] = torch.einsum(
                "nbhw,nahw->ba", gd, xp[:, :, r:r + h, s:s + h])
    assert ref.abs().max().item() < 2 ** 24
    return x.bfloat16(), g.bfloat16(), ref


def _ringed(x):
    return F.pad(x, (1,) * 4).contiguous(memory_format=CL)


def _yring(g, yr, fill=0.0):
    if not yr:
        return g.contiguous(memory_format=CL)
    return F.pad(g, (yr,) * 4, value=fill).contiguous(memory_format=CL)


def _call(ext, x, g, yr=1, splitp=0, acc=None, taps=2, ks=3, st=1, x2=None,
          form="ringed", yfill=0.0):
    """form 'ringed': zero-ringed X, pad=0.  form 'unpadded': dense X, pad=1.
    Returns dW as (B, A, ks, ks)."""
    if form == "ringed":
        xp, pad = _ringed(x), 0
        x2p = _ringed(x2) if x2 is not None else None
    else:
        xp, pad, x2p = x.contiguous(memory_format=CL), 1, None
    ws = ext.conv2d_nhwc_wgrad(_yring(g, yr, yfill), xp, ks, ks, st, pad,
                               splitp, acc, yr, x2p, -1, taps)
    return ws.permute(0, 3, 1, 2)


#   n  A    B    h  splitp
SHAPES = [
    (1, 64, 64, 64, 0),     # 64 slabs of one row: every chunk is a restart
    (1, 64, 64, 64, 1),     # one slab: the ring rotates through an image
    (3, 64, 64, 64, 2),     # slab boundary at row 32 of the middle image
    (2, 64, 64, 64, 5),     # 26-row slabs off the images, last one 24 rows
    (2, 128, 64, 64, 0),    # single X with A = 128
    (2, 64, 128, 64, 0),    # two tiles in b
    (1, 128, 128, 64, 0),   # tiles on both sides
]
DUAL = (2, 64, 64, 64, 64)  # n, A1, A2, B, h


@pytest.mark.parametrize("taps", ROWS)
@pytest.mark.parametrize("yr", [0, 1])
@pytest.mark.parametrize("n,a,b,h,splitp", SHAPES)
def test_rows_bitwise_equals_per_tap(ext, n, a, b, h, splitp, yr, taps):
    x, g = _operands(n, a, b, h)
    got = _call(ext, x, g, yr, splitp, taps=taps)
    assert tuple(got.shape) == (b, a, 3, 3)
    assert torch.equal(got, _call(ext, x, g, yr, splitp, taps=0))


@pytest.mark.parametrize("taps", ROWS)
@pytest.mark.parametrize("yr", [0, 1])
def test_rows_dual_x(ext, yr, taps):
    """Two X sources: bitwise the per-tap dual-X call, and the same call on
    the concatenated X."""
    n, a1, a2, b, h = DUAL
    x, g = _operands(n, a1 + a2, b, h)
    x1, x2 = x[:, :a1].contiguous(), x[:, a1:].contiguous()
    dual = _call(ext, x1, g, yr, x2=x2, taps=taps)
    assert torch.equal(dual, _call(ext, x1, g, yr, x2=x2, taps=0))
    assert torch.equal(dual, _call(ext, x, g, yr, taps=taps))


@pytest.mark.parametrize("taps", ROWS)
@pytest.mark.parametrize("yr", [0, 1])
@pytest.mark.parametrize("n,a,b,h,splitp", SHAPES)
def test_rows_exact_on_integers(ext, n, a, b, h, splitp, yr, taps):
    """Independent of the per-tap kernel: a wrong row, shift or tap plane
    cannot give the exact integer gradient."""
    x, g, ref = _int_operands(n, a, b, h)
    got = _call(ext, x, g, yr, splitp, taps=taps)
    assert (got.double() == ref).all()


@pytest.mark.parametrize("taps", ROWS)
def test_rows_dual_x_exact_on_integers(ext, taps):
    n, a1, a2, b, h = DUAL
    x, g, ref = _int_operands(n, a1 + a2, b, h)
    x1, x2 = x[:, :a1].contiguous(), x[:, a1:].contiguous()
    for yr in (0, 1):
        assert (_call(ext, x1, g, yr, x2=x2, taps=taps).double() == ref).all()


@pytest.mark.parametrize("taps", ROWS)
def test_rows_accumulate_matches_fresh(ext, taps):
    x, g = _operands(2, 64, 64, 64)
    fresh = _call(ext, x, g, taps=taps)
    acc = torch.full((64, 3, 3, 64), 5.0, device="cuda", dtype=torch.float32)
    base = acc.clone()
    out = _call(ext, x, g, acc=acc, taps=taps)
    assert out.data_ptr() == acc.data_ptr()
    assert torch.equal(acc.permute(0, 3, 1, 2),
                       base.permute(0, 3, 1, 2) + fresh)


@pytest.mark.parametrize("taps", ROWS)
def test_rows_bitwise_deterministic(ext, taps):
    x, g = _operands(2, 64, 64, 64)
    assert torch.equal(_call(ext, x, g, taps=taps),
                       _call(ext, x, g, taps=taps))


@pytest.mark.parametrize("taps", ROWS)
def test_rows_reads_stay_in_bounds(ext, taps):
    """The in-bounds contract: shifted images reach column wo + 2 <= 65, rows
    reach ho + 2 <= 65, nothing lies beyond the last image. Y's ring may hold
    anything: NaN there leaves the result unchanged. X is a view whose
    storage ends exactly at its last element, and the same view between NaN
    guards: the result is that of the ordinary tensor."""
    x, g = _operands(2, 64, 64, 64)
    base = _call(ext, x, g, taps=taps)
    assert torch.isfinite(base).all()
    assert torch.equal(_call(ext, x, g, taps=taps, yfill=float("nan")), base)

    xp = _ringed(x)                                   # (2, 64, 66, 66) CL
    flat = xp.permute(0, 2, 3, 1).reshape(-1)
    gp = _yring(g, 1, float("nan"))

    exact = flat.clone()
    assert exact.untyped_storage().nbytes() == exact.numel() * 2
    xv = exact.view(2, 66, 66, 64).permute(0, 3, 1, 2)
    got = ext.conv2d_nhwc_wgrad(gp, xv, 3, 3, 1, 0, 0, None, 1, None, -1, taps)
    assert torch.equal(got.permute(0, 3, 1, 2), base)

    guard = 64
    buf = torch.full((flat.numel() + 2 * guard,), float("nan"),
                     device="cuda", dtype=torch.bfloat16)
    buf[guard:guard + flat.numel()] = flat
    xv = buf[guard:guard + flat.numel()].view(2, 66, 66, 64).permute(0, 3, 1, 2)
    got = ext.conv2d_nhwc_wgrad(gp, xv, 3, 3, 1, 0, 0, None, 1, None, -1, taps)
    assert torch.equal(got.permute(0, 3, 1, 2), base)


@pytest.mark.parametrize("kw", [
    dict(shape=(2, 64, 64, 32)),                      # 32 wide
    dict(shape=(1, 64, 64, 128)),                     # 128 wide
    dict(shape=(2, 64, 64, 64), ks=4, st=2),          # k4 s2
    dict(shape=(2, 64, 64, 64), form="unpadded"),     # pad=1, dense X
], ids=["w32", "w128", "k4s2", "pad1"])
def test_rows_non_eligible_geometry_raises(ext, kw):
    n, a, b, h = kw["shape"]
    ks, st, form = kw.get("ks", 3), kw.get("st", 1), kw.get("form", "ringed")
    x, g = _operands(n, a, b, h, ks, st)
    for taps in ROWS:
        with pytest.raises(RuntimeError):
            _call(ext, x, g, taps=taps, ks=ks, st=st, form=form)


def test_rows_path_name(ext):
    """auto's choice is invisible in the bits, so the host-side path function
    shows it: the two headline classes take the row-order kernel, the
    switch and every class left out keep the per-tap path."""
    path = ext.conv2d_wgrad_path
    was = ext.wgrad_rows()
    try:
        ext.set_wgrad_rows(True)
        #           B    A   A1  HO  WO  yr
        assert path(64, 64, 64, 64, 64, 1, -1) == "taps_rows"      # c1.1
        assert path(64, 128, 64, 64, 64, 1, -1) == "taps_rows"     # upc5.0
        assert path(64, 64, 64, 64, 64, 1, 0) == "per_tap"
        assert path(64, 64, 64, 64, 64, 1, 1) == "taps_strip"
        assert path(64, 64, 64, 64, 64, 0, 2) == "taps_rows"
        # the measured 64-wide classes of the 128-pixel model
        assert path(128, 64, 64, 64, 64, 1, -1) == "taps_rows"
        assert path(128, 256, 128, 64, 64, 1, -1) == "taps_rows"
        # left out: wider channel counts, 128-wide maps
        assert path(256, 64, 64, 64, 64, 1, -1) == "per_tap"
        assert path(64, 512, 512, 64, 64, 1, -1) == "per_tap"
        assert path(64, 64, 64, 128, 128, 1, -1) == "per_tap"
        assert path(64, 64, 64, 32, 32, 1, -1) == "taps_strip"
        with pytest.raises(RuntimeError):
            path(64, 64, 64, 32, 32, 1, 2)
        ext.set_wgrad_rows(False)
        assert path(64, 64, 64, 64, 64, 1, -1) == "per_tap"
        assert path(64, 128, 64, 64, 64, 1, -1) == "per_tap"
        assert path(64, 64, 64, 64, 64, 1, 2) == "taps_rows"
    finally:
        ext.set_wgrad_rows(was)
