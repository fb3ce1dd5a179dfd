"""GPU tests: all-taps 3x3 wgrad for 16-wide maps (the narrow kernel).

`conv2d_nhwc_wgrad(..., taps=5)` requires the narrow kernel (6 and 7 the same
with the 64x64 and the 128x64 tile forced, where 5 picks by B), `taps=0`
forces the per-tap path. The acceptance property is bitwise equality with the
per-tap path: same slabs, same 64-pixel chunks and K-steps in the same order,
one accumulator chain per element. Operands are the training form: X
zero-ringed with pad=0, Y carrying a ring of width yr. Every shape keeps
n * 256 >= 256 pixels, so `taps=0` is the glds per-tap kernel.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
NARROW = 5
TILES = [5, 6, 7]       # tile by B, 64x64 tiles, 128x64 tiles
H = 16


def _b(b, taps):
    """The 128x64 tile needs B a multiple of 128: a 64-channel case of the
    matrix runs there with 128."""
    return 128 if taps == 7 and b == 64 else b


@pytest.fixture(scope="module")
def ext():
    from p2pvg_amd.ops import _hip_ext_loader

    return _hip_ext_loader.load()


@functools.lru_cache(maxsize=None)
def _operands(n, a, b, h=H, ks=3, st=1, seed=0):
    """Dense bf16 operands of a pad-1 conv. Computed once per shape and
    shared; callers must not modify them."""
    torch.manual_seed(seed)
    x = torch.randn(n, a, h, h, device="cuda").bfloat16()
    ho = (h + 2 - ks) // st + 1
    g = torch.randn(n, b, ho, ho, device="cuda").bfloat16()
    return x, g


@functools.lru_cache(maxsize=None)
def _int_operands(n, a, b, h=H):
    """Integer-valued operands in [-2, 2] and the float64 weight gradient.
    A product is at most 4 and an element sums n*h*h <= 768 of them, so
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


def _call(ext, x, g, yr=1, splitp=0, acc=None, taps=NARROW, ks=3, st=1,
          x2=None, yfill=0.0):
    """Zero-ringed X, pad=0. Returns dW as (B, A, ks, ks)."""
    x2p = _ringed(x2) if x2 is not None else None
    ws = ext.conv2d_nhwc_wgrad(_yring(g, yr, yfill), _ringed(x), ks, ks, st,
                               0, splitp, acc, yr, x2p, -1, taps)
    return ws.permute(0, 3, 1, 2)


#   n  A    B   splitp
SHAPES = [
    (1, 64, 64, 0),     # auto sp clamps to one chunk per slab: all restarts
    (3, 64, 64, 1),     # one slab, three images: the ring wraps in image 2
    (3, 64, 64, 5),     # three-chunk slabs at chunks 0, 3, 6, 9: mid-image
    (2, 64, 64, 3),     # slabs of 3, 3 and 2 chunks: short last, nch = 2
    (2, 128, 64, 0),    # single X with A = 128
    (2, 64, 128, 0),    # two tiles in b
    (1, 128, 128, 0),   # tiles on both sides
]
DUAL = (2, 64, 64, 64)  # n, A1, A2, B


@pytest.mark.parametrize("taps", TILES)
@pytest.mark.parametrize("yr", [0, 1])
@pytest.mark.parametrize("n,a,b,splitp", SHAPES)
def test_narrow_bitwise_equals_per_tap(ext, n, a, b, splitp, yr, taps):
    b = _b(b, taps)
    x, g = _operands(n, a, b)
    got = _call(ext, x, g, yr, splitp, taps=taps)
    assert tuple(got.shape) == (b, a, 3, 3)
    assert torch.equal(got, _call(ext, x, g, yr, splitp, taps=0))


@pytest.mark.parametrize("taps", TILES)
def test_narrow_ignores_y_ring(ext, taps):
    """A non-zero Y ring: a read of it would show in the bits."""
    x, g = _operands(3, 64, _b(64, taps))
    want = _call(ext, x, g, 1, 5, taps=0)
    assert torch.equal(_call(ext, x, g, 1, 5, yfill=3.0, taps=taps), want)
    assert torch.equal(
        _call(ext, x, g, 1, 5, yfill=float("nan"), taps=taps), want)


@pytest.mark.parametrize("taps", TILES)
@pytest.mark.parametrize("yr", [0, 1])
def test_narrow_dual_x(ext, yr, taps):
    """Two X sources: bitwise the per-tap dual-X call, and the same call on
    the concatenated X."""
    n, a1, a2, b = DUAL
    x, g = _operands(n, a1 + a2, _b(b, taps))
    x1, x2 = x[:, :a1].contiguous(), x[:, a1:].contiguous()
    dual = _call(ext, x1, g, yr, x2=x2, taps=taps)
    assert torch.equal(dual, _call(ext, x1, g, yr, x2=x2, taps=0))
    assert torch.equal(dual, _call(ext, x, g, yr, taps=taps))
    assert torch.equal(dual, _call(ext, x, g, yr, taps=0))


@pytest.mark.parametrize("taps", TILES)
@pytest.mark.parametrize("yr", [0, 1])
@pytest.mark.parametrize("n,a,b,splitp", SHAPES)
def test_narrow_exact_on_integers(ext, n, a, b, splitp, yr, taps):
    """Independent of the per-tap kernel: a wrong row, shift or tap plane
    cannot give the exact integer gradient."""
    x, g, ref = _int_operands(n, a, _b(b, taps))
    got = _call(ext, x, g, yr, splitp, taps=taps)
    assert (got.double() == ref).all()


@pytest.mark.parametrize("taps", TILES)
def test_narrow_dual_x_exact_on_integers(ext, taps):
    n, a1, a2, b = DUAL
    x, g, ref = _int_operands(n, a1 + a2, _b(b, taps))
    x1, x2 = x[:, :a1].contiguous(), x[:, a1:].contiguous()
    for yr in (0, 1):
        got = _call(ext, x1, g, yr, x2=x2, taps=taps)
        assert (got.double() == ref).all()


@pytest.mark.parametrize("tile", TILES)
def test_narrow_accumulate_twice_equals_per_tap_twice(ext, tile):
    b = _b(64, tile)
    x, g = _operands(2, 64, b)
    accs = []
    for taps in (tile, 0):
        acc = torch.full((b, 3, 3, 64), 5.0, device="cuda",
                         dtype=torch.float32)
        for _ in range(2):
            out = _call(ext, x, g, acc=acc, splitp=3, taps=taps)
            assert out.data_ptr() == acc.data_ptr()
        accs.append(acc)
    assert torch.equal(accs[0], accs[1])
    fresh = _call(ext, x, g, splitp=3, taps=tile)
    assert torch.equal(accs[0].permute(0, 3, 1, 2), (5.0 + fresh) + fresh)


@pytest.mark.parametrize("taps", TILES)
def test_narrow_taller_map(ext, taps):
    """HO = 32 on a 16-wide map: eight chunks per image."""
    torch.manual_seed(3)
    x = torch.randn(2, 64, 32, 16, device="cuda").bfloat16()
    g = torch.randn(2, _b(64, taps), 32, 16, device="cuda").bfloat16()
    for splitp in (1, 3):
        assert torch.equal(_call(ext, x, g, 1, splitp, taps=taps),
                           _call(ext, x, g, 1, splitp, taps=0))


@pytest.mark.parametrize("kw", [
    dict(shape=(2, 64, 64, 32)),                 # 32 wide
    dict(shape=(1, 64, 64, 64)),                 # 64 wide
    dict(shape=(4, 64, 64, 8)),                  # 8 wide
    dict(shape=(2, 96, 64, 16)),                 # A not 64-aligned
    dict(shape=(2, 64, 32, 16)),                 # B not 64-aligned
    dict(shape=(2, 64, 64, 16), st=2),           # stride 2
], ids=["w32", "w64", "w8", "a96", "b32", "s2"])
def test_narrow_non_eligible_geometry_raises(ext, kw):
    n, a, b, h = kw["shape"]
    st = kw.get("st", 1)
    x, g = _operands(n, a, b, h, 3, st)
    for taps in TILES:
        with pytest.raises(RuntimeError):
            _call(ext, x, g, st=st, taps=taps)


def test_narrow_wide_tile_needs_b128(ext):
    x, g = _operands(2, 64, 64)
    with pytest.raises(RuntimeError):
        _call(ext, x, g, taps=7)
    x, g = _operands(2, 64, 192)
    with pytest.raises(RuntimeError):
        _call(ext, x, g, taps=7)
    assert torch.equal(_call(ext, x, g), _call(ext, x, g, taps=0))


def test_narrow_path_name(ext):
    path = ext.conv2d_wgrad_path
    was = ext.wgrad_narrow()
    try:
        ext.set_wgrad_narrow(True)
        #           B    A   A1  HO  WO  yr
        assert path(256, 256, 256, 16, 16, 1, -1) == "taps_narrow"
        assert path(256, 256, 256, 16, 16, 1, 0) == "per_tap"
        for taps in (5, 6):
            assert path(64, 64, 64, 16, 16, 0, taps) == "taps_narrow"
        assert path(128, 64, 64, 16, 16, 0, 7) == "taps_narrow"
        ext.set_wgrad_narrow(False)
        assert path(256, 256, 256, 16, 16, 1, -1) == "per_tap"
        assert path(256, 256, 256, 16, 16, 1, 5) == "taps_narrow"
    finally:
        ext.set_wgrad_narrow(was)
