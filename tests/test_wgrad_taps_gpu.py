"""GPU tests: single-pass 3x3 wgrad (all nine taps from one staged read).

`conv2d_nhwc_wgrad(..., taps=1)` requires the all-taps kernel, `taps=0`
forces the per-tap path it replaces, `taps=-1` picks. Operands are the
training form: X zero-ringed with pad=0, Y carrying a ring of width yr.
Reference and bound are those of test_wgrad_thin_gpu.py:
torch.nn.grad.conv2d_weight in fp32 on the bf16-rounded operands,
err < 2e-2*scale + 2e-2.
"""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last


@pytest.fixture(scope="module")
def ext():
    from p2pvg_amd.ops import _hip_ext_loader

    return _hip_ext_loader.load()


@functools.lru_cache(maxsize=None)
def _operands(n, a, b, h, ks=3, st=1, seed=0):
    """Dense bf16-exact operands of a pad-1 conv and the fp32 reference dW.
    Computed once per shape and shared; callers must not modify them."""
    torch.manual_seed(seed)
    x = torch.randn(n, a, h, h, device="cuda").bfloat16()
    ho = (h + 2 - ks) // st + 1
    g = torch.randn(n, b, ho, ho, device="cuda").bfloat16()
    ref = torch.nn.grad.conv2d_weight(
        x.float(), (b, a, ks, ks), g.float(), stride=st, padding=1)
    return x, g, ref


def _ringed(x):
    return F.pad(x, (1,) * 4).contiguous(memory_format=CL)


def _yring(g, yr, fill=0.0):
    if not yr:
        return g.contiguous(memory_format=CL)
    return F.pad(g, (yr,) * 4, value=fill).contiguous(memory_format=CL)


def _call(ext, x, g, yr=1, splitp=0, acc=None, taps=1, ks=3, st=1, x2=None,
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


def _check(got, ref):
    scale = ref.abs().max().item() + 1e-6
    err = (got.float() - ref).abs().max().item()
    print(f"err {err:.3e} scale {scale:.3e}")
    assert err < 2e-2 * scale + 2e-2, f"wgrad err {err} scale {scale}"
    return err, scale


#   n  A    B    h   yr splitp
CASES = [
    (2, 64, 64, 32, 1, 0),
    (2, 64, 64, 32, 1, 1),
    (2, 64, 64, 32, 1, 2),
    (2, 64, 64, 32, 0, 0),     # dense Y
    (1, 64, 64, 64, 1, 0),     # two strips, ring rotation over 64 rows
    (1, 64, 64, 64, 1, 1),
    (3, 64, 64, 32, 1, 2),     # slab boundary in the middle of an image
    (2, 128, 64, 32, 1, 0),    # several tiles per side
    (2, 64, 128, 32, 1, 0),
    (2, 128, 128, 32, 0, 0),
    (1, 64, 64, 128, 1, 0),    # four strips per row
    (1, 64, 64, 128, 0, 3),
]


@pytest.mark.parametrize("n,a,b,h,yr,splitp", CASES)
def test_taps_matches_reference(ext, n, a, b, h, yr, splitp):
    x, g, ref = _operands(n, a, b, h)
    got = _call(ext, x, g, yr, splitp)
    assert tuple(got.shape) == (b, a, 3, 3)
    _check(got, ref)


@pytest.mark.parametrize("n,a1,a2,b,h", [(2, 64, 64, 64, 32),
                                         (2, 128, 128, 128, 32)])
def test_taps_dual_x(ext, n, a1, a2, b, h):
    """Two X sources (skip-concat elimination) against the same call on the
    concatenated X: the same products in the same order."""
    x, g, ref = _operands(n, a1 + a2, b, h)
    x1, x2 = x[:, :a1].contiguous(), x[:, a1:].contiguous()
    dual = _call(ext, x1, g, x2=x2)
    _check(dual, ref)
    assert torch.equal(dual, _call(ext, x, g))


def test_taps_reads_stay_in_bounds(ext):
    """Parity check of the in-bounds contract. Y's ring may hold anything
    (conv-output rings are garbage): NaN there leaves the result unchanged.
    X is a view whose storage ends exactly at its last element, and the same
    view between NaN guards: the result is that of the ordinary tensor."""
    x, g, ref = _operands(2, 64, 64, 32)
    base = _call(ext, x, g)
    assert torch.equal(_call(ext, x, g, yfill=float("nan")), base)

    xp = _ringed(x)                                   # (2, 64, 34, 34) CL
    flat = xp.permute(0, 2, 3, 1).reshape(-1)
    gp = _yring(g, 1, float("nan"))

    exact = flat.clone()
    assert exact.untyped_storage().nbytes() == exact.numel() * 2
    xv = exact.view(2, 34, 34, 64).permute(0, 3, 1, 2)
    got = ext.conv2d_nhwc_wgrad(gp, xv, 3, 3, 1, 0, 0, None, 1, None, -1, 1)
    assert torch.isfinite(got).all()
    assert torch.equal(got.permute(0, 3, 1, 2), base)

    guard = 64
    buf = torch.full((flat.numel() + 2 * guard,), float("nan"),
                     device="cuda", dtype=torch.bfloat16)
    buf[guard:guard + flat.numel()] = flat
    xv = buf[guard:guard + flat.numel()].view(2, 34, 34, 64).permute(0, 3, 1, 2)
    got = ext.conv2d_nhwc_wgrad(gp, xv, 3, 3, 1, 0, 0, None, 1, None, -1, 1)
    assert torch.isfinite(got).all()
    assert torch.equal(got.permute(0, 3, 1, 2), base)


@pytest.mark.parametrize("kw", [
    dict(shape=(2, 64, 64, 16)),                      # 16 wide: below a strip
    dict(shape=(2, 64, 64, 32), ks=4, st=2),          # k4 s2
    dict(shape=(2, 64, 64, 32), form="unpadded"),     # pad=1, dense X
], ids=["h16", "k4s2", "pad1"])
def test_taps_non_eligible_geometry(ext, kw):
    """Auto keeps the per-tap path and matches; taps=1 raises."""
    n, a, b, h = kw["shape"]
    ks, st, form = kw.get("ks", 3), kw.get("st", 1), kw.get("form", "ringed")
    x, g, ref = _operands(n, a, b, h, ks, st)
    _check(_call(ext, x, g, taps=-1, ks=ks, st=st, form=form), ref)
    with pytest.raises(RuntimeError):
        _call(ext, x, g, taps=1, ks=ks, st=st, form=form)


# 32-wide shapes: a K-step is one output row on both paths and the slabs
# are the same, so the all-taps result is the per-tap result bit for bit.
# These are also the (B, A, width) classes auto sends to the all-taps kernel
# (taps_auto in conv2d_wgrad.hip), at test size.
W32 = [(2, 64, 64, 32), (3, 64, 64, 32), (2, 128, 64, 32), (2, 64, 128, 32),
       (2, 128, 128, 32)]


@pytest.mark.parametrize("n,a,b,h", W32)
@pytest.mark.parametrize("splitp", [0, 2])
def test_taps_bitwise_equals_per_tap_on_32_wide(ext, n, a, b, h, splitp):
    x, g, _ = _operands(n, a, b, h)
    assert torch.equal(_call(ext, x, g, 1, splitp, taps=1),
                       _call(ext, x, g, 1, splitp, taps=0))


def test_taps_dual_x_bitwise_equals_per_tap(ext):
    x, g, _ = _operands(2, 256, 128, 32)
    x1, x2 = x[:, :128].contiguous(), x[:, 128:].contiguous()
    assert torch.equal(_call(ext, x1, g, x2=x2, taps=1),
                       _call(ext, x1, g, x2=x2, taps=0))


def test_taps_auto_takes_taps_path_on_32_wide_only(ext):
    """On a 64-wide map the two paths sum in another order, so bitwise
    equality with taps=0 (and not taps=1) shows auto stayed per-tap."""
    x, g, _ = _operands(1, 64, 64, 64)
    auto = _call(ext, x, g, taps=-1)
    assert torch.equal(auto, _call(ext, x, g, taps=0))
    assert not torch.equal(auto, _call(ext, x, g, taps=1))
    x, g, _ = _operands(2, 64, 64, 32)
    assert torch.equal(_call(ext, x, g, taps=-1), _call(ext, x, g, taps=1))


def test_taps_bitwise_deterministic(ext):
    x, g, _ = _operands(3, 64, 64, 32)
    assert torch.equal(_call(ext, x, g), _call(ext, x, g))


@pytest.mark.parametrize("splitp", [0, 1])
def test_taps_accumulate_matches_fresh(ext, splitp):
    x, g, _ = _operands(2, 64, 64, 32)
    fresh = _call(ext, x, g, 1, splitp)
    acc = torch.full((64, 3, 3, 64), 5.0, device="cuda", dtype=torch.float32)
    base = acc.clone()
    out = _call(ext, x, g, 1, splitp, acc)
    assert out.data_ptr() == acc.data_ptr()
    assert torch.equal(acc.permute(0, 3, 1, 2), base.permute(0, 3, 1, 2) + fresh)


def test_taps_no_worse_than_per_tap_path(ext):
    """Inputs are bf16-exact and both kernels accumulate in fp32, so both
    errors are summation-order noise: the new one may not exceed twice the
    old (ordering luck) plus a floor for e_old == 0."""
    x, g, ref = _operands(2, 64, 64, 32)
    e_old, scale = _check(_call(ext, x, g, taps=0), ref)
    e_new, _ = _check(_call(ext, x, g, taps=1), ref)
    print(f"e_old {e_old:.3e} e_new {e_new:.3e} scale {scale:.3e}")
    assert e_new <= 2 * e_old + 1e-6 * scale


def test_module_vgg_64_64_weight_grad():
    """Conv2d(64,64,3,1,1) inside a vgg_layer fed a zero-ringed 32x32 map, as
    Encoder64.c1's second layer is: backward reaches the wgrad with pad=0,
    ringed X and yring=1, the geometry of the all-taps kernel. Inputs and
    parameters are bf16-exact and the bound is that of
    test_module_first_conv_weight_grad (see there for what dominates it)."""
    from p2pvg_amd.models.backbones.blocks import vgg_layer
    from p2pvg_amd.ops.conv import interior_view

    torch.manual_seed(6)
    ref = nn.Sequential(
        nn.Conv2d(64, 64, 3, 1, 1), nn.BatchNorm2d(64), nn.LeakyReLU(0.2),
    ).cuda()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.bfloat16().float())
    hip = vgg_layer(64, 64, pad_out=True).cuda()
    with torch.no_grad():
        hip.main[0].weight.copy_(ref[0].weight)
        hip.main[0].bias.copy_(ref[0].bias)
        hip.main[1].weight.copy_(ref[1].weight)
        hip.main[1].bias.copy_(ref[1].bias)

    x = torch.randn(2, 64, 32, 32, device="cuda").bfloat16().float()
    y_ref = ref(x)
    g = torch.randn_like(y_ref).bfloat16().float()
    y_ref.backward(g)

    xin = _ringed(x.bfloat16())
    xin._pvg_pad = 1
    y = hip(xin)
    assert getattr(y, "_pvg_pad", 0) == 1
    interior_view(y).backward(g.bfloat16())
    want, got = ref[0].weight.grad, hip.main[0].weight.grad.float()
    s = want.abs().max().item() + 1e-6
    e = (want - got).abs().max().item()
    print(f"vgg 64->64 dw: err {e:.3e} scale {s:.3e}")
    assert e < 0.05 * s + 0.05, f"dw err {e} scale {s}"
