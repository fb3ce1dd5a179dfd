"""GPU tests: thin-channel wgrad (taps folded into <= 32 GEMM columns).

The first encoder conv and the last decoder ConvT have A = 1..3 channels on
the thin side. `conv2d_nhwc_wgrad(..., thin=1)` requires the tap-folded
kernel, `thin=0` forces the per-tap path it replaces, `thin=-1` picks.
Reference and bound are those of test_wgrad_padded_matches_reference:
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
def _operands(n, a, b, h, ks, st, seed=0):
    """Dense bf16-exact operands of a pad-1 conv and the fp32 reference dW.
    Computed once per shape and shared; callers must not modify them."""
    torch.manual_seed(seed)
    x = torch.randn(n, a, h, h, device="cuda").bfloat16()
    ho = (h + 2 - ks) // st + 1
    g = torch.randn(n, b, ho, ho, device="cuda").bfloat16()
    ref = torch.nn.grad.conv2d_weight(
        x.float(), (b, a, ks, ks), g.float(), stride=st, padding=1)
    return x, g, ref


def _call(ext, x, g, ks, st, form, yr, splitp=0, acc=None, thin=1):
    """form 'unpadded': dense X, pad=1.  form 'ringed': zero-ringed X, pad=0.
    Y carries a zero ring of width yr. Returns dW as (B, A, ks, ks)."""
    if form == "ringed":
        xp, pad = F.pad(x, (1,) * 4), 0
    else:
        xp, pad = x, 1
    xp = xp.contiguous(memory_format=CL)
    gp = (F.pad(g, (yr,) * 4) if yr else g).contiguous(memory_format=CL)
    ws = ext.conv2d_nhwc_wgrad(gp, xp, ks, ks, st, pad, splitp, acc, yr,
                               None, thin)
    return ws.permute(0, 3, 1, 2)


def _check(got, ref):
    scale = ref.abs().max().item() + 1e-6
    err = (got.float() - ref).abs().max().item()
    assert err < 2e-2 * scale + 2e-2, f"wgrad err {err} scale {scale}"
    return err, scale


#   n  A  B    h  ks st form        yr splitp
CASES = [
    (2, 3, 64, 8, 3, 1, "unpadded", 1, 0),   # headline form, both conv and
    (2, 3, 64, 8, 3, 1, "unpadded", 1, 1),   # ConvT (Y=x ringed, X=gout)
    (3, 3, 64, 4, 3, 1, "unpadded", 1, 0),   # 48 pixels: tail only
    (5, 3, 64, 8, 3, 1, "unpadded", 1, 2),   # uneven slabs 192 + 128
    (4, 3, 64, 16, 3, 1, "unpadded", 1, 1),  # 16 chunks: buffer rotation
    (4, 3, 64, 16, 3, 1, "unpadded", 1, 0),
    (3, 1, 64, 16, 4, 2, "unpadded", 0, 0),  # dcgan first conv, 16 columns
    (3, 1, 64, 16, 4, 2, "unpadded", 1, 1),
    (2, 2, 64, 9, 4, 1, "unpadded", 1, 0),   # exactly 32 columns
    (2, 2, 64, 9, 4, 1, "unpadded", 1, 1),
    (2, 3, 128, 8, 3, 1, "unpadded", 1, 0),  # two b-tiles
    (2, 3, 64, 8, 3, 1, "ringed", 1, 0),     # pad=0 with ringed X
    (3, 3, 64, 8, 3, 1, "ringed", 0, 1),     # 3 chunks, dense Y
]


@pytest.mark.parametrize("n,a,b,h,ks,st,form,yr,splitp", CASES)
def test_thin_matches_reference(ext, n, a, b, h, ks, st, form, yr, splitp):
    x, g, ref = _operands(n, a, b, h, ks, st)
    got = _call(ext, x, g, ks, st, form, yr, splitp)
    assert tuple(got.shape) == (b, a, ks, ks)
    _check(got, ref)


def test_thin_convt_call_form(ext):
    """ConvTranspose2d(64,3,3,1,1).backward hands the 64-channel input as Y
    (ringed) and the 3-channel grad_out as X; the result, read as
    (Ci,Co,k,k), is autograd's conv_transpose2d weight gradient."""
    torch.manual_seed(3)
    xin = torch.randn(2, 64, 8, 8, device="cuda").bfloat16()
    gout = torch.randn(2, 3, 8, 8, device="cuda").bfloat16()
    w = torch.zeros(64, 3, 3, 3, device="cuda", requires_grad=True)
    F.conv_transpose2d(xin.float(), w, None, 1, 1).backward(gout.float())
    got = _call(ext, gout, xin, 3, 1, "unpadded", 1)
    _check(got, w.grad)


def test_thin_non_eligible_geometry(ext):
    """12x12 is not a power of two: auto keeps the old path, thin=1 raises."""
    x, g, ref = _operands(2, 3, 64, 12, 3, 1)
    _check(_call(ext, x, g, 3, 1, "unpadded", 1, thin=-1), ref)
    with pytest.raises(RuntimeError):
        _call(ext, x, g, 3, 1, "unpadded", 1, thin=1)


def test_thin_auto_takes_thin_path(ext):
    x, g, _ = _operands(2, 3, 64, 8, 3, 1)
    auto = _call(ext, x, g, 3, 1, "unpadded", 1, thin=-1)
    thin = _call(ext, x, g, 3, 1, "unpadded", 1, thin=1)
    assert torch.equal(auto, thin)


@pytest.mark.parametrize("splitp", [0, 1])
def test_thin_accumulate_matches_fresh(ext, splitp):
    x, g, _ = _operands(4, 3, 64, 16, 3, 1)
    fresh = _call(ext, x, g, 3, 1, "unpadded", 1, splitp)
    acc = torch.full((64, 3, 3, 3), 5.0, device="cuda", dtype=torch.float32)
    base = acc.clone()
    out = _call(ext, x, g, 3, 1, "unpadded", 1, splitp, acc)
    assert out.data_ptr() == acc.data_ptr()
    assert torch.equal(acc.permute(0, 3, 1, 2), base.permute(0, 3, 1, 2) + fresh)


def test_thin_bitwise_deterministic(ext):
    x, g, _ = _operands(4, 3, 64, 16, 3, 1)
    a = _call(ext, x, g, 3, 1, "unpadded", 1)
    b = _call(ext, x, g, 3, 1, "unpadded", 1)
    assert torch.equal(a, b)


def test_thin_no_worse_than_per_tap_path(ext):
    """Inputs are bf16-exact and both kernels accumulate in fp32, so both
    errors are summation-order noise: the new one may not exceed twice the
    old (ordering luck) plus a floor for e_old == 0."""
    x, g, ref = _operands(2, 3, 64, 8, 3, 1)
    e_old, scale = _check(_call(ext, x, g, 3, 1, "unpadded", 1, thin=0), ref)
    e_new, _ = _check(_call(ext, x, g, 3, 1, "unpadded", 1, thin=1), ref)
    print(f"e_old {e_old:.3e} e_new {e_new:.3e} scale {scale:.3e}")
    assert e_new <= 2 * e_old + 1e-6 * scale


def _bf16_exact_(module):
    """Round parameters to bf16-representable values in place, so the fp32
    reference and the bf16 path start from the same numbers (as the op-level
    reference does with its operands): what is left is arithmetic, not input
    quantisation."""
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(p.bfloat16().float())
    return module


def _copy_layer(dst_conv, dst_bn, src_conv, src_bn):
    with torch.no_grad():
        dst_conv.weight.copy_(src_conv.weight)
        dst_conv.bias.copy_(src_conv.bias)
        dst_bn.weight.copy_(src_bn.weight)
        dst_bn.bias.copy_(src_bn.bias)


def _grad_close(name, ref, got, tol=0.05):
    s = ref.abs().max().item() + 1e-6
    e = (ref - got.float()).abs().max().item()
    print(f"{name}: err {e:.3e} scale {s:.3e}")
    assert e < tol * s + tol, f"{name} err {e} scale {s}"


def test_module_first_conv_weight_grad():
    """Conv2d(3,64,3,1,1) inside its FusedSequential with BatchNorm and
    LeakyReLU (a vgg_layer), emitting the zero-ringed map Encoder64.c1 hands
    on: backward reaches the wgrad with pad=1, unpadded X and yring=1.

    The grad_out this wgrad receives has been through the bf16 BatchNorm
    backward, whose output is orthogonal to the conv output, so dW is a sum
    with heavy cancellation and upstream rounding dominates: measured
    err/scale 3.2 % here (3.76 on 118.5), identical on the per-tap path,
    while the wgrad itself reproduces the exact fp32 result on the captured
    operands to 3e-5. With unrounded fp32 inputs and weights on the
    reference side the same chain measured 5.5 %, and 7.2 % with a second
    vgg_layer behind it, so inputs and parameters are made bf16-exact."""
    from p2pvg_amd.models.backbones.blocks import vgg_layer
    from p2pvg_amd.ops.conv import interior_view

    torch.manual_seed(4)
    ref = _bf16_exact_(nn.Sequential(
        nn.Conv2d(3, 64, 3, 1, 1), nn.BatchNorm2d(64), nn.LeakyReLU(0.2),
    ).cuda())
    hip = vgg_layer(3, 64, pad_out=True).cuda()
    _copy_layer(hip.main[0], hip.main[1], ref[0], ref[1])

    x = torch.rand(2, 3, 16, 16, device="cuda").bfloat16().float()
    y_ref = ref(x)
    g = torch.randn_like(y_ref).bfloat16().float()
    y_ref.backward(g)

    y = hip(x.bfloat16().contiguous(memory_format=CL))
    assert getattr(y, "_pvg_pad", 0) == 1
    interior_view(y).backward(g.bfloat16())
    _grad_close("first conv dw", ref[0].weight.grad, hip.main[0].weight.grad)


def test_module_last_convt_weight_grad():
    """ConvTranspose2d(64,3,3,1,1) behind its vgg neighbour, as in
    Decoder64.upc5."""
    from p2pvg_amd.models.backbones.blocks import vgg_layer
    from p2pvg_amd.ops.conv import ConvTranspose2d
    from p2pvg_amd.ops.fused_norm import FusedSequential

    torch.manual_seed(5)
    ref = _bf16_exact_(nn.Sequential(
        nn.Conv2d(128, 64, 3, 1, 1), nn.BatchNorm2d(64), nn.LeakyReLU(0.2),
        nn.ConvTranspose2d(64, 3, 3, 1, 1), nn.Sigmoid(),
    ).cuda())
    hip = FusedSequential(vgg_layer(128, 64, pad_out=True),
                          ConvTranspose2d(64, 3, 3, 1, 1), nn.Sigmoid()).cuda()
    _copy_layer(hip[0].main[0], hip[0].main[1], ref[0], ref[1])
    with torch.no_grad():
        hip[1].weight.copy_(ref[3].weight)
        hip[1].bias.copy_(ref[3].bias)

    x = torch.randn(2, 128, 16, 16, device="cuda").bfloat16().float()
    y_ref = ref(x)
    g = torch.randn_like(y_ref).bfloat16().float()
    y_ref.backward(g)

    y = hip(x.bfloat16().contiguous(memory_format=CL))
    y.backward(g.bfloat16().contiguous(memory_format=CL))
    _grad_close("last convT dw", ref[3].weight.grad, hip[1].weight.grad)
