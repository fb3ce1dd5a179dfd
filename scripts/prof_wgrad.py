#!/usr/bin/env python
"""A/B the single-pass all-taps 3x3 wgrad against the per-tap kernel.

Run on a GPU box: python scripts/prof_wgrad.py [batch]
For every vgg k3 wgrad shape (training form: X zero-ringed with pad=0, Y with
a ring of 1; the decoder's concat layers as dual-X pairs) prints the per-tap
pair time (taps=0), the all-taps pair time (taps=1, where eligible), their
ratio, the TF and staged-bytes rate of the faster one's column and the max
error of both against fp32 torch.nn.grad.conv2d_weight. "Pair" is kernel plus
combine: the whole conv2d_nhwc_wgrad call.
"""
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from p2pvg_amd.ops import _hip_ext_loader  # noqa: E402

CL = torch.channels_last
ext = _hip_ext_loader.load()
N = int(sys.argv[1]) if len(sys.argv) > 1 else 128

# tag, A (X channels; a tuple is a dual-X pair), spatial, B (Y channels)
SHAPES = [
    ("vgg c1.1", 64, 64, 64),
    ("vgg c2.0", 64, 32, 128),
    ("vgg c2.1", 128, 32, 128),
    ("vgg c3.0", 128, 16, 256),
    ("vgg c3.x", 256, 16, 256),
    ("vgg c4.0", 256, 8, 512),
    ("vgg c4.x", 512, 8, 512),
    ("vgg d2cat", (512, 512), 8, 512),
    ("vgg d3cat", (256, 256), 16, 256),
    ("vgg d4cat", (128, 128), 32, 128),
    ("vgg d5cat", (64, 64), 64, 64),
    ("vgg upc4.1", 128, 32, 64),
]


def timeit(f, n=20):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1000


def reference(x, g, b, a):
    """fp32 conv2d_weight, in batch pieces summed in fp64."""
    ref = torch.zeros(b, a, 3, 3, device="cuda", dtype=torch.float64)
    for i in range(0, x.shape[0], 64):
        ref += torch.nn.grad.conv2d_weight(
            x[i:i + 64].float(), (b, a, 3, 3), g[i:i + 64].float(),
            stride=1, padding=1).double()
    return ref.float()


def tile(ch):
    return 128 if ch % 128 == 0 else 64


print(f"batch {N}")
print(f"{'shape':<10} {'B':>4} {'A':>9} {'hw':>3} {'per-tap us':>10} "
      f"{'taps us':>8} {'ratio':>6} {'TF':>5} {'staged TB/s':>11} "
      f"{'err old':>9} {'err new':>9} {'scale':>8}")
for tag, a_spec, h, b in SHAPES:
    parts = a_spec if isinstance(a_spec, tuple) else (a_spec,)
    a = sum(parts)
    torch.manual_seed(0)
    x = torch.randn(N, a, h, h, device="cuda").bfloat16()
    g = torch.randn(N, b, h, h, device="cuda").bfloat16()
    ref = reference(x, g, b, a)
    scale = ref.abs().max().item()
    xs = [F.pad(p, (1,) * 4).contiguous(memory_format=CL)
          for p in torch.split(x, list(parts), dim=1)]
    x2 = xs[1] if len(xs) > 1 else None
    gp = F.pad(g, (1,) * 4).contiguous(memory_format=CL)
    del x, g

    def call(taps):
        return ext.conv2d_nhwc_wgrad(gp, xs[0], 3, 3, 1, 0, 0, None, 1, x2,
                                     -1, taps)

    def err(ws):
        return (ws.permute(0, 3, 1, 2) - ref).abs().max().item()

    e_old = err(call(0))
    t_old = timeit(lambda: call(0))
    try:
        e_new = err(call(1))
    except RuntimeError:
        e_new = None
    flops = 2.0 * N * h * h * b * a * 9
    ybytes = gp.numel() * 2
    xbytes = sum(t.numel() for t in xs) * 2
    if e_new is None:
        staged = 9 * (a // tile(a) * ybytes + b // tile(b) * xbytes)
        print(f"{tag:<10} {b:>4} {str(a_spec):>9} {h:>3} {t_old:>10.1f} "
              f"{'-':>8} {'-':>6} {flops / t_old / 1e6:>5.0f} "
              f"{staged / t_old / 1e6:>11.2f} {e_old:>9.2e} {'-':>9} "
              f"{scale:>8.1f}")
        continue
    t_new = timeit(lambda: call(1))
    # every Y pixel once per a-tile, every X row as three shifted images
    # once per b-tile
    staged = a // 64 * ybytes + b // 64 * 3 * xbytes
    print(f"{tag:<10} {b:>4} {str(a_spec):>9} {h:>3} {t_old:>10.1f} "
          f"{t_new:>8.1f} {t_old / t_new:>6.2f} {flops / t_new / 1e6:>5.0f} "
          f"{staged / t_new / 1e6:>11.2f} {e_old:>9.2e} {e_new:>9.2e} "
          f"{scale:>8.1f}")
