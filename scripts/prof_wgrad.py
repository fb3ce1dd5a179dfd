#!/usr/bin/env python
"""A/B the single-pass all-taps 3x3 wgrad kernels against the per-tap kernel.

Run on a GPU box: python scripts/prof_wgrad.py [batch] [w64|w16]
For every vgg k3 wgrad shape (training form: X zero-ringed with pad=0, Y with
a ring of 1; the decoder's concat layers as dual-X pairs) prints the pair time
of the per-tap path (taps=0), of the strip all-taps kernel (taps=1) and of the
row-order all-taps kernel with 64x64 and with 32x64 tiles (taps=3, taps=4;
64-wide maps only) and of the narrow all-taps kernel with 64x64 and with
128x64 tiles (taps=6, taps=7; 16-wide maps only), each where eligible. "Pair" is kernel plus combine: the
whole conv2d_nhwc_wgrad call, with the per-tap path's slabs in every column.
Each time is the mean of REPS timings of 20 calls, followed by their max-min
spread; "ratio" is per-tap over the fastest all-taps column, TF and staged
TB/s are that column's. "bits" tells whether that column's result is bitwise
the per-tap one. The argument w64 keeps only the 64-wide shapes, the two of
the 64-pixel model and those the 128-pixel model adds. The argument w16
keeps the 16-wide shapes of the 64-pixel model, adds its 8-wide ones (per-tap
only: what the other half of the <128,128> per-tap row costs) and the 16-wide
ones of the 128-pixel model at a quarter of the batch.
"""
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from p2pvg_amd.ops import _hip_ext_loader  # noqa: E402

CL = torch.channels_last
ext = _hip_ext_loader.load()
ARGS = sys.argv[1:]
W64 = "w64" in ARGS
W16 = "w16" in ARGS
ARGS = [a for a in ARGS if a not in ("w64", "w16")]
N = int(ARGS[0]) if ARGS else 128
REPS = 3

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
# the 64-wide classes the 128-pixel model reaches one level down
SHAPES_128 = [
    ("v128 c2.0", 64, 64, 128),
    ("v128 c2.1", 128, 64, 128),
    ("v128 d4cat", (128, 128), 64, 128),
    ("v128 upc4.1", 128, 64, 64),
]
# the 16- and 8-wide layers of the 64-pixel model that SHAPES lacks, and the
# 16-wide classes of the 128-pixel model (fifth field: batch divisor)
SHAPES_16 = [
    ("vgg c3.0", 128, 16, 256),
    ("vgg c3.x", 256, 16, 256),
    ("vgg d3cat", (256, 256), 16, 256),
    ("vgg upc3.2", 256, 16, 128),
    ("vgg c4.0", 256, 8, 512),
    ("vgg c4.x", 512, 8, 512),
    ("vgg d2cat", (512, 512), 8, 512),
    ("vgg upc2.2", 512, 8, 256),
    ("v128 c4.0", 256, 16, 512, 4),
    ("v128 c4.x", 512, 16, 512, 4),
    ("v128 d3cat", (512, 512), 16, 512, 4),
    ("v128 upc3.2", 512, 16, 256, 4),
]
if W64:
    SHAPES = [s for s in SHAPES if s[2] == 64] + SHAPES_128
if W16:
    SHAPES = SHAPES_16


def timeit(f, n=20):
    """(mean, max - min) in us over REPS timings of n calls."""
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            f()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) / n * 1000)
    return sum(ts) / len(ts), max(ts) - min(ts)


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


def cell(t):
    return f"{t[0]:>7.1f} ±{t[1]:<5.1f}" if t else f"{'-':>7} {'':<6}"


MODES = [(1, "strip"), (3, "rows64"), (4, "rows32"), (6, "nar64"),
         (7, "nar128")]
print(f"batch {N}")
print(f"{'shape':<11} {'n':>4} {'B':>4} {'A':>10} {'hw':>3} {'per-tap us':>14} "
      + " ".join(f"{name + ' us':>14}" for _, name in MODES)
      + f" {'best':>6} {'ratio':>6} {'TF':>5} {'staged TB/s':>11} {'bits':>5} "
      f"{'err old':>9} {'err new':>9} {'scale':>8}")
for tag, a_spec, h, b, *div in SHAPES:
    n = N // div[0] if div else N
    parts = a_spec if isinstance(a_spec, tuple) else (a_spec,)
    a = sum(parts)
    torch.manual_seed(0)
    x = torch.randn(n, a, h, h, device="cuda").bfloat16()
    g = torch.randn(n, b, h, h, device="cuda").bfloat16()
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

    w_old = call(0)
    e_old = err(w_old)
    t_old = timeit(lambda: call(0))
    times, outs = {}, {}
    for taps, name in MODES:
        try:
            outs[name] = call(taps)
        except RuntimeError:
            times[name] = None
            continue
        times[name] = timeit(lambda: call(taps))
    flops = 2.0 * n * h * h * b * a * 9
    ybytes = gp.numel() * 2
    xbytes = sum(t.numel() for t in xs) * 2
    head = (f"{tag:<11} {n:>4} {b:>4} {str(a_spec):>10} {h:>3} {cell(t_old)} "
            + " ".join(cell(times[name]) for _, name in MODES))
    if not outs:
        staged = 9 * (a // tile(a) * ybytes + b // tile(b) * xbytes)
        print(f"{head} {'-':>6} {'-':>6} {flops / t_old[0] / 1e6:>5.0f} "
              f"{staged / t_old[0] / 1e6:>11.2f} {'-':>5} {e_old:>9.2e} "
              f"{'-':>9} {scale:>8.1f}")
        continue
    best = min(outs, key=lambda k: times[k][0])
    t_new = times[best][0]
    # every Y pixel once per a-tile, every X row as three shifted images
    # once per b-tile (32-row b-tiles for rows32, 128-row ones for nar128)
    btile = {"rows32": 32, "nar128": 128}.get(best, 64)
    staged = a // 64 * ybytes + b // btile * 3 * xbytes
    same = "same" if torch.equal(outs[best], w_old) else "differ"
    print(f"{head} {best:>6} {t_old[0] / t_new:>6.2f} "
          f"{flops / t_new / 1e6:>5.0f} {staged / t_new / 1e6:>11.2f} "
          f"{same:>5} {e_old:>9.2e} {err(outs[best]):>9.2e} {scale:>8.1f}")
