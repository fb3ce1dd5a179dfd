"""GPU tests: the fused BN statistics tail (one launch per BN pass) against an
emulation of its fixed association and against the split launch sequence.

The sums are defined by their association: 64-row chunks summed serially from
zero in row order, again while more than 64 rows remain, then one serial walk.
The emulation below does exactly that with torch fp32 elementwise adds (exact
IEEE, so independent of the kernels); everything is compared with torch.equal.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
DEV = "cuda"


@pytest.fixture(scope="module")
def ext():
    from p2pvg_amd.ops import _hip_ext_loader

    e = _hip_ext_loader.load()
    was = e.bn_tail_fused()
    e.set_bn_tail_fused(True)
    yield e
    e.set_bn_tail_fused(was)


class split_tail:
    """Run the enclosed calls through the split fold/finalize/combine path."""

    def __init__(self, ext):
        self.ext = ext

    def __enter__(self):
        self.ext.set_bn_tail_fused(False)

    def __exit__(self, *exc):
        self.ext.set_bn_tail_fused(True)


def emulate(rows):
    """rows (R, ...) fp32 -> (...): the fixed association, one fp32 add per
    step; the chunks of a level advance side by side, each serial."""
    def walk(block):  # (n, rows_in_chunk, ...) -> (n, ...), serial from zero
        t = torch.zeros_like(block[:, 0])
        for j in range(block.shape[1]):
            t = t + block[:, j]
        return t

    while rows.shape[0] > 64:
        R = rows.shape[0]
        full = R // 64
        parts = []
        if full:
            parts.append(walk(rows[: full * 64].reshape(full, 64, *rows.shape[1:])))
        if R % 64:
            parts.append(walk(rows[full * 64:].unsqueeze(0)))
        rows = torch.cat(parts, 0)
    return walk(rows.unsqueeze(0))[0]


def mixed(gen, *shape):
    """Values of mixed sign and magnitude (1e-3 .. 1e3): a different order of
    the adds rounds differently."""
    v = torch.randn(*shape, generator=gen, device=DEV)
    e = torch.randint(-3, 4, shape, generator=gen, device=DEV)
    return v * (10.0 ** e.float())


def make_stats(gen, R, C):
    s = mixed(gen, R, 2, C)
    s[:, 1] = s[:, 1].abs()  # sums of squares
    return s.contiguous()


def fwd(ext, stats, C, gamma, beta, rm=None, rv=None):
    x = torch.zeros(1, C, 2, 2, device=DEV, dtype=torch.bfloat16).contiguous(
        memory_format=CL)
    return ext.bn_act_fwd_train(x, stats, gamma, beta, rm, rv, 0.1, 1e-5, 1, 0)


FWD_SHAPES = [(1, 8), (64, 8), (65, 8), (4096, 64), (4097, 16), (300, 512)]
COUNT = 4.0  # x is (1, C, 2, 2)


@pytest.mark.parametrize("R,C", FWD_SHAPES)
def test_forward_sums_match_emulation(ext, R, C):
    gen = torch.Generator(device=DEV).manual_seed(R * 1000 + C)
    stats = make_stats(gen, R, C)
    gamma = torch.randn(C, generator=gen, device=DEV)
    beta = torch.randn(C, generator=gen, device=DEV)
    _, mean, _, _ = fwd(ext, stats, C, gamma, beta)
    want = emulate(stats)  # (2, C)
    assert torch.equal(mean, want[0] / COUNT)


@pytest.mark.parametrize("R,C", FWD_SHAPES)
def test_forward_finalize_equals_split(ext, R, C):
    gen = torch.Generator(device=DEV).manual_seed(R * 1000 + C + 1)
    stats = make_stats(gen, R, C)
    gamma = torch.randn(C, generator=gen, device=DEV)
    beta = torch.randn(C, generator=gen, device=DEV)
    rm0 = torch.randn(C, generator=gen, device=DEV)
    rv0 = torch.rand(C, generator=gen, device=DEV) + 0.5
    rm_f, rv_f = rm0.clone(), rv0.clone()
    out_f = fwd(ext, stats, C, gamma, beta, rm_f, rv_f)
    rm_s, rv_s = rm0.clone(), rv0.clone()
    with split_tail(ext):
        out_s = fwd(ext, stats, C, gamma, beta, rm_s, rv_s)
    for name, a, b in zip(("y", "mean", "invstd", "scale"), out_f, out_s):
        assert torch.equal(a, b), name
    assert torch.equal(rm_f, rm_s) and torch.equal(rv_f, rv_s)
    assert not torch.equal(rm_f, rm0)


def bwd_inputs(gen, N, C, Hp, Wp):
    x = torch.randn(N, C, Hp, Wp, generator=gen, device=DEV).bfloat16().contiguous(
        memory_format=CL)
    dy = mixed(gen, N, C, Hp, Wp).bfloat16().contiguous(memory_format=CL)
    mean = torch.randn(C, generator=gen, device=DEV) * 0.1
    invstd = torch.rand(C, generator=gen, device=DEV) + 0.5
    gamma = torch.randn(C, generator=gen, device=DEV)
    beta = torch.randn(C, generator=gen, device=DEV)
    scale = gamma * invstd
    return x, dy, mean, invstd, gamma, beta, scale


@pytest.mark.parametrize("N,C,Hp,Wp", [(130, 8, 3, 3), (4, 512, 34, 34)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_backward_equals_split(ext, N, C, Hp, Wp, accumulate):
    gen = torch.Generator(device=DEV).manual_seed(N * 100 + C)
    args = bwd_inputs(gen, N, C, Hp, Wp)
    acc0 = [mixed(gen, C), mixed(gen, C)] if accumulate else [None, None]

    def run():
        acc = [a.clone() if a is not None else None for a in acc0]
        return ext.bn_act_bwd(*args, 1, acc[0], acc[1], 1)

    got = run()
    with split_tail(ext):
        want = run()
    for name, a, b in zip(("dx", "dgamma", "dbeta"), got, want):
        assert torch.equal(a, b), name
    if accumulate:
        assert not torch.equal(got[1], acc0[0])


@pytest.mark.parametrize("accumulate", [False, True])
def test_channel_sum_equals_split(ext, accumulate):
    gen = torch.Generator(device=DEV).manual_seed(7)
    # 65536 vectors of 8 -> 256 partial rows -> four chunks
    x = mixed(gen, 8, 64, 32, 32).bfloat16().contiguous(memory_format=CL)
    acc0 = mixed(gen, 64) if accumulate else None

    def run():
        return ext.channel_sum_nhwc(x, acc0.clone() if accumulate else None)

    got = run()
    with split_tail(ext):
        want = run()
    assert torch.equal(got, want)
    assert torch.isfinite(got).all()


def test_rearming_and_no_stale_rows(ext):
    """50 calls in a row on one stream over ONE rows buffer, rewritten before
    each: counters re-arm every call and no call sees the previous rows."""
    R, C, calls = 300, 8, 50
    gen = torch.Generator(device=DEV).manual_seed(50)
    inputs = mixed(gen, calls, R, 2, C)
    inputs[:, :, 1] = inputs[:, :, 1].abs()
    want = emulate(inputs.transpose(0, 1).contiguous())  # (calls, 2, C)
    gamma = torch.ones(C, device=DEV)
    beta = torch.zeros(C, device=DEV)
    stats = torch.empty(R, 2, C, device=DEV)
    means = []
    for i in range(calls):
        stats.copy_(inputs[i])
        means.append(fwd(ext, stats, C, gamma, beta)[1])
    got = torch.stack(means)
    assert torch.equal(got, want[:, 0] / COUNT)


def test_graph_replay(ext):
    """One forward tail and one backward captured in a graph; three replays
    with the input buffers rewritten equal the eager results."""
    R, C = 4097, 16
    gen = torch.Generator(device=DEV).manual_seed(99)
    gamma = torch.randn(C, generator=gen, device=DEV)
    beta = torch.randn(C, generator=gen, device=DEV)
    stats_in = [make_stats(gen, R, C) for _ in range(3)]
    bwd_in = [bwd_inputs(gen, 130, 8, 3, 3) for _ in range(3)]
    eager = []
    for s, b in zip(stats_in, bwd_in):
        f = fwd(ext, s, C, gamma, beta)
        g = ext.bn_act_bwd(*b, 1, None, None, 1)
        eager.append([t.clone() for t in (*f, *g)])
        assert torch.equal(f[1], emulate(s)[0] / COUNT)

    stats = stats_in[0].clone()
    bargs = [t.clone() for t in bwd_in[0]]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        f = fwd(ext, stats, C, gamma, beta)
        g = ext.bn_act_bwd(*bargs, 1, None, None, 1)
    outs = (*f, *g)
    for s, b, want in zip(stats_in, bwd_in, eager):
        stats.copy_(s)
        for dst, src in zip(bargs, b):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for a, w in zip(outs, want):
            assert torch.equal(a, w)
