"""Frame-bank gather kernel (csrc/clip_gather.hip) against the CPU op.

The CPU implementation of ops.clip_gather, bank[idx, :L].float().div(255) in
the generator's layout, is the oracle and every comparison is torch.equal: the
kernel has to produce the correctly rounded fp32 quotient of every byte value.

No test feeds the kernel an out-of-range index: the validation test asserts
that such a call raises before the extension is reached, and the 64-bit offset
case puts a decoy clip at the truncated offset, so a kernel that drops the
high bits reads wrong data, not foreign memory.
"""
import dataclasses

import numpy as np
import pytest
import torch
from PIL import Image

from p2pvg_amd import data as data_utils
from p2pvg_amd import ops
from p2pvg_amd.ops import clip_gather

pytestmark = pytest.mark.gpu


def _i32(x):
    return torch.tensor(x, dtype=torch.int32)


def _rand_bank(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


def test_every_byte_value():
    v = (np.arange(2 * 3 * 4 * 8 * 3) * 37 + 11) % 256
    assert len(set(v.tolist())) == 256
    bank = torch.from_numpy(v.astype(np.uint8).reshape(2, 3, 4, 8, 3))
    idx = _i32([1, 0, 1])
    want = clip_gather(bank, idx, 3)
    numpy_q = torch.from_numpy(bank.numpy().astype(np.float32) / 255.0)
    assert torch.equal(want, numpy_q[[1, 0, 1]].permute(1, 0, 4, 2, 3))
    got = clip_gather(bank.cuda(), idx, 3)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (3, 3, 3, 4, 8)
    assert torch.equal(got.cpu(), want)


def test_torch_backend_on_device_is_exact(monkeypatch):
    """P2PVG_KERNELS=torch on the GPU is the same oracle as the CPU op."""
    bank = _rand_bank((3, 4, 8, 8, 3), 2)
    bank.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    idx = _i32([2, 0, 2, 1])
    monkeypatch.setenv("P2PVG_KERNELS", "torch")
    got = clip_gather(bank.cuda(), idx, 3)
    monkeypatch.delenv("P2PVG_KERNELS")
    assert got.is_cuda and torch.equal(got.cpu(), clip_gather(bank, idx, 3))
    assert got.stride() == clip_gather(bank.cuda(), idx, 3).stride()


T = 4
N = 3
FRAMES = {
    "64x64x3 whole blocks": (64, 64, 3),      # 768 units of 16 bytes
    "20x12x3 partial block": (20, 12, 3),     # 45 units
    "8x8x1 four units": (8, 8, 1),            # 4 units
    "128x128x3": (128, 128, 3),
}


@pytest.fixture(scope="module")
def banks():
    out = {}
    for seed, (name, hwc) in enumerate(FRAMES.items()):
        cpu = _rand_bank((N, T) + hwc, 100 + seed)
        out[name] = (cpu, cpu.cuda())
    return out


@pytest.mark.parametrize("L", [1, T - 1, T])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_sizes(banks, name, B, L):
    cpu, gpu = banks[name]
    H, W, C = FRAMES[name]
    # the last clip, and one clip twice in a batch
    idx = _i32([N - 1, 0, N - 1, 1, 0][:B])
    want = clip_gather(cpu, idx, L)
    got = clip_gather(gpu, idx, L)
    assert got.shape == (L, B, C, H, W) and got.dtype == torch.float32
    assert got.stride() == want.stride() == (B * H * W * C, H * W * C, 1, W * C, C)
    assert torch.equal(got.cpu(), want)


def test_source_offset_beyond_32_bits():
    n, t, H, W, C = 174764, 2, 64, 64, 3
    clip = t * H * W * C
    assert n * clip > (n - 1) * clip >= 2 ** 32  # the last clip starts past 2^32
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 2 ** 30:
        pytest.skip("needs 6 GB of free device memory")
    low = ((n - 1) * clip) % 2 ** 32           # where a 32-bit offset lands
    assert low % 16 == 0 and low + clip < (n - 1) * clip
    real = _rand_bank((1, t, H, W, C), 31)
    decoy = _rand_bank((1, t, H, W, C), 32)
    bank = torch.empty(n, t, H, W, C, dtype=torch.uint8, device="cuda")
    bank.view(-1)[low:low + clip] = decoy.view(-1).cuda()
    bank[n - 1] = real[0].cuda()
    got = clip_gather(bank, _i32([n - 1]), t).cpu()
    assert torch.equal(got, clip_gather(real, _i32([0]), t))
    assert not torch.equal(got, clip_gather(decoy, _i32([0]), t))
    del bank
    torch.cuda.empty_cache()


def test_layout_stream_and_repeatability(banks):
    cpu, gpu = banks["64x64x3 whole blocks"]
    idx = _i32([2, 1, 1, 0, 2])
    L, B = 3, 5
    want = clip_gather(cpu, idx, L)
    # the strides of get_generator's CUDA branch for a (B, T, C, H, W) batch
    loader_batch = torch.zeros(B, L, 3, 64, 64, device="cuda")
    ref = loader_batch.permute(1, 0, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = clip_gather(gpu, idx, L)
        host = got.cpu()       # DtoH on s, ordered behind the kernel on s
    s.synchronize()
    assert torch.equal(host, want)
    assert got.shape == ref.shape and got.stride() == ref.stride()
    assert all(f.is_contiguous(memory_format=torch.channels_last) for f in got)
    again = clip_gather(gpu, idx, L)
    assert torch.equal(again, got) and again.data_ptr() != got.data_ptr()


class _RecordingExt:
    """Stands in for the extension and counts gather launches."""

    def __init__(self, real):
        self._real = real
        self.calls = 0

    def clip_gather(self, *a):
        self.calls += 1
        return self._real.clip_gather(*a)

    def __getattr__(self, name):
        return getattr(self._real, name)


def test_validation_raises_before_launch(monkeypatch):
    cpu = _rand_bank((3, 4, 4, 4, 3), 5)
    bank = cpu.cuda()
    idx = _i32([0, 2])
    wide = torch.zeros(3, 4, 4, 8, 3, dtype=torch.uint8, device="cuda")
    bad = {
        "idx==N": (bank, _i32([0, 3]), 4),
        "idx==-1": (bank, _i32([-1, 0]), 4),
        "int64 idx": (bank, idx.long(), 4),
        "device idx": (bank, idx.cuda(), 4),
        "L==0": (bank, idx, 0),
        "L==T+1": (bank, idx, 5),
        "non-contiguous bank": (wide[:, :, :, ::2], idx, 4),
        "float bank": (bank.float(), idx, 4),
        "H*W*C % 16 != 0": (torch.zeros(3, 4, 3, 3, 3, dtype=torch.uint8, device="cuda"), idx, 4),
        "unaligned bank": (torch.zeros(3 * 4 * 48 + 1, dtype=torch.uint8,
                                       device="cuda")[1:].view(3, 4, 4, 4, 3), idx, 4),
    }
    rec = _RecordingExt(ops._load_hip_ext())
    monkeypatch.setattr(ops, "_load_hip_ext", lambda: rec)
    for name, (b, i, L) in bad.items():
        with pytest.raises(ValueError):
            clip_gather(b, i, L)
        assert rec.calls == 0, f"{name}: reached the extension"
    got = clip_gather(bank, idx, 4)
    assert rec.calls == 1  # the probe does see a valid call's launch
    assert torch.equal(got.cpu(), clip_gather(cpu, idx, 4))


def _write_tree(root, split, clips, frames=6, size=64):
    rng = np.random.RandomState(7 + clips)
    for n in range(clips):
        d = root / "bair" / "processed_data" / split / "traj" / str(n)
        d.mkdir(parents=True)
        for i in range(frames):
            px = rng.randint(0, 256, (size, size, 3), dtype=np.uint8)
            Image.fromarray(px, "RGB").save(d / f"{i}.png")


def test_device_generator_end_to_end(tiny_cfg, tmp_path):
    from p2pvg_amd.models import P2PModel

    _write_tree(tmp_path, "train", 4)
    _write_tree(tmp_path, "test", 3)
    cfg = dataclasses.replace(tiny_cfg, dataset="bair", channels=3,
                              max_seq_len=6, device="cuda", dtype="bf16",
                              skip_prob=0.0, frame_cache="device",
                              data_root=str(tmp_path))
    train, test = data_utils.load_dataset(cfg)
    B = cfg.batch_size
    torch.manual_seed(3)
    gen = data_utils.get_data_generator(train, train=True, opt=cfg)
    got = [next(gen) for _ in range(2)]
    # replay the generator's stream through the dataset
    train.seed_is_set = True
    np.random.seed(3)
    for x in got:
        clips = torch.stack([train[i] for i in range(B)])       # (B, T, C, H, W)
        seq_len = int(np.random.randint(6 - 2, 6 + 1))
        want = (clips.cuda().permute(1, 0, 3, 4, 2).contiguous()
                .permute(0, 1, 4, 2, 3))[:seq_len]
        assert x.is_cuda and x.shape == want.shape and x.stride() == want.stride()
        assert torch.equal(x, want)
    x = next(data_utils.get_data_generator(test, train=False, opt=cfg))
    assert x.is_cuda and x.shape[1:] == (B, 3, 64, 64) and 4 <= len(x) <= 6

    torch.manual_seed(0)
    model = P2PModel(cfg).to("cuda").to(memory_format=torch.channels_last)
    x = got[0]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        losses = model(x, 0, len(x) - 1)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v) for v in losses), losses
