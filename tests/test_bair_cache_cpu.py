"""Device-resident BAIR frame cache, host side (CPU): the frame pack and its
disk cache, the batch planner, the validation and the torch path of
ops.clip_gather (the oracle of tests/test_bair_cache_gpu.py), the generator,
the config flag and the train/evaluate CLIs. Every comparison is torch.equal."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

from p2pvg_amd import data as data_utils
from p2pvg_amd.core import Config
from p2pvg_amd.data import bair as bair_mod
from p2pvg_amd.data.bair import BairRobotPush
from p2pvg_amd.ops import clip_gather

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_tree(root, split="train", clips=5, frames=6, size=16, seed=0):
    """processed_data/<split>/<d1>/<d2>/<i>.png; the second file of clip 0 is
    grayscale and the third RGBA, every other one RGB."""
    rng = np.random.RandomState(seed)
    base = root / "bair" / "processed_data" / split
    n = 0
    for d1 in ("a", "b"):
        for d2 in range((clips + 1) // 2 if d1 == "a" else clips // 2):
            d = base / d1 / str(d2)
            d.mkdir(parents=True)
            for i in range(frames):
                if n == 0 and i == 1:
                    im = Image.fromarray(rng.randint(0, 256, (size, size), dtype=np.uint8), "L")
                elif n == 0 and i == 2:
                    im = Image.fromarray(rng.randint(0, 256, (size, size, 4), dtype=np.uint8), "RGBA")
                else:
                    im = Image.fromarray(rng.randint(0, 256, (size, size, 3), dtype=np.uint8), "RGB")
                im.save(d / f"{i}.png")
            n += 1
    return base


def make_ds(root, train=True, max_seq_len=6, size=16, delta_len=1):
    return BairRobotPush(str(root), train=train, max_seq_len=max_seq_len,
                         delta_len=delta_len, image_size=size)


def as_bank(pack):
    return torch.from_numpy(np.array(pack))


# -- 1. frame pack -----------------------------------------------------------

def test_pack_bytes_and_cache(tmp_path, monkeypatch):
    write_tree(tmp_path)
    ds = make_ds(tmp_path)
    pack = ds.load_pack()
    assert pack.dtype == np.uint8 and pack.shape == (5, 6, 16, 16, 3)
    for n, d in enumerate(ds.dirs):
        for i in range(6):
            with Image.open(os.path.join(d, f"{i}.png")) as im:
                assert np.array_equal(pack[n, i], np.asarray(im.convert("RGB")))
    want = torch.stack([torch.stack([ds._load_png(os.path.join(d, f"{i}.png"))
                                     for i in range(6)]) for d in ds.dirs])
    got = (as_bank(pack).float() / 255).permute(0, 1, 4, 2, 3)
    assert torch.equal(got, want)

    npy, sidecar = ds.pack_paths()
    assert os.path.dirname(npy) == os.path.dirname(ds.data_dir)
    assert os.path.isfile(npy) and os.path.isfile(sidecar)
    with open(sidecar) as f:
        meta = json.load(f)
    assert meta["image_size"] == 16 and meta["T"] == 6
    assert meta["dirs"] == [os.path.relpath(d, ds.data_dir) for d in ds.dirs]

    # a second call reads the file: the decoder is never entered
    def no_decode(task):
        raise AssertionError("decoded again instead of reading the pack")

    monkeypatch.setattr(bair_mod, "_decode_clip", no_decode)
    again = make_ds(tmp_path).load_pack()
    assert isinstance(again, np.memmap) and np.array_equal(again, pack)
    # a shorter max_seq_len reads the same pack (T is the clip's, not the run's)
    assert make_ds(tmp_path, max_seq_len=4).load_pack().shape == (5, 6, 16, 16, 3)


def test_pack_rebuilds_when_a_clip_is_added(tmp_path):
    base = write_tree(tmp_path)
    first = np.array(make_ds(tmp_path).load_pack())
    d = base / "b" / "9"
    d.mkdir()
    for i in range(6):
        Image.fromarray(np.full((16, 16, 3), 10 * i + 7, dtype=np.uint8)).save(d / f"{i}.png")
    ds = make_ds(tmp_path)
    pack = ds.load_pack()
    assert pack.shape[0] == 6 == len(ds.dirs)
    assert np.array_equal(pack[:5], first)
    assert all(int(pack[5, i].min()) == int(pack[5, i].max()) == 10 * i + 7 for i in range(6))
    # another image_size is another pack file
    assert make_ds(tmp_path, size=16).pack_paths() != make_ds(tmp_path, size=32).pack_paths()


def test_pack_unwritable_location_stays_in_memory(tmp_path, monkeypatch):
    base = write_tree(tmp_path)
    ds = make_ds(tmp_path)

    def refuse(path, shape):
        raise PermissionError(13, "read-only location", path)

    monkeypatch.setattr(bair_mod, "_open_pack_for_write", refuse)
    monkeypatch.setattr(bair_mod, "_warned_unwritable", False)
    with pytest.warns(UserWarning, match="keeping it in memory"):
        pack = ds.load_pack()
    assert not isinstance(pack, np.memmap) and pack.shape == (5, 6, 16, 16, 3)
    with warnings.catch_warnings():  # warned once
        warnings.simplefilter("error")
        assert np.array_equal(ds.load_pack(), pack)
    assert sorted(os.listdir(base.parent)) == ["train"]
    monkeypatch.undo()
    assert np.array_equal(ds.load_pack(), pack)

    if os.geteuid() != 0:  # a real read-only directory (root writes anywhere)
        other = tmp_path / "ro"
        base = write_tree(other)
        os.chmod(base.parent, 0o555)
        try:
            bair_mod._warned_unwritable = False
            with pytest.warns(UserWarning):
                pack = make_ds(other).load_pack()
            assert pack.shape == (5, 6, 16, 16, 3)
            assert sorted(os.listdir(base.parent)) == ["train"]
        finally:
            os.chmod(base.parent, 0o755)


# -- 2. errors ---------------------------------------------------------------

def _no_pack_files(base):
    return sorted(os.listdir(base.parent)) == [base.name]


def test_pack_errors_leave_no_file(tmp_path):
    base = write_tree(tmp_path / "size")
    bad = base / "b" / "0" / "3.png"
    Image.fromarray(np.zeros((16, 20, 3), dtype=np.uint8)).save(bad)
    with pytest.raises(ValueError, match="3.png"):
        make_ds(tmp_path / "size").load_pack()
    assert _no_pack_files(base)

    base = write_tree(tmp_path / "short")
    os.unlink(base / "b" / "1" / "5.png")
    with pytest.raises(ValueError, match=os.path.join("b", "1")):
        make_ds(tmp_path / "short").load_pack()
    assert _no_pack_files(base)

    base = write_tree(tmp_path / "long")
    with pytest.raises(ValueError, match="max_seq_len"):
        make_ds(tmp_path / "long", max_seq_len=7).load_pack()
    assert _no_pack_files(base)

    ds = make_ds(tmp_path / "absent")
    assert ds.synthetic
    with pytest.raises(ValueError, match="absent"):
        ds.load_pack()
    with pytest.raises(ValueError):
        ds.plan_batch(2, np.random.RandomState(0))
    assert not (tmp_path / "absent").exists()


def test_pack_worker_pool_matches_single_process(tmp_path):
    write_tree(tmp_path / "one")
    write_tree(tmp_path / "two")
    a = make_ds(tmp_path / "one").load_pack()
    b = make_ds(tmp_path / "two").load_pack(workers=2)
    assert np.array_equal(a, b)


# -- 3. planner parity -------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1234])
def test_plan_matches_train_dataset_stream(tmp_path, seed):
    write_tree(tmp_path)
    ds = make_ds(tmp_path)
    bank = as_bank(ds.load_pack())
    B, T = 7, 6

    ds.seed_is_set = True
    np.random.seed(seed)
    want = torch.stack([ds[i] for i in range(B)]).permute(1, 0, 2, 3, 4)
    next_global = np.random.randint(1 << 30)

    rng = np.random.RandomState(seed)
    plan = ds.plan_batch(B, rng)
    assert plan.dtype == torch.int32 and plan.shape == (B,) and plan.device.type == "cpu"
    assert torch.equal(clip_gather(bank, plan, T), want)
    assert rng.randint(1 << 30) == next_global


def test_plan_matches_ordered_test_scan(tmp_path):
    write_tree(tmp_path, split="test", clips=3)
    ds, ref = make_ds(tmp_path, train=False), make_ds(tmp_path, train=False)
    bank = as_bank(ds.load_pack())
    rng = np.random.RandomState(3)
    state = rng.get_state()[1].copy()
    for B in (7, 2):  # 7 > 3 clips: the counter wraps; the second batch goes on
        want = torch.stack([ref[i] for i in range(B)]).permute(1, 0, 2, 3, 4)
        plan = ds.plan_batch(B, rng)
        assert torch.equal(clip_gather(bank, plan, 6), want)
        assert ds.d == ref.d
    assert plan.tolist() == [1, 2] and ds.d == 0
    assert np.array_equal(rng.get_state()[1], state), "the ordered scan draws nothing"


# -- 4. clip_gather on the torch path ----------------------------------------

def every_byte_bank():
    """(2, 3, 4, 8, 3) with all 256 byte values, none in index order."""
    v = (np.arange(2 * 3 * 4 * 8 * 3) * 37 + 11) % 256
    assert len(set(v.tolist())) == 256
    return torch.from_numpy(v.astype(np.uint8).reshape(2, 3, 4, 8, 3))


def test_gather_every_byte_value_is_the_numpy_quotient():
    bank = every_byte_bank()
    out = clip_gather(bank, torch.tensor([1, 0, 1], dtype=torch.int32), 3)
    assert out.shape == (3, 3, 3, 4, 8) and out.dtype == torch.float32
    want = (bank.numpy().astype(np.float32) / 255.0)[[1, 0, 1]]  # (B, L, H, W, C)
    want = torch.from_numpy(want).permute(1, 0, 4, 2, 3)
    assert torch.equal(out, want)
    recip = bank.float() * (1.0 / 255.0)
    assert not torch.equal(recip, bank.float() / 255.0), "a reciprocal multiply differs"


def test_gather_layout_short_length_and_repeats():
    g = torch.Generator().manual_seed(0)
    bank = torch.randint(0, 256, (4, 5, 4, 4, 3), dtype=torch.uint8, generator=g)
    idx = torch.tensor([3, 3, 0, 2, 1, 0], dtype=torch.int32)
    for L in (1, 4, 5):
        out = clip_gather(bank, idx, L)
        assert out.shape == (L, 6, 3, 4, 4)
        assert out.permute(0, 1, 3, 4, 2).is_contiguous()
        assert all(out[l].is_contiguous(memory_format=torch.channels_last) for l in range(L))
        for b, n in enumerate(idx.tolist()):
            assert torch.equal(out[:, b], (bank[n, :L].float() / 255).permute(0, 3, 1, 2))
    rev = clip_gather(bank, idx.flip(0).contiguous(), 5)
    assert torch.equal(rev, clip_gather(bank, idx, 5).flip(1))
    assert clip_gather(bank, torch.empty(0, dtype=torch.int32), 2).shape == (2, 0, 3, 4, 4)


def bad_gather_args():
    bank = torch.zeros(3, 4, 4, 4, 3, dtype=torch.uint8)
    idx = torch.tensor([0, 2], dtype=torch.int32)
    wide = torch.zeros(3, 4, 4, 8, 3, dtype=torch.uint8)
    return {
        "idx==N": (bank, torch.tensor([0, 3], dtype=torch.int32), 4),
        "idx==-1": (bank, torch.tensor([-1, 0], dtype=torch.int32), 4),
        "int64 idx": (bank, idx.long(), 4),
        "device idx": (bank, idx.to("meta"), 4),
        "2-d idx": (bank, idx.view(1, 2), 4),
        "L==0": (bank, idx, 0),
        "L==T+1": (bank, idx, 5),
        "float L": (bank, idx, 2.0),
        "non-contiguous bank": (wide[:, :, :, ::2], idx, 4),
        "float bank": (bank.float(), idx, 4),
        "4-d bank": (bank[0], idx, 4),
        "H*W*C % 16 != 0": (torch.zeros(3, 4, 3, 3, 3, dtype=torch.uint8), idx, 4),
        "numpy bank": (bank.numpy(), idx, 4),
    }


@pytest.mark.parametrize("name", list(bad_gather_args()))
def test_gather_validation_raises(name):
    bank, idx, L = bad_gather_args()[name]
    with pytest.raises(ValueError):
        clip_gather(bank, idx, L)


# -- 5. generator, config, CLIs ----------------------------------------------

def _gen_cfg(root, **kw):
    base = dict(dataset="bair", channels=3, image_width=16, batch_size=3,
                max_seq_len=6, delta_len=1, data_root=str(root), device="cpu",
                num_workers=0, frame_cache="device")
    base.update(kw)
    return Config(**base)


def test_generator_output_and_seeding(tmp_path):
    write_tree(tmp_path)
    write_tree(tmp_path, split="test", clips=3)
    cfg = _gen_cfg(tmp_path)
    train, test = data_utils.load_dataset(cfg)

    def batches(data, train_flag, rank=0, n=12, **kw):
        torch.manual_seed(5)
        g = data_utils.get_data_generator(data, train=train_flag, opt=cfg, rank=rank, **kw)
        return [next(g) for _ in range(n)]

    ref = batches(train, True)
    lengths = set()
    for x in ref:
        t, b, c, h, w = x.shape
        assert (b, c, h, w) == (3, 3, 16, 16) and 4 <= t <= 6
        assert x.dtype == torch.float32 and x.device.type == "cpu"
        assert x.stride() == (b * h * w * c, h * w * c, 1, w * c, c)
        assert all(f.is_contiguous(memory_format=torch.channels_last) for f in x)
        assert 0.0 <= float(x.min()) and float(x.max()) <= 1.0
        lengths.add(t)
    assert len(lengths) > 1

    def same(a, b):
        return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))

    assert same(ref, batches(train, True))
    assert not same(ref, batches(train, True, rank=1))
    assert all(x.shape[0] == 6 for x in batches(train, True, n=3, dynamic_length=False))
    assert all(x.shape[1:] == (3, 3, 16, 16) for x in batches(test, False, n=2))


def test_generator_matches_dataset_stream(tmp_path):
    """plan_batch + one seq_len draw per batch on the generator's RandomState:
    replaying that stream through the dataset gives its frames."""
    write_tree(tmp_path)
    cfg = _gen_cfg(tmp_path)
    train, _ = data_utils.load_dataset(cfg)
    torch.manual_seed(9)
    gen = data_utils.get_data_generator(train, train=True, opt=cfg)
    got = [next(gen) for _ in range(2)]

    train.seed_is_set = True
    np.random.seed(9 % 2**31)
    for x in got:
        want = torch.stack([train[i] for i in range(3)]).permute(1, 0, 2, 3, 4)
        seq_len = int(np.random.randint(6 - 2, 6 + 1))
        assert torch.equal(x, want[:seq_len])


def test_dispatch_and_config(tmp_path, monkeypatch):
    write_tree(tmp_path)
    made = []
    real = data_utils.DataLoader

    def recording_loader(*a, **kw):
        made.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(data_utils, "DataLoader", recording_loader)
    cfg = _gen_cfg(tmp_path, frame_cache="loader")
    train, _ = data_utils.load_dataset(cfg)
    x = next(data_utils.get_data_generator(train, train=True, opt=cfg))
    assert len(made) == 1 and x.shape[1:] == (3, 3, 16, 16)
    x = next(data_utils.get_data_generator(train, train=True, opt=_gen_cfg(tmp_path)))
    assert len(made) == 1, "the device path must not build a DataLoader"
    assert x.shape[1:] == (3, 3, 16, 16)

    with pytest.raises(ValueError, match="frame_cache"):
        data_utils.get_data_generator(train, opt=_gen_cfg(tmp_path, frame_cache="gpu"))
    mnist_cfg = _gen_cfg(tmp_path, dataset="mnist", channels=1, image_width=64)
    mnist, _ = data_utils.load_dataset(mnist_cfg)
    with pytest.raises(ValueError, match="bair"):
        data_utils.get_data_generator(mnist, opt=mnist_cfg)
    # synthetic data has no frames to pack: an error, not a silent switch
    absent = _gen_cfg(tmp_path / "nowhere")
    synth, _ = data_utils.load_dataset(absent)
    assert synth.synthetic
    with pytest.raises(ValueError):
        data_utils.get_data_generator(synth, opt=absent)

    assert Config().frame_cache == "loader"
    assert Config.from_dict(Config().to_dict()).to_dict() == Config().to_dict()
    assert Config.from_dict(_gen_cfg(tmp_path).to_dict()).frame_cache == "device"
    old = Config().to_dict()
    del old["frame_cache"]
    assert Config.from_dict(old).frame_cache == "loader"


def test_pack_cli_builds_both_splits(tmp_path):
    write_tree(tmp_path)
    write_tree(tmp_path, split="test", clips=3)
    from p2pvg_amd.data import pack_bair

    assert pack_bair.main(["--data_root", str(tmp_path), "--image_size", "16",
                           "--workers", "1"]) == 0
    for train, n in ((True, 5), (False, 3)):
        npy, sidecar = make_ds(tmp_path, train=train).pack_paths()
        assert np.load(npy, mmap_mode="r").shape == (n, 6, 16, 16, 3)
        assert os.path.isfile(sidecar)
    with pytest.raises(ValueError):
        pack_bair.main(["--data_root", str(tmp_path / "nowhere")])


def test_train_and_evaluate_cli_device_cache_cpu(tmp_path):
    write_tree(tmp_path, clips=4, size=64)
    write_tree(tmp_path, split="test", clips=3, size=64)
    env = os.environ.copy()
    env["PYTHONPATH"] = ROOT
    log_dir = tmp_path / "logs" / "run"
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "train.py"),
         "--dataset", "bair", "--frame_cache", "device", "--channels", "3",
         "--backbone", "dcgan", "--batch_size", "2", "--max_seq_len", "6",
         "--delta_len", "1", "--g_dim", "32", "--z_dim", "4",
         "--rnn_size", "32", "--nepochs", "1", "--epoch_size", "2",
         "--nsample", "2", "--device", "cpu", "--qual_iter", "100",
         "--data_root", str(tmp_path), "--num_workers", "0",
         "--log_dir", str(log_dir)],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
    )
    assert r.returncode == 0, r.stderr[-3000:]
    run = [d for d in (tmp_path / "logs").iterdir() if d.is_dir()][0]
    assert (run / "model.pth").exists()
    assert os.path.isfile(make_ds(tmp_path, size=64).pack_paths()[0])

    out = tmp_path / "eval.json"
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "evaluate.py"),
         "--ckpt", str(run / "model.pth"), "--frame_cache", "device",
         "--nsample", "2", "--n_batches", "1", "--device", "cpu",
         "--out", str(out)],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
    )
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out) as f:
        result = json.load(f)
    assert result["dataset"] == "bair" and result["data_synthetic"] is False
    assert result["n_sequences"] == 2
