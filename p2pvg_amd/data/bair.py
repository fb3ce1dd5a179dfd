"""BAIR robot-push dataset: PNG frame-directory reader.

Capability parity with reference data/bair.py:11-75: frames live in
data_root/bair/processed_data/{train,test}/<d1>/<d2>/<i>.png (produced by the
offline converter, see p2pvg_amd/data/convert_bair.py). Train samples a random
clip directory, test scans in order; __len__ is the reference's fixed 10000;
dynamic length via get_seq_len() U[max-2*delta, max].

If the dataset directory is absent, `synthetic=True` generates random clips of
the right shape so plumbing/bench runs work offline (and report data=synthetic).

`load_pack()` decodes a whole split once into a uint8 array (N, T, S, S, 3),
cached as one .npy beside the split directory, and `plan_batch()` makes the
clip draws of a batch without touching a file: together with ops.clip_gather
they feed `--frame_cache device` (data.get_device_bair_generator), which keeps
the decoded frames on the GPU and ships only clip indices per batch.
"""
from __future__ import annotations

import json
import os
import warnings

import numpy as np
import torch

_warned_unwritable = False


def _decode_clip(task):
    """(clip directory, T, S) -> (T, S, S, 3) uint8, the integers that
    `BairRobotPush._load_png` divides by 255. ValueError names the file."""
    from PIL import Image

    d, T, S = task
    out = np.empty((T, S, S, 3), dtype=np.uint8)
    for i in range(T):
        fname = os.path.join(d, f"{i}.png")
        if not os.path.isfile(fname):
            raise ValueError(f"{d}: clip has fewer than {T} frames ({fname} is missing)")
        with Image.open(fname) as im:
            arr = np.asarray(im.convert("RGB"))
        if arr.shape != (S, S, 3):
            raise ValueError(
                f"{fname}: frame is {arr.shape[1]}x{arr.shape[0]}, image_size is {S}")
        out[i] = arr
    return out


def _open_pack_for_write(path: str, shape):
    return np.lib.format.open_memmap(path, mode="w+", dtype=np.uint8, shape=shape)


class BairRobotPush(torch.utils.data.Dataset):
    def __init__(
        self,
        data_root: str,
        train: bool = True,
        transform=None,
        max_seq_len: int = 30,
        delta_len: int = 5,
        image_size: int = 64,
        opt=None,
        synthetic: bool = False,
    ):
        self.root_dir = os.path.join(data_root, "bair")
        self.train = train
        self.max_seq_len = max_seq_len
        self.delta_len = delta_len
        self.image_size = image_size
        self.seed_is_set = False
        self.channels = 3

        sub = "train" if train else "test"
        self.data_dir = os.path.join(self.root_dir, "processed_data", sub)
        self.ordered = not train
        self.dirs = []
        if os.path.isdir(self.data_dir):
            for d1 in sorted(os.listdir(self.data_dir)):
                p1 = os.path.join(self.data_dir, d1)
                if not os.path.isdir(p1):
                    continue
                for d2 in sorted(os.listdir(p1)):
                    self.dirs.append(os.path.join(p1, d2))
        self.synthetic = synthetic or not self.dirs
        self.d = 0

    def get_seq_len(self) -> int:
        return int(
            np.random.randint(
                low=self.max_seq_len - self.delta_len * 2, high=self.max_seq_len + 1
            )
        )

    def set_seed(self, seed: int) -> None:
        if not self.seed_is_set:
            self.seed_is_set = True
            np.random.seed(seed)

    def __len__(self) -> int:
        return 10000

    def _load_png(self, fname: str) -> torch.Tensor:
        from PIL import Image

        with Image.open(fname) as im:
            arr = np.asarray(im.convert("RGB"), dtype=np.float32) / 255.0
        return torch.from_numpy(arr).permute(2, 0, 1)

    def get_seq(self) -> torch.Tensor:
        s = self.image_size
        if self.synthetic:
            # smooth random video of the right shape (offline plumbing path)
            base = torch.rand(3, s, s)
            drift = torch.randn(self.max_seq_len, 3, 1, 1) * 0.05
            return (base.unsqueeze(0) + drift.cumsum(0)).clamp_(0, 1)

        if self.ordered:
            d = self.dirs[self.d]
            self.d = 0 if self.d == len(self.dirs) - 1 else self.d + 1
        else:
            d = self.dirs[np.random.randint(len(self.dirs))]

        image_seq = torch.zeros(self.max_seq_len, 3, s, s)
        for i in range(self.max_seq_len):
            image_seq[i] = self._load_png(os.path.join(d, f"{i}.png"))
        return image_seq

    def __getitem__(self, index: int) -> torch.Tensor:
        self.set_seed(index)
        return self.get_seq()

    # -- frame pack + batch planner (`--frame_cache device`) -----------------

    def pack_paths(self):
        """(.npy, .json sidecar) of this split's pack, beside the split directory."""
        stem = f"{self.data_dir}_pack{self.image_size}"
        return stem + ".npy", stem + ".json"

    def frames_per_clip(self) -> int:
        """T: the number of frames 0.png, 1.png, ... of the first clip (30 for
        BAIR). Every clip must hold at least as many."""
        T = 0
        while os.path.isfile(os.path.join(self.dirs[0], f"{T}.png")):
            T += 1
        return T

    def load_pack(self, workers: int = 0) -> np.ndarray:
        """Every frame of the split as uint8 (N, T, S, S, 3), N = len(self.dirs)
        in self.dirs order: np.asarray(Image.open(f).convert("RGB")) per file.

        Cached as one .npy beside the split directory with a JSON sidecar
        (clip names, image_size, T); a matching pack is memory-mapped, any
        other is rebuilt (with `workers` decoder processes, at most 16). If the
        location is not writable the pack stays in memory. ValueError, before
        a pack file exists, for an absent dataset, a frame of another size, a
        short clip or max_seq_len > T.
        """
        global _warned_unwritable
        if not self.dirs:
            raise ValueError(
                f"{self.data_dir}: no clip directories; the synthetic fallback "
                "has no frames to pack (frame_cache='device' needs real data)")
        S = self.image_size
        T = self.frames_per_clip()
        if T == 0:
            raise ValueError(f"{self.dirs[0]}: clip has no frame 0.png")
        if self.max_seq_len > T:
            raise ValueError(
                f"{self.data_dir}: max_seq_len={self.max_seq_len} exceeds the "
                f"{T} frames per clip")
        N = len(self.dirs)
        shape = (N, T, S, S, 3)
        meta = {"dirs": [os.path.relpath(d, self.data_dir) for d in self.dirs],
                "image_size": S, "T": T}
        npy, sidecar = self.pack_paths()
        try:
            with open(sidecar) as f:
                if json.load(f) == meta:
                    pack = np.load(npy, mmap_mode="r")
                    if pack.shape == shape and pack.dtype == np.uint8:
                        return pack
        except (OSError, ValueError):
            pass  # absent, unreadable or stale: rebuild

        tmp = f"{npy}.{os.getpid()}.tmp"
        try:
            pack = _open_pack_for_write(tmp, shape)
        except OSError as e:
            if not _warned_unwritable:
                _warned_unwritable = True
                warnings.warn(f"cannot write the frame pack {npy} ({e}); "
                              "keeping it in memory for this run")
            tmp, pack = None, np.empty(shape, dtype=np.uint8)
        tasks = [(d, T, S) for d in self.dirs]
        try:
            workers = min(int(workers), 16, N)
            if workers > 1:
                import multiprocessing as mp

                with mp.get_context("spawn").Pool(workers) as pool:
                    for n, clip in enumerate(pool.imap(_decode_clip, tasks, chunksize=8)):
                        pack[n] = clip
            else:
                for n, task in enumerate(tasks):
                    pack[n] = _decode_clip(task)
        except BaseException:
            if tmp is not None:
                del pack
                os.unlink(tmp)
            raise
        if tmp is None:
            return pack
        pack.flush()
        del pack
        os.replace(tmp, npy)
        with open(sidecar + f".{os.getpid()}.tmp", "w") as f:
            json.dump(meta, f)
        os.replace(f.name, sidecar)  # last: a sidecar vouches for a whole .npy
        return np.load(npy, mmap_mode="r")

    def plan_batch(self, B: int, rng: np.random.RandomState) -> torch.Tensor:
        """Clip indices (B,) int32 of one batch: exactly the draws that B
        consecutive ds[i] make (train: rng.randint(len(dirs)) per sample; test:
        the ordered counter self.d, advanced and wrapped as get_seq does)."""
        if not self.dirs:
            raise ValueError(f"{self.data_dir}: no clip directories to plan over")
        idx = np.empty(B, dtype=np.int32)
        for i in range(B):
            if self.ordered:
                idx[i] = self.d
                self.d = 0 if self.d == len(self.dirs) - 1 else self.d + 1
            else:
                idx[i] = rng.randint(len(self.dirs))
        return torch.from_numpy(idx)
