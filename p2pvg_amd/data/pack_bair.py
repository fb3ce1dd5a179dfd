"""Build the BAIR frame packs ahead of time.

    python -m p2pvg_amd.data.pack_bair --data_root DIR [--image_size 64] [--workers K]

Decodes every PNG of data_root/bair/processed_data/{train,test} once, with a
pool of K processes (at most 16), into the uint8 packs that
`BairRobotPush.load_pack` reads and `--frame_cache device` uploads. Without
this step the first run with that flag builds them itself, in one process.
A split whose pack is up to date is left alone.
"""
from __future__ import annotations

import argparse
import sys
import time

from .bair import BairRobotPush

MAX_WORKERS = 16


def main(argv=None) -> int:
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--data_root", type=str, required=True)
    parser.add_argument("--image_size", type=int, default=64)
    parser.add_argument("--workers", type=int, default=8,
                        help=f"decoder processes, at most {MAX_WORKERS}")
    args = parser.parse_args(argv)
    workers = max(1, min(args.workers, MAX_WORKERS))
    for train in (True, False):
        # max_seq_len=1: the pack always holds every frame of a clip
        ds = BairRobotPush(args.data_root, train=train, max_seq_len=1,
                           image_size=args.image_size)
        t0 = time.perf_counter()
        pack = ds.load_pack(workers=workers)
        print(f"[pack_bair] {ds.pack_paths()[0]}: {pack.shape[0]} clips x "
              f"{pack.shape[1]} frames, {pack.nbytes / 2**20:.1f} MiB, "
              f"{time.perf_counter() - t0:.1f} s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
