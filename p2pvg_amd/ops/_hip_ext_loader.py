"""Loader for the in-tree compiled extension (p2pvg_amd/ops/_C*.so)."""
from __future__ import annotations

import os

_tail_env_applied = False


def load():
    global _tail_env_applied
    from . import _C  # in-tree .so built by setup_ext.py

    if not _tail_env_applied:
        # P2PVG_BN_TAIL=fused|split, read once at the first load: the BN
        # statistics tail as one launch (default) or as the earlier
        # fold/finalize/combine sequence, for A/B timing. Later loads leave
        # the mode alone, so _C.set_bn_tail_fused() holds in-process.
        tail = os.environ.get("P2PVG_BN_TAIL", "fused")
        if tail not in ("fused", "split"):
            raise ValueError(
                f"P2PVG_BN_TAIL must be 'fused' or 'split', got {tail!r}")
        # P2PVG_WGRAD_ROWS=rows|pertap, likewise: whether the automatic
        # choice may send the 64-wide 3x3 weight-gradient classes to the
        # row-order all-taps kernel (default) or keeps them on the per-tap
        # kernel, for A/B timing. The results are bitwise the same.
        rows = os.environ.get("P2PVG_WGRAD_ROWS", "rows")
        if rows not in ("rows", "pertap"):
            raise ValueError(
                f"P2PVG_WGRAD_ROWS must be 'rows' or 'pertap', got {rows!r}")
        # P2PVG_WGRAD_NARROW=narrow|pertap, likewise, for the 16-wide 3x3
        # weight-gradient classes and the narrow all-taps kernel.
        narrow = os.environ.get("P2PVG_WGRAD_NARROW", "narrow")
        if narrow not in ("narrow", "pertap"):
            raise ValueError(
                "P2PVG_WGRAD_NARROW must be 'narrow' or 'pertap', "
                f"got {narrow!r}")
        _C.set_bn_tail_fused(tail == "fused")
        _C.set_wgrad_rows(rows == "rows")
        _C.set_wgrad_narrow(narrow == "narrow")
        _tail_env_applied = True
    return _C
