"""The 3x3 wgrad path choice and its P2PVG_WGRAD_ROWS switch (no GPU)."""
import pytest


@pytest.fixture
def loader():
    from p2pvg_amd.ops import _hip_ext_loader

    ext = _hip_ext_loader.load()
    was_rows, was_tail = ext.wgrad_rows(), ext.bn_tail_fused()
    yield _hip_ext_loader
    ext.set_wgrad_rows(was_rows)
    ext.set_bn_tail_fused(was_tail)
    _hip_ext_loader._tail_env_applied = True


def first_load(loader):
    """load() as the first one of a process: reads the environment."""
    loader._tail_env_applied = False
    return loader.load()


def test_default_and_env(loader, monkeypatch):
    monkeypatch.delenv("P2PVG_WGRAD_ROWS", raising=False)
    assert first_load(loader).wgrad_rows() is True
    monkeypatch.setenv("P2PVG_WGRAD_ROWS", "pertap")
    ext = first_load(loader)
    assert ext.wgrad_rows() is False
    assert ext.conv2d_wgrad_path(64, 64, 64, 64, 64, 1, -1) == "per_tap"
    monkeypatch.setenv("P2PVG_WGRAD_ROWS", "rows")
    ext = first_load(loader)
    assert ext.wgrad_rows() is True
    assert ext.conv2d_wgrad_path(64, 64, 64, 64, 64, 1, -1) == "taps_rows"


def test_setter_survives_later_loads(loader, monkeypatch):
    monkeypatch.delenv("P2PVG_WGRAD_ROWS", raising=False)
    ext = first_load(loader)
    ext.set_wgrad_rows(False)
    assert loader.load().wgrad_rows() is False


def test_env_rejects_other_values(loader, monkeypatch):
    monkeypatch.setenv("P2PVG_WGRAD_ROWS", "strip")
    with pytest.raises(ValueError):
        first_load(loader)


def test_path_by_class(loader, monkeypatch):
    monkeypatch.delenv("P2PVG_WGRAD_ROWS", raising=False)
    path = first_load(loader).conv2d_wgrad_path
    #           B    A   A1  HO  WO  yr taps
    assert path(64, 64, 64, 64, 64, 1, -1) == "taps_rows"     # c1.1
    assert path(64, 128, 64, 64, 64, 1, -1) == "taps_rows"    # upc5.0, dual-X
    assert path(64, 64, 64, 64, 64, 1, 0) == "per_tap"
    assert path(64, 64, 64, 64, 64, 1, 1) == "taps_strip"
    for taps in (2, 3, 4):
        assert path(128, 128, 128, 64, 64, 0, taps) == "taps_rows"
    # the measured 64-wide classes of the 128-pixel model
    assert path(128, 64, 64, 64, 64, 1, -1) == "taps_rows"
    assert path(128, 128, 128, 64, 64, 1, -1) == "taps_rows"
    assert path(128, 256, 128, 64, 64, 1, -1) == "taps_rows"
    assert path(64, 128, 128, 64, 64, 1, -1) == "taps_rows"
    # 64-wide classes not measured, 128-wide maps: per-tap under auto
    assert path(256, 64, 64, 64, 64, 1, -1) == "per_tap"
    assert path(64, 512, 512, 64, 64, 1, -1) == "per_tap"
    assert path(64, 64, 64, 128, 128, 1, -1) == "per_tap"
    # 32-wide classes keep the strip kernel
    assert path(128, 128, 128, 32, 32, 1, -1) == "taps_strip"
    assert path(512, 512, 512, 8, 8, 1, -1) == "per_tap"


@pytest.mark.parametrize("args", [
    (64, 64, 64, 32, 32, 1, 2),      # 32 wide
    (64, 64, 64, 128, 128, 1, 2),    # 128 wide
    (64, 96, 96, 64, 64, 1, 2),      # channels not 64-aligned
    (64, 64, 64, 16, 16, 1, 1),      # below a strip
    (64, 64, 64, 64, 64, 1, 5),      # no such mode
])
def test_required_path_raises_when_not_eligible(loader, args):
    with pytest.raises(RuntimeError):
        loader.load().conv2d_wgrad_path(*args)
