"""The 16-wide 3x3 wgrad path choice and its P2PVG_WGRAD_NARROW switch
(no GPU)."""
import pytest


@pytest.fixture
def loader():
    from p2pvg_amd.ops import _hip_ext_loader

    ext = _hip_ext_loader.load()
    was = ext.wgrad_narrow(), ext.wgrad_rows(), ext.bn_tail_fused()
    yield _hip_ext_loader
    ext.set_wgrad_narrow(was[0])
    ext.set_wgrad_rows(was[1])
    ext.set_bn_tail_fused(was[2])
    _hip_ext_loader._tail_env_applied = True


def first_load(loader):
    """load() as the first one of a process: reads the environment."""
    loader._tail_env_applied = False
    return loader.load()


#  B    A    A1   the 16-wide classes of the 64-pixel model (batch 512)
HEADLINE_16 = [
    (256, 128, 128),    # c3.0
    (256, 256, 256),    # c3.1, c3.2, upc3.1
    (256, 512, 256),    # upc3.0, dual-X
    (128, 256, 256),    # upc3.2
]
#  the 16-wide classes of the 128-pixel model (batch 128)
V128_16 = [
    (512, 256, 256),    # c4.0
    (512, 512, 512),    # c4.1, c4.2, upc3.1
    (512, 1024, 512),   # upc3.0, dual-X
    (256, 512, 512),    # upc3.2
]
#  the 8-wide ones
HEADLINE_8 = [
    (512, 256, 256),    # c4.0
    (512, 512, 512),    # c4.1, c4.2, upc2.1
    (512, 1024, 512),   # upc2.0, dual-X
    (256, 512, 512),    # upc2.2
]


def test_default_and_env(loader, monkeypatch):
    monkeypatch.delenv("P2PVG_WGRAD_NARROW", raising=False)
    assert first_load(loader).wgrad_narrow() is True
    monkeypatch.setenv("P2PVG_WGRAD_NARROW", "pertap")
    ext = first_load(loader)
    assert ext.wgrad_narrow() is False
    assert ext.conv2d_wgrad_path(256, 256, 256, 16, 16, 1, -1) == "per_tap"
    monkeypatch.setenv("P2PVG_WGRAD_NARROW", "narrow")
    ext = first_load(loader)
    assert ext.wgrad_narrow() is True
    assert ext.conv2d_wgrad_path(256, 256, 256, 16, 16, 1, -1) == "taps_narrow"


def test_switches_are_independent(loader, monkeypatch):
    monkeypatch.setenv("P2PVG_WGRAD_NARROW", "pertap")
    monkeypatch.delenv("P2PVG_WGRAD_ROWS", raising=False)
    ext = first_load(loader)
    assert ext.wgrad_rows() is True
    assert ext.conv2d_wgrad_path(64, 64, 64, 64, 64, 1, -1) == "taps_rows"
    monkeypatch.setenv("P2PVG_WGRAD_NARROW", "narrow")
    monkeypatch.setenv("P2PVG_WGRAD_ROWS", "pertap")
    ext = first_load(loader)
    assert ext.wgrad_narrow() is True
    assert ext.conv2d_wgrad_path(64, 64, 64, 64, 64, 1, -1) == "per_tap"
    assert ext.conv2d_wgrad_path(256, 256, 256, 16, 16, 1, -1) == "taps_narrow"


def test_setter_survives_later_loads(loader, monkeypatch):
    monkeypatch.delenv("P2PVG_WGRAD_NARROW", raising=False)
    ext = first_load(loader)
    ext.set_wgrad_narrow(False)
    assert loader.load().wgrad_narrow() is False


@pytest.mark.parametrize("value", ["rows", "strip", "", "1"])
def test_env_rejects_other_values(loader, monkeypatch, value):
    monkeypatch.setenv("P2PVG_WGRAD_NARROW", value)
    with pytest.raises(ValueError):
        first_load(loader)


def test_path_by_class(loader, monkeypatch):
    monkeypatch.delenv("P2PVG_WGRAD_NARROW", raising=False)
    monkeypatch.delenv("P2PVG_WGRAD_ROWS", raising=False)
    path = first_load(loader).conv2d_wgrad_path
    for b, a, a1 in HEADLINE_16 + V128_16:
        for yr in (0, 1):
            assert path(b, a, a1, 16, 16, yr, -1) == "taps_narrow"
            assert path(b, a, a1, 16, 16, yr, 0) == "per_tap"
            for taps in (5, 6, 7):
                assert path(b, a, a1, 16, 16, yr, taps) == "taps_narrow"
    # every 8-wide class stays on the per-tap path under auto
    for b, a, a1 in HEADLINE_8 + HEADLINE_16 + [(64, 64, 64)]:
        assert path(b, a, a1, 8, 8, 1, -1) == "per_tap"
    # 16-wide classes nobody measured stay there too
    assert path(64, 64, 64, 16, 16, 1, -1) == "per_tap"
    assert path(1024, 1024, 1024, 16, 16, 1, -1) == "per_tap"
    assert path(128, 128, 128, 16, 16, 1, -1) == "per_tap"
    assert path(192, 256, 256, 16, 16, 1, -1) == "per_tap"
    assert path(256, 64, 64, 16, 16, 1, -1) == "per_tap"
    # a 16-wide map of one chunk per image is outside the kernel's ring
    assert path(256, 256, 256, 4, 16, 1, -1) == "per_tap"
    # the other widths keep their kernels
    assert path(64, 64, 64, 64, 64, 1, -1) == "taps_rows"
    assert path(128, 128, 128, 32, 32, 1, -1) == "taps_strip"
    assert path(64, 64, 64, 128, 128, 1, -1) == "per_tap"


def test_existing_path_assertions_still_hold(loader, monkeypatch):
    monkeypatch.delenv("P2PVG_WGRAD_NARROW", raising=False)
    monkeypatch.delenv("P2PVG_WGRAD_ROWS", raising=False)
    path = first_load(loader).conv2d_wgrad_path
    assert path(512, 512, 512, 8, 8, 1, -1) == "per_tap"
    assert path(64, 64, 64, 64, 64, 1, 1) == "taps_strip"
    for taps in (2, 3, 4):
        assert path(128, 128, 128, 64, 64, 0, taps) == "taps_rows"
    with pytest.raises(RuntimeError):
        path(64, 64, 64, 16, 16, 1, 1)       # below a strip
    with pytest.raises(RuntimeError):
        path(64, 64, 64, 64, 64, 1, 5)       # narrow kernel on a 64-wide map


@pytest.mark.parametrize("args", [
    (64, 64, 64, 32, 32, 1, 5),      # 32 wide
    (64, 64, 64, 64, 64, 1, 5),      # 64 wide
    (64, 64, 64, 8, 8, 1, 5),        # 8 wide
    (64, 96, 96, 16, 16, 1, 5),      # channels not 64-aligned
    (96, 64, 64, 16, 16, 1, 5),
    (64, 128, 96, 16, 16, 1, 5),     # dual-X split off a 64 boundary
    (64, 64, 64, 4, 16, 1, 5),       # one chunk per image
    (64, 64, 64, 16, 16, 1, 2),      # row-order kernel on a 16-wide map
    (64, 64, 64, 16, 16, 1, 7),      # 128x64 tiles on B = 64
    (192, 64, 64, 16, 16, 1, 7),
    (64, 64, 64, 32, 32, 1, 6),      # forced tiles off a 16-wide map
    (128, 64, 64, 64, 64, 1, 7),
    (64, 64, 64, 16, 16, 1, 8),      # no such mode
    (64, 64, 64, 16, 16, 1, -2),
])
def test_required_path_raises_when_not_eligible(loader, args):
    with pytest.raises(RuntimeError):
        loader.load().conv2d_wgrad_path(*args)
