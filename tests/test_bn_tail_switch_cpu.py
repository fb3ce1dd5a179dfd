"""The BN statistics tail switch: setter, getter and P2PVG_BN_TAIL (no GPU)."""
import pytest


@pytest.fixture
def loader():
    from p2pvg_amd.ops import _hip_ext_loader

    ext = _hip_ext_loader.load()
    was = ext.bn_tail_fused()
    yield _hip_ext_loader
    ext.set_bn_tail_fused(was)
    _hip_ext_loader._tail_env_applied = True


def first_load(loader):
    """load() as the first one of a process: reads the environment."""
    loader._tail_env_applied = False
    return loader.load()


def test_default_is_fused(loader, monkeypatch):
    monkeypatch.delenv("P2PVG_BN_TAIL", raising=False)
    assert first_load(loader).bn_tail_fused() is True


def test_env_is_read_at_first_load(loader, monkeypatch):
    monkeypatch.setenv("P2PVG_BN_TAIL", "split")
    assert first_load(loader).bn_tail_fused() is False
    monkeypatch.setenv("P2PVG_BN_TAIL", "fused")
    assert first_load(loader).bn_tail_fused() is True


def test_setter_survives_later_loads(loader, monkeypatch):
    monkeypatch.delenv("P2PVG_BN_TAIL", raising=False)
    ext = first_load(loader)
    ext.set_bn_tail_fused(False)
    assert loader.load().bn_tail_fused() is False
    ext.set_bn_tail_fused(True)
    assert loader.load().bn_tail_fused() is True


def test_env_rejects_other_values(loader, monkeypatch):
    monkeypatch.setenv("P2PVG_BN_TAIL", "both")
    with pytest.raises(ValueError):
        first_load(loader)
