"""Host-side dispatch of the contrastive loss (functional.set_loss_tiled / loss_tiled_mode /
loss_uses_tiled): which gathered batch sizes take the tiled MFMA kernels (csrc/loss_tiled.hip) and
which the one-workgroup ones.  Pure Python -- no GPU."""
import pytest


@pytest.fixture()
def Fn():
    from ctclip_mi355x import functional
    old = functional.loss_tiled_mode()
    yield functional
    functional.set_loss_tiled(old)


def test_default_mode_is_auto(Fn):
    assert Fn.loss_tiled_mode() == 'auto'


@pytest.mark.parametrize('mode,expect', [('auto', (False, False, True)), ('always', (True, True, True)),
                                         ('never', (False, False, False))])
def test_loss_uses_tiled(Fn, mode, expect):
    """'auto' switches exactly above the one-workgroup kernels' 128-row limit."""
    Fn.set_loss_tiled(mode)
    assert Fn.loss_tiled_mode() == mode
    assert tuple(Fn.loss_uses_tiled(Bg) for Bg in (1, 128, 129)) == expect


def test_set_returns_previous_mode(Fn):
    assert Fn.set_loss_tiled('always') == 'auto'
    assert Fn.set_loss_tiled('auto') == 'always'


@pytest.mark.parametrize('mode', ['Auto', 'tiled', '', None, 1])
def test_unknown_mode_is_rejected(Fn, mode):
    with pytest.raises(ValueError):
        Fn.set_loss_tiled(mode)
    assert Fn.loss_tiled_mode() == 'auto'
