"""The KL early stop's host side (no GPU): Algo_PPO's checks of target_kl, and the gate's executable
specification (mhppo.ppo.kl_limit, mhppo.ppo.kl_gate) that tests/test_target_kl_gpu.py holds the
device's decision to."""
import math

import pytest


class _Knobs:
    """Algo_PPO's hyper-parameter parsing alone (it reads nothing but its argument)."""

    def __init__(self, **kw):
        from mhppo.algo import Algo_PPO
        Algo_PPO._init_hyperparameters(self, kw)


@pytest.mark.parametrize("bad", [0, 0.0, -0.01, -math.inf, math.nan])
def test_target_kl_refused(bad):
    with pytest.raises(ValueError, match="target_kl"):
        _Knobs(target_kl=bad)


def test_target_kl_refused_with_minibatches():
    with pytest.raises(ValueError, match="target_kl"):
        _Knobs(target_kl=0.01, minibatches=4)
    assert _Knobs(minibatches=4).target_kl is None


def test_target_kl_stored_as_float():
    assert _Knobs().target_kl is None
    for given in (0.01, 1, math.inf, "0.02"):
        got = _Knobs(target_kl=given).target_kl
        assert type(got) is float and got == float(given)
    # the other knobs keep their own checks beside it
    both = _Knobs(target_kl=0.01, max_grad_norm=0.5, gae_lambda=0.95)
    assert (both.target_kl, both.max_grad_norm, both.gae_lambda) == (0.01, 0.5, 0.95)


def test_kl_limit():
    from mhppo import ppo
    assert ppo.kl_limit(0.01, 10240) == 1.5 * 0.01 * 10240.0
    assert ppo.kl_limit(0.02, 1.0) == 1.5 * 0.02
    assert ppo.kl_limit(math.inf, 7) == math.inf
    assert isinstance(ppo.kl_limit(1, 3), float) and ppo.kl_limit(1, 3) == 4.5
    # in sum units: mean <= 1.5 tau exactly where sum <= limit, for m a power of two
    m, tau = 4096.0, 0.015
    for s in (1.5 * tau * m, math.nextafter(1.5 * tau * m, math.inf), math.nextafter(1.5 * tau * m, 0.0)):
        assert (s <= ppo.kl_limit(tau, m)) == (s / m <= 1.5 * tau)


def test_kl_gate():
    from mhppo import ppo
    lim = 12.5
    assert ppo.kl_gate(lim, lim, 0, 3) == (True, 0)                       # open at equality
    assert ppo.kl_gate(0.0, lim, 0, 1) == (True, 0)
    assert ppo.kl_gate(math.nextafter(lim, math.inf), lim, 0, 3) == (False, 3)   # closed above
    assert ppo.kl_gate(math.nan, lim, 0, 2) == (False, 2)                 # NaN closes
    assert ppo.kl_gate(math.inf, math.inf, 0, 4) == (True, 0)             # inf never stops on a number
    assert ppo.kl_gate(math.nan, math.inf, 0, 4) == (False, 4)
    assert ppo.kl_gate(0.0, lim, 3, 4) == (False, 3)                      # sticky, the first epoch kept
    assert ppo.kl_gate(math.nan, lim, 3, 5) == (False, 3)
    # a trace: the stop is the first epoch above the limit, whatever follows
    stop, taken = 0, []
    for e, kl in enumerate([0.1, 5.0, 12.5, 13.0, 1.0, 0.0], 1):
        is_open, stop = ppo.kl_gate(kl, lim, stop, e)
        taken.append(is_open)
    assert taken == [True, True, True, False, False, False] and stop == 4
