"""The observation times tests/test_gpu_carried_slab.py writes to reach the slide at a PARTIAL window (helpers.slide_times), checked on
the host against the window rule itself (strict |t - now| < 6 h, wind_gp.py:183) and against the kernel's own bookkeeping
(csrc/ble_observe.h: n_dropped = (count - n_obs) - (count0 - n_chol0), slid when it is 0 or 1, refitted otherwise)."""
import numpy as np
import pytest

import helpers

SLIDE_SIZES = (2, 3, 5, 63, 64, 65, 118, 119, 120)


@pytest.mark.parametrize('leaving', (1, 2, 3))
@pytest.mark.parametrize('now', (720, 0, 40000))
def test_slide_times_drop_exactly_the_oldest(now, leaving):
  for m in SLIDE_SIZES:
    if m - 1 + leaving > helpers.GP_ROWS:
      continue
    t = helpers.slide_times(m, now, leaving)
    assert len(t) == m - 2 + leaving and np.all(np.diff(t) > 0) and np.all(t < now)
    first = np.concatenate([t, [now]])                         # the ring after the first observe() (it appends `now`)
    w1 = helpers.gp_window(first, now)
    assert w1.tolist() == list(range(len(first))), (m, 'every observation is inside the window of the first call')
    second = np.concatenate([first, [now + 180]])              # ... and after the second, one agent step later
    w2 = helpers.gp_window(second, now + 180)
    assert w2.tolist() == list(range(leaving, len(second))), (m, 'exactly the oldest `leaving` observations are outside')
    assert len(w2) == m
    # the kernel's bookkeeping for the second call: the factor carried from the first covers all of `first`
    count0, n_chol0, count, n_obs = len(first), len(first), len(second), len(w2)
    assert (count - n_obs) - (count0 - n_chol0) == leaving
    # one second earlier the newest leaving observation is still inside: it leaves exactly AT this call
    assert int(np.sum(np.abs(second - (now + 179)) < helpers.GP_HORIZON_S)) == m + 1          # (uncapped: 121 at m = 120)
