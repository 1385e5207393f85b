"""The ending batches of tests/test_gpu_split_form.py without a device: the fp64 oracle alone, flown over _ending_batch with the GPU test's
own actions and field, meets the conditions that test asserts from the one-lane flight (_ending_conditions) -- at every step length, and
with every battery 0.01 Wh higher and lower, so that no chosen end sits on a stride's edge.  This is how the constants of _ending_batch
(the ends of its battery linspaces) were chosen, kept reproducible."""
import numpy as np
import pytest

pytest.importorskip('torch')        # (the GPU test module imports it)

import oracle  # noqa: E402
import test_gpu_split_form as split_form  # noqa: E402
from test_gpu_parity import oracle_state_from_abi  # noqa: E402


def _fly_oracle(init, acts, field, substeps):
  """What _fly_with(1, ..., single=True) returns, as far as _ending_conditions reads it."""
  o = oracle_state_from_abi({k: np.array(v) for k, v in init.items()})
  snap = lambda: {k: o[k].copy() for k in ('time_elapsed_s', 'status')}      # noqa: E731
  states, terminal, reward = [snap()], [], []
  for a in acts:
    r, t, _, _ = oracle.step(o, a, field=field, threads=4, substeps=substeps)
    states.append(snap()); terminal.append(t.copy()); reward.append(r.copy())
  return dict(states=states, terminal=np.stack(terminal), reward=np.stack(reward), state=states[-1])


@pytest.mark.parametrize('substeps', split_form.SHORT_STEPS + split_form.LONG_STEPS)
def test_oracle_alone_meets_the_ending_conditions(substeps):
  base = split_form._ending_batch(substeps in split_form.LONG_STEPS)
  acts = split_form._actions(split_form._ending_steps(substeps), split_form.N_BATCH, 2000 + substeps)
  stopped = []
  for delta in (0.0, 0.01, -0.01):
    init = dict(base)
    init['battery_charge'] = (base['battery_charge'] + np.float32(delta)).astype(np.float32)
    stopped.append(split_form._ending_conditions(init, _fly_oracle(init, acts, split_form._field(8), substeps), substeps))
  assert stopped[0] == stopped[1] == stopped[2], 'a chosen end moves with 0.01 Wh of battery'
