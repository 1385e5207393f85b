"""The helper form (csrc/ble_step_helper.h, _lib.STEP_FORM_HELPER) with the solar nodes free of reciprocal roots (sun_one_minus_sin_f64,
solar_nodes_time).  Every case forces the form, asks the library which form it launched and compares every state array, the reward row and
the terminal row BIT FOR BIT with the plain one-lane kernel (_lib.step_form(1)) on the same inputs: the two inline the same lane functions,
whose every contraction is an explicit fma.  The launches, the limit of each of them and the comparison are test_gpu_helper_form's.
Shapes: 65 and 257 environments (a ragged last group); 1 substep (record 0 and the reward's record are the whole step), 2, 18 and 33 (the
ring wraps inside a step); 1 and 3 steps.  One batch holds an environment at x = 2e7 m (an angle of 3 rad over the earth's radius: far
outside the range the nodes' polynomials were written for, still finite, still the same bits on both forms).  One batch holds a group
without a live lane from the start.  (Writing record 0 from the first node alone, ahead of nodes 1 and 2, was measured and not kept --
DESIGN.md 3a, round 11; these are the shapes it was held to.)  Needs a real MI355X:  pytest -m gpu."""
import functools

import numpy as np
import pytest

from balloon_learning_environment_amd import _lib
from test_gpu_helper_form import _assert_same, _field, _fly, _frozen_lane0_batch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

SIZES = [65, 257]
SUBSTEPS = [1, 2, 18, 33]
N_STEPS = [1, 3]


@functools.lru_cache(maxsize=None)
def _initial(n):
  import reset_host
  state = reset_host.sample_initial_state(n, seed=1100 + n)
  for v in state.values():
    v.setflags(write=False)
  return state


@functools.lru_cache(maxsize=None)
def _shared_field():
  return _field()


def _both_forms(init, acts, field, **kw):
  """form 1, then the helper form forced (_lib.step_form: ble_set_step_form(12)), on the same inputs"""
  one = _fly(1, init, acts, field, **kw)
  helper = _fly(12, init, acts, field, **kw)
  assert _lib.lib().ble_last_step_form() == 12 == _lib.STEP_FORM_HELPER
  _assert_same(one, helper)
  return one


@pytest.mark.parametrize('n_steps', N_STEPS)
@pytest.mark.parametrize('substeps', SUBSTEPS)
@pytest.mark.parametrize('n', SIZES)
def test_helper_form_keeps_the_one_lane_bits(n, substeps, n_steps):
  init = {k: v.copy() for k, v in _initial(n).items()}
  acts = np.random.default_rng(2000 * n + 10 * substeps + n_steps).integers(0, 3, (n_steps, n)).astype(np.uint8)
  acts[:, ::5] = 0                                    # DOWN: the reward reads the end-of-step record
  _both_forms(init, acts, _shared_field(), substeps=substeps)


@pytest.mark.parametrize('substeps', [18, 33])
def test_an_environment_far_from_its_station(substeps):
  """Environment 70 starts 2e7 m east of its station: the wind query clamps to the field's edge; its wave's nodes are evaluated at 3 rad."""
  n = 257
  init = {k: v.copy() for k, v in _initial(n).items()}
  init['x'][70] = np.float32(2.0e7)
  acts = np.random.default_rng(71).integers(0, 3, (3, n)).astype(np.uint8)
  one = _both_forms(init, acts, _shared_field(), substeps=substeps)
  assert abs(float(one['state']['x'][70])) > 1.0e7      # still that far after the last step
  assert np.isfinite(one['reward']).all()


def test_a_group_without_a_live_lane_from_the_start():
  """test_gpu_helper_form's 199-environment batch with lane 0 frozen at launch, and its second group frozen whole: the helper of that group sees
  `live == 0` in its first publication and writes no record at all; the first group dies out lane by lane."""
  init = _frozen_lane0_batch(True)
  init['status'][64:128] = 1
  acts = np.random.default_rng(72).integers(0, 3, (32, 199)).astype(np.uint8)
  one = _both_forms(init, acts, _shared_field())
  assert (one['terminal'][0, 64:128] != 0).all(), 'the second group was not frozen from the first step'
  assert (one['terminal'][:, :64] != 0).any(0).all(), 'a lane of the first group was still live in the last step'
