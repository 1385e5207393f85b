"""The hand-over of the helper form (csrc/ble_step_helper.h, _lib.STEP_FORM_HELPER) after round 9: a 32-record ring and the publication
made at the START of the main wave's step.  Every case forces the form, compares every state array, reward, terminal and effective
action BIT FOR BIT with the plain one-lane kernel (_lib.step_form(1)) on the same inputs and asks the library which form it launched.
The launches, the limit of each of them and the comparison are test_gpu_helper_form's (a hand-over that never completes ends the session
there, once).  Shapes: 65 (a one-lane second group), 257 (a workgroup of one one-lane group next to a full one) and 4 x 64 x 3 + 1
environments (four workgroups, the last with three empty groups); records per step (substeps + 1) below, at and above the ring's 32, up
to 61 (the ring wraps inside a step); 1, 3 and 32 steps (the helper a whole step ahead).  Needs a real MI355X:  pytest -m gpu."""
import functools

import numpy as np
import pytest

from balloon_learning_environment_amd import _lib
from test_gpu_helper_form import _assert_same, _await, _field, _fly, _frozen_lane0_batch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

SIZES = [65, 257, 4 * 64 * 3 + 1]
SUBSTEPS = [1, 2, 13, 18, 31, 32, 33, 60]
N_STEPS = [1, 3, 32]


@functools.lru_cache(maxsize=None)
def _initial(n):
  import reset_host
  state = reset_host.sample_initial_state(n, seed=900 + n)
  for v in state.values():
    v.setflags(write=False)
  return state


@functools.lru_cache(maxsize=None)
def _shared_field():
  return _field()


def _both_forms(init, acts, field, **kw):
  """form 1, then the forced helper form, on the same inputs; the library must report the helper form for the launch it made last"""
  one = _fly(1, init, acts, field, **kw)
  helper = _fly(_lib.STEP_FORM_HELPER, init, acts, field, **kw)
  assert _lib.lib().ble_last_step_form() == _lib.STEP_FORM_HELPER == 12
  _assert_same(one, helper)
  return one


@pytest.mark.parametrize('n_steps', N_STEPS)
@pytest.mark.parametrize('substeps', SUBSTEPS)
@pytest.mark.parametrize('n', SIZES)
def test_ring_depths_and_ragged_groups(n, substeps, n_steps):
  """One fused launch (state, reward, terminal, live counts) and the same steps as single launches (the effective action too)."""
  init = {k: v.copy() for k, v in _initial(n).items()}
  acts = np.random.default_rng(1000 * n + 10 * substeps + n_steps).integers(0, 3, (n_steps, n)).astype(np.uint8)
  acts[:, ::5] = 0                                    # DOWN: the reward reads the end-of-step record
  field = _shared_field()
  _both_forms(init, acts, field, substeps=substeps)
  _both_forms(init, acts[:min(n_steps, 3)], field, substeps=substeps, single=True)


def _mixed_batch():
  """4 x 64 x 3 + 1 environments built as test_gpu_helper_form builds its batches: the first group's lanes run out of power one after the
  other AFTER its lane 0 (publications of a wave without a live lane: publish_idle), the second group frozen from the first step
  (all_frozen on the helper from its first publication), lanes 130 .. 159 out of power inside a step of the rollout, every status byte
  scattered over the rest."""
  n = SIZES[-1]
  init = {k: v.copy() for k, v in _initial(n).items()}
  first = _frozen_lane0_batch(False)
  for k in init:                                       # the whole first group is the 199-environment batch's first group
    init[k][:64] = first[k][:64]
  status = np.zeros(n, np.uint8)
  status[64:128] = 1
  status[400:n:7] = np.arange(len(range(400, n, 7)), dtype=np.uint8) % 4
  init['status'] = status
  init['battery_charge'][130:160] = np.linspace(0.05, 20.0, 30).astype(np.float32)
  return init


@pytest.mark.parametrize('substeps', [18, 33])
def test_lanes_that_end_and_groups_without_a_live_lane(substeps):
  init = _mixed_batch()
  n = init['status'].size
  acts = np.random.default_rng(61).integers(0, 3, (32, n)).astype(np.uint8)
  one = _both_forms(init, acts, _shared_field(), substeps=substeps)
  ended_at = np.where(one['terminal'][:, :64] != 0, np.arange(32)[:, None], 32).min(0)
  assert ended_at[0] == 0 and ended_at[1:].max() > 0 and ended_at.max() < 31, 'the first group did not die out after its lane 0'
  assert (one['terminal'][0, 64:128] != 0).all(), 'the second group was not frozen from the first step'
  assert (one['state']['status'][130:160] != 0).sum() >= 1, 'no lane ended inside a step'
  _both_forms(init, acts[:3], _shared_field(), substeps=substeps, single=True)


def _two_launches(form, init, acts, field, substeps):
  from balloon_learning_environment_amd import vec_state as ble
  k, n = acts.shape[1:]
  out = {'reward': [], 'terminal': [], 'active_count': []}
  with _lib.step_form(form):
    sim = ble.VecSimulator(n); sim.set_state(init); sim.set_grid(field)
    for j in range(2):
      a = torch.from_numpy(acts[j]).cuda()
      rew = torch.zeros((k, n), dtype=torch.float32).cuda(); term = torch.zeros((k, n), dtype=torch.uint8).cuda()
      cnt = torch.zeros((k, ble.COUNT_SLOTS), dtype=torch.int64).cuda()
      sim.step_n(a, rew, term, cnt, substeps=substeps)
      _await(f'form {form}, launch {j} of two on one state')
      assert _lib.lib().ble_last_step_form() == form
      out['reward'].append(rew.cpu().numpy()); out['terminal'].append(term.cpu().numpy()); out['active_count'].append(cnt.cpu().numpy())
    r, t = sim.step(torch.from_numpy(acts[1, 0]).cuda(), substeps=substeps)          # a third launch: the effective action
    _await(f'form {form}, a single step after two launches')
    assert _lib.lib().ble_last_step_form() == form
    out['reward'].append(r.cpu().numpy()[None].copy()); out['terminal'].append(t.cpu().numpy()[None].copy())
    out['effective_action'] = sim.effective_action.cpu().numpy().copy()
    out['err_flags'] = int(sim.err_flags.item())
    out['state'] = sim.get_state()
  for name in ('reward', 'terminal', 'active_count'):
    out[name] = np.concatenate(out[name])
  return out


@pytest.mark.parametrize('substeps', [18, 31])
def test_consecutive_launches_on_one_state(substeps):
  """The counters and the ring start from zero in every launch: 3 steps (57 or 96 records: not a multiple of the ring), 3 more steps and a
  single step on the state the launches before left."""
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  n = SIZES[1]
  init = {k: v.copy() for k, v in _initial(n).items()}
  acts = np.random.default_rng(62).integers(0, 3, (2, 3, n)).astype(np.uint8)
  one = _two_launches(1, init, acts, _shared_field(), substeps)
  helper = _two_launches(_lib.STEP_FORM_HELPER, init, acts, _shared_field(), substeps)
  _assert_same(one, helper)
