"""Prioritized replay and Marco Polo, CPU only: the fp64 restatement of the sum tree (prio_replay_host.py) against hand-computed trees,
and the argument checks of the new entry points (every one answers BLE_E_INVALID_ARG before any HIP call)."""
import ctypes

import numpy as np
import pytest

import prio_replay_host as ph
from balloon_learning_environment_amd import _abi, _lib

E_INVALID_ARG = -1
_FAKE = 0x100000


def test_tree_by_hand():
  """T = 3 steps, N = 2 envs, n = 1: six leaves padded to eight."""
  tr = ph.SumTree(3, 2, 1)
  assert tr.P == 8
  term = np.zeros((3, 2), np.uint8)
  end = np.zeros((3, 2), np.uint8)
  tr.add(term, end)                                       # step 0: row 0 zeroed, nothing complete
  assert tr.nodes[1] == 0.0
  end[1, 1] = 1                                           # step 1 of env 1 is a time-limit end
  tr.add(term, end)                                       # step 1: row 0 complete (window t = 0: steps 0 .. 0)
  np.testing.assert_array_equal(tr.leaf_view(), [[1, 1], [0, 0], [0, 0]])
  tr.add(term, end)                                       # step 2: row 1 complete; env 1 crosses the time limit
  np.testing.assert_array_equal(tr.leaf_view(), [[1, 1], [1, 0], [0, 0]])
  assert tr.nodes[1] == 3.0 and tr.nodes[4] == 2.0 and tr.nodes[5] == 1.0 and tr.nodes[2] == 3.0 and tr.nodes[3] == 0.0
  bad = tr.set_priority([0, 2, 0, -1], [3.0, 0.25, 8.0, 100.0])          # leaf 0 twice: the later row (8.0) wins; -1 skipped
  assert not bad
  v0, v2 = float(np.sqrt(np.float32(8.0) + np.float32(1e-10))), float(np.sqrt(np.float32(0.25) + np.float32(1e-10)))
  assert tr.nodes[8] == v0 and tr.nodes[10] == v2 and tr.nodes[1] == ((v0 + 1.0) + (v2 + 0.0)) + 0.0
  assert tr.max_priority == v0
  term[0, 0] = 1
  tr.add(term, end)                                       # step 3 overwrites row 0 (zeroed); row 2 complete with the max
  np.testing.assert_array_equal(tr.leaf_view(), [[0, 0], [v2, 0], [v0, v0]])
  assert tr.set_priority([3], [float('nan')])             # NaN: leaf unchanged, flagged
  assert tr.leaf_view()[1, 1] == 0.0
  assert tr.set_priority([0], [1e-12]) is False and tr.max_priority == v0      # the max never falls


def test_stratified_walk_by_hand():
  tr = ph.SumTree(2, 2, 1)
  tr.nodes[tr.P:tr.P + 4] = [1.0, 0.0, 2.0, 1.0]
  tr.rebuild()
  # total 4, B = 4 strata of width 1: [0,1) -> leaf 0, [1,2) and [2,3) -> leaf 2, [3,4) -> leaf 3
  np.testing.assert_array_equal(tr.stratified(np.array([0.5, 0.0, 0.999, 0.1])), [0, 2, 2, 3])
  # a query that rounding points at the empty leaf 1 takes its sibling
  assert tr.find(0.9999999) == 0 and tr.find(1.0) == 2
  tr.nodes[tr.P:tr.P + 4] = [0.0, 0.0, 0.0, 5.0]
  tr.rebuild()
  assert tr.find(0.0) == 3 and tr.find(7.0) == 3


def test_weighted_loss_formula():
  p = np.array([1.0, 4.0, 0.25, 0.0], np.float32)
  loss = np.array([2.0, 2.0, 2.0, 9.0], np.float32)
  got = ph.weighted_loss(p, loss, np.array([True, True, True, False]))
  np.testing.assert_allclose(got, [0.5 * 2.0, 0.25 * 2.0, 1.0 * 2.0, 0.0], rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------- argument checks
def _replay(**kw):
  v = dict(capacity=10, num_envs=4, update_horizon=5, obs_stride=1104, gamma=0.993, max_tries=64, reserved_=0, obs=_FAKE, action=_FAKE,
           reward=_FAKE, terminal=_FAKE, episode_end=_FAKE, count=_FAKE, counter=_FAKE)
  v.update(kw)
  return _abi.BleReplayF32(**v)


def _tree(**kw):
  v = dict(leaves=40, padded=64, nodes=_FAKE, max_priority=_FAKE)
  v.update(kw)
  return _abi.BleSumTreeF64(**v)


def _batch(**kw):
  v = dict(batch=32, state_stride=1104, state=_FAKE, next_state=_FAKE, ret=_FAKE, discount=_FAKE, action=_FAKE, index=_FAKE)
  v.update(kw)
  return _abi.BleTrainBatchF32(**v)


_TREE_CASES = {'leaves_mismatch': {'leaves': 39}, 'padded_small': {'padded': 32}, 'padded_not_pow2': {'padded': 48},
               'padded_too_large': {'padded': 128}, 'null_nodes': {'nodes': None}, 'null_max': {'max_priority': None},
               'misaligned_nodes': {'nodes': _FAKE + 4}}


@pytest.mark.parametrize('case', sorted(_TREE_CASES))
def test_tree_add_rejects(case):
  assert _lib.lib().ble_replay_tree_add_f64(ctypes.byref(_replay()), ctypes.byref(_tree(**_TREE_CASES[case])), None) == E_INVALID_ARG


def test_tree_add_rejects_bad_replay():
  assert _lib.lib().ble_replay_tree_add_f64(ctypes.byref(_replay(update_horizon=0)), ctypes.byref(_tree()), None) == E_INVALID_ARG
  assert _lib.lib().ble_replay_tree_add_f64(None, ctypes.byref(_tree()), None) == E_INVALID_ARG
  assert _lib.lib().ble_replay_tree_add_f64(ctypes.byref(_replay()), None, None) == E_INVALID_ARG


def _sample(rp=None, tr=None, bt=None, priority=_FAKE):
  return _lib.lib().ble_replay_sample_prioritized_f32(ctypes.byref(rp or _replay()), ctypes.byref(tr or _tree()), ctypes.byref(bt or _batch()),
                                                       priority, 1, None, None)


def _set(rp=None, tr=None, bt=None, priority=_FAKE, loss=_FAKE, out=_FAKE):
  return _lib.lib().ble_replay_set_priority_f32(ctypes.byref(rp or _replay()), ctypes.byref(tr or _tree()), ctypes.byref(bt or _batch()),
                                                 priority, loss, out, None, None)


@pytest.mark.parametrize('fn', [_sample, _set])
def test_sample_and_set_reject(fn):
  assert fn(rp=_replay(capacity=5)) == E_INVALID_ARG
  assert fn(rp=_replay(gamma=float('nan'))) == E_INVALID_ARG
  for case in _TREE_CASES.values():
    assert fn(tr=_tree(**case)) == E_INVALID_ARG, case
  assert fn(bt=_batch(index=None)) == E_INVALID_ARG
  assert fn(bt=_batch(batch=-1)) == E_INVALID_ARG
  assert fn(bt=_batch(state=_FAKE + 4)) == E_INVALID_ARG
  assert fn(priority=None) == E_INVALID_ARG
  assert fn(bt=_batch(batch=0)) == 0                      # an empty batch launches nothing


def test_set_rejects_null_outputs():
  assert _set(loss=None) == E_INVALID_ARG
  assert _set(out=None) == E_INVALID_ARG


def _mp(**kw):
  v = dict(n=16, obs_stride=1104, reserved_=0, exploratory_episode_probability=0.8, seed=1, obs=_FAKE, begin=_FAKE, step=_FAKE,
           phase_clock=_FAKE, walk_clock=_FAKE, exploratory_episode=_FAKE, exploratory_phase=_FAKE, target=_FAKE)
  v.update(kw)
  return _abi.BleMarcoPoloF32(**v)


_MP_CASES = {**{f'null_{p}': {p: None} for p in ('obs', 'begin', 'step', 'phase_clock', 'walk_clock', 'exploratory_episode',
                                                  'exploratory_phase', 'target')},
             'negative_n': {'n': -1}, 'stride_0': {'obs_stride': 0}, 'probability_high': {'exploratory_episode_probability': 1.5},
             'probability_nan': {'exploratory_episode_probability': float('nan')}, 'misaligned_target': {'target': _FAKE + 4}}


@pytest.mark.parametrize('case', sorted(_MP_CASES))
def test_marco_polo_rejects(case):
  assert _lib.lib().ble_marco_polo_u8(ctypes.byref(_mp(**_MP_CASES[case])), _FAKE, None) == E_INVALID_ARG


def test_marco_polo_null_action_and_empty():
  assert _lib.lib().ble_marco_polo_u8(ctypes.byref(_mp()), None, None) == E_INVALID_ARG
  assert _lib.lib().ble_marco_polo_u8(None, _FAKE, None) == E_INVALID_ARG
  assert _lib.lib().ble_marco_polo_u8(ctypes.byref(_mp(n=0)), _FAKE, None) == 0


def test_new_entry_points_are_declared_without_int64():
  lib = _lib.lib()
  for name in ('ble_replay_tree_add_f64', 'ble_replay_sample_prioritized_f32', 'ble_replay_set_priority_f32', 'ble_marco_polo_u8'):
    assert name in _lib.EXPORTS
    assert ctypes.c_int64 not in getattr(lib, name).argtypes, name
