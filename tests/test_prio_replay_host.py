"""Prioritized replay and Marco Polo, CPU only: the fp64 restatement of the sum tree (prio_replay_host.py) against hand-computed trees,
its level-by-level rebuild against the node-by-node one, the host build of the replay's uniforms against plan_host.philox4x32, the
precondition of the device draw test, and the argument checks of the new entry points (every one answers BLE_E_INVALID_ARG before any
HIP call)."""
import ctypes

import numpy as np
import pytest

import plan_host
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


def test_rebuild_level_by_level_gives_the_node_by_node_bits():
  """A random tree with padded leaves (5 x 13 = 65 leaves in 128) and some empty leaves, values that round in every sum."""
  rng = np.random.default_rng(0)
  a, b = ph.SumTree(5, 13, 2), ph.SumTree(5, 13, 2)
  assert a.P == 128 and a.leaves == 65
  leaves = np.where(rng.random(65) < 0.2, 0.0, np.sqrt(rng.random(65) * 4))
  for tr in (a, b):
    tr.nodes[:] = rng.random(2 * tr.P)                    # stale parents, and a stale node 0 that neither form touches
    tr.nodes[tr.P:] = 0.0
    tr.nodes[tr.P:tr.P + 65] = leaves
  b.nodes[:b.P] = a.nodes[:a.P]
  a.rebuild()
  b.rebuild_node_by_node()
  assert np.array_equal(a.nodes, b.nodes)
  assert a.nodes[1] > 0 and a.nodes[1] != float(np.float32(a.nodes[1]))
  assert not a.nodes[a.P + 65:].any()


def test_windows_valid_is_window_valid_per_environment():
  rng = np.random.default_rng(1)
  term = (rng.random((7, 40)) < 0.15).astype(np.uint8)
  end = np.maximum(term, (rng.random((7, 40)) < 0.15).astype(np.uint8))
  for t in range(14):
    for n in (1, 3, 5):
      want = [ph.window_valid(term, end, t, e, n) for e in range(40)]
      assert np.array_equal(ph.windows_valid(term, end, t, n), want), (t, n)


def test_find_candidates():
  tr = ph.SumTree(2, 2, 1)
  tr.nodes[tr.P:tr.P + 4] = [1.0, 0.5, 2.0, 1.0]
  tr.rebuild()
  assert tr.find_candidates(0.5) == {0} and tr.find_candidates(3.0) == {2}
  assert tr.find_candidates(1.0) == {0, 1} and tr.find_candidates(float(np.nextafter(1.5, 0.0))) == {1, 2}
  q = tr.stratified_queries(np.array([0.5, 0.25, 0.0]))                   # total 4.5, three strata of 1.5
  assert np.array_equal(q, [0.75, 1.875, 3.0])


@pytest.fixture(scope='module')
def draws(tmp_path_factory):
  return ph.build_replay_draws(tmp_path_factory.mktemp('rpd'))


@pytest.mark.parametrize('seed,b,counter', [(0, 0, 0), (11, 1, 0), (11, 64, 1), (0xFEDCBA9876543210, 3000, 7), (11, 5, 2 ** 32),
                                            (11, 5, 2 ** 32 + 3), (3, 70000, 0xABCDEF0123456789)])
def test_replay_draws_are_philox4x32(draws, seed, b, counter):
  """Row b's stream: key = the seed's words, counter block j = (j, counter low, b, counter high); the words are used from the last to
  the first, two per uniform (high word first), 53 bits."""
  tries = 5
  got = draws(seed, b + 1, counter, tries)[b]
  key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
  words = []
  for j in range(3):
    out = plan_host.philox4x32(np.array([j, counter & 0xFFFFFFFF, b & 0xFFFFFFFF, counter >> 32], np.uint64), key)
    words += [int(w) for w in out[::-1]]
  want = [(((words[2 * k] << 32) | words[2 * k + 1]) >> 11) / 2.0 ** 53 for k in range(tries)]
  assert got.tolist() == want
  assert all(0.0 <= u < 1.0 for u in want) and len(set(want)) == tries
  if counter >= 2 ** 32:                                                   # the high word is part of the key
    assert draws(seed, b + 1, counter & 0xFFFFFFFF, tries)[b].tolist() != want


def test_draw_case_rows_have_one_candidate_leaf(draws):
  """What test_gpu_prio_replay.py's draw test needs of its inputs: at every batch size and counter, every row's query and its two
  neighbours walk to one leaf, and that leaf is a complete valid window -- so the device's leaf is determined whether or not it fuses a
  product, and no row needs a second draw."""
  c = ph.DRAW_CASE
  h = ph.history(c['steps'], c['num_envs'], c['hist_seed'], obs=False, distinct_rewards=True)
  fed, tree = ph.draw_case_tree(h)
  last, lv = c['steps'] - 1, tree.leaf_view()
  assert (fed.leaf_view() > 0).sum() > 300 and np.array_equal(fed.leaf_view() > 0, lv > 0)
  for row in range(c['capacity']):
    t = ph.newest_step(last, c['capacity'], row)
    ok = np.array([t + c['horizon'] <= last and ph.window_valid(h['terminal'], h['episode_end'], t, e, c['horizon'])
                   for e in range(c['num_envs'])]) if t + c['horizon'] <= last else np.zeros(c['num_envs'], bool)
    assert np.array_equal(lv[row] > 0, ok), row
  for b in c['batches']:
    for counter in c['counters']:
      q = tree.stratified_queries(draws(c['seed'], b, counter)[:, 0])
      for i in range(b):
        cand = tree.find_candidates(float(q[i]))
        assert len(cand) == 1, (b, counter, i, cand)
        assert tree.nodes[tree.P + next(iter(cand))] > 0


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
