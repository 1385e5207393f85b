"""The entry points of a population's prioritized replay and Marco Polo exploration (ble_replay_tree_add_grouped_f64,
ble_replay_sample_prioritized_grouped_f32, ble_replay_set_priority_grouped_f32, ble_marco_polo_grouped_u8) on a machine
without a GPU, in the manner of test_population_td_entry_checks_host.py: declared, exported and mirrored field by field; every refusal
answers BLE_E_INVALID_ARG before any HIP call, over fake non-NULL pointers that are never dereferenced (the only calls below that answer
BLE_OK have nothing to launch: an empty batch, no lanes); the plain and the 3t entry points keep their answers."""
import ctypes
import os
import re
import subprocess

import pytest

from balloon_learning_environment_amd import _abi, _lib
from descriptors_host import E_INVALID_ARG, _FAKE, _batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()
ENTRIES = ('ble_replay_tree_add_grouped_f64', 'ble_replay_sample_prioritized_grouped_f32', 'ble_replay_set_priority_grouped_f32',
           'ble_marco_polo_grouped_u8')
NAN = float('nan')
P, R, T = 3, 5, 12                                        # 3 members of 5 columns, 12 ring rows: 60 leaves per member, padded to 64


def _fields(struct_name):
  body = HEADER[HEADER.index('typedef struct %s {' % struct_name):HEADER.index('} %s;' % struct_name)]
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  return re.findall(r'(\w+);', body)


def test_structs_match_header():
  names = _fields('ble_sum_tree_grouped_f64')
  assert names == [f[0] for f in _abi.BleSumTreeGroupedF64._fields_] == ['members', 'leaves', 'padded', 'member_stride', 'nodes',
                                                                         'max_priority']
  assert [getattr(_abi.BleSumTreeGroupedF64, n).offset for n in names] == [0, 8, 16, 24, 32, 40]
  assert [getattr(_abi.BleSumTreeGroupedF64, n).size for n in names] == [8] * 6
  assert ctypes.sizeof(_abi.BleSumTreeGroupedF64) == 48
  names = _fields('ble_marco_polo_grouped_f32')
  assert names == [f[0] for f in _abi.BleMarcoPoloGroupedF32._fields_]
  assert names == ['n', 'obs_stride', 'reserved_', 'members', 'probability', 'seed', 'obs', 'begin', 'step', 'phase_clock', 'walk_clock',
                   'exploratory_episode', 'exploratory_phase', 'target']
  assert [getattr(_abi.BleMarcoPoloGroupedF32, n).offset for n in names] == [0, 8, 12] + list(range(16, 16 + 8 * 11, 8))
  assert [getattr(_abi.BleMarcoPoloGroupedF32, n).size for n in names] == [8, 4, 4] + [8] * 11
  assert ctypes.sizeof(_abi.BleMarcoPoloGroupedF32) == 104
  # ble_marco_polo_f32's fields, with members and the two device arrays in place of the two scalars
  plain = [f[0] for f in _abi.BleMarcoPoloF32._fields_]
  assert [n for n in names if n not in ('members', 'probability', 'seed')] == \
      [n for n in plain if n not in ('exploratory_episode_probability', 'seed')]


def test_entries_declared_exported_and_without_int64_arguments():
  declared = set(re.findall(r'^int (ble_\w+)\(', HEADER, re.M))
  out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.build()]).decode()
  exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
  lib = _lib.lib()
  for name in ENTRIES:
    assert name in declared and name in exported and name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS, name
    assert ctypes.c_int64 not in getattr(lib, name).argtypes, name
  assert _lib.ABI_VERSION == 5 and lib.ble_abi_version() == 5 and any(s.endswith('ble_population_prio.h') for s in _lib._SOURCES)


# ---- the descriptors -------------------------------------------------------------------------------------------------------------------
def _replay(**fields):
  d = dict(capacity=T, num_envs=P * R, update_horizon=5, obs_stride=1104, gamma=0.993, max_tries=64, reserved_=0, obs=_FAKE, action=_FAKE,
           reward=_FAKE, terminal=_FAKE, episode_end=_FAKE, count=_FAKE, counter=_FAKE)
  d.update(fields)
  return _abi.BleReplayF32(**d)


def _trees(**fields):
  d = dict(members=P, leaves=T * R, padded=64, member_stride=128, nodes=_FAKE, max_priority=_FAKE)
  d.update(fields)
  return _abi.BleSumTreeGroupedF64(**d)


def _prio_batch(**fields):
  return _batch(**{**dict(batch=99, index=_FAKE), **fields})


def _ref(x):
  return None if x is None else ctypes.byref(x)


def _add(rp, tr):
  return _lib.lib().ble_replay_tree_add_grouped_f64(_ref(rp), _ref(tr), None)


def _sample(rp, tr, bt, seeds=_FAKE, priority=_FAKE):
  return _lib.lib().ble_replay_sample_prioritized_grouped_f32(_ref(rp), _ref(tr), seeds, _ref(bt), priority, None, None)


def _set(rp, tr, bt, priority=_FAKE, loss=_FAKE, weighted=_FAKE):
  return _lib.lib().ble_replay_set_priority_grouped_f32(_ref(rp), _ref(tr), _ref(bt), priority, loss, weighted, None, None)


# what every one of the three refuses of the ring and the trees: (replay fields, tree fields)
_RING_TREE_CASES = {
    # the ring: what the plain entry points refuse
    'horizon_0': (dict(update_horizon=0), {}), 'horizon_65': (dict(update_horizon=65), {}), 'capacity_5': (dict(capacity=5), dict(leaves=25, padded=32)),
    'envs_0': (dict(num_envs=0), {}), 'obs_stride_1098': (dict(obs_stride=1098), {}), 'obs_stride_1102': (dict(obs_stride=1102), {}),
    'gamma_nan': (dict(gamma=NAN), {}), 'tries_0': (dict(max_tries=0), {}), 'tries_1025': (dict(max_tries=1025), {}),
    'null_obs': (dict(obs=None), {}), 'unaligned_obs': (dict(obs=_FAKE + 4), {}), 'null_action': (dict(action=None), {}),
    'null_reward': (dict(reward=None), {}), 'null_terminal': (dict(terminal=None), {}), 'null_episode_end': (dict(episode_end=None), {}),
    'null_count': (dict(count=None), {}), 'null_counter': (dict(counter=None), {}),
    # the members
    'members_0': ({}, dict(members=0)), 'members_negative': ({}, dict(members=-3)),
    'members_do_not_divide_envs': ({}, dict(members=2, leaves=90, padded=128, member_stride=256)),
    'members_do_not_divide_envs_16': (dict(num_envs=16), {}),
    # the per-member sizes
    'leaves_of_the_whole_ring': ({}, dict(leaves=T * P * R, padded=256, member_stride=512)),
    'leaves_short': ({}, dict(leaves=T * R - 1)), 'leaves_long': ({}, dict(leaves=T * R + 1)),
    'padded_128': ({}, dict(padded=128, member_stride=256)), 'padded_32': ({}, dict(padded=32)), 'padded_60': ({}, dict(padded=60)),
    'padded_0': ({}, dict(padded=0)), 'padded_negative': ({}, dict(padded=-64)),
    'leaves_above_max': (dict(capacity=2 ** 31 // R + 1), dict(leaves=(2 ** 31 // R + 1) * R, padded=2 ** 32, member_stride=2 ** 33)),
    'stride_short': ({}, dict(member_stride=127)), 'stride_padded': ({}, dict(member_stride=64)), 'stride_0': ({}, dict(member_stride=0)),
    'stride_negative': ({}, dict(member_stride=-128)),
    # the per-member arrays
    'null_nodes': ({}, dict(nodes=None)), 'null_max_priority': ({}, dict(max_priority=None)),
    'unaligned_nodes': ({}, dict(nodes=_FAKE + 4)), 'unaligned_max_priority': ({}, dict(max_priority=_FAKE + 4)),
}


@pytest.mark.parametrize('case', sorted(_RING_TREE_CASES))
def test_ring_and_tree_refusals(case):
  ring, tree = _RING_TREE_CASES[case]
  rp, tr = _replay(**ring), _trees(**tree)
  assert _add(rp, tr) == E_INVALID_ARG, case
  assert _sample(rp, tr, _prio_batch()) == E_INVALID_ARG, case
  assert _set(rp, tr, _prio_batch()) == E_INVALID_ARG, case
  # ... and with nothing to launch: the descriptors are checked before the empty batch is noticed
  assert _sample(rp, tr, _prio_batch(batch=0)) == E_INVALID_ARG, case
  assert _set(rp, tr, _prio_batch(batch=0)) == E_INVALID_ARG, case


def test_one_member_of_all_columns_and_a_wide_stride_pass_the_checks():
  """The fixture descriptors are otherwise valid: an empty batch answers BLE_OK with nothing launched (no HIP call: there is no device
  here), also at P = 1 (the solo sizes) and at a stride that leaves a gap between the trees."""
  for tr in (_trees(), _trees(member_stride=128 + 7), _trees(members=1, leaves=T * P * R, padded=256, member_stride=512),
             _trees(members=P * R, leaves=T, padded=16, member_stride=32)):
    bt = _prio_batch(batch=0)
    assert _sample(_replay(), tr, bt) == 0
    assert _set(_replay(), tr, bt) == 0


_BATCH_CASES = {
    'batch_is_not_p_b': dict(batch=98), 'batch_negative': dict(batch=-99), 'batch_above_max': dict(batch=3 * 2 ** 20),
    'state_stride_1099': dict(state_stride=1099), 'state_stride_1098': dict(state_stride=1098), 'null_state': dict(state=None),
    'unaligned_state': dict(state=_FAKE + 4), 'null_next_state': dict(next_state=None), 'unaligned_next_state': dict(next_state=_FAKE + 8),
    'null_ret': dict(ret=None), 'null_discount': dict(discount=None), 'null_action': dict(action=None), 'null_index': dict(index=None),
    'null_index_empty_batch': dict(index=None, batch=0),
}


@pytest.mark.parametrize('case', sorted(_BATCH_CASES))
def test_batch_refusals(case):
  bt = _prio_batch(**_BATCH_CASES[case])
  assert _sample(_replay(), _trees(), bt) == E_INVALID_ARG, case
  assert _set(_replay(), _trees(), bt) == E_INVALID_ARG, case


def test_nulls_and_the_calls_own_arrays():
  rp, tr, bt = _replay(), _trees(), _prio_batch()
  assert _add(None, tr) == E_INVALID_ARG and _add(rp, None) == E_INVALID_ARG
  for bad in (_sample(None, tr, bt), _sample(rp, None, bt), _sample(rp, tr, None), _sample(rp, tr, bt, seeds=None),
              _sample(rp, tr, bt, seeds=_FAKE + 4), _sample(rp, tr, bt, priority=None),
              _set(None, tr, bt), _set(rp, None, bt), _set(rp, tr, None), _set(rp, tr, bt, priority=None), _set(rp, tr, bt, loss=None),
              _set(rp, tr, bt, weighted=None)):
    assert bad == E_INVALID_ARG


# ---- ble_marco_polo_grouped_u8 ---------------------------------------------------------------------------------------------------------
def _marco(action=_FAKE, **fields):
  d = dict(n=195, obs_stride=1099, reserved_=0, members=3, probability=_FAKE, seed=_FAKE, obs=_FAKE, begin=_FAKE, step=_FAKE,
           phase_clock=_FAKE, walk_clock=_FAKE, exploratory_episode=_FAKE, exploratory_phase=_FAKE, target=_FAKE)
  d.update(fields)
  return _lib.lib().ble_marco_polo_grouped_u8(ctypes.byref(_abi.BleMarcoPoloGroupedF32(**d)), action, None)


def test_grouped_marco_polo_refusals():
  assert _marco(n=0) == 0                                            # nothing to launch
  assert _lib.lib().ble_marco_polo_grouped_u8(None, _FAKE, None) == E_INVALID_ARG
  for bad in (_marco(action=None), _marco(n=-3), _marco(n=4 * 2147483647 * 256 + 3), _marco(obs_stride=0), _marco(reserved_=1),
              _marco(members=0), _marco(members=-1), _marco(n=196), _marco(members=2), _marco(probability=None), _marco(seed=None),
              _marco(probability=_FAKE + 4), _marco(seed=_FAKE + 4), _marco(obs=None), _marco(begin=None), _marco(step=None),
              _marco(phase_clock=None), _marco(walk_clock=None), _marco(exploratory_episode=None), _marco(exploratory_phase=None),
              _marco(target=None), _marco(target=_FAKE + 4), _marco(n=0, reserved_=1), _marco(n=0, members=0), _marco(n=0, seed=None)):
    assert bad == E_INVALID_ARG


# ---- the plain and the 3t entry points keep their answers ------------------------------------------------------------------------------
def test_plain_and_grouped_uniform_entry_points_keep_their_answers():
  lib = _lib.lib()
  assert all(hasattr(lib, name) for name in ENTRIES)                  # (in the library that has the grouped entry points)
  solo_rp = _replay(num_envs=R)
  tree = lambda **f: _abi.BleSumTreeF64(**{**dict(leaves=T * R, padded=64, nodes=_FAKE, max_priority=_FAKE), **f})
  add = lambda rp, tr: lib.ble_replay_tree_add_f64(ctypes.byref(rp), ctypes.byref(tr), None)
  sample = lambda rp, tr, bt: lib.ble_replay_sample_prioritized_f32(ctypes.byref(rp), ctypes.byref(tr), ctypes.byref(bt), _FAKE, 5, None, None)
  setp = lambda rp, tr, bt: lib.ble_replay_set_priority_f32(ctypes.byref(rp), ctypes.byref(tr), ctypes.byref(bt), _FAKE, _FAKE, _FAKE, None, None)
  empty = _prio_batch(batch=0)
  assert sample(solo_rp, tree(), empty) == 0 and setp(solo_rp, tree(), empty) == 0
  for bad in (add(solo_rp, tree(leaves=61)), add(solo_rp, tree(padded=128)), add(solo_rp, tree(nodes=None)), add(_replay(), tree()),
              sample(solo_rp, tree(), _prio_batch(batch=0, index=None)), sample(solo_rp, tree(padded=32), empty),
              setp(solo_rp, tree(max_priority=_FAKE + 4), empty), setp(solo_rp, tree(), _prio_batch(batch=-1))):
    assert bad == E_INVALID_ARG
  mp = lambda **f: lib.ble_marco_polo_u8(ctypes.byref(_abi.BleMarcoPoloF32(**{**dict(
      n=0, obs_stride=1099, reserved_=0, exploratory_episode_probability=0.8, seed=3, obs=_FAKE, begin=_FAKE, step=_FAKE, phase_clock=_FAKE,
      walk_clock=_FAKE, exploratory_episode=_FAKE, exploratory_phase=_FAKE, target=_FAKE), **f})), _FAKE, None)
  assert mp() == 0 and mp(exploratory_episode_probability=1.5) == E_INVALID_ARG and mp(n=-1) == E_INVALID_ARG and mp(obs=None) == E_INVALID_ARG
  grouped = lambda rp, bt, members=3, seeds=_FAKE: lib.ble_replay_sample_grouped_f32(ctypes.byref(rp), members, seeds, ctypes.byref(bt), None, None)
  assert grouped(_replay(), _batch()) == 0
  for bad in (grouped(_replay(), _batch(batch=99), members=2), grouped(_replay(), _batch(batch=98)), grouped(_replay(), _batch(batch=99), seeds=None)):
    assert bad == E_INVALID_ARG
  ex = lambda **f: lib.ble_qnet_explore_grouped_u8(ctypes.byref(_abi.BleExploreGroupedF32(**{**dict(
      n=0, members=3, reserved_=0, epsilon=_FAKE, seed=_FAKE, step=7), **f})), _FAKE, None)
  assert ex() == 0 and ex(members=0) == E_INVALID_ARG and ex(n=196) == E_INVALID_ARG and ex(reserved_=1) == E_INVALID_ARG
