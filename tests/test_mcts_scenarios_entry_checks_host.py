"""The guided tree search in scenario winds without a GPU: the two entry points are declared, exported and mirrored; every
refusal the header lists answers BLE_E_INVALID_ARG before any HIP call, with an empty batch and with a non-empty one (no call below has
valid arguments and n > 0, so none launches); n == 0 answers BLE_OK.  The pool, expand and state fixtures are test_mcts_host.py's."""
import ctypes
import os
import re
import subprocess

import pytest

from balloon_learning_environment_amd import _abi, _lib
from descriptors_host import E_INVALID_ARG, _FAKE
from test_mcts_host import _DEFAULT, _EX_BAD, _POOL_BAD, _bad_pool, _ex, _header, _nodes, _pool, _ref, _state, _POOL

ENTRIES = ('ble_mcts_expand_scenarios_f32', 'ble_mcts_backup_scenarios_f32')
_GROUPS = _FAKE + 0x20000


def _scn(**over):
  f = dict(slab=_FAKE, stride=_abi.gp_scenario_doubles(3), n_obs=_FAKE, n=0, num=3, reserved_=0)
  f.update(over)
  f['stride'] = over.get('stride', _abi.gp_scenario_doubles(max(1, min(int(f['num']), _abi.SCENARIO_MAX))))
  return _abi.BleGpScenarios(*(f[k] for k in ('slab', 'stride', 'n_obs', 'n', 'num', 'reserved_')))


def _sgen(**over):
  f = dict(seed=3, env_seed=None, episode=_FAKE, env_offset=0)
  f.update(over)
  return _abi.BleScenarioGen(*(f[k] for k in ('seed', 'env_seed', 'episode', 'env_offset')))


def _expand(pool=_DEFAULT, ex=_DEFAULT, st=_DEFAULT, scn=_DEFAULT, gen=_DEFAULT):
  pool, ex, st = (_pool() if pool is _DEFAULT else pool), (_ex() if ex is _DEFAULT else ex), (_state() if st is _DEFAULT else st)
  scn = _scn(n=pool.n if pool is not None else 0) if scn is _DEFAULT else scn
  gen = _sgen() if gen is _DEFAULT else gen
  return _lib.lib().ble_mcts_expand_scenarios_f32(_ref(st), _ref(pool), _ref(ex), _ref(scn), _ref(gen), None, None)


def _backup(pool=_DEFAULT, round_=1, num=3, tail=2, value=None, probs=None, group_status=_GROUPS, group_g=_GROUPS + 0x1000):
  pool = _pool() if pool is _DEFAULT else pool
  return _lib.lib().ble_mcts_backup_scenarios_f32(_ref(pool), round_, num, tail, value, probs, group_status, group_g, None)


def test_declared_exported_and_mirrored():
  header = _header()
  assert re.search(r'\bint ble_mcts_expand_scenarios_f32\(const ble_state_f32\* st, const struct ble_mcts_pool\* pool, '
                   r'const struct ble_mcts_expand\* ex,\s*const ble_gp_scenarios\* scn, const ble_scenario_gen\* gen, uint32_t\* err_flags, '
                   r'void\* stream\);', header)
  assert re.search(r'\bint ble_mcts_backup_scenarios_f32\(const struct ble_mcts_pool\* pool, int32_t round, int32_t num, int32_t tail, '
                   r'const float\* value,\s*const float\* probs, uint8_t\* group_status, double\* group_g, void\* stream\);', header)
  assert re.search(r'#define BLE_ABI_VERSION 5\b', header) and _lib.ABI_VERSION == 5            # additive: the ABI stays 5
  # the rules stand in the header before the code
  for words in ('STOPPED', 'SPENT', 'VOID', 'never EXPAND', 'G_m = acc_m \\+ disc_m \\* V_m', "ble_plan_risk_f32's order", 'group_status', 'group_g'):
    assert re.search(words, header), words
  symbols = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
  for name in ENTRIES:
    assert name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS, name
    assert re.search(r' T ' + name + r'$', symbols, re.M), name
    fn = getattr(_lib.lib(), name)
    assert fn.argtypes is not None and fn.restype is ctypes.c_int
    assert not any(issubclass(t, ctypes.c_int64) for t in fn.argtypes if isinstance(t, type)), name      # every size travels in a struct


def test_empty_batch_is_ok_without_a_launch():
  for r in (0, 3):
    assert _expand(ex=_ex(round=r)) == _lib.BLE_OK and _backup(round_=r) == _lib.BLE_OK
  for num in (1, 16):
    assert _expand(scn=_scn(num=num)) == _lib.BLE_OK
    for tail in (1, num):
      assert _backup(num=num, tail=tail) == _lib.BLE_OK
  assert _backup(value=_FAKE, probs=_FAKE) == _lib.BLE_OK
  assert _expand(gen=_sgen(env_seed=_FAKE)) == _lib.BLE_OK and _expand(gen=_sgen(episode=None)) == _lib.BLE_OK
  assert _expand(_pool(max_depth=6, segment=40), _ex(action_repeat=4, gamma=0.0)) == _lib.BLE_OK      # 960 agent steps


# a pool whose n * cap is in range and whose n * 3L * num is not: n = 2^23, L = 16, R = 1 (cap = 49), num = 8 -> 2^23 * 48 * 8 = 2^31.5
_WIDE = dict(n=2 ** 23, num_rounds=1, leaves_per_round=16)

_CASES = {
    **{f'{call.__name__[1:]}_pool_{k}': (lambda n, k=k, call=call: call(_bad_pool(k, n))) for k in _POOL_BAD for call in (_expand, _backup)},
    **{f'{call.__name__[1:]}_null_pool': (lambda n, call=call: call(None)) for call in (_expand, _backup)},
    # -- expand: what ble_mcts_expand_f32 refuses of st and ex
    **{f'expand_{k}': (lambda n, k=k: _expand(_pool(n=n), _ex(**_EX_BAD[k]))) for k in _EX_BAD},
    'expand_null_struct': lambda n: _expand(_pool(n=n), None),
    'expand_null_state': lambda n: _expand(_pool(n=n), st=None),
    'expand_null_state_array': lambda n: _expand(_pool(n=n), st=_state(null='pressure')),
    'expand_bad_vehicle': lambda n: _expand(_pool(n=n), st=_state(vehicle=_abi.vehicle_struct(envelope_mass=-1.0))),
    'expand_nodes_array_is_the_sources': lambda n: _expand(_pool(n=n, nodes=_nodes(state=_state(_POOL, same='x')))),
    'expand_nodes_are_the_source': lambda n: _expand(_pool(n=n, nodes=_nodes(state=_state(_FAKE)))),
    # -- expand: what ble_gp_fit_scenarios_f32 refuses of scn and gen, and a slab of another batch
    'expand_null_scn': lambda n: _expand(_pool(n=n), scn=None),
    'expand_null_gen': lambda n: _expand(_pool(n=n), gen=None),
    'expand_scn_null_slab': lambda n: _expand(_pool(n=n), scn=_scn(n=n, slab=None)),
    'expand_scn_null_n_obs': lambda n: _expand(_pool(n=n), scn=_scn(n=n, n_obs=None)),
    'expand_scn_num_0': lambda n: _expand(_pool(n=n), scn=_scn(n=n, num=0)),
    'expand_scn_num_17': lambda n: _expand(_pool(n=n), scn=_scn(n=n, num=17)),
    'expand_scn_short_stride': lambda n: _expand(_pool(n=n), scn=_scn(n=n, stride=_abi.gp_scenario_doubles(3) - 2)),
    'expand_scn_odd_stride': lambda n: _expand(_pool(n=n), scn=_scn(n=n, stride=_abi.gp_scenario_doubles(3) + 1)),
    'expand_scn_unaligned_slab': lambda n: _expand(_pool(n=n), scn=_scn(n=n, slab=_FAKE + 8)),
    'expand_scn_negative_n': lambda n: _expand(_pool(n=n), scn=_scn(n=-1)),
    'expand_scn_of_another_batch': lambda n: _expand(_pool(n=n), scn=_scn(n=n + 1)),
    'expand_gen_negative_offset': lambda n: _expand(_pool(n=n), gen=_sgen(env_offset=-1)),
    'expand_nodes_2_31': lambda n: _expand(_pool(**_WIDE), scn=_scn(n=_WIDE['n'], num=8)),
    # -- backup
    'backup_round_negative': lambda n: _backup(_pool(n=n), round_=-1),
    'backup_round_4': lambda n: _backup(_pool(n=n), round_=4),
    'backup_value_without_probs': lambda n: _backup(_pool(n=n), value=_FAKE),
    'backup_probs_without_value': lambda n: _backup(_pool(n=n), probs=_FAKE),
    'backup_num_0': lambda n: _backup(_pool(n=n), num=0, tail=1),
    'backup_num_negative': lambda n: _backup(_pool(n=n), num=-3, tail=1),
    'backup_num_17': lambda n: _backup(_pool(n=n), num=17, tail=1),
    'backup_tail_0': lambda n: _backup(_pool(n=n), tail=0),
    'backup_tail_negative': lambda n: _backup(_pool(n=n), tail=-1),
    'backup_tail_above_num': lambda n: _backup(_pool(n=n), num=3, tail=4),
    'backup_null_group_status': lambda n: _backup(_pool(n=n), group_status=None),
    'backup_null_group_g': lambda n: _backup(_pool(n=n), group_g=None),
    'backup_nodes_2_31': lambda n: _backup(_pool(**_WIDE), round_=0, num=8),
}


def test_the_wide_pool_is_refused_for_its_nodes_alone():
  """_WIDE with one scenario is a pool the plain calls take (n * cap < 2^31): only n * 3L * num refuses it.  n > 0, so a valid call would
  launch: the plain backup is NOT called here, the sizes are checked by hand."""
  assert _WIDE['n'] * (1 + 3 * _WIDE['leaves_per_round'] * _WIDE['num_rounds']) < 2 ** 31 <= _WIDE['n'] * 3 * _WIDE['leaves_per_round'] * 8
  assert _WIDE['n'] * 3 * _WIDE['leaves_per_round'] * 5 < 2 ** 31


@pytest.mark.parametrize('n', [0, 64])
@pytest.mark.parametrize('case', sorted(_CASES))
def test_invalid_argument(case, n):
  assert _CASES[case](n) == E_INVALID_ARG
