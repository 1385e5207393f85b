"""The guided tree search without a GPU: the four entry points are declared, exported and mirrored; every refusal the header
lists answers BLE_E_INVALID_ARG before any HIP call, with an empty batch and with a non-empty one (no call below has valid arguments and
n > 0, so none launches); n == 0 answers BLE_OK."""
import ctypes
import os
import re
import subprocess

import pytest

from balloon_learning_environment_amd import _abi, _lib
from descriptors_host import E_INVALID_ARG, _FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')
ENTRIES = ('ble_mcts_select_f32', 'ble_mcts_expand_f32', 'ble_mcts_backup_f32', 'ble_mcts_finish_f32')
_POOL = _FAKE + 0x10000          # the pool's node arrays: not the source's
_STATS = ('parent', 'first_child', 'depth', 'visits', 'pending', 'value_sum', 'g', 'prior', 'g_range', 'leaf', 'kind')


def _header():
  return open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()


def _ref(x):
  return ctypes.byref(x) if x is not None else None


def _state(address=_FAKE, null=None, vehicle=None, same=None):
  fields = {name: 0 if name == null else (_FAKE if name == same else address) for name in _abi.FIELD_NAMES}
  return _abi.state_struct(fields, 0, vehicle)


_KEEP = []        # the states the arena structs point at


def _nodes(state='default', **over):
  st = _state(_POOL) if state == 'default' else state
  _KEEP.append(st)
  f = dict(state=ctypes.pointer(st) if st is not None else None, acc=_POOL + 0x1000, disc=_POOL + 0x2000, flown=_POOL + 0x3000,
           ret=_POOL + 0x4000)
  f.update(over)
  return _abi.BleTreeArena(**{k: v for k, v in f.items() if v is not None})


def _pool(**over):
  f = dict(n=0, num_rounds=4, leaves_per_round=2, max_depth=3, segment=2, reserved_=0, nodes=_nodes(),
           **{name: _FAKE + 0x100 * (k + 1) for k, name in enumerate(_STATS)})
  f.update(over)
  return _abi.BleMctsPool(**{k: v for k, v in f.items() if v is not None})


def _ex(**over):
  f = dict(round=1, action_repeat=1, substeps=18, reserved_=0, gamma=0.993, wind_grid=_FAKE, grid_env_stride=0)
  f.update(over)
  return _abi.BleMctsExpand(**{k: v for k, v in f.items() if v is not None})


def _fin(**over):
  f = dict(source_status=_FAKE, best_plan=_FAKE, action=_FAKE, best_return=_FAKE, q=_FAKE, visits=_FAKE, pv_length=_FAKE)
  f.update(over)
  return _abi.BleMctsFinish(**{k: v for k, v in f.items() if v is not None})


def _belief(**over):
  f = dict(slab=_FAKE, stride=720, n_obs=_FAKE, n=0)
  f.update(over)
  return _abi.BleGpBelief(**f)


def _gen(**over):
  f = dict(seed=3, episode=_FAKE, harmonic_cache=None, env_offset=0)
  f.update(over)
  return _abi.BleNoiseGen(**f)


_DEFAULT = object()


def _select(pool=_DEFAULT, round_=1, c_puct=1.25, status=_FAKE, prior=None):
  pool = _pool() if pool is _DEFAULT else pool
  return _lib.lib().ble_mcts_select_f32(_ref(pool), round_, c_puct, status, prior, None)


def _expand(pool=_DEFAULT, ex=_DEFAULT, st=_DEFAULT, noise=None, belief=None):
  pool, ex, st = (_pool() if pool is _DEFAULT else pool), (_ex() if ex is _DEFAULT else ex), (_state() if st is _DEFAULT else st)
  return _lib.lib().ble_mcts_expand_f32(_ref(st), _ref(pool), _ref(ex), _ref(noise), _ref(belief), None, None)


def _backup(pool=_DEFAULT, round_=1, value=None, probs=None):
  pool = _pool() if pool is _DEFAULT else pool
  return _lib.lib().ble_mcts_backup_f32(_ref(pool), round_, value, probs, None)


def _finish(pool=_DEFAULT, fin=_DEFAULT):
  pool, fin = (_pool() if pool is _DEFAULT else pool), (_fin() if fin is _DEFAULT else fin)
  return _lib.lib().ble_mcts_finish_f32(_ref(pool), _ref(fin), None)


# ---- declared, exported, mirrored ----------------------------------------------------------------------------------------------------
def test_declared_exported_and_mirrored():
  header = _header()
  assert re.search(r'\bint ble_mcts_select_f32\(const struct ble_mcts_pool\* pool, int32_t round, double c_puct, const uint8_t\* source_status, '
                   r'const float\* root_prior,\s*void\* stream\);', header)
  assert re.search(r'\bint ble_mcts_expand_f32\(const ble_state_f32\* st, const struct ble_mcts_pool\* pool, const struct ble_mcts_expand\* ex, '
                   r'const ble_noise_gen\* noise,\s*const ble_gp_belief\* belief, uint32_t\* err_flags, void\* stream\);', header)
  assert re.search(r'\bint ble_mcts_backup_f32\(const struct ble_mcts_pool\* pool, int32_t round, const float\* value, const float\* probs, '
                   r'void\* stream\);', header)
  assert re.search(r'\bint ble_mcts_finish_f32\(const struct ble_mcts_pool\* pool, const struct ble_mcts_finish\* fin, void\* stream\);', header)
  assert re.search(r'#define BLE_MCTS_MAX_LEAVES 256\b', header) and _abi.MCTS_MAX_LEAVES == 256
  for name, value in (('EMPTY', _abi.MCTS_EMPTY), ('EXPAND', _abi.MCTS_EXPAND), ('REVISIT', _abi.MCTS_REVISIT)):
    assert re.search(r'#define BLE_MCTS_%s %d\b' % (name, value), header)
  assert re.search(r'#define BLE_ABI_VERSION 5\b', header) and _lib.ABI_VERSION == 5            # additive: the ABI stays 5
  symbols = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
  for name in ENTRIES:
    assert name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS, name
    assert re.search(r' T ' + name + r'$', symbols, re.M), name
    fn = getattr(_lib.lib(), name)
    assert fn.argtypes is not None and fn.restype is ctypes.c_int
    assert not any(issubclass(t, ctypes.c_int64) for t in fn.argtypes if isinstance(t, type)), name      # every size travels in a struct


_C_SIZES = {'int64_t': 8, 'int32_t': 4, 'double': 8, 'struct ble_tree_arena': 40}


@pytest.mark.parametrize('tag, mirror, size', [('ble_mcts_pool', _abi.BleMctsPool, 160), ('ble_mcts_expand', _abi.BleMctsExpand, 40),
                                               ('ble_mcts_finish', _abi.BleMctsFinish, 56)])
def test_struct_layout_matches_the_header(tag, mirror, size):
  body = re.search(r'struct ' + tag + r' \{(.*?)\n\}', _header(), re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  declared = [d.strip() for d in body.split(';') if d.strip()]
  names = [re.search(r'(\w+)\s*$', d).group(1) for d in declared]
  assert names == [f[0] for f in mirror._fields_]
  offset = 0                    # the header's own size: every member at its natural alignment (pointers 8 bytes)
  for d, name in zip(declared, names):
    kind = d[:d.rindex(name)].strip()
    width = 8 if kind.endswith('*') else _C_SIZES[kind]
    offset = -(-offset // min(width, 8)) * min(width, 8)
    assert getattr(mirror, name).offset == offset, (tag, name)
    offset += width
  assert ctypes.sizeof(mirror) == -(-offset // 8) * 8 == size


# ---- empty batches -------------------------------------------------------------------------------------------------------------------
def test_empty_batch_is_ok_without_a_launch():
  for r in (0, 3):
    assert _select(round_=r) == _lib.BLE_OK and _backup(round_=r) == _lib.BLE_OK and _expand(ex=_ex(round=r)) == _lib.BLE_OK
  assert _select(prior=_FAKE, c_puct=0.0) == _lib.BLE_OK
  assert _backup(value=_FAKE, probs=_FAKE) == _lib.BLE_OK
  assert _expand(noise=_gen()) == _lib.BLE_OK and _expand(belief=_belief()) == _lib.BLE_OK
  assert _finish() == _lib.BLE_OK
  big = dict(num_rounds=32, leaves_per_round=8, max_depth=240, segment=4)                    # L R = 256, 960 plan entries
  assert _select(_pool(**big), round_=31) == _lib.BLE_OK and _finish(_pool(**big)) == _lib.BLE_OK
  assert _expand(_pool(max_depth=6, segment=40), _ex(action_repeat=4, gamma=0.0)) == _lib.BLE_OK      # 960 agent steps


# ---- invalid arguments ---------------------------------------------------------------------------------------------------------------
_POOL_BAD = {                   # what all four calls refuse of the pool
    **{f'null_{name}': {name: None} for name in _STATS},
    'null_nodes_state': lambda: dict(nodes=_nodes(state=None)), 'null_nodes_array': lambda: dict(nodes=_nodes(state=_state(_POOL, null='y'))),
    'null_nodes_constant': lambda: dict(nodes=_nodes(state=_state(_POOL, null='start_unix'))),
    'null_nodes_acc': lambda: dict(nodes=_nodes(acc=0)), 'null_nodes_disc': lambda: dict(nodes=_nodes(disc=0)),
    'null_nodes_flown': lambda: dict(nodes=_nodes(flown=0)), 'null_nodes_ret': lambda: dict(nodes=_nodes(ret=0)),
    'negative_n': dict(n=-1), 'n_times_cap_2_31': dict(n=2 ** 27),
    'rounds_0': dict(num_rounds=0), 'rounds_negative': dict(num_rounds=-4), 'leaves_0': dict(leaves_per_round=0),
    'leaves_times_rounds_257': dict(num_rounds=1, leaves_per_round=257), 'leaves_times_rounds_260': dict(num_rounds=20, leaves_per_round=13),
    'depth_0': dict(max_depth=0), 'segment_0': dict(segment=0), 'plan_961': dict(max_depth=31, segment=31), 'reserved': dict(reserved_=1),
}


def _bad_pool(k, n):
  over = _POOL_BAD[k]() if callable(_POOL_BAD[k]) else _POOL_BAD[k]
  return _pool(**{'n': n, **over})


_EX_BAD = {
    'null_grid': dict(wind_grid=None), 'round_negative': dict(round=-1), 'round_4': dict(round=4), 'repeat_0': dict(action_repeat=0),
    'steps_times_repeat_966': dict(action_repeat=161), 'substeps_0': dict(substeps=0), 'substeps_huge': dict(substeps=10 ** 6),
    'reserved': dict(reserved_=1), 'negative_grid_stride': dict(grid_env_stride=-1),
    'gamma_nan': dict(gamma=NAN), 'gamma_negative': dict(gamma=-0.1), 'gamma_above_1': dict(gamma=1.0001), 'gamma_inf': dict(gamma=INF),
}

_CASES = {
    **{f'{call.__name__[1:]}_pool_{k}': (lambda n, k=k, call=call: call(_bad_pool(k, n))) for k in _POOL_BAD
       for call in (_select, _expand, _backup, _finish)},
    **{f'{call.__name__[1:]}_null_pool': (lambda n, call=call: call(None)) for call in (_select, _expand, _backup, _finish)},
    # -- select
    'select_round_negative': lambda n: _select(_pool(n=n), round_=-1),
    'select_round_4': lambda n: _select(_pool(n=n), round_=4),
    'select_null_status': lambda n: _select(_pool(n=n), status=None),
    'select_c_puct_nan': lambda n: _select(_pool(n=n), c_puct=NAN),
    'select_c_puct_inf': lambda n: _select(_pool(n=n), c_puct=INF),
    'select_c_puct_negative': lambda n: _select(_pool(n=n), c_puct=-0.5),
    # -- expand
    **{f'expand_{k}': (lambda n, k=k: _expand(_pool(n=n), _ex(**_EX_BAD[k]))) for k in _EX_BAD},
    'expand_null_struct': lambda n: _expand(_pool(n=n), None),
    'expand_null_state': lambda n: _expand(_pool(n=n), st=None),
    'expand_null_state_array': lambda n: _expand(_pool(n=n), st=_state(null='pressure')),
    'expand_both_winds': lambda n: _expand(_pool(n=n), noise=_gen(), belief=_belief(n=n)),
    'expand_negative_noise_offset': lambda n: _expand(_pool(n=n), noise=_gen(env_offset=-1)),
    'expand_bad_vehicle': lambda n: _expand(_pool(n=n), st=_state(vehicle=_abi.vehicle_struct(envelope_mass=-1.0))),
    'expand_belief_of_another_batch': lambda n: _expand(_pool(n=n), belief=_belief(n=n + 1)),
    'expand_belief_null_slab': lambda n: _expand(_pool(n=n), belief=_belief(n=n, slab=None)),
    'expand_belief_short_stride': lambda n: _expand(_pool(n=n), belief=_belief(n=n, stride=718)),
    'expand_nodes_array_is_the_sources': lambda n: _expand(_pool(n=n, nodes=_nodes(state=_state(_POOL, same='x')))),
    'expand_nodes_are_the_source': lambda n: _expand(_pool(n=n, nodes=_nodes(state=_state(_FAKE)))),
    # -- backup
    'backup_round_negative': lambda n: _backup(_pool(n=n), round_=-1),
    'backup_round_4': lambda n: _backup(_pool(n=n), round_=4),
    'backup_value_without_probs': lambda n: _backup(_pool(n=n), value=_FAKE),
    'backup_probs_without_value': lambda n: _backup(_pool(n=n), probs=_FAKE),
    # -- finish
    'finish_null_struct': lambda n: _finish(_pool(n=n), None),
    **{f'finish_null_{f}': (lambda n, f=f: _finish(_pool(n=n), _fin(**{f: None})))
       for f in ('source_status', 'best_plan', 'action', 'best_return', 'q', 'visits', 'pv_length')},
}


@pytest.mark.parametrize('n', [0, 64])
@pytest.mark.parametrize('case', sorted(_CASES))
def test_invalid_argument(case, n):
  assert _CASES[case](n) == E_INVALID_ARG
