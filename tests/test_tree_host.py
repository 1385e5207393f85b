"""The beam search without a GPU: the three entry points are declared, exported and mirrored; every refusal answers
BLE_E_INVALID_ARG before any HIP call, with an empty batch and with a non-empty one (no call below has valid arguments and n > 0, so
none launches); and the select and finish lane functions of csrc/ble_tree.h, built for the host (tests/emul/tree_emul.cpp), equal the
NumPy twin (tests/tree_host.py) on crafted returns.  No tolerance anywhere: integers and bits."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import tree_host
from balloon_learning_environment_amd import _abi, _lib
from descriptors_host import E_INVALID_ARG, _FAKE
from emul import tree_emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')
ENTRIES = ('ble_tree_expand_f32', 'ble_tree_select_f32', 'ble_tree_finish_f32')
_SRC, _DST = _FAKE + 0x10000, _FAKE + 0x20000        # the two arenas' arrays: not the source's, not each other's


def _header():
  return open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()


def _ref(x):
  return ctypes.byref(x) if x is not None else None


def _state(address=_FAKE, null=None, vehicle=None, same=None, same_as=_FAKE):
  fields = {name: 0 if name == null else (same_as if name == same else address) for name in _abi.FIELD_NAMES}
  return _abi.state_struct(fields, 0, vehicle)


_KEEP = []        # the states the arena structs point at


def _arena(address, state='default', **over):
  st = _state(address) if state == 'default' else state
  _KEEP.append(st)
  f = dict(state=ctypes.pointer(st) if st is not None else None, acc=address + 0x1000, disc=address + 0x2000, flown=address + 0x3000,
           ret=address + 0x4000)
  f.update(over)
  return _abi.BleTreeArena(**{k: v for k, v in f.items() if v is not None})


def _ex(level=2, **over):
  """A valid descriptor of level 1 (the parents are st's environments) or of a later level."""
  f = dict(n=0, beam=4, depth=3, n_parents=1 if level == 1 else 3, parent_children=0 if level == 1 else 3, segment=2, action_repeat=1,
           substeps=18, reserved_=0, gamma=0.993, wind_grid=_FAKE, grid_env_stride=0, parent=None if level == 1 else _FAKE,
           src=_abi.BleTreeArena() if level == 1 else _arena(_SRC), dst=_arena(_DST))
  f.update(over)
  return _abi.BleTreeExpand(**f)


def _belief(**over):
  f = dict(slab=_FAKE, stride=720, n_obs=_FAKE, n=0)
  f.update(over)
  return _abi.BleGpBelief(**f)


def _gen(**over):
  f = dict(seed=3, episode=_FAKE, harmonic_cache=None, env_offset=0)
  f.update(over)
  return _abi.BleNoiseGen(**f)


_DEFAULT = object()


def _expand(ex=_DEFAULT, st=_DEFAULT, noise=None, belief=None):
  st = _state() if st is _DEFAULT else st
  ex = _ex() if ex is _DEFAULT else ex
  return _lib.lib().ble_tree_expand_f32(_ref(st), _ref(ex), _ref(noise), _ref(belief), None, None)


def _sel(**over):
  f = dict(n=0, n_children=9, beam=4, ret=_FAKE, parent=_FAKE, choice=_FAKE)
  f.update(over)
  return _abi.BleTreeSelect(**f)


def _fin(**over):
  f = dict(n=0, n_children=12, beam=4, depth=3, segment=2, ret=_FAKE, score=None, source_status=_FAKE, choice=_FAKE, best_plan=_FAKE,
           action=_FAKE, best_return=_FAKE, q=None, visits=None)
  f.update(over)
  return _abi.BleTreeFinish(**f)


def _select(s):
  return _lib.lib().ble_tree_select_f32(_ref(s), None)


def _finish(f):
  return _lib.lib().ble_tree_finish_f32(_ref(f), None)


# ---- declared, exported, mirrored ----------------------------------------------------------------------------------------------------
def test_declared_exported_and_mirrored():
  header = _header()
  assert re.search(r'\bint ble_tree_expand_f32\(const ble_state_f32\* st, const struct ble_tree_expand\* ex, const ble_noise_gen\* noise, '
                   r'const ble_gp_belief\* belief,\s*uint32_t\* err_flags, void\* stream\);', header)
  assert re.search(r'\bint ble_tree_select_f32\(const struct ble_tree_select\* sel, void\* stream\);', header)
  assert re.search(r'\bint ble_tree_finish_f32\(const struct ble_tree_finish\* fin, void\* stream\);', header)
  assert re.search(r'#define BLE_TREE_MAX_BEAM 256\b', header) and _abi.TREE_MAX_BEAM == 256
  assert re.search(r'#define BLE_ABI_VERSION 5\b', header) and _lib.ABI_VERSION == 5            # additive: the ABI stays 5
  symbols = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
  for name in ENTRIES:
    assert name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS, name
    assert re.search(r' T ' + name + r'$', symbols, re.M), name
    fn = getattr(_lib.lib(), name)
    assert fn.argtypes is not None and fn.restype is ctypes.c_int
    assert not any(issubclass(t, ctypes.c_int64) for t in fn.argtypes if isinstance(t, type)), name      # every size travels in a struct


_C_SIZES = {'int64_t': 8, 'int32_t': 4, 'double': 8, 'struct ble_tree_arena': 40}


@pytest.mark.parametrize('tag, mirror, size', [('ble_tree_arena', _abi.BleTreeArena, 40), ('ble_tree_expand', _abi.BleTreeExpand, 152),
                                               ('ble_tree_select', _abi.BleTreeSelect, 40), ('ble_tree_finish', _abi.BleTreeFinish, 96)])
def test_struct_layout_matches_the_header(tag, mirror, size):
  body = re.search(r'struct ' + tag + r' \{(.*?)\n\}', _header(), re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  declared = [d.strip() for d in body.split(';') if d.strip()]
  names = [re.search(r'(\w+)\s*$', d).group(1) for d in declared]
  assert names == [f[0] for f in mirror._fields_]
  # the header's own size: every member at its natural alignment (pointers 8 bytes)
  offset = 0
  for d, name in zip(declared, names):
    kind = d[:d.rindex(name)].strip()
    width = 8 if kind.endswith('*') else _C_SIZES[kind]
    offset = -(-offset // min(width, 8)) * min(width, 8)
    assert getattr(mirror, name).offset == offset, (tag, name)
    offset += width
  assert ctypes.sizeof(mirror) == -(-offset // 8) * 8 == size


# ---- empty batches -------------------------------------------------------------------------------------------------------------------
def test_empty_batch_is_ok_without_a_launch():
  assert _expand(_ex(level=1)) == _lib.BLE_OK
  assert _expand() == _lib.BLE_OK
  assert _expand(noise=_gen()) == _lib.BLE_OK
  assert _expand(belief=_belief()) == _lib.BLE_OK
  assert _expand(_ex(beam=256, n_parents=256, parent_children=768, depth=8, segment=4)) == _lib.BLE_OK
  assert _expand(_ex(beam=1, n_parents=1, parent_children=3, depth=960, segment=1)) == _lib.BLE_OK
  assert _expand(_ex(depth=6, segment=40, action_repeat=4, gamma=0.0)) == _lib.BLE_OK               # 960 agent steps
  assert _select(_sel()) == _lib.BLE_OK
  assert _select(_sel(n_children=768, beam=256)) == _lib.BLE_OK
  assert _select(_sel(n_children=3, beam=1)) == _lib.BLE_OK
  assert _finish(_fin()) == _lib.BLE_OK
  assert _finish(_fin(score=_FAKE, q=_FAKE, visits=_FAKE)) == _lib.BLE_OK
  assert _finish(_fin(depth=1, n_children=3)) == _lib.BLE_OK
  assert _finish(_fin(depth=240, segment=4)) == _lib.BLE_OK


# ---- invalid arguments ---------------------------------------------------------------------------------------------------------------
_EX_BAD = {                     # what ble_tree_expand_f32 refuses of its struct at a later level
    'null_grid': dict(wind_grid=None), 'null_parent': dict(parent=None),
    'negative_n': dict(n=-1), 'n_times_3_beam_2_31': dict(n=2 ** 29),
    'beam_0': dict(beam=0), 'beam_negative': dict(beam=-4), 'beam_257': dict(beam=257, n_parents=3),
    'segment_0': dict(segment=0), 'repeat_0': dict(action_repeat=0), 'depth_0': dict(depth=0),
    'steps_961': dict(depth=31, segment=31), 'steps_times_repeat_962': dict(depth=13, segment=37, action_repeat=2),
    'substeps_0': dict(substeps=0), 'substeps_huge': dict(substeps=10 ** 6), 'negative_grid_stride': dict(grid_env_stride=-1),
    'gamma_nan': dict(gamma=NAN), 'gamma_negative': dict(gamma=-0.1), 'gamma_above_1': dict(gamma=1.0001), 'gamma_inf': dict(gamma=INF),
    'reserved': dict(reserved_=1),
    'parents_0': dict(n_parents=0), 'parents_above_beam': dict(n_parents=5, parent_children=9),
    'parents_above_children': dict(n_parents=4, parent_children=3), 'children_not_3k': dict(parent_children=4),
    'children_above_3_beam': dict(parent_children=15), 'children_negative': dict(parent_children=-3),
}
_LATER = {                      # the arenas of a later level
    'null_src_state': lambda: dict(src=_arena(_SRC, state=None)), 'null_src_array': lambda: dict(src=_arena(_SRC, state=_state(_SRC, null='y'))),
    'null_src_acc': lambda: dict(src=_arena(_SRC, acc=0)), 'null_src_disc': lambda: dict(src=_arena(_SRC, disc=0)),
    'null_src_flown': lambda: dict(src=_arena(_SRC, flown=0)),
    'null_dst_state': lambda: dict(dst=_arena(_DST, state=None)),
    'null_dst_array': lambda: dict(dst=_arena(_DST, state=_state(_DST, null='last_command'))),
    'null_dst_constant': lambda: dict(dst=_arena(_DST, state=_state(_DST, null='start_unix'))),
    'null_dst_acc': lambda: dict(dst=_arena(_DST, acc=0)), 'null_dst_disc': lambda: dict(dst=_arena(_DST, disc=0)),
    'null_dst_flown': lambda: dict(dst=_arena(_DST, flown=0)), 'null_dst_ret': lambda: dict(dst=_arena(_DST, ret=0)),
    'dst_array_is_the_sources': lambda: dict(dst=_arena(_DST, state=_state(_DST, same='x'))),
    'dst_status_is_the_sources': lambda: dict(dst=_arena(_DST, state=_state(_DST, same='status'))),
    'dst_is_the_source': lambda: dict(dst=_arena(_FAKE)),
    'dst_array_is_srcs': lambda: dict(dst=_arena(_DST, state=_state(_DST, same='pressure', same_as=_SRC))),
    'dst_is_src': lambda: dict(dst=_arena(_SRC)),
    'dst_acc_is_srcs': lambda: dict(dst=_arena(_DST, acc=_SRC + 0x1000)),
}

_CASES = {
    **{f'expand_{k}': (lambda n, k=k: _expand(_ex(**{'n': n, **_EX_BAD[k]}))) for k in _EX_BAD},
    **{f'expand_{k}': (lambda n, k=k: _expand(_ex(n=n, **_LATER[k]()))) for k in _LATER},
    'expand_null_state': lambda n: _expand(_ex(n=n), st=None),
    'expand_null_state_array': lambda n: _expand(_ex(n=n), st=_state(null='pressure')),
    'expand_null_struct': lambda n: _expand(None),
    'expand_both_winds': lambda n: _expand(_ex(n=n), noise=_gen(), belief=_belief(n=n)),
    'expand_negative_noise_offset': lambda n: _expand(_ex(n=n), noise=_gen(env_offset=-1)),
    'expand_bad_vehicle': lambda n: _expand(_ex(n=n), st=_state(vehicle=_abi.vehicle_struct(envelope_mass=-1.0))),
    'expand_belief_of_another_batch': lambda n: _expand(_ex(n=n), belief=_belief(n=n + 1)),
    'expand_belief_null_slab': lambda n: _expand(_ex(n=n), belief=_belief(n=n, slab=None)),
    'expand_belief_short_stride': lambda n: _expand(_ex(n=n), belief=_belief(n=n, stride=718)),
    'expand_belief_misaligned_slab': lambda n: _expand(_ex(n=n), belief=_belief(n=n, slab=_FAKE + 8)),
    'expand_level_1_two_parents': lambda n: _expand(_ex(level=1, n=n, n_parents=2)),
    'expand_level_1_dst_is_the_source': lambda n: _expand(_ex(level=1, n=n, dst=_arena(_FAKE))),
    'expand_level_1_null_dst_ret': lambda n: _expand(_ex(level=1, n=n, dst=_arena(_DST, ret=0))),
    'expand_level_1_steps_961': lambda n: _expand(_ex(level=1, n=n, depth=961, segment=1)),
    # -- select
    'select_null_struct': lambda n: _lib.lib().ble_tree_select_f32(None, None),
    **{f'select_null_{f}': (lambda n, f=f: _select(_sel(n=n, **{f: None}))) for f in ('ret', 'parent', 'choice')},
    'select_negative_n': lambda n: _select(_sel(n=-1)),
    'select_n_times_3_beam_2_31': lambda n: _select(_sel(n=2 ** 29)),
    'select_beam_0': lambda n: _select(_sel(n=n, beam=0)),
    'select_beam_257': lambda n: _select(_sel(n=n, beam=257)),
    'select_children_0': lambda n: _select(_sel(n=n, n_children=0)),
    'select_children_not_3k': lambda n: _select(_sel(n=n, n_children=10)),
    'select_children_above_3_beam': lambda n: _select(_sel(n=n, n_children=15)),
    # -- finish
    'finish_null_struct': lambda n: _lib.lib().ble_tree_finish_f32(None, None),
    **{f'finish_null_{f}': (lambda n, f=f: _finish(_fin(n=n, **{f: None})))
       for f in ('ret', 'source_status', 'choice', 'best_plan', 'action', 'best_return')},
    'finish_q_without_visits': lambda n: _finish(_fin(n=n, q=_FAKE)),
    'finish_visits_without_q': lambda n: _finish(_fin(n=n, visits=_FAKE)),
    'finish_negative_n': lambda n: _finish(_fin(n=-1)),
    'finish_n_times_3_beam_2_31': lambda n: _finish(_fin(n=2 ** 29)),
    'finish_beam_0': lambda n: _finish(_fin(n=n, beam=0)),
    'finish_beam_257': lambda n: _finish(_fin(n=n, beam=257)),
    'finish_children_not_3k': lambda n: _finish(_fin(n=n, n_children=11)),
    'finish_children_above_3_beam': lambda n: _finish(_fin(n=n, n_children=15)),
    'finish_depth_0': lambda n: _finish(_fin(n=n, depth=0)),
    'finish_segment_0': lambda n: _finish(_fin(n=n, segment=0)),
    'finish_plan_961': lambda n: _finish(_fin(n=n, depth=31, segment=31)),
    'finish_depth_1_nine_children': lambda n: _finish(_fin(n=n, depth=1, n_children=9)),
}


@pytest.mark.parametrize('n', [0, 64])
@pytest.mark.parametrize('case', sorted(_CASES))
def test_invalid_argument(case, n):
  assert _CASES[case](n) == E_INVALID_ARG


# ---- the lane functions against the twin ----------------------------------------------------------------------------------------------
def _crafted(rng, C):
  """C returns with many exact ties, both zeros, both infinities and NaN."""
  pool = np.array([0.0, -0.0, 1.5, 1.5, -1.5, 3.25, INF, -INF, NAN, 1e-38, -1e-38, 2.0 ** -149, 7.0], np.float32)
  ret = rng.choice(pool, C)
  ret[rng.random(C) < 0.15] = np.float32(rng.standard_normal())
  return ret.astype(np.float32)


@pytest.mark.parametrize('beam', [1, 4, 27, 256])
@pytest.mark.parametrize('C', [3, 9, 12, 81, 195, 768])
def test_select_equals_the_twin(C, beam):
  if C > 3 * beam:
    return                                       # (not a level of any tree: the entry point refuses it, above)
  rng = np.random.default_rng(100 * C + beam)
  cases = [_crafted(rng, C) for _ in range(6)]
  cases += [np.zeros(C, np.float32), np.full(C, NAN, np.float32), np.where(np.arange(C) % 2 == 0, np.float32(0.0), np.float32(-0.0)),
            np.where(np.arange(C) % 3 == 0, np.float32(2.0), np.float32(NAN)),          # every parent dead: the a = 0 chain and two voids
            np.arange(C, dtype=np.float32), -np.arange(C, dtype=np.float32)]
  for ret in cases:
    want = tree_host.select(ret[None], beam)[0]
    parent, choice = tree_emul.select(ret, beam)
    assert np.array_equal(parent, want) and np.array_equal(choice, want)
    assert len(set(want.tolist())) == len(want) and want.min() >= 0 and want.max() < C


def _grow(rng, depth, beam, kind):
  """A whole search on crafted returns, one environment: per level the children's returns made from the parents' by the tree's own rules
  -- a void parent's children are void, a dead parent's a = 0 child carries its return and the other two are void -- selected by the twin.
  -> (ret of the last level [C], choice [depth, beam] int32, dead flags of the last level)."""
  choice = np.zeros((depth, beam), np.int32)
  parent_ret, parent_dead = np.zeros(1, np.float32), np.array([kind == 'all_dead'])
  for level, (P, C) in enumerate(tree_host.level_sizes(depth, beam), 1):
    ret, dead = np.empty(C, np.float32), np.empty(C, bool)
    fresh = _crafted(rng, C)
    for r in range(P):
      for a in range(3):
        c = 3 * r + a
        if np.isnan(parent_ret[r]):
          ret[c], dead[c] = NAN, True
        elif parent_dead[r]:
          ret[c], dead[c] = (parent_ret[r] if a == 0 else NAN), True
        else:
          ret[c] = fresh[c] if kind != 'ties' else np.float32(rng.integers(0, 2))
          dead[c] = kind == 'dying' and rng.random() < 0.3
    sel = tree_host.select(ret[None], beam)[0]
    got, _ = tree_emul.select(ret, beam)
    assert np.array_equal(got, sel)
    choice[level - 1, :len(sel)] = sel
    parent_ret, parent_dead = ret[sel], dead[sel]
  return ret, choice


@pytest.mark.parametrize('kind', ['crafted', 'ties', 'dying', 'all_dead'])
@pytest.mark.parametrize('depth, beam', [(1, 1), (1, 4), (3, 1), (2, 4), (3, 4), (4, 27), (5, 27), (7, 256)])      # C = 3, 3, 3, 9, 12, 81, 81, 768
def test_finish_equals_the_twin(depth, beam, kind):
  rng = np.random.default_rng(1000 * depth + beam + len(kind))
  for trial in range(3):
    ret, choice = _grow(rng, depth, beam, kind)
    score = None
    if trial == 2:                               # a leaf value: the keys are scores, the voids stay what ret says
      score = np.where(np.isnan(ret), ret, _crafted(rng, len(ret))).astype(np.float32)
    for source_ok in (True, False):
      want = tree_host.finish(ret[None], [c[None] for c in choice], depth, 2, [source_ok], None if score is None else score[None])
      got = tree_emul.finish(ret, choice, depth, 2, beam, source_ok, score)
      assert np.array_equal(got[0], want[0][:, 0]) and got[1] == want[1][0]
      assert np.array_equal(np.float32(got[2]).view(np.uint32), want[2][:1].view(np.uint32)[0])
      assert np.array_equal(got[3].view(np.uint32), want[3][0].view(np.uint32)) and np.array_equal(got[4], want[4][0])
      if kind == 'all_dead' and score is None and source_ok:       # the a = 0 chain stands for the dead source: all DOWN, return 0
        assert np.all(got[0] == 0) and got[2] == 0.0 and got[4].tolist() == [1, 0, 0]
    plain = tree_emul.finish(ret, choice, depth, 2, beam, True, score, want_q=False)
    assert plain[3] is None and np.array_equal(plain[0], tree_emul.finish(ret, choice, depth, 2, beam, True, score)[0])


def test_finish_on_a_level_of_195_children():
  """C = 195 is no level of a tree of the widths above, but the lane functions take any consistent lists: three levels, 65 parents."""
  rng = np.random.default_rng(195)
  depth, beam, C = 3, 256, 195
  choice = np.zeros((depth, beam), np.int32)
  choice[0, :3] = rng.permutation(3)
  choice[1, :65] = rng.integers(0, 9, 65)
  for _ in range(4):
    ret = _crafted(rng, C)
    want = tree_host.finish(ret[None], [c[None] for c in choice], depth, 3, [True])
    got = tree_emul.finish(ret, choice, depth, 3, beam)
    assert np.array_equal(got[0], want[0][:, 0]) and got[1] == want[1][0]
    assert np.float32(got[2]).view(np.uint32) == want[2].view(np.uint32)[0]
    assert np.array_equal(got[3].view(np.uint32), want[3][0].view(np.uint32)) and np.array_equal(got[4], want[4][0])
