"""The beam search in scenario winds without a GPU: the entry point is declared, exported and mirrored; every refusal answers
BLE_E_INVALID_ARG before any HIP call, with an empty batch and with a non-empty one (no call below has valid arguments and n > 0, so
none launches); the fly / carry / void lane function of csrc/ble_tree_scenarios.h, built for the host (tests/emul/tree_scenarios_emul.cpp),
equals the NumPy twin (tests/tree_scenarios_host.py) on EVERY status pattern of M = 1, 3 and 16; the twin's level loop equals the host
builds of plan_risk_score, tree_select_lane and the finish on crafted returns; and the Python refusals that need no device.  No
tolerance anywhere: integers and bits."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import test_tree_host as tth
import tree_host
import tree_scenarios_host as twin
from balloon_learning_environment_amd import _abi, _lib
from descriptors_host import E_INVALID_ARG, _FAKE
from emul import tree_emul, tree_scenarios_emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')
ENTRY = 'ble_tree_expand_scenarios_f32'
_ref, _ex, _arena, _state = tth._ref, tth._ex, tth._arena, tth._state


def _scn(**over):
  f = dict(slab=_FAKE, stride=_abi.gp_scenario_doubles(3), n_obs=_FAKE, n=0, num=3, reserved_=0)
  f.update(over)
  return _abi.BleGpScenarios(**f)


def _sgen(**over):
  f = dict(seed=3, env_seed=None, episode=_FAKE, env_offset=0)
  f.update(over)
  return _abi.BleScenarioGen(**f)


_DEFAULT = object()


def _expand(ex=_DEFAULT, st=_DEFAULT, scn=_DEFAULT, gen=_DEFAULT):
  st = _state() if st is _DEFAULT else st
  ex = _ex() if ex is _DEFAULT else ex
  scn = _scn(n=ex.n if ex is not None else 0) if scn is _DEFAULT else scn
  gen = _sgen() if gen is _DEFAULT else gen
  return _lib.lib().ble_tree_expand_scenarios_f32(_ref(st), _ref(ex), _ref(scn), _ref(gen), None, None)


# ---- declared, exported, mirrored ----------------------------------------------------------------------------------------------------
def test_declared_exported_and_mirrored():
  header = open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()
  assert re.search(r'\bint ble_tree_expand_scenarios_f32\(const ble_state_f32\* st, const struct ble_tree_expand\* ex, '
                   r'const ble_gp_scenarios\* scn,\s*const ble_scenario_gen\* gen, uint32_t\* err_flags, void\* stream\);', header)
  assert re.search(r'#define BLE_ABI_VERSION 5\b', header) and _lib.ABI_VERSION == 5            # additive: the ABI stays 5
  symbols = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
  assert ENTRY in _lib.EXPORTS and ENTRY in _lib.ADDITIVE_EXPORTS
  assert re.search(r' T ' + ENTRY + r'$', symbols, re.M)
  fn = getattr(_lib.lib(), ENTRY)
  assert fn.argtypes is not None and fn.restype is ctypes.c_int
  assert not any(issubclass(t, ctypes.c_int64) for t in fn.argtypes if isinstance(t, type))        # every size travels in a struct
  assert any(s.endswith('ble_tree_scenarios.h') for s in _lib._SOURCES)
  hip = open(_lib._SOURCES[0]).read()
  assert hip.index('#include "ble_tree.h"') < hip.index('#include "ble_scenarios.h"') < hip.index('#include "ble_tree_scenarios.h"')


# ---- empty batches -------------------------------------------------------------------------------------------------------------------
def test_empty_batch_is_ok_without_a_launch():
  assert _expand(_ex(level=1)) == _lib.BLE_OK
  assert _expand() == _lib.BLE_OK
  assert _expand(gen=_sgen(env_seed=_FAKE)) == _lib.BLE_OK
  assert _expand(scn=_scn(num=1, stride=_abi.gp_scenario_doubles(1))) == _lib.BLE_OK
  assert _expand(scn=_scn(num=16, stride=_abi.gp_scenario_doubles(16))) == _lib.BLE_OK
  assert _expand(scn=_scn(num=3, stride=_abi.gp_scenario_doubles(16))) == _lib.BLE_OK            # a longer slab
  assert _expand(_ex(beam=256, n_parents=256, parent_children=768, depth=8, segment=4)) == _lib.BLE_OK
  assert _expand(_ex(depth=6, segment=40, action_repeat=4, gamma=0.0)) == _lib.BLE_OK               # 960 agent steps


# ---- invalid arguments ---------------------------------------------------------------------------------------------------------------
_SCN_BAD = {
    'null_slab': dict(slab=None), 'null_n_obs': dict(n_obs=None), 'num_0': dict(num=0), 'num_negative': dict(num=-1),
    'num_17': dict(num=17, stride=_abi.gp_scenario_doubles(17)), 'short_stride': dict(stride=_abi.gp_scenario_doubles(3) - 2),
    'stride_of_fewer_scenarios': dict(stride=_abi.gp_scenario_doubles(2)), 'odd_stride': dict(stride=_abi.gp_scenario_doubles(3) + 1),
    'misaligned_slab': dict(slab=_FAKE + 8),
}

_CASES = {
    # everything ble_tree_expand_f32 refuses of st and ex
    **{f'ex_{k}': (lambda n, k=k: _expand(_ex(**{'n': n, **tth._EX_BAD[k]}))) for k in tth._EX_BAD},
    **{f'ex_{k}': (lambda n, k=k: _expand(_ex(n=n, **tth._LATER[k]()))) for k in tth._LATER},
    'null_state': lambda n: _expand(_ex(n=n), st=None),
    'null_state_array': lambda n: _expand(_ex(n=n), st=_state(null='pressure')),
    'null_struct': lambda n: _expand(None, scn=_scn(n=n)),
    'bad_vehicle': lambda n: _expand(_ex(n=n), st=_state(vehicle=_abi.vehicle_struct(envelope_mass=-1.0))),
    'level_1_two_parents': lambda n: _expand(_ex(level=1, n=n, n_parents=2)),
    'level_1_dst_is_the_source': lambda n: _expand(_ex(level=1, n=n, dst=_arena(_FAKE))),
    'level_1_null_dst_ret': lambda n: _expand(_ex(level=1, n=n, dst=_arena(tth._DST, ret=0))),
    'level_1_steps_961': lambda n: _expand(_ex(level=1, n=n, depth=961, segment=1)),
    # the bound with the scenarios: n * 3 * beam * num >= 2^31 where n * 3 * beam is still below it
    'n_times_3_beam_num_2_31': lambda n: _expand(_ex(n=2 ** 26, beam=4), scn=_scn(n=2 ** 26, num=3)),
    'n_times_3_beam_num_2_31_level_1': lambda n: _expand(_ex(level=1, n=2 ** 26, beam=4), scn=_scn(n=2 ** 26, num=3)),
    'n_times_3_beam_16_2_31': lambda n: _expand(_ex(n=2 ** 24, beam=4), scn=_scn(n=2 ** 24, num=16, stride=_abi.gp_scenario_doubles(16))),
    # everything ble_gp_fit_scenarios_f32 refuses of scn and gen
    **{f'scn_{k}': (lambda n, k=k: _expand(_ex(n=n), scn=_scn(**{'n': n, **_SCN_BAD[k]}))) for k in _SCN_BAD},
    'scn_null': lambda n: _expand(_ex(n=n), scn=None),
    'scn_negative_n': lambda n: _expand(_ex(n=n), scn=_scn(n=-1)),
    'scn_n_2_31': lambda n: _expand(_ex(n=n), scn=_scn(n=2 ** 31)),
    'gen_null': lambda n: _expand(_ex(n=n), gen=None),
    'gen_negative_offset': lambda n: _expand(_ex(n=n), gen=_sgen(env_offset=-1)),
    # scenarios of another batch
    'scn_of_a_larger_batch': lambda n: _expand(_ex(n=n), scn=_scn(n=n + 1)),
    'scn_of_a_smaller_batch': lambda n: _expand(_ex(n=n + 1), scn=_scn(n=n)),
}


@pytest.mark.parametrize('n', [0, 64])
@pytest.mark.parametrize('case', sorted(_CASES))
def test_invalid_argument(case, n):
  assert _CASES[case](n) == E_INVALID_ARG


def test_the_bound_cases_are_below_the_plain_bound():
  """What the 2^31 cases refuse is the scenario count: n * 3 * beam alone is below the bound in each of them."""
  assert 2 ** 26 * 12 < 2 ** 31 <= 2 ** 26 * 12 * 3 and 2 ** 24 * 12 < 2 ** 31 <= 2 ** 24 * 12 * 16


# ---- fly, carry, void: the lane function against the twin ------------------------------------------------------------------------------
def _check_group(status, acc):
  M = len(status)
  stopped = [twin.stopped(int(s), float(a)) for s, a in zip(status, acc)]
  for m in range(M):
    for act in range(3):
      want = twin.lane(status, acc, m, act)
      assert tree_scenarios_emul.lane(status, acc, m, act) == want, (status, acc, m, act)
      # the rule itself, restated: live flies; stopped is carried, unless the whole group is spent and a != 0
      if not stopped[m]:
        assert want == twin.FLY
      elif all(stopped):
        assert want == (twin.CARRY if act == 0 else twin.VOID)
      else:
        assert want == twin.CARRY


@pytest.mark.parametrize('M', [1, 3])
def test_lane_on_every_status_and_acc_pattern(M):
  """Small groups: every node OK, terminal by either code, or with a NaN acc, in every combination."""
  kinds = [(0, 1.5), (1, 1.5), (2, -0.25), (0, NAN), (2, NAN), (0, INF), (0, -INF)]
  for combo in itertools.product(kinds, repeat=M):
    _check_group(np.array([k[0] for k in combo], np.uint8), np.array([k[1] for k in combo], np.float64))


def test_lane_on_every_status_pattern_of_16():
  """M = 16: all 2^16 patterns of stopped-by-status; then a NaN acc inside live groups and inside spent ones."""
  lib = tree_scenarios_emul.lib()
  acc = np.arange(16, dtype=np.float64)
  for bits in range(1 << 16):
    status = np.array([2 if (bits >> m) & 1 else 0 for m in range(16)], np.uint8)
    spent = bits == 0xFFFF
    for m in (0, 7, 15):
      mine = (bits >> m) & 1
      for act in range(3):
        want = twin.FLY if not mine else (twin.VOID if spent and act else twin.CARRY)
        assert lib.emul_tree_scenario_lane(status.ctypes.data, acc.ctypes.data, 16, m, act) == want, (bits, m, act)
  rng = np.random.default_rng(16)
  for _ in range(200):
    status = np.where(rng.random(16) < 0.6, rng.integers(1, 3, 16), 0).astype(np.uint8)
    a = np.where(rng.random(16) < 0.3, NAN, rng.standard_normal(16))
    _check_group(status, a)
  # spent only through NaN accs, spent through a mix, and one live node left
  _check_group(np.zeros(16, np.uint8), np.full(16, NAN))
  mix = np.array([2, 0] * 8, np.uint8)
  _check_group(mix, np.where(mix == 0, NAN, 1.0))
  one = np.where(mix == 0, NAN, 1.0)
  one[5] = 0.5
  _check_group(mix, one)


def test_lane_at_level_1():
  """Level 1: the group is the environment itself; spent exactly when its status is not OK."""
  for status in (0, 1, 2, 255):
    for m in (0, 2, 15):
      for act in range(3):
        want = twin.lane(np.array([status], np.uint8), None, m, act)
        assert tree_scenarios_emul.lane(np.array([status], np.uint8), None, m, act) == want
        assert want == (twin.FLY if status == 0 else (twin.CARRY if act == 0 else twin.VOID))


# ---- the level loop against the host builds --------------------------------------------------------------------------------------------
def _crafted(rng, C, M, kind):
  """[C, M] returns with exact ties, both zeros, and groups holding a NaN or an infinity in one scenario."""
  pool = np.array([0.0, -0.0, 1.5, 1.5, -1.5, 3.25, 1e-38, -1e-38, 2.0 ** -149, 7.0, -7.0], np.float32)
  ret = rng.choice(pool, (C, M)).astype(np.float32)
  fresh = rng.random((C, M)) < 0.3
  ret[fresh] = rng.standard_normal(int(fresh.sum())).astype(np.float32)
  if kind == 'ties':
    ret = rng.integers(0, 2, (C, M)).astype(np.float32) * np.where(rng.random((C, M)) < 0.5, np.float32(1.0), np.float32(-1.0))
  if kind != 'finite':
    for c in np.nonzero(rng.random(C) < 0.25)[0]:
      ret[c, rng.integers(0, M)] = rng.choice(np.array([NAN, INF, -INF], np.float32))
    ret[np.nonzero(rng.random(C) < 0.1)[0]] = NAN                                        # void groups
  return ret


@pytest.mark.parametrize('kind', ['finite', 'ties', 'crafted'])
@pytest.mark.parametrize('M, tail', [(1, 1), (3, 1), (3, 2), (3, 3), (8, 3), (16, 1), (16, 16)])
@pytest.mark.parametrize('depth, beam', [(1, 1), (2, 4), (3, 4), (4, 27), (5, 27), (6, 256)])
def test_level_loop_equals_the_host_builds(depth, beam, M, tail, kind):
  rng = np.random.default_rng(10000 * depth + 100 * beam + 10 * M + tail + len(kind))
  sizes = tree_host.level_sizes(depth, beam)
  returns = [_crafted(rng, C, M, kind) for _, C in sizes]
  for source_ok in (True, False):
    scores, parents, fin = twin.search([r[None] for r in returns], tail, beam, 2, [source_ok])
    choice = np.zeros((depth, beam), np.int32)
    for d, ret in enumerate(returns):
      score, parent, chosen = tree_scenarios_emul.level(ret, tail, beam)
      assert np.array_equal(score.view(np.uint32), scores[d][0].view(np.uint32))           # NaN where any scenario is non-finite
      assert np.array_equal(np.isnan(score), ~np.isfinite(ret).all(axis=1))
      assert np.array_equal(parent, parents[d][0]) and np.array_equal(chosen, parents[d][0])
      choice[d, :len(parent)] = parent
    got = tree_emul.finish(score, choice, depth, 2, beam, source_ok, None)                 # ret := score, score := NULL
    assert np.array_equal(got[0], fin[0][:, 0]) and got[1] == fin[1][0]
    assert np.float32(got[2]).view(np.uint32) == fin[2].view(np.uint32)[0]
    assert np.array_equal(got[3].view(np.uint32), fin[3][0].view(np.uint32)) and np.array_equal(got[4], fin[4][0])
    assert got[4].sum() == int((~np.isnan(score)).sum())                                  # visits: the groups whose score is not NaN
    if source_ok and np.isfinite(score).any():
      assert got[2] == np.max(score[np.isfinite(score)])


def test_score_of_one_scenario_is_the_return():
  rng = np.random.default_rng(1)
  ret = _crafted(rng, 81, 1, 'finite')
  score, _, _ = tree_scenarios_emul.level(ret, 1, 27)
  assert np.array_equal(score, ret[:, 0])                                                # as floats (-0 == +0)


# ---- Python refusals that need no device -----------------------------------------------------------------------------------------------
def test_agent_refusals_without_a_device():
  from balloon_learning_environment_amd.agents import beam_agent
  for m in (0, -1, 17):
    with pytest.raises(ValueError, match='num_scenarios'):
      beam_agent.VecScenarioBeamSearchAgent(num_scenarios=m)
  for m, tail in ((8, 0), (8, 9), (1, 2), (16, 17), (3, -1)):
    with pytest.raises(ValueError, match='risk_tail'):
      beam_agent.VecScenarioBeamSearchAgent(num_scenarios=m, risk_tail=tail)
  with pytest.raises(ValueError, match='leaf_value'):
    beam_agent.VecScenarioBeamSearchAgent(leaf_value=object())
  with pytest.raises(ValueError, match='VecScenarioBeamSearchAgent'):                     # the belief tree's refusal names the class
    beam_agent.VecBeamSearchAgent(wind='scenarios')
  assert issubclass(beam_agent.VecScenarioBeamSearchAgent, beam_agent.VecBeamSearchAgent)
