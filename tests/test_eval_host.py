"""The evaluation mirror without a GPU: suites, the JSON shape of results, the ABI additions, and no CPU path."""
import json
import os
import re
import datetime as dt

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'balloon_learning_environment_amd')


def test_range_suites():
  from balloon_learning_environment_amd.eval import suites
  want = {'big_eval': 10_000, 'medium_eval': 1_000, 'small_eval': 100, 'tiny_eval': 10, 'micro_eval': 1}
  assert set(suites.available_suites()) == set(want)
  for name, count in want.items():
    s = suites.get_eval_suite(name)
    assert list(s.seeds) == list(range(count)) and s.max_episode_length == 960
    s.seeds.append(-1)                                    # a copy
    assert len(suites.get_eval_suite(name).seeds) == count
  for name in ('hardest_strata', 'hard_strata', 'mid_strata', 'easy_strata', 'easiest_strata', 'all_strata'):
    with pytest.raises(NotImplementedError, match='strata'):
      suites.get_eval_suite(name)
  with pytest.raises(ValueError):
    suites.get_eval_suite('no_such_suite')


def test_result_json_shape():
  from balloon_learning_environment_amd.eval import eval_lib
  from balloon_learning_environment_amd.utils import units
  p = eval_lib.SimpleBalloonState(units.Distance(m=1500.0), units.Distance(km=-2.0), 5000.0, 120.5, dt.timedelta(seconds=180), 0.95)
  r = eval_lib.EvaluationResult(seed=3, cumulative_reward=np.float64(12.5), time_within_radius=0.25, out_of_power=False,
                                envelope_burst=True, zeropressure=False, final_timestep=np.int32(7), flight_path=[p])
  d = json.loads(json.dumps(r, cls=eval_lib.EvalResultEncoder))
  assert d == {'seed': 3, 'cumulative_reward': 12.5, 'time_within_radius': 0.25, 'out_of_power': False, 'envelope_burst': True,
               'zeropressure': False, 'final_timestep': 7,
               'flight_path': [{'x': 1.5, 'y': -2.0, 'pressure': 5000.0, 'superpressure': 120.5, 'elapsed_seconds': 180.0, 'power': 0.95}]}
  assert str(r).startswith('EvaluationResult(seed=3, cumulative_reward=12.5')


def test_abi_additions():
  from balloon_learning_environment_amd import _abi, _lib, vec_state
  hdr = open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()
  for name in ('ble_station_seeker_f32', 'ble_eval_accumulate_f32', 'ble_reset_seeded_f32', 'ble_wind_noise_seeded_f32',
               'ble_observe_live_f32'):
    assert re.search(r'\bint ' + name + r'\(', hdr), name
    assert name in _lib.EXPORTS
  assert re.search(r'#define BLE_FLAG_AGENT_NO_LEVEL 1024u', hdr) and _lib.FLAG_AGENT_NO_LEVEL == 1024
  assert re.search(r'#define BLE_ABI_VERSION 5\b', hdr) and _lib.ABI_VERSION == 5
  fields = re.search(r'typedef struct ble_eval_acc \{(.*?)\} ble_eval_acc;', hdr, re.S).group(1)
  names = re.findall(r'\*\s*(\w+);', fields)
  assert names == [f for f, _ in _abi.BleEvalAcc._fields_]
  with pytest.raises(AssertionError):
    vec_state.raise_for_flags(_lib.FLAG_AGENT_NO_LEVEL)


def test_hysteresis_table_is_the_reference_term():
  """csrc/ble_agent.h tabulates 0.05 exp(-0.001 k), k = 0 .. 180, as the oracle (and the reference) evaluate it."""
  src = open(os.path.join(PKG, 'csrc', 'ble_agent.h')).read()
  body = re.search(r'kSeekerHysteresis\[181\] = \{(.*?)\};', src, re.S).group(1)
  got = np.array([float.fromhex(v.strip()) for v in body.split(',') if v.strip()])
  k = np.abs(np.arange(361) - 180)
  want = 0.05 * np.exp(-0.001 * k)
  np.testing.assert_array_equal(got[k], want)


def test_no_cpu_path():
  from balloon_learning_environment_amd.agents import station_seeker_agent
  from balloon_learning_environment_amd.eval import eval_lib, suites
  with pytest.raises(RuntimeError, match='no CPU path'):
    station_seeker_agent.VecStationSeekerAgent(device='cpu')
  with pytest.raises(RuntimeError, match='no CPU path'):
    station_seeker_agent.StationSeekerAgent(3, (1099,), device='cpu')
  with pytest.raises(RuntimeError, match='no CPU path'):
    eval_lib.eval_agent_vec(lambda o: o, suites.get_eval_suite('micro_eval'), device='cpu')


def test_new_modules_hold_no_host_twin():
  for sub in ('agents', 'eval'):
    for f in os.listdir(os.path.join(PKG, sub)):
      if f.endswith('.py'):
        src = open(os.path.join(PKG, sub, f)).read()
        assert 'scipy' not in src and 'np.linalg' not in src and 'numpy.linalg' not in src, f
        assert 'reset_host' not in src and 'wind_gp' not in src, f
