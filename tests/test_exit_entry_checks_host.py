"""Every host-side argument check of the expert-iteration entry points (ble_plan_prior_u16, ble_plan_sample_prior_u8,
ble_plan_action_values_f32, ble_qnet_soft_bc_step_f32), CPU only, in the style of test_bc_entry_checks_host.py: an invalid
argument answers BLE_E_INVALID_ARG before any HIP call, with an empty batch and with a non-empty one -- the checks come before the early
return.  Their sizes travel in structs.  The entry points they stand next to answer on the same descriptors as they did.  No call below
launches."""
import ctypes
import os
import re
import subprocess

import pytest

import descriptors_host
from balloon_learning_environment_amd import _abi, _lib
from descriptors_host import E_INVALID_ARG, _FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')
ENTRIES = ('ble_plan_prior_u16', 'ble_plan_sample_prior_u8', 'ble_plan_action_values_f32', 'ble_qnet_soft_bc_step_f32')


def _header():
  return open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()


def _ref(x):
  return ctypes.byref(x) if x is not None else None


def _prior(**over):
  f = dict(n=0, segments=6, strength=64, probs=_FAKE, prior_counts=_FAKE)
  f.update(over)
  return _abi.BlePlanPrior(**f)


def _ps(**over):
  f = dict(n=0, n_plans=8, n_plan_steps=6, segment=2, iteration=0, seed=1, env_seed=None, env_offset=0, decision_counter=_FAKE,
           elite_counts=_FAKE, best_plan=_FAKE, plans=_FAKE, prior_counts=_FAKE)
  f.update(over)
  return _abi.BlePlanSamplePrior(**f)


def _av(**over):
  f = dict(n=0, n_plans=8, accumulate=0, ret=_FAKE, first_action=_FAKE, q=_FAKE, q_k=_FAKE, visits=_FAKE)
  f.update(over)
  return _abi.BlePlanActionValues(**f)


def _qnet(**fields):
  return descriptors_host._qnet(**{'num_atoms': 2, **fields})


def _train(**fields):
  return descriptors_host._train(**{'net': _qnet(), 'target': None, 'kappa': 0.0, **fields})


def _batch(**fields):
  return descriptors_host._batch(**{'next_state': None, 'discount': None, 'action': None, **fields})


def _soft(**fields):
  d = dict(inv_temperature=2.0, label_smoothing=0.1, value_coef=0.5, reserved_=0, target_q=_FAKE)
  d.update(fields)
  return _abi.BleSoftBcF32(**d)


def _call(name, s):
  return getattr(_lib.lib(), name)(_ref(s), None)


# ---- declared, exported, mirrored ----------------------------------------------------------------------------------------------------
def test_declared_exported_and_mirrored():
  header = _header()
  assert re.search(r'\bint ble_plan_prior_u16\(const struct ble_plan_prior\* pr, void\* stream\);', header)
  assert re.search(r'\bint ble_plan_sample_prior_u8\(const struct ble_plan_sample_prior\* ps, void\* stream\);', header)
  assert re.search(r'\bint ble_plan_action_values_f32\(const struct ble_plan_action_values\* av, void\* stream\);', header)
  assert re.search(r'\bint ble_qnet_soft_bc_step_f32\(const ble_qnet_train_f32\* tr, const ble_soft_bc_f32\* soft,', header)
  assert re.search(r'#define BLE_ABI_VERSION 5\b', header) and _lib.ABI_VERSION == 5            # additive: the ABI stays 5
  symbols = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
  for name in ENTRIES:
    assert name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS, name
    assert re.search(r' T ' + name + r'$', symbols, re.M), name
    fn = getattr(_lib.lib(), name)
    assert fn.argtypes is not None and fn.restype is ctypes.c_int
    assert ctypes.c_int64 not in fn.argtypes, name          # sizes travel in the structs


@pytest.mark.parametrize('tag, mirror, size', [('ble_plan_prior', _abi.BlePlanPrior, 32), ('ble_plan_sample_prior', _abi.BlePlanSamplePrior, 88),
                                               ('ble_plan_action_values', _abi.BlePlanActionValues, 56), ('ble_soft_bc_f32', _abi.BleSoftBcF32, 24)])
def test_struct_layout_matches_the_header(tag, mirror, size):
  body = re.search(r'struct ' + tag + r' \{(.*?)\n\}', _header(), re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  declared = [re.search(r'(\w+)\s*$', d).group(1) for d in body.split(';') if d.strip()]
  assert declared == [f[0] for f in mirror._fields_]
  assert ctypes.sizeof(mirror) == size
  # every pointer lies on an 8-byte boundary without padding the compiler would have to guess
  for name, kind in mirror._fields_:
    if kind in (ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64):
      assert getattr(mirror, name).offset % 8 == 0, name


def test_the_sampler_with_a_prior_extends_the_samplers_struct():
  assert _abi.BlePlanSamplePrior._fields_[:-1] == _abi.BlePlanSample._fields_
  assert _abi.BlePlanSamplePrior._fields_[-1][0] == 'prior_counts'
  for name, _ in _abi.BlePlanSample._fields_:
    assert getattr(_abi.BlePlanSamplePrior, name).offset == getattr(_abi.BlePlanSample, name).offset, name


# ---- empty batches -------------------------------------------------------------------------------------------------------------------
def test_empty_batch_is_ok_without_a_launch():
  assert _call('ble_plan_prior_u16', _prior()) == _lib.BLE_OK
  assert _call('ble_plan_prior_u16', _prior(strength=0, segments=1)) == _lib.BLE_OK
  assert _call('ble_plan_prior_u16', _prior(strength=65535, segments=960)) == _lib.BLE_OK
  assert _call('ble_plan_sample_prior_u8', _ps()) == _lib.BLE_OK
  assert _call('ble_plan_sample_prior_u8', _ps(elite_counts=None)) == _lib.BLE_OK           # iteration 0 reads no elite counts
  assert _call('ble_plan_sample_prior_u8', _ps(iteration=15, env_seed=_FAKE, n_plans=1024, n_plan_steps=960, segment=1000)) == _lib.BLE_OK
  assert _call('ble_plan_action_values_f32', _av()) == _lib.BLE_OK
  assert _call('ble_plan_action_values_f32', _av(accumulate=1, n_plans=1024)) == _lib.BLE_OK
  assert _call('ble_plan_action_values_f32', _av(n_plans=1)) == _lib.BLE_OK


# ---- invalid arguments ---------------------------------------------------------------------------------------------------------------
_SIZES = {                      # what ble_plan_sample_u8 refuses
    'plans_0': dict(n_plans=0), 'plans_negative': dict(n_plans=-1), 'plans_1025': dict(n_plans=1025),
    'steps_0': dict(n_plan_steps=0), 'steps_961': dict(n_plan_steps=961), 'steps_negative': dict(n_plan_steps=-3),
    'segment_0': dict(segment=0), 'segment_negative': dict(segment=-1),
    'iteration_16': dict(iteration=16), 'iteration_negative': dict(iteration=-1),
    'negative_n': dict(n=-1), 'n_2_31': dict(n=2 ** 31, n_plans=1), 'n_times_k_2_31': dict(n=2 ** 21, n_plans=1024),
}

_CASES = {
    'prior_null_struct': lambda n: _lib.lib().ble_plan_prior_u16(None, None),
    'prior_null_probs': lambda n: _call('ble_plan_prior_u16', _prior(n=n, probs=None)),
    'prior_null_counts': lambda n: _call('ble_plan_prior_u16', _prior(n=n, prior_counts=None)),
    'prior_negative_n': lambda n: _call('ble_plan_prior_u16', _prior(n=-1)),
    'prior_segments_0': lambda n: _call('ble_plan_prior_u16', _prior(n=n, segments=0)),
    'prior_segments_negative': lambda n: _call('ble_plan_prior_u16', _prior(n=n, segments=-1)),
    'prior_segments_961': lambda n: _call('ble_plan_prior_u16', _prior(n=n, segments=961)),
    'prior_strength_negative': lambda n: _call('ble_plan_prior_u16', _prior(n=n, strength=-1)),
    'prior_strength_65536': lambda n: _call('ble_plan_prior_u16', _prior(n=n, strength=65536)),
    'prior_n_times_segments_2_31': lambda n: _call('ble_plan_prior_u16', _prior(n=2 ** 22, segments=512)),
    'sample_null_struct': lambda n: _lib.lib().ble_plan_sample_prior_u8(None, None),
    **{f'sample_{k}': (lambda n, k=k: _call('ble_plan_sample_prior_u8', _ps(**{'n': n, **_SIZES[k]}))) for k in _SIZES},
    **{f'sample_null_{f}': (lambda n, f=f: _call('ble_plan_sample_prior_u8', _ps(n=n, **{f: None})))
       for f in ('plans', 'decision_counter', 'best_plan', 'prior_counts')},
    'sample_null_counts_in_iteration_1': lambda n: _call('ble_plan_sample_prior_u8', _ps(n=n, iteration=1, elite_counts=None)),
    'sample_null_prior_in_iteration_1': lambda n: _call('ble_plan_sample_prior_u8', _ps(n=n, iteration=1, prior_counts=None)),
    'sample_negative_env_offset': lambda n: _call('ble_plan_sample_prior_u8', _ps(n=n, env_offset=-1)),
    'values_null_struct': lambda n: _lib.lib().ble_plan_action_values_f32(None, None),
    **{f'values_null_{f}': (lambda n, f=f: _call('ble_plan_action_values_f32', _av(n=n, **{f: None})))
       for f in ('ret', 'first_action', 'q', 'q_k', 'visits')},
    'values_plans_0': lambda n: _call('ble_plan_action_values_f32', _av(n=n, n_plans=0)),
    'values_plans_negative': lambda n: _call('ble_plan_action_values_f32', _av(n=n, n_plans=-1)),
    'values_plans_1025': lambda n: _call('ble_plan_action_values_f32', _av(n=n, n_plans=1025)),
    'values_negative_n': lambda n: _call('ble_plan_action_values_f32', _av(n=-1)),
    'values_n_2_31': lambda n: _call('ble_plan_action_values_f32', _av(n=2 ** 31, n_plans=1)),
    'values_n_times_k_2_31': lambda n: _call('ble_plan_action_values_f32', _av(n=2 ** 21, n_plans=1024)),
}


@pytest.mark.parametrize('n', [0, 64])
@pytest.mark.parametrize('case', sorted(_CASES))
def test_invalid_argument(case, n):
  assert _CASES[case](n) == E_INVALID_ARG


# ---- ble_qnet_soft_bc_step_f32 -------------------------------------------------------------------------------------------------------
def _step(tr=None, soft=None, bt=None, loss=_FAKE):
  return _lib.lib().ble_qnet_soft_bc_step_f32(_ref(tr or _train()), _ref(soft or _soft()), _ref(bt or _batch()), loss, None, None)


def test_soft_step_empty_batch_is_ok():
  assert _step() == 0
  # what the update does not read may be NULL or anything: target, next_state, discount, kappa, action
  assert _step(_train(target=_FAKE, kappa=NAN), bt=_batch(next_state=_FAKE, discount=_FAKE, action=_FAKE)) == 0
  assert _step(_train(apply_update=0, adam_m=None, adam_v=None, adam_step=None, lr=2e-6)) == 0
  assert _step(_train(net=_qnet(num_layers=1, hidden_units=0), weights_t=None)) == 0
  for soft in (_soft(label_smoothing=0.0), _soft(label_smoothing=0.999), _soft(value_coef=-0.5), _soft(inv_temperature=1e-6),
               _soft(inv_temperature=1e6)):
    assert _step(soft=soft) == 0
  # no value term: ret is not read and may be NULL (-0.0 is 0 too)
  assert _step(soft=_soft(value_coef=0.0), bt=_batch(ret=None)) == 0
  assert _step(soft=_soft(value_coef=-0.0), bt=_batch(ret=None)) == 0


_STEP_CASES = {
    'atoms_1': dict(tr={'net': _qnet(num_atoms=1)}), 'atoms_3': dict(tr={'net': _qnet(num_atoms=3)}),
    'atoms_51': dict(tr={'net': _qnet(num_atoms=51)}),
    'actions_2': dict(tr={'net': _qnet(num_actions=2)}), 'layers_0': dict(tr={'net': _qnet(num_layers=0)}),
    'beta_0': dict(soft={'inv_temperature': 0.0}), 'beta_negative': dict(soft={'inv_temperature': -1.0}),
    'beta_nan': dict(soft={'inv_temperature': NAN}), 'beta_inf': dict(soft={'inv_temperature': INF}),
    'null_target_q': dict(soft={'target_q': None}),
    'smoothing_1': dict(soft={'label_smoothing': 1.0}), 'smoothing_negative': dict(soft={'label_smoothing': -0.1}),
    'smoothing_nan': dict(soft={'label_smoothing': NAN}), 'smoothing_inf': dict(soft={'label_smoothing': INF}),
    'value_coef_nan': dict(soft={'value_coef': NAN}), 'value_coef_inf': dict(soft={'value_coef': INF}),
    'value_coef_nan_null_ret': dict(soft={'value_coef': NAN}, bt={'ret': None}),
    'null_ret_with_value_coef': dict(bt={'ret': None}),
    'lr_nan': dict(tr={'lr': NAN}), 'lr_inf': dict(tr={'lr': INF}),
    'adam_without_m': dict(tr={'adam_m': None}), 'adam_without_v': dict(tr={'adam_v': None}), 'adam_without_step': dict(tr={'adam_step': None}),
    'adam_b1_nan': dict(tr={'adam_b1': NAN}), 'adam_b2_nan': dict(tr={'adam_b2': NAN}), 'adam_eps_inf': dict(tr={'adam_eps': INF}),
    'misaligned_weights': dict(tr={'net': _qnet(weights=_FAKE + 4)}), 'misaligned_grad': dict(tr={'grad': _FAKE + 4}),
    'misaligned_weights_t': dict(tr={'weights_t': _FAKE + 4}), 'misaligned_workspace': dict(tr={'workspace': _FAKE + 8}),
    'misaligned_adam_m': dict(tr={'adam_m': _FAKE + 8}), 'misaligned_state': dict(bt={'state': _FAKE + 8}),
    'null_weights': dict(tr={'net': _qnet(weights=None)}), 'null_grad': dict(tr={'grad': None}), 'null_workspace': dict(tr={'workspace': None}),
    'null_weights_t': dict(tr={'weights_t': None}), 'null_state': dict(bt={'state': None}),
    'negative_batch': dict(bt={'batch': -1}), 'batch_above_max': dict(bt={'batch': 1048577}),
    'stride_below_obs_dim': dict(bt={'state_stride': 1096}), 'stride_not_multiple_of_4': dict(bt={'state_stride': 1101}),
}


@pytest.mark.parametrize('case', sorted(_STEP_CASES))
def test_soft_step_invalid(case):
  c = _STEP_CASES[case]
  for b in ((c['bt']['batch'],) if 'batch' in c.get('bt', {}) else (0, 64)):
    assert _step(_train(**dict(c.get('tr', {}))), _soft(**c.get('soft', {})), _batch(**{'batch': b, **c.get('bt', {})})) == E_INVALID_ARG, b


def test_soft_step_null_arguments():
  lib = _lib.lib()
  assert _step(loss=None) == E_INVALID_ARG
  assert lib.ble_qnet_soft_bc_step_f32(None, _ref(_soft()), _ref(_batch()), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_soft_bc_step_f32(_ref(_train()), _ref(_soft()), None, _FAKE, None, None) == E_INVALID_ARG
  for b in (0, 64):
    assert lib.ble_qnet_soft_bc_step_f32(_ref(_train()), None, _ref(_batch(batch=b)), _FAKE, None, None) == E_INVALID_ARG


# ---- the entry points next to them keep their answers ---------------------------------------------------------------------------------
def test_the_existing_entry_points_keep_their_answers():
  """The soft update reads no batch->action: that relaxation is its alone.  Cloning, PPO and the replay learners refuse a batch
  without one as they did; the sampler and the selection answer on their descriptors as they did."""
  lib = _lib.lib()
  bc = _abi.BleBcF32(0.1, 0.5, 0)
  ppo = _abi.BlePpoF32(0.2, 0.5, 0.01, 0, _FAKE, _FAKE)
  with_action = _batch(action=_FAKE)
  assert lib.ble_qnet_bc_step_f32(_ref(_train()), _ref(bc), _ref(with_action), _FAKE, None, None) == 0
  assert lib.ble_qnet_ppo_step_f32(_ref(_train()), _ref(ppo), _ref(with_action), _FAKE, None, None) == 0
  for b in (0, 64):
    assert lib.ble_qnet_bc_step_f32(_ref(_train()), _ref(bc), _ref(_batch(batch=b)), _FAKE, None, None) == E_INVALID_ARG
    assert lib.ble_qnet_ppo_step_f32(_ref(_train()), _ref(ppo), _ref(_batch(batch=b)), _FAKE, None, None) == E_INVALID_ARG
    assert lib.ble_qnet_train_step_f32(_ref(descriptors_host._train()), _ref(descriptors_host._batch(batch=b, action=None)), _FAKE, None,
                                       None) == E_INVALID_ARG
  assert lib.ble_qnet_train_step_f32(_ref(descriptors_host._train()), _ref(descriptors_host._batch()), _FAKE, None, None) == 0
  # the sampler without a prior: the same struct prefix, the same answers
  fields = {name: getattr(_ps(), name) for name, _ in _abi.BlePlanSample._fields_}
  assert lib.ble_plan_sample_u8(_ref(_abi.BlePlanSample(**fields)), None) == 0
  assert lib.ble_plan_sample_u8(_ref(_abi.BlePlanSample(**{**fields, 'n_plans': 1025})), None) == E_INVALID_ARG
  assert lib.ble_plan_sample_u8(_ref(_abi.BlePlanSample(**{**fields, 'iteration': 1, 'elite_counts': None})), None) == E_INVALID_ARG
  sel = _abi.BlePlanSelect(0, 8, 6, 2, 0, 2, 0, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, None)
  assert lib.ble_plan_select_f32(_ref(sel), None) == 0
  sel.elite = 9
  assert lib.ble_plan_select_f32(_ref(sel), None) == E_INVALID_ARG
