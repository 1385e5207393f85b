"""Every host-side argument check of the on-policy entry points (ble_ac_act_f32, ble_gae_f32, ble_adv_normalize_f32,
ble_qnet_ppo_step_f32), CPU only, in the style of test_entry_checks_host.py: an invalid argument answers BLE_E_INVALID_ARG before any
HIP call, with an empty batch and with a non-empty one -- the checks come before the early return.  Their sizes travel in descriptors,
so test_entry_checks_host.py's table (the entry points with an int64_t argument) does not hold them.  No call below launches."""
import ctypes

import pytest

import descriptors_host
from balloon_learning_environment_amd import _abi, _lib
from descriptors_host import E_INVALID_ARG, _FAKE

NAN, INF = float('nan'), float('inf')


def _qnet(**fields):
  return descriptors_host._qnet(**{'num_atoms': 2, **fields})


def _train(**fields):
  return descriptors_host._train(**{'net': _qnet(), 'target': None, 'kappa': 0.0, **fields})


def _batch(**fields):
  return descriptors_host._batch(**{'next_state': None, 'discount': None, **fields})


def _ppo(**fields):
  d = dict(clip=0.2, value_coef=0.5, entropy_coef=0.01, reserved_=0, old_logp=_FAKE, advantage=_FAKE)
  d.update(fields)
  return _abi.BlePpoF32(**d)


def _rows(**fields):
  d = dict(n=0, obs_row_stride=_lib.OBS_DIM, obs=_FAKE, action=_FAKE, logp=_FAKE, value=_FAKE, probs=None)
  d.update(fields)
  return _abi.BleAcRowsF32(**d)


def _sample(**fields):
  d = dict(seed=1, env_offset=0, step=_FAKE, reserved_=0)
  d.update(fields)
  return _abi.BleAcSample(**d)


def _gae(**fields):
  d = dict(steps=0, num_envs=0, gamma=0.993, lam=0.95, reward=_FAKE, value=_FAKE, boot_value=_FAKE, terminal=_FAKE, episode_end=_FAKE,
           advantage=_FAKE, ret=_FAKE)
  d.update(fields)
  return _abi.BleGaeBlockF32(**d)


def _ref(x):
  return ctypes.byref(x) if x is not None else None


# ---- ble_qnet_ppo_step_f32 -----------------------------------------------------------------------------------------------------------
def _step(tr=None, ppo=None, bt=None, loss=_FAKE):
  return _lib.lib().ble_qnet_ppo_step_f32(_ref(tr or _train()), _ref(ppo or _ppo()), _ref(bt or _batch()), loss, None, None)


def test_ppo_step_empty_batch_is_ok():
  assert _step() == 0
  # what the update does not read may be NULL or anything: target, next_state, discount, kappa
  assert _step(_train(target=_FAKE, kappa=NAN), bt=_batch(next_state=_FAKE, discount=_FAKE)) == 0
  assert _step(_train(apply_update=0, adam_m=None, adam_v=None, adam_step=None, lr=2e-6)) == 0
  assert _step(_train(net=_qnet(num_layers=1, hidden_units=0), weights_t=None)) == 0
  assert _step(ppo=_ppo(value_coef=0.0, entropy_coef=0.0)) == 0


_STEP_CASES = {
    'atoms_1': dict(tr={'net': _qnet(num_atoms=1)}), 'atoms_51': dict(tr={'net': _qnet(num_atoms=51)}),
    'actions_2': dict(tr={'net': _qnet(num_actions=2)}), 'layers_0': dict(tr={'net': _qnet(num_layers=0)}),
    'clip_0': dict(ppo={'clip': 0.0}), 'clip_negative': dict(ppo={'clip': -0.2}), 'clip_nan': dict(ppo={'clip': NAN}),
    'clip_inf': dict(ppo={'clip': INF}), 'value_coef_nan': dict(ppo={'value_coef': NAN}), 'value_coef_inf': dict(ppo={'value_coef': INF}),
    'entropy_coef_nan': dict(ppo={'entropy_coef': NAN}), 'entropy_coef_inf': dict(ppo={'entropy_coef': -INF}),
    'null_old_logp': dict(ppo={'old_logp': None}), 'null_advantage': dict(ppo={'advantage': None}),
    'lr_nan': dict(tr={'lr': NAN}), 'lr_inf': dict(tr={'lr': INF}),
    'adam_without_m': dict(tr={'adam_m': None}), 'adam_without_v': dict(tr={'adam_v': None}), 'adam_without_step': dict(tr={'adam_step': None}),
    'adam_b1_nan': dict(tr={'adam_b1': NAN}), 'adam_eps_inf': dict(tr={'adam_eps': INF}),
    'misaligned_weights': dict(tr={'net': _qnet(weights=_FAKE + 4)}), 'misaligned_grad': dict(tr={'grad': _FAKE + 4}),
    'misaligned_weights_t': dict(tr={'weights_t': _FAKE + 4}), 'misaligned_workspace': dict(tr={'workspace': _FAKE + 8}),
    'misaligned_adam_m': dict(tr={'adam_m': _FAKE + 8}), 'misaligned_state': dict(bt={'state': _FAKE + 8}),
    'null_weights': dict(tr={'net': _qnet(weights=None)}), 'null_grad': dict(tr={'grad': None}), 'null_workspace': dict(tr={'workspace': None}),
    'null_weights_t': dict(tr={'weights_t': None}), 'null_state': dict(bt={'state': None}), 'null_ret': dict(bt={'ret': None}),
    'null_action': dict(bt={'action': None}), 'negative_batch': dict(bt={'batch': -1}), 'batch_above_max': dict(bt={'batch': 1048577}),
    'stride_below_obs_dim': dict(bt={'state_stride': 1096}), 'stride_not_multiple_of_4': dict(bt={'state_stride': 1101}),
}


@pytest.mark.parametrize('case', sorted(_STEP_CASES))
def test_ppo_step_invalid(case):
  c = _STEP_CASES[case]
  for b in ((c['bt']['batch'],) if 'batch' in c.get('bt', {}) else (0, 64)):
    assert _step(_train(**dict(c.get('tr', {}))), _ppo(**c.get('ppo', {})), _batch(**{'batch': b, **c.get('bt', {})})) == E_INVALID_ARG, b


def test_ppo_step_null_arguments():
  lib = _lib.lib()
  assert _step(loss=None) == E_INVALID_ARG
  assert lib.ble_qnet_ppo_step_f32(None, _ref(_ppo()), _ref(_batch()), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_ppo_step_f32(_ref(_train()), None, _ref(_batch()), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_ppo_step_f32(_ref(_train()), _ref(_ppo()), None, _FAKE, None, None) == E_INVALID_ARG


def test_the_sibling_updates_keep_their_answers():
  """The replay learners' entry points still refuse what PPO alone accepts: a batch without next_state or discount, a two-atom network
  under ble_qnet_td_step_f32, no target image."""
  lib = _lib.lib()
  qr = descriptors_host._train()
  for bt in (_batch(), descriptors_host._batch(next_state=None), descriptors_host._batch(discount=None)):
    assert lib.ble_qnet_train_step_f32(_ref(qr), _ref(bt), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_train_step_f32(_ref(descriptors_host._train(target=None)), _ref(descriptors_host._batch()), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_train_step_f32(_ref(qr), _ref(descriptors_host._batch()), _FAKE, None, None) == 0
  td = _abi.BleTdF32(_abi.TD_DQN_MSE, _abi.TD_OPT_ADAM, 0.9, 0, None, None)
  assert lib.ble_qnet_td_step_f32(_ref(descriptors_host._train(net=_qnet())), _ref(td), _ref(descriptors_host._batch()), _FAKE, None,
                                  None) == E_INVALID_ARG


# ---- ble_ac_act_f32 ------------------------------------------------------------------------------------------------------------------
def _act(net=None, rows=None, scratch=_FAKE, sample=None):
  return _lib.lib().ble_ac_act_f32(_ref(net or _qnet()), _ref(rows or _rows()), scratch, _ref(sample), None)


def test_act_no_rows_is_ok():
  assert _act() == 0 and _act(sample=_sample()) == 0 and _act(rows=_rows(probs=_FAKE)) == 0
  assert _act(sample=_sample(env_offset=2 ** 40, seed=2 ** 64 - 1)) == 0


_ACT_CASES = {
    'atoms_1': dict(net={'num_atoms': 1}), 'atoms_51': dict(net={'num_atoms': 51}), 'actions_2': dict(net={'num_actions': 2}),
    'layers_0': dict(net={'num_layers': 0}), 'layers_65': dict(net={'num_layers': 65}), 'hidden_0': dict(net={'hidden_units': 0}),
    'input_dim': dict(net={'input_dim': 1098}), 'null_weights': dict(net={'weights': None}), 'misaligned_weights': dict(net={'weights': _FAKE + 4}),
    'null_obs': dict(rows={'obs': None}), 'null_action': dict(rows={'action': None}), 'null_logp': dict(rows={'logp': None}),
    'null_value': dict(rows={'value': None}), 'stride_below_obs_dim': dict(rows={'obs_row_stride': 1098}),
    'negative_n': dict(rows={'n': -1}), 'null_scratch': dict(scratch=None), 'misaligned_scratch': dict(scratch=_FAKE + 8),
    'sample_without_step': dict(sample={'step': None}), 'sample_negative_env_offset': dict(sample={'env_offset': -1}),
}


@pytest.mark.parametrize('case', sorted(_ACT_CASES))
def test_act_invalid(case):
  c = _ACT_CASES[case]
  for n in ((c['rows']['n'],) if 'n' in c.get('rows', {}) else (0, 64)):
    got = _act(_qnet(**c.get('net', {})), _rows(**{'n': n, **c.get('rows', {})}), c.get('scratch', _FAKE),
               _sample(**c['sample']) if 'sample' in c else None)
    assert got == E_INVALID_ARG, n


def test_act_null_descriptors():
  lib = _lib.lib()
  assert lib.ble_ac_act_f32(None, _ref(_rows()), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_ac_act_f32(_ref(_qnet()), None, _FAKE, None, None) == E_INVALID_ARG


# ---- ble_gae_f32 and ble_adv_normalize_f32 -------------------------------------------------------------------------------------------
def test_gae_empty_block_is_ok():
  lib = _lib.lib()
  for steps, n in ((0, 0), (0, 64), (8, 0)):
    assert lib.ble_gae_f32(_ref(_gae(steps=steps, num_envs=n)), None) == 0
    assert lib.ble_adv_normalize_f32(_ref(_gae(steps=steps, num_envs=n)), None) == 0
  # the normalisation reads the sizes and advantage only
  assert lib.ble_adv_normalize_f32(_ref(_gae(reward=None, value=None, boot_value=None, terminal=None, episode_end=None, ret=None,
                                             gamma=NAN, lam=NAN)), None) == 0


_GAE_CASES = {**{f'null_{p}': {p: None} for p in ('reward', 'value', 'boot_value', 'terminal', 'episode_end', 'advantage', 'ret')},
              'gamma_nan': {'gamma': NAN}, 'gamma_inf': {'gamma': INF}, 'lambda_nan': {'lam': NAN}, 'lambda_inf': {'lam': -INF},
              'negative_steps': {'steps': -1}, 'negative_envs': {'num_envs': -1}, 'block_too_large': {'steps': 2 ** 21, 'num_envs': 2 ** 20},
              'envs_too_many': {'steps': 1, 'num_envs': 2 ** 33}}


@pytest.mark.parametrize('case', sorted(_GAE_CASES))
def test_gae_invalid(case):
  c = _GAE_CASES[case]
  for sizes in (({},) if 'steps' in c or 'num_envs' in c else ({'steps': 0, 'num_envs': 0}, {'steps': 8, 'num_envs': 64})):
    assert _lib.lib().ble_gae_f32(_ref(_gae(**{**sizes, **c})), None) == E_INVALID_ARG, sizes
  assert _lib.lib().ble_gae_f32(None, None) == E_INVALID_ARG


@pytest.mark.parametrize('case', ['null_advantage', 'negative_steps', 'negative_envs', 'block_too_large', 'envs_too_many'])
def test_adv_normalize_invalid(case):
  c = _GAE_CASES[case]
  for sizes in (({},) if 'steps' in c or 'num_envs' in c else ({'steps': 0, 'num_envs': 0}, {'steps': 8, 'num_envs': 64})):
    assert _lib.lib().ble_adv_normalize_f32(_ref(_gae(**{**sizes, **c})), None) == E_INVALID_ARG, sizes
  assert _lib.lib().ble_adv_normalize_f32(None, None) == E_INVALID_ARG
