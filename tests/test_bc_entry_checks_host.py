"""Every host-side argument check of the imitation entry points (ble_qnet_bc_step_f32, ble_dagger_mix_u8), CPU only, in the style of
test_ppo_entry_checks_host.py: an invalid argument answers BLE_E_INVALID_ARG before any HIP call, with an empty batch and with a
non-empty one -- the checks come before the early return.  Their sizes travel in descriptors.  The sibling updates answer on the same
descriptors as they did.  No call below launches."""
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


def _bc(**fields):
  d = dict(label_smoothing=0.1, value_coef=0.5, reserved_=0)
  d.update(fields)
  return _abi.BleBcF32(**d)


def _ppo(**fields):
  d = dict(clip=0.2, value_coef=0.5, entropy_coef=0.01, reserved_=0, old_logp=_FAKE, advantage=_FAKE)
  d.update(fields)
  return _abi.BlePpoF32(**d)


def _mix(**fields):
  d = dict(n=0, beta=0.5, reserved_=0, seed=1, env_offset=0, step=_FAKE, learner=_FAKE, expert=_FAKE, action=_FAKE, took_expert=None)
  d.update(fields)
  return _abi.BleDaggerMixF32(**d)


def _ref(x):
  return ctypes.byref(x) if x is not None else None


# ---- ble_qnet_bc_step_f32 ------------------------------------------------------------------------------------------------------------
def _step(tr=None, bc=None, bt=None, loss=_FAKE):
  return _lib.lib().ble_qnet_bc_step_f32(_ref(tr or _train()), _ref(bc or _bc()), _ref(bt or _batch()), loss, None, None)


def test_bc_step_empty_batch_is_ok():
  assert _step() == 0
  # what the update does not read may be NULL or anything: target, next_state, discount, kappa
  assert _step(_train(target=_FAKE, kappa=NAN), bt=_batch(next_state=_FAKE, discount=_FAKE)) == 0
  assert _step(_train(apply_update=0, adam_m=None, adam_v=None, adam_step=None, lr=2e-6)) == 0
  assert _step(_train(net=_qnet(num_layers=1, hidden_units=0), weights_t=None)) == 0
  assert _step(bc=_bc(label_smoothing=0.0)) == 0
  assert _step(bc=_bc(label_smoothing=0.999)) == 0
  assert _step(bc=_bc(value_coef=-0.5)) == 0
  # no value term: ret is not read and may be NULL (-0.0 is 0 too); with one it may of course be there
  assert _step(bc=_bc(value_coef=0.0), bt=_batch(ret=None)) == 0
  assert _step(bc=_bc(value_coef=-0.0), bt=_batch(ret=None)) == 0
  assert _step(bc=_bc(value_coef=0.0)) == 0


_STEP_CASES = {
    'atoms_1': dict(tr={'net': _qnet(num_atoms=1)}), 'atoms_3': dict(tr={'net': _qnet(num_atoms=3)}),
    'atoms_51': dict(tr={'net': _qnet(num_atoms=51)}),
    'actions_2': dict(tr={'net': _qnet(num_actions=2)}), 'layers_0': dict(tr={'net': _qnet(num_layers=0)}),
    'smoothing_1': dict(bc={'label_smoothing': 1.0}), 'smoothing_negative': dict(bc={'label_smoothing': -0.1}),
    'smoothing_nan': dict(bc={'label_smoothing': NAN}), 'smoothing_inf': dict(bc={'label_smoothing': INF}),
    'smoothing_minus_inf': dict(bc={'label_smoothing': -INF}),
    'value_coef_nan': dict(bc={'value_coef': NAN}), 'value_coef_inf': dict(bc={'value_coef': INF}),
    'value_coef_minus_inf': dict(bc={'value_coef': -INF}),
    'value_coef_nan_null_ret': dict(bc={'value_coef': NAN}, bt={'ret': None}),
    'null_ret_with_value_coef': dict(bt={'ret': None}), 'null_ret_with_negative_value_coef': dict(bc={'value_coef': -1e-3}, bt={'ret': None}),
    'lr_nan': dict(tr={'lr': NAN}), 'lr_inf': dict(tr={'lr': INF}),
    'adam_without_m': dict(tr={'adam_m': None}), 'adam_without_v': dict(tr={'adam_v': None}), 'adam_without_step': dict(tr={'adam_step': None}),
    'adam_b1_nan': dict(tr={'adam_b1': NAN}), 'adam_b2_nan': dict(tr={'adam_b2': NAN}), 'adam_eps_inf': dict(tr={'adam_eps': INF}),
    'misaligned_weights': dict(tr={'net': _qnet(weights=_FAKE + 4)}), 'misaligned_grad': dict(tr={'grad': _FAKE + 4}),
    'misaligned_weights_t': dict(tr={'weights_t': _FAKE + 4}), 'misaligned_workspace': dict(tr={'workspace': _FAKE + 8}),
    'misaligned_adam_m': dict(tr={'adam_m': _FAKE + 8}), 'misaligned_state': dict(bt={'state': _FAKE + 8}),
    'null_weights': dict(tr={'net': _qnet(weights=None)}), 'null_grad': dict(tr={'grad': None}), 'null_workspace': dict(tr={'workspace': None}),
    'null_weights_t': dict(tr={'weights_t': None}), 'null_state': dict(bt={'state': None}),
    'null_action': dict(bt={'action': None}), 'negative_batch': dict(bt={'batch': -1}), 'batch_above_max': dict(bt={'batch': 1048577}),
    'stride_below_obs_dim': dict(bt={'state_stride': 1096}), 'stride_not_multiple_of_4': dict(bt={'state_stride': 1101}),
}


@pytest.mark.parametrize('case', sorted(_STEP_CASES))
def test_bc_step_invalid(case):
  c = _STEP_CASES[case]
  for b in ((c['bt']['batch'],) if 'batch' in c.get('bt', {}) else (0, 64)):
    assert _step(_train(**dict(c.get('tr', {}))), _bc(**c.get('bc', {})), _batch(**{'batch': b, **c.get('bt', {})})) == E_INVALID_ARG, b


def test_bc_step_null_arguments():
  lib = _lib.lib()
  assert _step(loss=None) == E_INVALID_ARG
  assert lib.ble_qnet_bc_step_f32(None, _ref(_bc()), _ref(_batch()), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_bc_step_f32(_ref(_train()), None, _ref(_batch()), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_bc_step_f32(_ref(_train()), _ref(_bc()), None, _FAKE, None, None) == E_INVALID_ARG
  for b in (0, 64):
    assert lib.ble_qnet_bc_step_f32(_ref(_train()), None, _ref(_batch(batch=b)), _FAKE, None, None) == E_INVALID_ARG


def test_the_sibling_updates_keep_their_answers():
  """On the descriptors above the other updates answer as before: PPO still wants ret whatever its value coefficient, the replay
  learners still refuse a batch without next_state or discount, a two-atom network under ble_qnet_td_step_f32 and a missing target."""
  lib = _lib.lib()
  # PPO: accepts the on-policy batch, refuses one without ret (with c_v = 0 too) -- cloning's relaxation is cloning's alone
  assert lib.ble_qnet_ppo_step_f32(_ref(_train()), _ref(_ppo()), _ref(_batch()), _FAKE, None, None) == 0
  for b in (0, 64):
    for ppo in (_ppo(), _ppo(value_coef=0.0)):
      assert lib.ble_qnet_ppo_step_f32(_ref(_train()), _ref(ppo), _ref(_batch(batch=b, ret=None)), _FAKE, None, None) == E_INVALID_ARG
    assert lib.ble_qnet_ppo_step_f32(_ref(_train(net=_qnet(num_atoms=1))), _ref(_ppo()), _ref(_batch(batch=b)), _FAKE, None, None) == E_INVALID_ARG
  # QR-DQN
  qr = descriptors_host._train()
  for bt in (_batch(), descriptors_host._batch(next_state=None), descriptors_host._batch(discount=None), descriptors_host._batch(ret=None)):
    assert lib.ble_qnet_train_step_f32(_ref(qr), _ref(bt), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_train_step_f32(_ref(descriptors_host._train(target=None)), _ref(descriptors_host._batch()), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_train_step_f32(_ref(descriptors_host._train(kappa=0.0)), _ref(descriptors_host._batch()), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_train_step_f32(_ref(qr), _ref(descriptors_host._batch()), _FAKE, None, None) == 0
  # TD
  td = _abi.BleTdF32(_abi.TD_DQN_MSE, _abi.TD_OPT_ADAM, 0.9, 0, None, None)
  one = descriptors_host._train(net=descriptors_host._qnet(num_atoms=1))
  assert lib.ble_qnet_td_step_f32(_ref(one), _ref(td), _ref(descriptors_host._batch()), _FAKE, None, None) == 0
  assert lib.ble_qnet_td_step_f32(_ref(descriptors_host._train(net=_qnet())), _ref(td), _ref(descriptors_host._batch()), _FAKE, None,
                                  None) == E_INVALID_ARG
  for bt in (_batch(), descriptors_host._batch(ret=None)):
    assert lib.ble_qnet_td_step_f32(_ref(one), _ref(td), _ref(bt), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_td_step_f32(_ref(descriptors_host._train(net=descriptors_host._qnet(num_atoms=1), target=None)), _ref(td),
                                  _ref(descriptors_host._batch()), _FAKE, None, None) == E_INVALID_ARG


# ---- ble_dagger_mix_u8 ---------------------------------------------------------------------------------------------------------------
def test_mix_no_rows_is_ok():
  lib = _lib.lib()
  assert lib.ble_dagger_mix_u8(_ref(_mix()), None) == 0
  for beta in (0.0, 1.0, -0.0):
    assert lib.ble_dagger_mix_u8(_ref(_mix(beta=beta)), None) == 0
  assert lib.ble_dagger_mix_u8(_ref(_mix(took_expert=_FAKE, env_offset=2 ** 40, seed=2 ** 64 - 1)), None) == 0
  assert lib.ble_dagger_mix_u8(_ref(_mix(action=_FAKE, learner=_FAKE)), None) == 0        # action may alias learner
  # n == 0 needs no pointer
  assert lib.ble_dagger_mix_u8(_ref(_mix(step=None, learner=None, expert=None, action=None)), None) == 0


_MIX_CASES = {
    'beta_negative': {'beta': -0.01}, 'beta_above_1': {'beta': 1.01}, 'beta_nan': {'beta': NAN}, 'beta_inf': {'beta': INF},
    'beta_minus_inf': {'beta': -INF}, 'negative_n': {'n': -1}, 'n_too_large': {'n': 2 ** 40}, 'negative_env_offset': {'env_offset': -1},
}
_MIX_POINTER_CASES = {f'null_{p}': {p: None} for p in ('step', 'learner', 'expert', 'action')}


@pytest.mark.parametrize('case', sorted(_MIX_CASES))
def test_mix_invalid(case):
  c = _MIX_CASES[case]
  for n in ((c['n'],) if 'n' in c else (0, 64)):
    assert _lib.lib().ble_dagger_mix_u8(_ref(_mix(**{'n': n, **c})), None) == E_INVALID_ARG, n
  assert _lib.lib().ble_dagger_mix_u8(None, None) == E_INVALID_ARG


@pytest.mark.parametrize('case', sorted(_MIX_POINTER_CASES))
def test_mix_null_pointer_with_rows(case):
  assert _lib.lib().ble_dagger_mix_u8(_ref(_mix(n=64, **_MIX_POINTER_CASES[case])), None) == E_INVALID_ARG
  assert _lib.lib().ble_dagger_mix_u8(_ref(_mix(n=1, **_MIX_POINTER_CASES[case])), None) == E_INVALID_ARG
