"""The Q-network descriptors of the host argument-check tests (test_train_host, test_td_host, test_entry_checks_host): each builder
gives a valid descriptor over fake device addresses, a case replaces some of its fields.  No call with them launches."""
from balloon_learning_environment_amd import _abi, _lib

E_INVALID_ARG = -1
_FAKE = 0x100000          # a non-NULL, 16-byte aligned address for every device pointer (never dereferenced)


def _qnet(**fields):
  d = dict(num_layers=2, input_dim=_lib.OBS_DIM, hidden_units=64, num_actions=3, num_atoms=51, reserved_=0, weights=_FAKE)
  d.update(fields)
  return _abi.BleQnetF32(**d)


def _batch(**fields):
  d = dict(batch=0, state_stride=1104, state=_FAKE, next_state=_FAKE, ret=_FAKE, discount=_FAKE, action=_FAKE, index=None)
  d.update(fields)
  return _abi.BleTrainBatchF32(**d)


def _train(**fields):
  net = fields.pop('net', None) or _qnet()
  d = dict(net=net, target=_FAKE, weights_t=_FAKE, grad=_FAKE, adam_m=_FAKE, adam_v=_FAKE, adam_step=_FAKE, workspace=_FAKE, lr=2e-6,
           adam_b1=0.9, adam_b2=0.999, adam_eps=2e-5, kappa=1.0, apply_update=1)
  d.update(fields)
  return _abi.BleQnetTrainF32(**d)
