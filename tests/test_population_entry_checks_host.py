"""The population entry points (ble_qnet_forward_grouped_f32, ble_es_perturb_f32, ble_es_gradient_f32, ble_qnet_apply_grad_f32) on a
machine without a GPU, in the manner of test_fleet_host.py: declared, exported and mirrored field by field (their sizes travel in
structs: no int64 argument); every refusal answers BLE_E_INVALID_ARG before any HIP call, over fake non-NULL pointers that are never
dereferenced.  No call below has valid arguments and something to launch (n = 0 cannot occur for a population), so a case differs from
the valid descriptor the GPU tests use in the one field it names.  The plain entry points keep their answers."""
import ctypes
import os
import re
import subprocess

import pytest

from balloon_learning_environment_amd import _abi, _lib
from descriptors_host import E_INVALID_ARG, _FAKE, _batch, _qnet, _train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()
ENTRIES = ('ble_qnet_forward_grouped_f32', 'ble_es_perturb_f32', 'ble_es_gradient_f32', 'ble_qnet_apply_grad_f32')
NAN, INF = float('nan'), float('inf')
IMAGE_2_64_51 = (1104 * 64 + 64) + (64 * 192 + 192)          # the packed floats of descriptors_host._qnet(): 83 200


def _fields(struct_name):
  body = HEADER[HEADER.index('typedef struct %s {' % struct_name):HEADER.index('} %s;' % struct_name)]
  return re.findall(r'(\w+);', body)


def test_structs_match_header():
  assert _fields('ble_qnet_grouped_f32') == [f[0] for f in _abi.BleQnetGroupedF32._fields_]
  assert _fields('ble_es_f32') == [f[0] for f in _abi.BleEsF32._fields_]
  q = ctypes.sizeof(_abi.BleQnetF32)
  assert q == 32
  assert [getattr(_abi.BleQnetGroupedF32, n).offset for n in _fields('ble_qnet_grouped_f32')] == [0, q, q + 4] + [q + 8 * k for k in range(1, 10)]
  assert [getattr(_abi.BleEsF32, n).offset for n in _fields('ble_es_f32')] == [0, q, q + 4, q + 8, q + 16, q + 24, q + 28, q + 32, q + 40]
  defines = dict(re.findall(r'#define (BLE_POP_HEAD_\w+) (\d+)', HEADER))
  assert int(defines['BLE_POP_HEAD_Q']) == _abi.POP_HEAD_Q == 0 and int(defines['BLE_POP_HEAD_ACTOR_GREEDY']) == _abi.POP_HEAD_ACTOR_GREEDY == 1


def test_entries_declared_exported_and_without_int64_arguments():
  declared = set(re.findall(r'^int (ble_\w+)\(', HEADER, re.M))
  out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.build()]).decode()
  exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
  lib = _lib.lib()
  for name in ENTRIES:
    assert name in declared and name in exported and name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS, name
    assert ctypes.c_int64 not in getattr(lib, name).argtypes, name
  assert _lib.ABI_VERSION == 5 and any(s.endswith('ble_population.h') for s in _lib._SOURCES)


# ---- ble_qnet_forward_grouped_f32 ----------------------------------------------------------------------------------------------------
def _grouped(**fields):
  d = dict(net=_qnet(), members=3, head=_abi.POP_HEAD_Q, member_stride=IMAGE_2_64_51, rows_per_member=33, obs_row_stride=_lib.OBS_DIM,
           obs=_FAKE, scratch=_FAKE, action=_FAKE, q_values=_FAKE, value=None, probs=None)
  d.update(fields)
  return _abi.BleQnetGroupedF32(**d)


def test_image_size_is_the_library_s():
  floats = ctypes.c_int64()
  net = _qnet()
  assert _lib.lib().ble_qnet_workspace_f32(ctypes.byref(net), 0, ctypes.byref(floats), None) == 0
  assert floats.value == IMAGE_2_64_51 and IMAGE_2_64_51 % 64 == 0


_GROUPED_CASES = {
    'layers_0': dict(net=_qnet(num_layers=0)), 'input_dim': dict(net=_qnet(input_dim=1098)), 'actions_2': dict(net=_qnet(num_actions=2)),
    'atoms_0': dict(net=_qnet(num_atoms=0)), 'hidden_0': dict(net=_qnet(hidden_units=0)), 'null_weights': dict(net=_qnet(weights=None)),
    'unaligned_weights': dict(net=_qnet(weights=_FAKE + 4)), 'null_obs': dict(obs=None), 'null_scratch': dict(scratch=None),
    'unaligned_scratch': dict(scratch=_FAKE + 8), 'null_action': dict(action=None), 'obs_stride_1098': dict(obs_row_stride=1098),
    'members_0': dict(members=0), 'members_negative': dict(members=-2), 'rows_0': dict(rows_per_member=0),
    'rows_negative': dict(rows_per_member=-1),
    # groups = 192 / 64 = 3: P R >= 2^31 / 3 is refused, whichever factor is large
    'grid_rows': dict(members=1, rows_per_member=2 ** 31 // 3), 'grid_members': dict(members=2 ** 31 // 3, rows_per_member=1),
    'grid_product': dict(members=2 ** 16, rows_per_member=2 ** 15), 'rows_2_63': dict(members=2, rows_per_member=2 ** 62),
    'stride_short': dict(member_stride=IMAGE_2_64_51 - 64), 'stride_0': dict(member_stride=0),
    'stride_unaligned': dict(member_stride=IMAGE_2_64_51 + 32), 'stride_negative': dict(member_stride=-IMAGE_2_64_51),
    'head_2': dict(head=2), 'head_negative': dict(head=-1),
    'actor_on_51_atoms': dict(head=_abi.POP_HEAD_ACTOR_GREEDY, q_values=None), 'actor_on_1_atom': dict(net=_qnet(num_atoms=1),
                                                                                                     head=_abi.POP_HEAD_ACTOR_GREEDY, q_values=None),
    'actor_with_q_values': dict(net=_qnet(num_atoms=2), head=_abi.POP_HEAD_ACTOR_GREEDY, member_stride=1104 * 64 + 64 + 64 * 64 + 64),
    'value_with_q_head': dict(value=_FAKE), 'probs_with_q_head': dict(probs=_FAKE),
}


@pytest.mark.parametrize('case', sorted(_GROUPED_CASES))
def test_grouped_forward_refusals(case):
  desc = _grouped(**_GROUPED_CASES[case])
  assert _lib.lib().ble_qnet_forward_grouped_f32(ctypes.byref(desc), None) == E_INVALID_ARG, case


def test_grouped_forward_null_descriptor():
  assert _lib.lib().ble_qnet_forward_grouped_f32(None, None) == E_INVALID_ARG


# ---- ble_es_perturb_f32, ble_es_gradient_f32 -----------------------------------------------------------------------------------------
def _es(**fields):
  d = dict(net=_qnet(), members=8, antithetic=1, member_stride=IMAGE_2_64_51, population=_FAKE, sigma=0.02, weight_decay=0.0, seed=1,
           generation=_FAKE)
  d.update(fields)
  return _abi.BleEsF32(**d)


_ES_CASES = {
    'layers_0': dict(net=_qnet(num_layers=0)), 'atoms_0': dict(net=_qnet(num_atoms=0)), 'members_0': dict(members=0),
    'members_negative': dict(members=-4), 'odd_antithetic': dict(members=7), 'null_generation': dict(generation=None),
    'sigma_0': dict(sigma=0.0), 'sigma_negative': dict(sigma=-0.02), 'sigma_nan': dict(sigma=NAN), 'sigma_inf': dict(sigma=INF),
    'weight_decay_nan': dict(weight_decay=NAN), 'weight_decay_inf': dict(weight_decay=INF),
}
_PERTURB_CASES = {
    **_ES_CASES, 'null_theta': dict(net=_qnet(weights=None)), 'null_population': dict(population=None),
    'unaligned_population': dict(population=_FAKE + 4), 'stride_short': dict(member_stride=IMAGE_2_64_51 - 64),
    'stride_unaligned': dict(member_stride=IMAGE_2_64_51 + 16),
}


@pytest.mark.parametrize('case', sorted(_PERTURB_CASES))
def test_perturb_refusals(case):
  es = _es(**_PERTURB_CASES[case])
  assert _lib.lib().ble_es_perturb_f32(ctypes.byref(es), None) == E_INVALID_ARG, case


@pytest.mark.parametrize('case', sorted(_ES_CASES))
def test_gradient_refusals_of_the_descriptor(case):
  es, tr = _es(**_ES_CASES[case]), _train()
  assert _lib.lib().ble_es_gradient_f32(ctypes.byref(es), ctypes.byref(tr), _FAKE, None) == E_INVALID_ARG, case


@pytest.mark.parametrize('case', ['null_es', 'null_tr', 'null_w', 'null_grad', 'null_theta', 'other_shape', 'other_atoms', 'unaligned_grad'])
def test_gradient_refusals_of_the_trainer(case):
  es, tr, w = _es(), _train(), _FAKE
  if case == 'null_w':
    w = None
  elif case == 'null_grad':
    tr = _train(grad=None)
  elif case == 'null_theta':
    tr = _train(net=_qnet(weights=None))
  elif case == 'other_shape':
    tr = _train(net=_qnet(hidden_units=128))
  elif case == 'other_atoms':
    tr = _train(net=_qnet(num_atoms=2))
  elif case == 'unaligned_grad':
    tr = _train(grad=_FAKE + 4)
  got = _lib.lib().ble_es_gradient_f32(None if case == 'null_es' else ctypes.byref(es), None if case == 'null_tr' else ctypes.byref(tr), w, None)
  assert got == E_INVALID_ARG, case


# ---- ble_qnet_apply_grad_f32 ---------------------------------------------------------------------------------------------------------
def test_apply_grad_without_apply_update_does_nothing():
  lib = _lib.lib()
  assert lib.ble_qnet_apply_grad_f32(ctypes.byref(_train(apply_update=0)), None) == 0
  # what Adam alone reads may then be anything
  assert lib.ble_qnet_apply_grad_f32(ctypes.byref(_train(apply_update=0, adam_m=None, adam_v=None, adam_step=None, lr=NAN, adam_b1=NAN)), None) == 0
  assert lib.ble_qnet_apply_grad_f32(ctypes.byref(_train(apply_update=0, net=_qnet(num_layers=1, hidden_units=0), weights_t=None)), None) == 0


_APPLY_CASES = {
    'layers_0': dict(net=_qnet(num_layers=0)), 'null_weights': dict(net=_qnet(weights=None)), 'null_grad': dict(grad=None),
    'null_workspace': dict(workspace=None), 'null_weights_t': dict(weights_t=None), 'lr_nan': dict(lr=NAN), 'lr_inf': dict(lr=INF),
    'adam_without_m': dict(adam_m=None), 'adam_without_v': dict(adam_v=None), 'adam_without_step': dict(adam_step=None),
    'adam_b1_nan': dict(adam_b1=NAN), 'adam_b2_inf': dict(adam_b2=INF), 'adam_eps_nan': dict(adam_eps=NAN),
    'unaligned_grad': dict(grad=_FAKE + 4), 'unaligned_m': dict(adam_m=_FAKE + 8), 'unaligned_workspace': dict(workspace=_FAKE + 4),
}


@pytest.mark.parametrize('case', sorted(_APPLY_CASES))
def test_apply_grad_refusals(case):
  assert _lib.lib().ble_qnet_apply_grad_f32(ctypes.byref(_train(**_APPLY_CASES[case])), None) == E_INVALID_ARG, case


def test_apply_grad_null_descriptor():
  assert _lib.lib().ble_qnet_apply_grad_f32(None, None) == E_INVALID_ARG


# ---- the plain entry points keep their answers ---------------------------------------------------------------------------------------
def test_plain_entry_points_keep_their_answers():
  lib = _lib.lib()
  net = _qnet()
  fwd = lambda net, obs=_FAKE, stride=_lib.OBS_DIM, scratch=_FAKE, action=_FAKE, n=0: lib.ble_qnet_forward_f32(
      ctypes.byref(net), obs, stride, scratch, action, None, n, None)
  assert fwd(net) == 0
  for bad in (fwd(_qnet(num_layers=0)), fwd(_qnet(weights=None)), fwd(net, obs=None), fwd(net, scratch=None), fwd(net, action=None),
              fwd(net, n=-1), fwd(net, stride=1098), fwd(net, scratch=_FAKE + 4), fwd(net, n=2 ** 31 // 3 * 128 + 1),
              fwd(_qnet(weights=None), n=64)):
    assert bad == E_INVALID_ARG
  rows = lambda **f: _abi.BleAcRowsF32(**{**dict(n=0, obs_row_stride=_lib.OBS_DIM, obs=_FAKE, action=_FAKE, logp=_FAKE, value=_FAKE, probs=None), **f})
  act = lambda net, r: lib.ble_ac_act_f32(ctypes.byref(net), ctypes.byref(r), _FAKE, None, None)
  assert act(_qnet(num_atoms=2), rows()) == 0
  for bad in (act(_qnet(num_atoms=51), rows()), act(_qnet(num_atoms=2), rows(logp=None)), act(_qnet(num_atoms=2), rows(n=-1)),
              act(_qnet(num_atoms=2), rows(obs_row_stride=1098)), act(_qnet(num_atoms=2, weights=None), rows(n=64))):
    assert bad == E_INVALID_ARG
  step = lambda tr, bt: lib.ble_qnet_train_step_f32(ctypes.byref(tr), ctypes.byref(bt), _FAKE, None, None)
  assert step(_train(), _batch()) == 0
  assert step(_train(apply_update=0, adam_m=None, adam_v=None, adam_step=None), _batch()) == 0
  for bad in (step(_train(kappa=0.0), _batch()), step(_train(target=None), _batch()), step(_train(grad=None), _batch()),
              step(_train(lr=NAN), _batch()), step(_train(adam_m=None), _batch()), step(_train(), _batch(batch=-1)),
              step(_train(), _batch(state_stride=1099)), step(_train(weights_t=None), _batch(batch=32))):
    assert bad == E_INVALID_ARG
