"""The entry points of a population trained by gradient (ble_qnet_ppo_grouped_workspace_f32, ble_qnet_ppo_step_grouped_f32,
ble_ac_act_grouped_f32) on a machine without a GPU, in the manner of test_population_entry_checks_host.py: declared,
exported and mirrored field by field; every refusal answers BLE_E_INVALID_ARG before any HIP call, over fake non-NULL pointers that are
never dereferenced (no call below has valid arguments: a population has something to launch); the workspace layout at (P, B) = (3, 515)
and (2, 4 100) from a hand computation; the plain entry points keep their answers."""
import ctypes
import os
import re
import subprocess

import pytest

from balloon_learning_environment_amd import _abi, _lib
from descriptors_host import E_INVALID_ARG, _FAKE, _batch, _qnet, _train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()
ENTRIES = ('ble_qnet_ppo_grouped_workspace_f32', 'ble_qnet_ppo_step_grouped_f32', 'ble_ac_act_grouped_f32')
NAN, INF = float('nan'), float('inf')
IMAGE_2_64_2 = (1104 * 64 + 64) + (64 * 64 + 64)          # the packed floats of _qnet(num_atoms=2): 74 880
TRANSPOSED_2_64_2 = 8 * 64                                # W^T of layer 1: kp' = round8(6), mp' = 64


def _fields(struct_name):
  body = HEADER[HEADER.index('typedef struct %s {' % struct_name):HEADER.index('} %s;' % struct_name)]
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  return re.findall(r'(\w+);', body)


def test_struct_matches_header():
  names = _fields('ble_ppo_grouped_f32')
  assert names == [f[0] for f in _abi.BlePpoGroupedF32._fields_]
  t = ctypes.sizeof(_abi.BleQnetTrainF32)
  assert t == 32 + 7 * 8 + 2 * 8 + 4 * 4 == 120
  assert [getattr(_abi.BlePpoGroupedF32, n).offset for n in names] == [0, t, t + 4] + [t + 8 * k for k in range(1, 10)]
  assert [getattr(_abi.BlePpoGroupedF32, n).size for n in names] == [t, 4, 4] + [8] * 9
  assert ctypes.sizeof(_abi.BlePpoGroupedF32) == t + 80


def test_entries_declared_exported_and_without_int64_arguments():
  declared = set(re.findall(r'^int (ble_\w+)\(', HEADER, re.M))
  out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.build()]).decode()
  exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
  lib = _lib.lib()
  for name in ENTRIES:
    assert name in declared and name in exported and name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS, name
    assert ctypes.c_int64 not in getattr(lib, name).argtypes, name
  assert _lib.ABI_VERSION == 5 and lib.ble_abi_version() == 5 and any(s.endswith('ble_population_train.h') for s in _lib._SOURCES)


def test_image_sizes_are_the_library_s():
  floats, lay = ctypes.c_int64(), _abi.BleQnetTrainLayout()
  net = _qnet(num_atoms=2)
  assert _lib.lib().ble_qnet_workspace_f32(ctypes.byref(net), 0, ctypes.byref(floats), None) == 0
  assert floats.value == IMAGE_2_64_2 and IMAGE_2_64_2 % 64 == 0
  tr, bt = _train(net=net), _batch()
  assert _lib.lib().ble_qnet_train_workspace_f32(ctypes.byref(tr), ctypes.byref(bt), ctypes.byref(lay)) == 0
  assert lay.transposed_floats == TRANSPOSED_2_64_2


# ---- ble_qnet_ppo_step_grouped_f32 ---------------------------------------------------------------------------------------------------
def _grouped(**fields):
  tr = fields.pop('tr', None) or _train(net=fields.pop('net', None) or _qnet(num_atoms=2), target=None, lr=NAN, kappa=NAN)
  d = dict(tr=tr, members=3, reserved_=0, member_stride=IMAGE_2_64_2, transposed_stride=TRANSPOSED_2_64_2, rows_per_member=33, lr=_FAKE,
           clip=_FAKE, value_coef=_FAKE, entropy_coef=_FAKE, old_logp=_FAKE, advantage=_FAKE)
  d.update(fields)
  return _abi.BlePpoGroupedF32(**d)


def _ppo_batch(**fields):
  return _batch(**{**dict(batch=99, next_state=None, discount=None), **fields})


def _tr(**fields):
  return _train(**{**dict(net=_qnet(num_atoms=2), target=None), **fields})


def _step(g, bt, loss=_FAKE):
  return _lib.lib().ble_qnet_ppo_step_grouped_f32(ctypes.byref(g), ctypes.byref(bt), loss, None, None)


_STEP_CASES = {
    # the network descriptor and the trainer's pointers: what ble_qnet_ppo_step_f32 refuses
    'layers_0': dict(net=_qnet(num_layers=0, num_atoms=2)), 'input_dim': dict(net=_qnet(input_dim=1098, num_atoms=2)),
    'actions_2': dict(net=_qnet(num_actions=2, num_atoms=2)), 'hidden_0': dict(net=_qnet(hidden_units=0, num_atoms=2)),
    'atoms_1': dict(net=_qnet(num_atoms=1)), 'atoms_51': dict(net=_qnet(num_atoms=51)), 'atoms_3': dict(net=_qnet(num_atoms=3)),
    'null_weights': dict(tr=_tr(net=_qnet(num_atoms=2, weights=None))), 'null_grad': dict(tr=_tr(grad=None)),
    'null_workspace': dict(tr=_tr(workspace=None)), 'null_weights_t': dict(tr=_tr(weights_t=None)),
    'adam_without_m': dict(tr=_tr(adam_m=None)), 'adam_without_v': dict(tr=_tr(adam_v=None)), 'adam_without_step': dict(tr=_tr(adam_step=None)),
    'adam_b1_nan': dict(tr=_tr(adam_b1=NAN)), 'adam_b2_inf': dict(tr=_tr(adam_b2=INF)), 'adam_eps_nan': dict(tr=_tr(adam_eps=NAN)),
    'unaligned_weights': dict(tr=_tr(net=_qnet(num_atoms=2, weights=_FAKE + 4))), 'unaligned_grad': dict(tr=_tr(grad=_FAKE + 8)),
    'unaligned_m': dict(tr=_tr(adam_m=_FAKE + 4)), 'unaligned_v': dict(tr=_tr(adam_v=_FAKE + 4)),
    'unaligned_workspace': dict(tr=_tr(workspace=_FAKE + 4)), 'unaligned_weights_t': dict(tr=_tr(weights_t=_FAKE + 8)),
    # the population's sizes
    'members_0': dict(members=0), 'members_negative': dict(members=-3), 'rows_0': dict(rows_per_member=0),
    'rows_negative': dict(rows_per_member=-33), 'reserved': dict(reserved_=1),
    # the strides
    'stride_short': dict(member_stride=IMAGE_2_64_2 - 64), 'stride_0': dict(member_stride=0),
    'stride_unaligned': dict(member_stride=IMAGE_2_64_2 + 32), 'stride_negative': dict(member_stride=-IMAGE_2_64_2),
    'tstride_short': dict(transposed_stride=TRANSPOSED_2_64_2 - 64), 'tstride_0': dict(transposed_stride=0),
    'tstride_unaligned': dict(transposed_stride=TRANSPOSED_2_64_2 + 16),
    # the per-member arrays and the rows' arrays
    'null_lr': dict(lr=None), 'null_clip': dict(clip=None), 'null_value_coef': dict(value_coef=None),
    'null_entropy_coef': dict(entropy_coef=None), 'null_old_logp': dict(old_logp=None), 'null_advantage': dict(advantage=None),
    'unaligned_lr': dict(lr=_FAKE + 2), 'unaligned_clip': dict(clip=_FAKE + 1), 'unaligned_old_logp': dict(old_logp=_FAKE + 2),
    'unaligned_advantage': dict(advantage=_FAKE + 3),
}


@pytest.mark.parametrize('case', sorted(_STEP_CASES))
def test_grouped_step_refusals_of_the_descriptor(case):
  assert _step(_grouped(**_STEP_CASES[case]), _ppo_batch()) == E_INVALID_ARG, case


_BATCH_CASES = {
    'batch_is_not_p_b': dict(batch=98), 'batch_of_one_member': dict(batch=33), 'batch_0': dict(batch=0), 'batch_negative': dict(batch=-99),
    'state_stride_1099': dict(state_stride=1099), 'state_stride_1098': dict(state_stride=1098), 'null_state': dict(state=None),
    'unaligned_state': dict(state=_FAKE + 4), 'null_ret': dict(ret=None), 'null_action': dict(action=None),
}


@pytest.mark.parametrize('case', sorted(_BATCH_CASES))
def test_grouped_step_refusals_of_the_batch(case):
  assert _step(_grouped(), _ppo_batch(**_BATCH_CASES[case])) == E_INVALID_ARG, case


# (P, B): P B > BLE_TRAIN_MAX_BATCH = 2^20, and the grid's y (P > 65 535).  The entry also refuses P * slabs > 65 535 (the grid's z) and
# groups * P * ceil(B / 128) >= 2^31, but neither can be reached below 2^20 rows (P * slabs <= P B / 256 <= 4 096): the cases that would
# name them are refused for the batch already.
_SIZE_CASES = {
    'batch_above_max': (2, 2 ** 19 + 1), 'batch_above_max_by_members': (2 ** 10 + 1, 2 ** 10), 'rows_above_max': (1, 2 ** 20 + 1),
    'members_65536': (65536, 1), 'members_times_slabs_above_max': (4096, 4096), 'p_b_overflows': (2 ** 31 - 1, 2 ** 33),
}


@pytest.mark.parametrize('case', sorted(_SIZE_CASES))
def test_grouped_step_and_workspace_refuse_sizes(case):
  p, b = _SIZE_CASES[case]
  g = _grouped(members=p, rows_per_member=b)
  assert _step(g, _ppo_batch(batch=min(p * b, 2 ** 20))) == E_INVALID_ARG, case
  assert _lib.lib().ble_qnet_ppo_grouped_workspace_f32(ctypes.byref(g), ctypes.byref(_abi.BleQnetTrainLayout())) == E_INVALID_ARG, case


def test_grouped_step_nulls():
  lib = _lib.lib()
  g, bt = _grouped(), _ppo_batch()
  assert lib.ble_qnet_ppo_step_grouped_f32(None, ctypes.byref(bt), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_ppo_step_grouped_f32(ctypes.byref(g), None, _FAKE, None, None) == E_INVALID_ARG
  assert _step(g, bt, loss=None) == E_INVALID_ARG


def test_what_the_update_does_not_read_may_be_anything():
  """A one-layer network has no weights_t and no transposed stride; without apply_update Adam's state is not wanted.  Both are still
  refused for the one field named: the descriptor is otherwise valid (it would launch)."""
  one = _qnet(num_layers=1, hidden_units=0, num_atoms=2)
  image = 1104 * 64 + 64
  ok = dict(tr=_tr(net=one, weights_t=None), member_stride=image, transposed_stride=-7)
  assert _step(_grouped(**ok, lr=None), _ppo_batch()) == E_INVALID_ARG
  assert _step(_grouped(**{**ok, 'member_stride': image - 64}), _ppo_batch()) == E_INVALID_ARG
  lazy = _tr(apply_update=0, adam_m=None, adam_v=None, adam_step=None, adam_b1=NAN)
  assert _step(_grouped(tr=lazy, clip=None), _ppo_batch()) == E_INVALID_ARG
  assert _step(_grouped(tr=lazy), _ppo_batch(batch=98)) == E_INVALID_ARG


# ---- the workspace layout ------------------------------------------------------------------------------------------------------------
def _r64(v):
  return -(-v // 64) * 64


@pytest.mark.parametrize('p,b,slabs', [(3, 515, 2), (2, 4100, 16), (5, 33, 1), (1, 4096, 16)])
def test_workspace_layout_by_hand(p, b, slabs):
  """(2, 64, 2): ld = 64, two layers, the largest block is layer 0's 1104 * 64 + 64 floats.  n = P B rows; the slabs are B // 256
  clamped to [1, 16]; partial holds P * slabs blocks when slabs > 1."""
  lay = _abi.BleQnetTrainLayout()
  g = _grouped(members=p, rows_per_member=b, member_stride=0, transposed_stride=0, lr=None)      # (the query reads the sizes only)
  assert _lib.lib().ble_qnet_ppo_grouped_workspace_f32(ctypes.byref(g), ctypes.byref(lay)) == 0
  n, ld, block = p * b, 64, 1104 * 64 + 64
  assert min(max(b // 256, 1), 16) == slabs
  at, want = 0, {}
  for name, floats in (('acts', 2 * n * ld), ('target_logits', n * ld), ('targets', 2 * n), ('dlogits', n * ld), ('scratch', 4 * n * ld),
                       ('partial', p * slabs * block if slabs > 1 else 0), ('corrections', 4)):
    want[name] = at
    at += _r64(floats)
  got = {k: getattr(lay, k) for k in want}
  assert got == want and lay.total == at and lay.slabs == slabs and lay.ld == ld and lay.transposed_floats == TRANSPOSED_2_64_2
  if (p, b) == (3, 515):
    assert (lay.acts, lay.target_logits, lay.targets, lay.dlogits, lay.scratch, lay.partial, lay.corrections, lay.total) == \
        (0, 197760, 296640, 299776, 398656, 794176, 1218496, 1218560)
  # one member: the plain layout of the same batch
  if p == 1:
    plain = _abi.BleQnetTrainLayout()
    tr, bt = _tr(), _batch(batch=b)
    assert _lib.lib().ble_qnet_train_workspace_f32(ctypes.byref(tr), ctypes.byref(bt), ctypes.byref(plain)) == 0
    assert all(getattr(plain, f) == getattr(lay, f) for f, _ in _abi.BleQnetTrainLayout._fields_)


def test_workspace_refusals():
  lib = _lib.lib()
  lay = _abi.BleQnetTrainLayout()
  q = lambda **f: lib.ble_qnet_ppo_grouped_workspace_f32(ctypes.byref(_grouped(**f)), ctypes.byref(lay))
  assert q() == 0
  for bad in (q(net=_qnet(num_atoms=51)), q(net=_qnet(num_layers=0, num_atoms=2)), q(members=0), q(rows_per_member=0), q(reserved_=2),
              lib.ble_qnet_ppo_grouped_workspace_f32(None, ctypes.byref(lay)),
              lib.ble_qnet_ppo_grouped_workspace_f32(ctypes.byref(_grouped()), None)):
    assert bad == E_INVALID_ARG


# ---- ble_ac_act_grouped_f32 ----------------------------------------------------------------------------------------------------------
def _pop(**fields):
  d = dict(net=_qnet(num_atoms=2), members=3, head=_abi.POP_HEAD_ACTOR_GREEDY, member_stride=IMAGE_2_64_2, rows_per_member=33,
           obs_row_stride=_lib.OBS_DIM, obs=_FAKE, scratch=_FAKE, action=_FAKE, q_values=None, value=_FAKE, probs=None)
  d.update(fields)
  return _abi.BleQnetGroupedF32(**d)


def _sample(**fields):
  return _abi.BleAcSample(**{**dict(seed=5, env_offset=0, step=_FAKE, reserved_=0), **fields})


_ACT_CASES = {
    'layers_0': dict(net=_qnet(num_layers=0, num_atoms=2)), 'atoms_51': dict(net=_qnet(num_atoms=51)), 'atoms_1': dict(net=_qnet(num_atoms=1)),
    'null_weights': dict(net=_qnet(num_atoms=2, weights=None)), 'unaligned_weights': dict(net=_qnet(num_atoms=2, weights=_FAKE + 4)),
    'null_obs': dict(obs=None), 'null_scratch': dict(scratch=None), 'unaligned_scratch': dict(scratch=_FAKE + 8), 'null_action': dict(action=None),
    'obs_stride_1098': dict(obs_row_stride=1098), 'members_0': dict(members=0), 'rows_0': dict(rows_per_member=0),
    'grid_product': dict(members=2 ** 16, rows_per_member=2 ** 15), 'stride_short': dict(member_stride=IMAGE_2_64_2 - 64),
    'stride_unaligned': dict(member_stride=IMAGE_2_64_2 + 32), 'head_q': dict(head=_abi.POP_HEAD_Q, value=None),
    'head_q_on_q_network': dict(head=_abi.POP_HEAD_Q, net=_qnet(), member_stride=(1104 * 64 + 64) + (64 * 192 + 192), value=None),
    'head_2': dict(head=2), 'with_q_values': dict(q_values=_FAKE),
}


@pytest.mark.parametrize('sampled', [False, True])
@pytest.mark.parametrize('case', sorted(_ACT_CASES))
def test_grouped_act_refusals(case, sampled):
  s = _sample()
  got = _lib.lib().ble_ac_act_grouped_f32(ctypes.byref(_pop(**_ACT_CASES[case])), ctypes.byref(s) if sampled else None, _FAKE, None)
  assert got == E_INVALID_ARG, case


def test_grouped_act_refusals_of_logp_and_sample():
  lib = _lib.lib()
  pop, s = _pop(), _sample()
  assert lib.ble_ac_act_grouped_f32(None, ctypes.byref(s), _FAKE, None) == E_INVALID_ARG
  assert lib.ble_ac_act_grouped_f32(ctypes.byref(pop), ctypes.byref(s), None, None) == E_INVALID_ARG
  assert lib.ble_ac_act_grouped_f32(ctypes.byref(pop), None, None, None) == E_INVALID_ARG
  for bad in (_sample(step=None), _sample(env_offset=-1)):
    assert lib.ble_ac_act_grouped_f32(ctypes.byref(pop), ctypes.byref(bad), _FAKE, None) == E_INVALID_ARG


# ---- the plain entry points keep their answers ---------------------------------------------------------------------------------------
def test_plain_entry_points_keep_their_answers():
  lib = _lib.lib()
  ppo = lambda **f: _abi.BlePpoF32(**{**dict(clip=0.2, value_coef=0.5, entropy_coef=0.01, reserved_=0, old_logp=_FAKE, advantage=_FAKE), **f})
  step = lambda tr, p, bt: lib.ble_qnet_ppo_step_f32(ctypes.byref(tr), ctypes.byref(p), ctypes.byref(bt), _FAKE, None, None)
  empty = _batch(next_state=None, discount=None)
  assert step(_tr(), ppo(), empty) == 0
  assert step(_tr(apply_update=0, adam_m=None, adam_v=None, adam_step=None, lr=NAN), ppo(), empty) == 0
  for bad in (step(_tr(net=_qnet()), ppo(), empty), step(_tr(), ppo(clip=0.0), empty), step(_tr(), ppo(clip=NAN), empty),
              step(_tr(), ppo(old_logp=None), empty), step(_tr(), ppo(advantage=None), empty), step(_tr(lr=NAN), ppo(), empty),
              step(_tr(grad=None), ppo(), empty), step(_tr(adam_m=None), ppo(), empty), step(_tr(), ppo(), _batch(batch=-1)),
              step(_tr(weights_t=None), ppo(), _batch(batch=32, next_state=None, discount=None)),
              lib.ble_qnet_ppo_step_f32(ctypes.byref(_tr()), None, ctypes.byref(empty), _FAKE, None, None)):
    assert bad == E_INVALID_ARG
  # the grouped forward: its refusals, head by head, as before the checks moved into one function
  grouped = lambda **f: lib.ble_qnet_forward_grouped_f32(ctypes.byref(_pop(**f)), None)
  for bad in (grouped(members=0), grouped(rows_per_member=0), grouped(head=2), grouped(q_values=_FAKE), grouped(net=_qnet(num_atoms=51)),
              grouped(head=_abi.POP_HEAD_Q), grouped(scratch=None), grouped(member_stride=IMAGE_2_64_2 + 32),
              grouped(members=2, rows_per_member=2 ** 62), grouped(members=2 ** 31 // 1, rows_per_member=1),
              lib.ble_qnet_forward_grouped_f32(None, None)):
    assert bad == E_INVALID_ARG
  rows = lambda **f: _abi.BleAcRowsF32(**{**dict(n=0, obs_row_stride=_lib.OBS_DIM, obs=_FAKE, action=_FAKE, logp=_FAKE, value=_FAKE, probs=None), **f})
  act = lambda net, r, s=None: lib.ble_ac_act_f32(ctypes.byref(net), ctypes.byref(r), _FAKE, None if s is None else ctypes.byref(s), None)
  assert act(_qnet(num_atoms=2), rows()) == 0 and act(_qnet(num_atoms=2), rows(), _sample(env_offset=99)) == 0
  for bad in (act(_qnet(num_atoms=51), rows()), act(_qnet(num_atoms=2), rows(logp=None)), act(_qnet(num_atoms=2), rows(n=-1)),
              act(_qnet(num_atoms=2), rows(), _sample(step=None)), act(_qnet(num_atoms=2), rows(), _sample(env_offset=-1)),
              act(_qnet(num_atoms=2, weights=None), rows(n=64))):
    assert bad == E_INVALID_ARG
