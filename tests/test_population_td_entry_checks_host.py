"""The entry points of a population of replay learners (ble_qnet_td_grouped_workspace_f32, ble_qnet_td_step_grouped_f32,
ble_replay_sample_grouped_f32, ble_qnet_explore_grouped_u8) on a machine without a GPU, in the manner of
test_population_train_entry_checks_host.py: declared, exported and mirrored field by field; every refusal answers BLE_E_INVALID_ARG
before any HIP call, over fake non-NULL pointers that are never dereferenced (no update below has valid arguments: a population has
something to launch); the workspace layout at (P, B) = (3, 515) and (2, 4 100) from a hand computation; the plain and the PPO-grouped
entry points keep their answers."""
import ctypes
import os
import re
import subprocess

import pytest

from balloon_learning_environment_amd import _abi, _lib
from descriptors_host import E_INVALID_ARG, _FAKE, _batch, _qnet, _train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()
ENTRIES = ('ble_qnet_td_grouped_workspace_f32', 'ble_qnet_td_step_grouped_f32', 'ble_replay_sample_grouped_f32',
           'ble_qnet_explore_grouped_u8')
NAN, INF = float('nan'), float('inf')
IMAGE_2_64_51 = (1104 * 64 + 64) + (64 * 192 + 192)       # the packed floats of _qnet(): 153 -> 192 padded outputs
IMAGE_2_64_1 = (1104 * 64 + 64) + (64 * 64 + 64)          # of _qnet(num_atoms=1): 3 -> 64 padded outputs
QUANTILE, DQN_MSE, DQN_HUBER = _abi.TD_GROUPED_QUANTILE, _abi.TD_DQN_MSE + 1, _abi.TD_DQN_HUBER + 1


def _fields(struct_name):
  body = HEADER[HEADER.index('typedef struct %s {' % struct_name):HEADER.index('} %s;' % struct_name)]
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  return re.findall(r'(\w+);', body)


def test_structs_match_header():
  names = _fields('ble_td_grouped_f32')
  assert names == [f[0] for f in _abi.BleTdGroupedF32._fields_]
  t = ctypes.sizeof(_abi.BleQnetTrainF32)
  assert t == 120
  assert [getattr(_abi.BleTdGroupedF32, n).offset for n in names] == [0, t, t + 4, t + 8, t + 16, t + 24, t + 32, t + 36, t + 40, t + 48]
  assert [getattr(_abi.BleTdGroupedF32, n).size for n in names] == [t, 4, 4, 8, 8, 8, 4, 4, 8, 8]
  assert ctypes.sizeof(_abi.BleTdGroupedF32) == t + 56
  names = _fields('ble_explore_grouped_f32')
  assert names == [f[0] for f in _abi.BleExploreGroupedF32._fields_] == ['n', 'members', 'reserved_', 'epsilon', 'seed', 'step']
  assert [getattr(_abi.BleExploreGroupedF32, n).offset for n in names] == [0, 8, 12, 16, 24, 32]
  assert ctypes.sizeof(_abi.BleExploreGroupedF32) == 40
  assert (QUANTILE, DQN_MSE, DQN_HUBER) == (0, 1, 2)
  assert re.search(r'#define BLE_TD_GROUPED_QUANTILE 0\b', HEADER)


def test_entries_declared_exported_and_without_int64_arguments():
  declared = set(re.findall(r'^int (ble_\w+)\(', HEADER, re.M))
  out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.build()]).decode()
  exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
  lib = _lib.lib()
  for name in ENTRIES:
    assert name in declared and name in exported and name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS, name
    assert ctypes.c_int64 not in getattr(lib, name).argtypes, name
  assert _lib.ABI_VERSION == 5 and lib.ble_abi_version() == 5 and any(s.endswith('ble_population_td.h') for s in _lib._SOURCES)


def test_image_sizes_are_the_library_s():
  floats = ctypes.c_int64()
  for net, image in ((_qnet(), IMAGE_2_64_51), (_qnet(num_atoms=1), IMAGE_2_64_1)):
    assert _lib.lib().ble_qnet_workspace_f32(ctypes.byref(net), 0, ctypes.byref(floats), None) == 0
    assert floats.value == image and image % 64 == 0


# ---- ble_qnet_td_step_grouped_f32 ------------------------------------------------------------------------------------------------------
def _tr(**fields):
  return _train(**{**dict(lr=NAN, kappa=NAN), **fields})       # (tr.lr and tr.kappa are not read)


def _grouped(**fields):
  net = fields.pop('net', None)
  tr = fields.pop('tr', None) or _tr(net=net or _qnet())
  atoms = tr.net.num_atoms
  d = dict(tr=tr, members=3, reserved_=0, member_stride=IMAGE_2_64_1 if atoms == 1 else IMAGE_2_64_51,
           transposed_stride=64 * 64 if atoms == 1 else 192 * 64, rows_per_member=33, kind=QUANTILE, reserved2_=0, lr=_FAKE, kappa=_FAKE)
  d.update(fields)
  return _abi.BleTdGroupedF32(**d)


def _td_batch(**fields):
  return _batch(**{**dict(batch=99), **fields})


def _step(g, bt, loss=_FAKE):
  return _lib.lib().ble_qnet_td_step_grouped_f32(ctypes.byref(g), ctypes.byref(bt), loss, None, None)


def test_transposed_floats_of_the_fixture_shapes():
  lay = _abi.BleQnetTrainLayout()
  for net, floats in ((_qnet(), 192 * 64), (_qnet(num_atoms=1), 64 * 64)):       # W^T of layer 1: kp' = round8(M), mp' = 64
    g = _grouped(net=net, kind=QUANTILE)
    assert _lib.lib().ble_qnet_td_grouped_workspace_f32(ctypes.byref(g), ctypes.byref(lay)) == 0
    assert lay.transposed_floats <= floats and floats % 64 == 0


_STEP_CASES = {
    # the network descriptor and the trainer's pointers: what the plain entry points refuse
    'layers_0': dict(net=_qnet(num_layers=0)), 'input_dim': dict(net=_qnet(input_dim=1098)), 'actions_2': dict(net=_qnet(num_actions=2)),
    'hidden_0': dict(net=_qnet(hidden_units=0)), 'atoms_0': dict(net=_qnet(num_atoms=0)),
    'null_weights': dict(tr=_tr(net=_qnet(weights=None))), 'null_grad': dict(tr=_tr(grad=None)), 'null_workspace': dict(tr=_tr(workspace=None)),
    'null_weights_t': dict(tr=_tr(weights_t=None)), 'null_target': dict(tr=_tr(target=None)),
    'adam_without_m': dict(tr=_tr(adam_m=None)), 'adam_without_v': dict(tr=_tr(adam_v=None)), 'adam_without_step': dict(tr=_tr(adam_step=None)),
    'adam_b1_nan': dict(tr=_tr(adam_b1=NAN)), 'adam_b2_inf': dict(tr=_tr(adam_b2=INF)), 'adam_eps_nan': dict(tr=_tr(adam_eps=NAN)),
    'unaligned_weights': dict(tr=_tr(net=_qnet(weights=_FAKE + 4))), 'unaligned_grad': dict(tr=_tr(grad=_FAKE + 8)),
    'unaligned_target': dict(tr=_tr(target=_FAKE + 4)), 'unaligned_m': dict(tr=_tr(adam_m=_FAKE + 4)), 'unaligned_v': dict(tr=_tr(adam_v=_FAKE + 4)),
    'unaligned_workspace': dict(tr=_tr(workspace=_FAKE + 4)), 'unaligned_weights_t': dict(tr=_tr(weights_t=_FAKE + 8)),
    # the kind, and the atoms it fits
    'kind_3': dict(kind=3), 'kind_negative': dict(kind=-1), 'kind_sarsa': dict(kind=_abi.TD_SARSA_MSE + 1),
    'dqn_mse_on_51_atoms': dict(kind=DQN_MSE), 'dqn_huber_on_51_atoms': dict(kind=DQN_HUBER),
    'dqn_mse_on_2_atoms': dict(kind=DQN_MSE, net=_qnet(num_atoms=2)),
    # the population's sizes
    'members_0': dict(members=0), 'members_negative': dict(members=-3), 'rows_0': dict(rows_per_member=0),
    'rows_negative': dict(rows_per_member=-33), 'reserved': dict(reserved_=1), 'reserved2': dict(reserved2_=1),
    # the strides
    'stride_short': dict(member_stride=IMAGE_2_64_51 - 64), 'stride_0': dict(member_stride=0),
    'stride_unaligned': dict(member_stride=IMAGE_2_64_51 + 32), 'stride_negative': dict(member_stride=-IMAGE_2_64_51),
    'tstride_short': dict(transposed_stride=64), 'tstride_0': dict(transposed_stride=0), 'tstride_unaligned': dict(transposed_stride=192 * 64 + 16),
    # the per-member arrays
    'null_lr': dict(lr=None), 'null_kappa': dict(kappa=None), 'unaligned_lr': dict(lr=_FAKE + 2), 'unaligned_kappa': dict(kappa=_FAKE + 1),
    'dqn_unaligned_kappa': dict(kind=DQN_MSE, net=_qnet(num_atoms=1), kappa=_FAKE + 2),
    'dqn_null_lr': dict(kind=DQN_HUBER, net=_qnet(num_atoms=1), lr=None),
    'dqn_null_target': dict(kind=DQN_HUBER, tr=_tr(net=_qnet(num_atoms=1), target=None)),
}


@pytest.mark.parametrize('case', sorted(_STEP_CASES))
def test_grouped_step_refusals_of_the_descriptor(case):
  assert _step(_grouped(**_STEP_CASES[case]), _td_batch()) == E_INVALID_ARG, case


_BATCH_CASES = {
    'batch_is_not_p_b': dict(batch=98), 'batch_of_one_member': dict(batch=33), 'batch_0': dict(batch=0), 'batch_negative': dict(batch=-99),
    'state_stride_1099': dict(state_stride=1099), 'state_stride_1098': dict(state_stride=1098), 'null_state': dict(state=None),
    'unaligned_state': dict(state=_FAKE + 4), 'null_next_state': dict(next_state=None), 'unaligned_next_state': dict(next_state=_FAKE + 8),
    'null_ret': dict(ret=None), 'null_discount': dict(discount=None), 'null_action': dict(action=None),
}


@pytest.mark.parametrize('kind,atoms', [(QUANTILE, 51), (QUANTILE, 1), (DQN_MSE, 1), (DQN_HUBER, 1)])
@pytest.mark.parametrize('case', sorted(_BATCH_CASES))
def test_grouped_step_refusals_of_the_batch(case, kind, atoms):
  assert _step(_grouped(net=_qnet(num_atoms=atoms), kind=kind), _td_batch(**_BATCH_CASES[case])) == E_INVALID_ARG, case


_SIZE_CASES = {
    'batch_above_max': (2, 2 ** 19 + 1), 'batch_above_max_by_members': (2 ** 10 + 1, 2 ** 10), 'rows_above_max': (1, 2 ** 20 + 1),
    'members_65536': (65536, 1), 'members_times_slabs_above_max': (4096, 4096), 'p_b_overflows': (2 ** 31 - 1, 2 ** 33),
}


@pytest.mark.parametrize('case', sorted(_SIZE_CASES))
def test_grouped_step_and_workspace_refuse_sizes(case):
  p, b = _SIZE_CASES[case]
  g = _grouped(members=p, rows_per_member=b)
  assert _step(g, _td_batch(batch=min(p * b, 2 ** 20))) == E_INVALID_ARG, case
  assert _lib.lib().ble_qnet_td_grouped_workspace_f32(ctypes.byref(g), ctypes.byref(_abi.BleQnetTrainLayout())) == E_INVALID_ARG, case


def test_grouped_step_nulls():
  lib = _lib.lib()
  g, bt = _grouped(), _td_batch()
  assert lib.ble_qnet_td_step_grouped_f32(None, ctypes.byref(bt), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_td_step_grouped_f32(ctypes.byref(g), None, _FAKE, None, None) == E_INVALID_ARG
  assert _step(g, bt, loss=None) == E_INVALID_ARG


def test_what_the_update_does_not_read_may_be_anything():
  """A one-layer network has no weights_t and no transposed stride; without apply_update Adam's state is not wanted; the DQN kinds read
  no kappa.  Each descriptor is still refused for the one field named: it is otherwise valid (it would launch)."""
  one = _qnet(num_layers=1, hidden_units=0, num_atoms=1)
  image = 1104 * 64 + 64
  ok = dict(tr=_tr(net=one, weights_t=None), member_stride=image, transposed_stride=-7, kind=DQN_MSE, kappa=None)
  assert _step(_grouped(**ok, lr=None), _td_batch()) == E_INVALID_ARG
  assert _step(_grouped(**{**ok, 'member_stride': image - 64}), _td_batch()) == E_INVALID_ARG
  assert _step(_grouped(**ok), _td_batch(batch=98)) == E_INVALID_ARG
  lazy = _tr(apply_update=0, adam_m=None, adam_v=None, adam_step=None, adam_b1=NAN)
  assert _step(_grouped(tr=lazy, kappa=None), _td_batch()) == E_INVALID_ARG
  assert _step(_grouped(tr=lazy), _td_batch(batch=98)) == E_INVALID_ARG


# ---- the workspace layout ------------------------------------------------------------------------------------------------------------
def _r64(v):
  return -(-v // 64) * 64


@pytest.mark.parametrize('atoms,kind', [(51, QUANTILE), (1, QUANTILE), (1, DQN_MSE), (1, DQN_HUBER)])
@pytest.mark.parametrize('p,b,slabs', [(3, 515, 2), (2, 4100, 16), (5, 33, 1), (1, 4096, 16)])
def test_workspace_layout_by_hand(p, b, slabs, atoms, kind):
  """(2, 64, atoms): ld = the padded outputs (192 for 51 atoms, 64 for one), two layers, the largest block is layer 0's 1104 * 64 + 64
  floats.  n = P B rows; targets holds n * atoms floats; the slabs are B // 256 clamped to [1, 16]; partial holds P * slabs blocks when
  slabs > 1."""
  lay = _abi.BleQnetTrainLayout()
  g = _grouped(net=_qnet(num_atoms=atoms), kind=kind, members=p, rows_per_member=b, member_stride=0, transposed_stride=0, lr=None,
               kappa=None)                                                                      # (the query reads the sizes only)
  assert _lib.lib().ble_qnet_td_grouped_workspace_f32(ctypes.byref(g), ctypes.byref(lay)) == 0
  n, ld, block = p * b, _r64(3 * atoms), 1104 * 64 + 64
  assert min(max(b // 256, 1), 16) == slabs
  at, want = 0, {}
  for name, floats in (('acts', 2 * n * ld), ('target_logits', n * ld), ('targets', n * atoms), ('dlogits', n * ld), ('scratch', 4 * n * ld),
                       ('partial', p * slabs * block if slabs > 1 else 0), ('corrections', 4)):
    want[name] = at
    at += _r64(floats)
  got = {k: getattr(lay, k) for k in want}
  assert got == want and lay.total == at and lay.slabs == slabs and lay.ld == ld
  if (p, b, atoms) == (3, 515, 51):
    assert (lay.acts, lay.target_logits, lay.targets, lay.dlogits, lay.scratch, lay.partial, lay.corrections, lay.total) == \
        (0, 593280, 889920, 968768, 1265408, 2451968, 2876288, 2876352)
  if (p, b, atoms) == (2, 4100, 1):
    assert (lay.acts, lay.target_logits, lay.targets, lay.dlogits, lay.scratch, lay.partial, lay.corrections, lay.total) == \
        (0, 1049600, 1574400, 1582656, 2107456, 4206656, 6469696, 6469760)      # (partial: 2 * 16 * 70 720 floats)
  # one member: the plain layout of the same batch
  if p == 1:
    plain = _abi.BleQnetTrainLayout()
    tr, bt = _train(net=_qnet(num_atoms=atoms)), _batch(batch=b)
    if kind == QUANTILE:
      assert _lib.lib().ble_qnet_train_workspace_f32(ctypes.byref(tr), ctypes.byref(bt), ctypes.byref(plain)) == 0
    else:
      td = _abi.BleTdF32(kind - 1, _abi.TD_OPT_ADAM, 0.0, 0, None, None)
      assert _lib.lib().ble_qnet_td_workspace_f32(ctypes.byref(tr), ctypes.byref(td), ctypes.byref(bt), ctypes.byref(plain)) == 0
    assert all(getattr(plain, f) == getattr(lay, f) for f, _ in _abi.BleQnetTrainLayout._fields_)


def test_workspace_refusals():
  lib = _lib.lib()
  lay = _abi.BleQnetTrainLayout()
  q = lambda **f: lib.ble_qnet_td_grouped_workspace_f32(ctypes.byref(_grouped(**f)), ctypes.byref(lay))
  assert q() == 0 and q(kind=DQN_MSE, net=_qnet(num_atoms=1)) == 0 and q(net=_qnet(num_atoms=1)) == 0
  for bad in (q(kind=DQN_MSE), q(kind=3), q(net=_qnet(num_layers=0)), q(members=0), q(rows_per_member=0), q(reserved_=2), q(reserved2_=2),
              lib.ble_qnet_td_grouped_workspace_f32(None, ctypes.byref(lay)),
              lib.ble_qnet_td_grouped_workspace_f32(ctypes.byref(_grouped()), None)):
    assert bad == E_INVALID_ARG


# ---- ble_replay_sample_grouped_f32 -----------------------------------------------------------------------------------------------------
def _replay(**fields):
  d = dict(capacity=12, num_envs=15, update_horizon=5, obs_stride=1104, gamma=0.993, max_tries=64, reserved_=0, obs=_FAKE, action=_FAKE,
           reward=_FAKE, terminal=_FAKE, episode_end=_FAKE, count=_FAKE, counter=_FAKE)
  d.update(fields)
  return _abi.BleReplayF32(**d)


def _sample(rp, bt, members=3, seeds=_FAKE):
  lib = _lib.lib()
  return lib.ble_replay_sample_grouped_f32(None if rp is None else ctypes.byref(rp), members, seeds, None if bt is None else ctypes.byref(bt),
                                           None, None)


def test_grouped_sampler_refusals():
  ok = _batch(batch=99)
  # an empty batch launches nothing, as the plain call
  assert _sample(_replay(), _batch()) == 0
  assert _lib.lib().ble_replay_sample_f32(ctypes.byref(_replay()), ctypes.byref(_batch()), 5, None, None) == 0
  for bad in (_sample(None, ok), _sample(_replay(), None), _sample(_replay(), ok, members=0), _sample(_replay(), ok, members=-3),
              _sample(_replay(), ok, members=2),                     # 15 columns, 2 members
              _sample(_replay(num_envs=16), ok, members=4),          # 99 rows, 4 members
              _sample(_replay(), ok, seeds=None), _sample(_replay(), ok, seeds=_FAKE + 4),
              # what the plain sampler refuses of the ring and the batch
              _sample(_replay(update_horizon=0), ok), _sample(_replay(update_horizon=65), ok), _sample(_replay(capacity=5), ok),
              _sample(_replay(num_envs=0), ok), _sample(_replay(obs_stride=1098), ok), _sample(_replay(obs_stride=1102), ok),
              _sample(_replay(gamma=NAN), ok), _sample(_replay(max_tries=0), ok), _sample(_replay(max_tries=1025), ok),
              _sample(_replay(obs=None), ok), _sample(_replay(obs=_FAKE + 4), ok), _sample(_replay(action=None), ok),
              _sample(_replay(reward=None), ok), _sample(_replay(terminal=None), ok), _sample(_replay(episode_end=None), ok),
              _sample(_replay(count=None), ok), _sample(_replay(counter=None), ok),
              _sample(_replay(), _batch(batch=-3)), _sample(_replay(), _batch(batch=99, state=None)),
              _sample(_replay(), _batch(batch=99, next_state=None)), _sample(_replay(), _batch(batch=99, discount=None)),
              _sample(_replay(), _batch(batch=99, state_stride=1099)), _sample(_replay(), _batch(batch=99, state=_FAKE + 4))):
    assert bad == E_INVALID_ARG


# ---- ble_qnet_explore_grouped_u8 -------------------------------------------------------------------------------------------------------
def _explore(action=_FAKE, **fields):
  ex = _abi.BleExploreGroupedF32(**{**dict(n=195, members=3, reserved_=0, epsilon=_FAKE, seed=_FAKE, step=7), **fields})
  return _lib.lib().ble_qnet_explore_grouped_u8(ctypes.byref(ex), action, None)


def test_grouped_explore_refusals():
  assert _explore(n=0) == 0                                          # nothing to launch
  assert _lib.lib().ble_qnet_explore_grouped_u8(None, _FAKE, None) == E_INVALID_ARG
  for bad in (_explore(action=None), _explore(n=-3), _explore(n=4 * 2147483647 * 256 + 3), _explore(members=0), _explore(members=-1),
              _explore(n=196), _explore(reserved_=1), _explore(epsilon=None), _explore(seed=None), _explore(epsilon=_FAKE + 2),
              _explore(seed=_FAKE + 4)):
    assert bad == E_INVALID_ARG


# ---- the plain and the PPO-grouped entry points keep their answers --------------------------------------------------------------------
def test_plain_and_ppo_grouped_entry_points_keep_their_answers():
  lib = _lib.lib()
  empty = _batch()
  train = lambda tr, bt=empty: lib.ble_qnet_train_step_f32(ctypes.byref(tr), ctypes.byref(bt), _FAKE, None, None)
  assert train(_train()) == 0 and train(_train(apply_update=0, adam_m=None, adam_v=None, adam_step=None, lr=NAN)) == 0
  for bad in (train(_train(kappa=0.0)), train(_train(kappa=NAN)), train(_train(target=None)), train(_train(lr=NAN)), train(_train(grad=None)),
              train(_train(), _batch(batch=-1)), train(_train(), _batch(next_state=None)), train(_train(net=_qnet(num_atoms=0)))):
    assert bad == E_INVALID_ARG
  td = lambda **f: _abi.BleTdF32(**{**dict(kind=_abi.TD_DQN_MSE, optimizer=_abi.TD_OPT_ADAM, gamma=0.0, reserved_=0, next_action=None, mask=None), **f})
  one = lambda **f: _train(net=_qnet(num_atoms=1), **f)
  step = lambda tr, d, bt=empty: lib.ble_qnet_td_step_f32(ctypes.byref(tr), ctypes.byref(d), ctypes.byref(bt), _FAKE, None, None)
  assert step(one(), td()) == 0 and step(one(kappa=NAN), td(kind=_abi.TD_DQN_HUBER)) == 0
  assert step(one(target=None), td(kind=_abi.TD_SARSA_MSE, next_action=_FAKE)) == 0
  for bad in (step(_train(), td()), step(one(), td(kind=3)), step(one(target=None), td()), step(one(lr=NAN), td()),
              step(one(), td(optimizer=2)), lib.ble_qnet_td_step_f32(ctypes.byref(one()), None, ctypes.byref(empty), _FAKE, None, None)):
    assert bad == E_INVALID_ARG
  ex = lambda **f: lib.ble_qnet_explore_u8(ctypes.byref(_abi.BleExploreF32(**{**dict(n=0, epsilon=0.5, reserved_=0, seed=1, step=2), **f})), _FAKE, None)
  assert ex() == 0 and ex(epsilon=1.5) == E_INVALID_ARG and ex(epsilon=NAN) == E_INVALID_ARG and ex(n=-1) == E_INVALID_ARG
  # the PPO-grouped update and its workspace: two atoms only, its own arrays, no target wanted
  two = _train(net=_qnet(num_atoms=2), target=None, lr=NAN, kappa=NAN)
  image, tfloats = (1104 * 64 + 64) + (64 * 64 + 64), 8 * 64
  ppo = lambda **f: _abi.BlePpoGroupedF32(**{**dict(tr=two, members=3, reserved_=0, member_stride=image, transposed_stride=tfloats,
                                                    rows_per_member=33, lr=_FAKE, clip=_FAKE, value_coef=_FAKE, entropy_coef=_FAKE,
                                                    old_logp=_FAKE, advantage=_FAKE), **f})
  pstep = lambda g, bt: lib.ble_qnet_ppo_step_grouped_f32(ctypes.byref(g), ctypes.byref(bt), _FAKE, None, None)
  on_policy = _batch(batch=98, next_state=None, discount=None)
  for bad in (pstep(ppo(), on_policy), pstep(ppo(lr=None), _batch(batch=99, next_state=None, discount=None)),
              pstep(ppo(clip=_FAKE + 2), _batch(batch=99, next_state=None, discount=None)),
              pstep(ppo(tr=_train(target=None)), _batch(batch=99, next_state=None, discount=None))):
    assert bad == E_INVALID_ARG
  lay = _abi.BleQnetTrainLayout()
  g = ppo(members=3, rows_per_member=515)
  assert lib.ble_qnet_ppo_grouped_workspace_f32(ctypes.byref(g), ctypes.byref(lay)) == 0
  assert (lay.acts, lay.target_logits, lay.targets, lay.dlogits, lay.scratch, lay.partial, lay.corrections, lay.total) == \
      (0, 197760, 296640, 299776, 398656, 794176, 1218496, 1218560)
  assert lib.ble_qnet_ppo_grouped_workspace_f32(ctypes.byref(ppo(tr=_train())), ctypes.byref(lay)) == E_INVALID_ARG
