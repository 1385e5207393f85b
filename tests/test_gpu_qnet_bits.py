"""The Q-network kernels -- ble_qnet_dense_kernel, ble_qnet_head_kernel, ble_qr_loss_kernel, ble_td_loss_kernel, ble_qnet_dgrad_kernel,
ble_qnet_wgrad_kernel, ble_wgrad_reduce_kernel -- against the fma-chain twin (emul/qnet_emul.cpp), bit for bit.

DESIGN §3f / §3g state that every output element is ONE k-ordered fp32 fma chain; every "member p == its own trainer" test in the
suite leans on that.  The twin walks that chain with std::fmaf from the documented order alone.  Every comparison here is on
view(np.uint32); a NaN is compared with isnan only (its payload is no part of the contract).  tests/test_qnet_emul_host.py shows, on
the host, which share of these elements each mutant of the order would change.

 a. one MFMA step against bits written out by hand, before anything else: if one of these fails, nothing below means anything;
 b. the forward at every shape of qnet_bits_cases.FORWARD_SHAPES: every layer with its padded columns, logits, q, action;
    subnormals, -0.0 and a NaN in a test of their own;
 c. the observation's row stride;
 d. the head on crafted logits;
 e. the QR and DQN loss heads, the chain held end to end from the twin's own logits;
 f. the gradient image, padding included, from one row to 16 ragged slabs; PPO's backward from the device's dlogits; the image
    after an update.
"""
import ctypes

import numpy as np
import pytest
import torch

import qnet_bits_cases as cases
from emul import qnet_emul

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mods():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  import types
  from balloon_learning_environment_amd import _lib, device
  from balloon_learning_environment_amd.agents import actor_critic, dqn_agent, qnet, qnet_train
  return types.SimpleNamespace(_lib=_lib, dev=device, actor_critic=actor_critic, dqn_agent=dqn_agent, qnet=qnet, qnet_train=qnet_train)


@pytest.fixture(scope='module')
def block(mods):
  """The 129-row block (qnet_bits_cases.block): 64 device observations of real balloons (reset + three random steps of 16
  environments), 48 random rows, 16 rows spanning 1e-6 .. 1e3 with both signs, one all-zero row."""
  from balloon_learning_environment_amd.env import balloon_env
  env = balloon_env.VecBalloonEnv(16, seed=3)
  rows = [env.reset().clone()]
  g = torch.Generator(device='cuda').manual_seed(0)
  for _ in range(3):
    obs, _, _ = env.step(torch.randint(0, 3, (16,), dtype=torch.uint8, device='cuda', generator=g))
    rows.append(obs.clone())
  env.check_errors()
  return cases.block(torch.cat(rows).cpu().numpy()[:, :cases.OBS_DIM])


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
  """Bitwise equality; on a mismatch the message names the stage, the first element and both values' bits."""
  got, want = _bits(got), _bits(want)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  bad = np.argwhere(got != want)
  assert len(bad) == 0, (f'{what}: {len(bad)} of {got.size} elements differ, first at {tuple(bad[0])}: device '
                         f'{hex(got[tuple(bad[0])])}, twin {hex(want[tuple(bad[0])])}')


def _device_forward(mods, net, x, stride=None):
  """ble_qnet_forward_f32 of one network on rows x (numpy [n, 1099]): (action uint8 [n], q [n, 3], the last layer's padded output
  [n, round64(3 atoms)]).  stride: the rows inside a NaN-filled buffer of that row stride."""
  net.to_device()
  n = x.shape[0]
  if stride is None:
    obs = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
  else:
    buf = torch.full((n, stride), float('nan'), dtype=torch.float32, device='cuda')
    buf[:, :cases.OBS_DIM] = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    obs = buf[:, :cases.OBS_DIM]
  floats = ctypes.c_int64()
  mods._lib.call('ble_qnet_workspace_f32', ctypes.byref(net._struct), n, None, ctypes.byref(floats))
  scratch = torch.zeros(floats.value, dtype=torch.float32, device='cuda')
  action = torch.empty(n, dtype=torch.uint8, device='cuda')
  q = torch.empty(n, 3, dtype=torch.float32, device='cuda')
  mods._lib.call('ble_qnet_forward_f32', ctypes.byref(net._struct), obs.data_ptr(), max(obs.stride(0), cases.OBS_DIM), scratch.data_ptr(),
                 action.data_ptr(), q.data_ptr(), n, mods.dev.stream_ptr(obs.device))
  ld = floats.value // (2 * n)
  off = ((net.num_layers - 1) & 1) * n * ld
  mp = qnet_emul.round_up(3 * net.num_atoms, 64)
  return action.cpu().numpy(), q.cpu().numpy(), scratch[off:off + n * ld].view(n, ld)[:, :mp].cpu().numpy()


def _network(mods, tree, atoms):
  return mods.qnet.QNetwork.from_params(tree, num_atoms=atoms)


def _packed(mods, tree, atoms):
  """The package's own packer: a logical tree's device image."""
  return _network(mods, tree, atoms).packed_host


def _train_batch(mods, state, next_state, ret, discount, action):
  return mods.qnet_train.TrainBatch.from_tensors(state, next_state, ret, discount, action, 'cuda')


def _set_image(mods, tensor, tree, atoms):
  tensor.copy_(torch.from_numpy(_packed(mods, tree, atoms)))


def _hold_forward_stages(tr, b, layers, up_acts):
  """Every online layer's kept output, padded columns included, against the twin's; the first layer that differs is named."""
  acts = tr.views(b)['acts']
  for l in range(len(layers)):
    mp = qnet_emul.round_up(layers[l][0].shape[1], 64)
    _same(acts[l][:, :mp].cpu().numpy(), up_acts[l], f'layer {l}')


def _hold_update(mods, tr, tree, bt, up, atoms):
  """One train_on_batch(apply_update=False) against twin_update's dict, stage by stage in launch order, then the gradient image."""
  b = len(bt[4])
  loss = tr.train_on_batch(_train_batch(mods, *bt), apply_update=False).cpu().numpy()
  layers = qnet_emul.layers_of(tree)
  _hold_forward_stages(tr, b, layers, up['acts'])
  v = tr.views(b)
  mp = qnet_emul.round_up(3 * atoms, 64)
  ws, lay, _ = tr.workspace(b)
  tl = ws[lay.target_logits:lay.target_logits + b * lay.ld].view(b, lay.ld)[:, :mp].cpu().numpy()
  _same(tl, up['target_logits'], 'target logits')
  _same(v['targets'].cpu().numpy(), up['targets'].reshape(b, -1), 'targets')
  _same(loss, up['loss'], 'loss')
  dl = v['dlogits'].cpu().numpy()
  _same(dl[:, :mp], up['dlogits'], 'dlogits')
  assert not _bits(dl[:, mp:]).any(), 'dlogits: the columns past the last layer\'s are not +0.0'
  _same(tr.grad.cpu().numpy(), _packed(mods, up['grad'], atoms), 'gradient image')


# ------------------------------------------------------------------------------------------------------------- a. one step, by hand
def _hand(mods, name):
  tree, rows, expected = cases.hand_case(cases.HAND_TRIPLES[name])
  _, _, logits = _device_forward(mods, _network(mods, tree, 1), rows)
  got = _bits(logits)
  for row, logit, bits, why in expected:
    assert got[row, logit] == bits, (f'{name}: row {row} logit {logit} ({why}): device {hex(got[row, logit])}, by hand {hex(bits)}')
  _same(logits, qnet_emul.forward(qnet_emul.layers_of(tree), rows)[-1], f'{name}: logits')


def test_one_step_columns_0_and_1(mods):
  _hand(mods, 'adjacent')


def test_one_step_columns_4_and_0_the_two_halves(mods):
  _hand(mods, 'halves')


def test_one_step_columns_8_and_0_two_chunks(mods):
  _hand(mods, 'chunks')


# ------------------------------------------------------------------------------------------------------------------------ b. forward
_TWIN = {}


def _twin_forward(shape, rows):
  """(tree, layers, the twin's padded layer outputs, q, action) of a shape on its rows, once."""
  if shape not in _TWIN:
    tree = cases.params(*shape)
    layers = qnet_emul.layers_of(tree)
    outs = qnet_emul.forward(layers, rows)
    _TWIN[shape] = (tree, layers, outs) + qnet_emul.head(outs[-1], shape[2])
  return _TWIN[shape]


def _hold_forward(mods, shape, rows, sizes):
  tree, layers, outs, q, action = _twin_forward(shape, rows)
  atoms = shape[2]
  net = _network(mods, tree, atoms)
  for n in sizes:                            # the whole block, then its first rows again: other row tiles, the same bits
    a_d, q_d, z_d = _device_forward(mods, net, rows[:n])
    _same(z_d, outs[-1][:n], f'{shape} n = {n}: logits')
    _same(q_d, q[:n], f'{shape} n = {n}: q')
    assert np.array_equal(a_d, action[:n]), (shape, n, 'action')
  # the layers below the last: the trainer keeps them (apply_update=False)
  n = len(rows)
  tr = mods.qnet_train.QNetworkTrainer(net)
  zeros = np.zeros(n, np.float32)
  tr.train_on_batch(_train_batch(mods, rows, rows, zeros, zeros, np.zeros(n, np.uint8)), apply_update=False)
  _hold_forward_stages(tr, n, layers, outs)
  # these rows (the device observations among them) meet the host test's condition too: each mutant changes a quarter of the logits
  out = 3 * atoms
  for order in qnet_emul.FORWARD_MUTANTS:
    mutant = qnet_emul.forward(layers, rows, order)[-1][:, :out]
    share = float((_bits(mutant) != _bits(outs[-1][:, :out])).mean())
    print(f'{shape}: mutant {order} changes {share:.3f} of the logits')
    assert share >= 0.25, (shape, order, share)


@pytest.mark.parametrize('shape', cases.FORWARD_SHAPES)
def test_forward(mods, block, shape):
  _hold_forward(mods, shape, block, (129, 33, 1))


def test_forward_reference_network(mods, block):
  _hold_forward(mods, cases.REFERENCE_SHAPE, cases.reference_rows(block), (cases.REFERENCE_ROWS, 1))


def test_forward_subnormals_negative_zero_and_nan(mods, block):
  """A row of subnormals, a row with -0.0 entries, a row with one NaN in column 1098, after the block: the NaN row is NaN where the
  twin's is, every other row's bits are the twin's, and the block's own rows are what they were without these neighbours."""
  shape = (3, 37, 7)
  tree, layers, outs, q, action = _twin_forward(shape, block)
  rows = np.concatenate([block, cases.special_rows(block[70])])
  extra = qnet_emul.forward(layers, rows[129:])[-1]
  q_x, a_x = qnet_emul.head(extra, 7)
  a_d, q_d, z_d = _device_forward(mods, _network(mods, tree, 7), rows)
  _same(z_d[:129], outs[-1], 'the block\'s logits next to the special rows')
  _same(q_d[:129], q, 'the block\'s q next to the special rows')
  _same(z_d[129], extra[0], 'subnormal row: logits')
  _same(z_d[130], extra[1], '-0.0 row: logits')
  _same(q_d[129:131], q_x[:2], 'subnormal and -0.0 rows: q')
  assert np.isnan(extra[2, :21]).all(), 'the twin\'s NaN row'
  assert np.array_equal(np.isnan(z_d[131]), np.isnan(extra[2])) and np.array_equal(np.isnan(q_d[131]), np.isnan(q_x[2]))
  assert np.array_equal(a_d[:129], action) and np.array_equal(a_d[129:], a_x)


# ----------------------------------------------------------------------------------------------------------------- c. the row stride
def test_observation_stride(mods, block):
  shape = (3, 37, 7)
  tree, _, outs, q, action = _twin_forward(shape, block)
  a_d, q_d, z_d = _device_forward(mods, _network(mods, tree, 7), block, stride=1157)
  _same(z_d, outs[-1], 'stride 1157: logits')
  _same(q_d, q, 'stride 1157: q')
  assert np.array_equal(a_d, action)


# ---------------------------------------------------------------------------------------------------------------------- d. the head
def _crafted(mods, table, atoms, scale=None):
  """Logits made to order: a 1-layer network whose kernel row r is table[r] and whose bias is 0, on one-hot rows x[r][r] = scale[r]
  (default 1): logit[r][m] = fma(scale, table[r][m], +0.0) + 0.0.  (device logits, q, action) and the twin's."""
  n, out = table.shape
  w = np.zeros((cases.OBS_DIM, out), np.float32)
  w[:n] = table
  x = np.zeros((n, cases.OBS_DIM), np.float32)
  x[np.arange(n), np.arange(n)] = 1.0 if scale is None else scale
  tree = {'params': {'Dense_0': {'kernel': w, 'bias': np.zeros(out, np.float32)}}}
  a_d, q_d, z_d = _device_forward(mods, _network(mods, tree, atoms), x)
  z_t = qnet_emul.forward(qnet_emul.layers_of(tree), x)[-1]
  _same(z_d, z_t, 'crafted logits')
  return z_t, q_d, a_d


def test_head_ties_and_nan(mods):
  big = 2e38                                  # x 2 = inf: a kernel must be finite, a logit need not be
  table = np.array([[1, 2, 3, 4, 3, 4],                    # q = 1.5, 3.5, 3.5: the lowest index of the equal maxima
                    [7, 7, 7, 7, 7, 7],                    # all equal: action 0
                    [1, 1, big, -big, 9, 9],               # q[1] = inf - inf = NaN: the first NaN
                    [1, 1, big, -big, -big, big],          # q[1] and q[2] NaN: the first
                    [big, -big, 5, 5, big, -big],          # q[0] NaN
                    [0, 0, -1, -1, big, big]], np.float32)    # q[2] = inf: a maximum like any other
  scale = np.array([1, 1, 2, 2, 2, 2], np.float32)
  z_t, q_d, a_d = _crafted(mods, table, 2, scale)
  q_t, a_t = qnet_emul.head(z_t, 2)
  assert a_t.tolist() == [1, 0, 1, 1, 0, 2]                # (the twin, by hand)
  assert np.array_equal(a_d, a_t)
  assert np.array_equal(np.isnan(q_d), np.isnan(q_t))
  finite = ~np.isnan(q_t)
  assert np.array_equal(_bits(q_d)[finite], _bits(q_t)[finite])


def test_head_sums_51_atoms_in_ascending_order(mods):
  """Action 0's atoms are (2^24, 1, ..., 1): ascending, every 1 is lost and q = 2^24 / 51; descending, q = (2^24 + 50) / 51."""
  table = np.zeros((2, 153), np.float32)
  table[0, 0], table[0, 1:51] = 2.0 ** 24, 1.0
  table[1, :51] = np.random.default_rng(0).standard_normal(51).astype(np.float32)
  z_t, q_d, a_d = _crafted(mods, table, 51)
  q_t, a_t = qnet_emul.head(z_t, 51)
  q_desc, _ = qnet_emul.head(z_t, 51, order=qnet_emul.ASCENDING)
  assert q_t[0, 0] == np.float32(2.0 ** 24) / np.float32(51) and q_desc[0, 0] == np.float32(2.0 ** 24 + 50) / np.float32(51)
  assert _bits(q_t)[1, 0] != _bits(q_desc)[1, 0], 'the random atoms do not tell the two orders apart: another seed'
  _same(q_d, q_t, 'q of 51 atoms')
  assert np.array_equal(a_d, a_t)


# ------------------------------------------------------------------------------------------------------------------ e. the loss heads
def _qr_case(mods, block, atoms, b, ret_scale=1.0, bad_action=None):
  tree = cases.params(2, 64, atoms)
  target = cases.scaled(tree, 1.5)                 # a target network other than the online one
  bt = list(cases.batch(block, b, seed=b, ret_scale=ret_scale))
  if bad_action is not None:
    bt[4][bad_action] = 3
  up = cases.twin_update(tree, target, *bt, atoms)
  tr = mods.qnet_train.QNetworkTrainer(_network(mods, tree, atoms))
  _set_image(mods, tr.target, target, atoms)
  _hold_update(mods, tr, tree, bt, up, atoms)
  return tr, target, bt, up


@pytest.mark.parametrize('atoms', [51, 1])
@pytest.mark.parametrize('b', [1, 32, 300])
def test_qr_loss_head(mods, block, atoms, b):
  tr, target, bt, up = _qr_case(mods, block, atoms, b)
  tr.check_errors()
  assert not up['flag']
  # the per-row a*: the target network's greedy action on next_state
  a_d, _, _ = _device_forward(mods, _network(mods, target, atoms), bt[1])
  assert np.array_equal(a_d, up['best'])


def test_qr_loss_head_on_extreme_targets(mods, block):
  _qr_case(mods, block, 51, 32, ret_scale=1e20)[0].check_errors()


def test_qr_loss_head_zeroes_an_invalid_action_and_flags_it(mods, block):
  tr, _, _, up = _qr_case(mods, block, 51, 32, bad_action=5)
  assert up['flag'] and not up['dlogits'][5].any() and up['loss'][5] == 0.0
  with pytest.raises(ValueError):
    tr.check_errors()


def _constant_logits(atoms, logits):
  """A 1-layer network with a zero kernel: every row's logits are the bias."""
  return {'params': {'Dense_0': {'kernel': np.zeros((cases.OBS_DIM, 3 * atoms), np.float32), 'bias': np.asarray(logits, np.float32)}}}


def test_qr_loss_head_at_u_exactly_kappa(mods, block):
  """theta_i = i / 4 - 3 + a and T = 1.25 (discount 0): u = T - theta is exactly +1 and -1 at some i of every action, which takes
  the quadratic branch (|u| <= kappa) and the unclipped derivative."""
  atoms = 51
  tree = _constant_logits(atoms, [0.25 * i - 3.0 + a for a in range(3) for i in range(atoms)])
  b = 6
  x = block[:b]
  bt = (x, x, np.full(b, 1.25, np.float32), np.zeros(b, np.float32), (np.arange(b) % 3).astype(np.uint8))
  up = cases.twin_update(tree, tree, *bt, atoms)
  theta = up['acts'][-1][:, :3 * atoms].reshape(b, 3, atoms)[np.arange(b), bt[4]]
  u = up['targets'][:, None, :] - theta[:, :, None]
  assert (u == 1.0).any() and (u == -1.0).any()
  tr = mods.qnet_train.QNetworkTrainer(_network(mods, tree, atoms))
  _hold_update(mods, tr, tree, bt, up, atoms)


def _dqn_case(mods, tree, target, bt, kind):
  up = cases.twin_update(tree, target, *bt, 1, kind=kind)
  tr = mods.dqn_agent.DQNTrainer(_network(mods, tree, 1), loss_type=kind)
  _set_image(mods, tr.target, target, 1)
  _hold_update(mods, tr, tree, bt, up, 1)
  tr.check_errors()
  return up


@pytest.mark.parametrize('kind', ['mse', 'huber'])
@pytest.mark.parametrize('b', [1, 32, 300])
def test_dqn_loss_head(mods, block, kind, b):
  tree = cases.params(2, 64, 1)
  _dqn_case(mods, tree, cases.scaled(tree, 1.5), cases.batch(block, b, seed=b), kind)


@pytest.mark.parametrize('kind', ['mse', 'huber'])
def test_dqn_loss_head_at_u_exactly_one(mods, block, kind):
  q = np.array([0.0, 0.5, -1.0], np.float32)
  tree = _constant_logits(1, q)
  act = np.array([0, 1, 2, 0, 1, 2], np.uint8)
  ret = (q[act] + np.array([1, 1, 1, -1, -1, -1], np.float32)).astype(np.float32)
  up = _dqn_case(mods, tree, tree, (block[:6], block[:6], ret, np.zeros(6, np.float32), act), kind)
  assert (np.abs(up['targets'] - q[act]) == 1.0).all()


# -------------------------------------------------------------------------------------------------------------------- f. the backward
@pytest.mark.parametrize('layers,hidden,atoms,b', cases.BACKWARD_CASES)
def test_gradient_image(mods, layers, hidden, atoms, b):
  tree, target, bt, up = cases.backward_case(layers, hidden, atoms, b)
  tr = mods.qnet_train.QNetworkTrainer(_network(mods, tree, atoms))
  _set_image(mods, tr.target, target, atoms)
  _hold_update(mods, tr, tree, bt, up, atoms)
  tr.check_errors()


def test_gradient_image_of_the_actor_critic(mods):
  """PPO's loss head has expf: the twin takes the device's own dlogits and holds the backward kernels at M = 6."""
  ac = mods.actor_critic
  tree = cases.params(2, 64, 2)
  b = 33
  x = cases.batch(cases.backward_pool(), b, seed=b)[0]
  rng = np.random.default_rng(b)
  bt = ac.PPOBatch.from_tensors(x, rng.standard_normal(b).astype(np.float32), rng.integers(0, 3, b).astype(np.uint8),
                                np.full(b, np.log(1.0 / 3.0), np.float32), rng.standard_normal(b).astype(np.float32), 'cuda')
  tr = ac.PPOTrainer(_network(mods, tree, 2))
  tr.train_on_batch(bt, apply_update=False)
  tr.check_errors()
  layers = qnet_emul.layers_of(tree)
  acts = qnet_emul.forward(layers, x)
  _hold_forward_stages(tr, b, layers, acts)
  dl = tr.views(b)['dlogits'].cpu().numpy()
  assert dl[:, :6].any() and not _bits(dl[:, 6:]).any()
  _same(tr.grad.cpu().numpy(), _packed(mods, qnet_emul.backward(layers, x, acts, dl[:, :64]), 2), 'gradient image')


def test_the_image_after_an_update(mods):
  """Adam has no twin (its fused product is the compiler's choice); what the NEXT update reads is held instead: weights_t is the
  re-transposed image, the padding stays zero, and the twin's forward on the unpacked new weights is the device's next forward."""
  layers, hidden, atoms, b = 3, 37, 7, 513
  tree, target, bt, _ = cases.backward_case(layers, hidden, atoms, b)
  tr = mods.qnet_train.QNetworkTrainer(_network(mods, tree, atoms), lr=1e-3)
  _set_image(mods, tr.target, target, atoms)
  batch = _train_batch(mods, *bt)
  tr.train_on_batch(batch)
  w = tr.weights.cpu().numpy()
  assert not np.array_equal(w, _packed(mods, tree, atoms))
  new = mods.qnet_train.unpack(tr._net, w)
  _same(_packed(mods, new, atoms), w, 'the updated image\'s padding')
  wt = tr.weights_t.cpu().numpy().copy()
  tr._retranspose()
  _same(wt, tr.weights_t.cpu().numpy(), 'weights_t after the update')
  up = cases.twin_update(new, target, *bt, atoms)
  _hold_update(mods, tr, new, bt, up, atoms)
