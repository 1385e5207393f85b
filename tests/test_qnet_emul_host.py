"""The fma-chain twin of the Q-network kernels (emul/qnet_emul.cpp) on the host, before tests/test_gpu_qnet_bits.py holds the device
to its bits:

 * accuracy: the twin against the float64 restatements (qnet_host.forward, train_host.backward) at the device test's shapes, inside
   the existing 1e-5 S magnitude bound; the worst ratio is printed (DESIGN §5 quotes it as the chain's own error);
 * sensitivity, a condition on the INPUTS: every mutant of the chain's order (qnet_emul.py: ascending k, halves swapped, unfused,
   one column dropped; for dW even rows first and the slabs descending) changes the bits of >= 25 % of the logits at every forward
   shape, and of at least one element of every layer's dW at every backward case -- so a device that walked a mutant's order would
   fail the bit comparison on that share, where the 1e-5 S bound lets all of them through;
 * exact-by-hand chains that pin the twin itself without any reference implementation;
 * the loss-head twins against the float64 restatements at the tolerances the device is held to today (the twin is float32: this
   shows only that it is the same function).
"""
import numpy as np
import pytest

import qnet_bits_cases as cases
import qnet_host
import td_host
import train_host
from emul import qnet_emul

ALL_FORWARD = cases.FORWARD_SHAPES + [cases.REFERENCE_SHAPE]


def _rows(shape):
  rows = cases.synthetic_rows()
  return cases.reference_rows(rows) if shape == cases.REFERENCE_SHAPE else rows


_FORWARD = {}


def _forward(shape):
  """(tree, rows, the twin's padded layer outputs), once per shape."""
  if shape not in _FORWARD:
    tree = cases.params(*shape)
    rows = _rows(shape)
    _FORWARD[shape] = (tree, rows, qnet_emul.forward(qnet_emul.layers_of(tree), rows))
  return _FORWARD[shape]


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


# -------------------------------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize('shape', ALL_FORWARD)
def test_forward_within_the_float64_bound(shape):
  tree, rows, outs = _forward(shape)
  atoms = shape[2]
  q, action = qnet_emul.head(outs[-1], atoms)
  q64 = qnet_host.forward(tree, rows, atoms)
  s = qnet_host.forward(tree, rows, atoms, magnitude=True)
  ratio = float((np.abs(q - q64) / (1e-5 * s)).max())
  print(f'{shape}: the chain\'s worst |q - q64| / (1e-5 S) = {ratio:.3g} over {len(rows)} rows')
  assert ratio <= 1.0
  assert np.array_equal(action, np.argmax(q, axis=1))


@pytest.mark.parametrize('layers,hidden,atoms,b', cases.BACKWARD_CASES)
def test_backward_within_the_float64_bound(layers, hidden, atoms, b):
  tree, _, bt, up = cases.backward_case(layers, hidden, atoms, b)
  x, out = bt[0], 3 * atoms
  acts = [a[:, :hidden] for a in up['acts'][:-1]] + [up['acts'][-1][:, :out]]
  dlog = up['dlogits'][:, :out]
  want = train_host.backward(tree, x, dlog, acts)
  mag = train_host.backward_magnitude(tree, x, dlog, acts)
  worst = 0.0
  for l in range(layers):
    for leaf, i in (('kernel', 0), ('bias', 1)):
      err = np.abs(up['grad']['params'][f'Dense_{l}'][leaf] - want[l][i])
      worst = max(worst, float((err / (1e-5 * mag[l][i] + 1e-30)).max()))
  print(f'({layers}, {hidden}, {atoms}) B = {b}: the chain\'s worst |g - g64| / (1e-5 S) = {worst:.3g}')
  assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize('shape', ALL_FORWARD)
def test_every_forward_mutant_changes_a_quarter_of_the_logits(shape):
  tree, rows, outs = _forward(shape)
  out = 3 * shape[2]
  base = _bits(outs[-1][:, :out])
  shares = {}
  for order in qnet_emul.FORWARD_MUTANTS:
    got = _bits(qnet_emul.forward(qnet_emul.layers_of(tree), rows, order)[-1][:, :out])
    shares[order] = float((got != base).mean())
  print(f'{shape}: share of logits whose bits change -- ascending k {shares[1]:.3f}, halves swapped {shares[2]:.3f}, '
        f'unfused {shares[3]:.3f}, column {qnet_emul.smallest_column(rows)} dropped {shares[4]:.3f}')
  assert min(shares.values()) >= 0.25, shares


@pytest.mark.parametrize('layers,hidden,atoms,b', [c for c in cases.BACKWARD_CASES if c[3] >= 9])
def test_every_wgrad_mutant_changes_every_layer(layers, hidden, atoms, b):
  tree, _, bt, up = cases.backward_case(layers, hidden, atoms, b)
  lay = qnet_emul.layers_of(tree)
  slabs = qnet_emul.wgrad_slabs(b)[0]
  # two slabs cannot tell their order: p[0] + p[1] == p[1] + p[0]; from three on, (p[0] + p[1]) + p[2] is not p[2] + p[1] + p[0]
  mutants = qnet_emul.WGRAD_MUTANTS + ((qnet_emul.SLABS_DESCENDING,) if slabs >= 3 else ())
  for order in mutants:
    got = qnet_emul.backward(lay, bt[0], up['acts'], up['dlogits'], order)['params']
    shares = []
    for l in range(layers):
      dw = float((_bits(got[f'Dense_{l}']['kernel']) != _bits(up['grad']['params'][f'Dense_{l}']['kernel'])).mean())
      db = float((_bits(got[f'Dense_{l}']['bias']) != _bits(up['grad']['params'][f'Dense_{l}']['bias'])).mean())
      shares.append((dw, db))
      assert dw > 0.0, (order, l)
      if order == qnet_emul.EVEN_FIRST:
        assert db > 0.0, (order, l)
    print(f'({layers}, {hidden}, {atoms}) B = {b} ({slabs} slabs), mutant {order}: share of (dW, db) changed per layer '
          + ', '.join(f'({dw:.3f}, {db:.3f})' for dw, db in shares))


def test_the_old_bound_lets_the_mutants_through():
  """What the bit comparison adds: at (3, 37, 7) every mutant of the ORDER stays inside 1e-5 S.  (The dropped column need not: on a
  row where it is large it is a real error.)"""
  shape = (3, 37, 7)
  tree, rows, _ = _forward(shape)
  q64 = qnet_host.forward(tree, rows, 7)
  s = qnet_host.forward(tree, rows, 7, magnitude=True)
  for order in (qnet_emul.ASCENDING, qnet_emul.HALVES_SWAPPED, qnet_emul.UNFUSED):
    q, _ = qnet_emul.head(qnet_emul.forward(qnet_emul.layers_of(tree), rows, order)[-1], 7)
    ratio = float((np.abs(q - q64) / (1e-5 * s)).max())
    print(f'mutant {order}: worst |q - q64| / (1e-5 S) = {ratio:.3g}')
    assert ratio <= 1.0


# --------------------------------------------------------------------------------------------------------------------- exact by hand
@pytest.mark.parametrize('name', list(cases.HAND_TRIPLES))
def test_hand_chains(name):
  tree, rows, expected = cases.hand_case(cases.HAND_TRIPLES[name])
  got = _bits(qnet_emul.forward(qnet_emul.layers_of(tree), rows)[-1])
  for row, logit, bits, why in expected:
    assert got[row, logit] == bits, (name, row, logit, hex(got[row, logit]), hex(bits), why)


def test_hand_chains_tell_the_mutants_apart():
  def logit(name, order, row, col):
    tree, rows, _ = cases.hand_case(cases.HAND_TRIPLES[name])
    return int(_bits(qnet_emul.forward(qnet_emul.layers_of(tree), rows, order)[-1])[row, col])
  # columns (0, 4, 1) hold (1, 1, 2^24) in chain order; ascending k walks 0, 1, 4: the second 1 comes after 2^24 and is lost
  assert logit('halves', qnet_emul.CONTRACT, 1, 0) == 0x40000000 and logit('halves', qnet_emul.ASCENDING, 1, 0) == 0x00000000
  # columns (0, 1, 5): with the halves swapped the chain walks 0, 5, 1
  assert logit('adjacent', qnet_emul.CONTRACT, 1, 0) == 0x40000000 and logit('adjacent', qnet_emul.HALVES_SWAPPED, 1, 0) == 0x00000000
  # the product rounded on its own is 1.0, and -1 + 1 = +0.0
  for name in cases.HAND_TRIPLES:
    assert logit(name, qnet_emul.CONTRACT, 3, 1) == 0xB2800000 and logit(name, qnet_emul.UNFUSED, 3, 1) == 0x00000000


def test_hand_chains_at_k_2_and_3():
  """The same arithmetic on the smallest layers, straight through dense(): K = 2 (kp = 8: six padded terms) and K = 3."""
  one = np.ones((2, 1), np.float32)
  y = qnet_emul.dense(np.array([[2.0 ** 24, 1.0]], np.float32), one, np.array([-2.0 ** 24], np.float32), True, False)
  assert y.shape == (1, 64) and _bits(y)[0, 0] == 0x00000000 and not _bits(y)[0, 1:].any()      # (the padded columns: +0.0)
  x = np.array([[1.0, 1.0 + 2.0 ** -12]], np.float32)
  w = np.array([[-1.0], [1.0 - 2.0 ** -12]], np.float32)
  for order in (qnet_emul.CONTRACT, qnet_emul.UNFUSED):                   # 1 - 2^-24 is a float32: fused or not, -2^-24
    assert _bits(qnet_emul.dense(x, w, np.zeros(1, np.float32), True, False, order))[0, 0] == 0xB3800000
  x = np.array([[1.0, 1.0 + 2.0 ** -13]], np.float32)
  w = np.array([[-1.0], [1.0 - 2.0 ** -13]], np.float32)
  assert _bits(qnet_emul.dense(x, w, np.zeros(1, np.float32), True, False))[0, 0] == 0xB2800000
  assert _bits(qnet_emul.dense(x, w, np.zeros(1, np.float32), True, False, qnet_emul.UNFUSED))[0, 0] == 0x00000000
  # K = 3: the live term at k = 2 underflows to -0.0; the chain goes on with k = 6, 3, 7, all padded: fma(0, 0, -0.0) = +0.0
  x = np.array([[0.0, 0.0, 2.0 ** -100]], np.float32)
  w = np.array([[0.0], [0.0], [-2.0 ** -100]], np.float32)
  assert _bits(qnet_emul.dense(x, w, np.array([-0.0], np.float32), True, False))[0, 0] == 0x00000000
  # ... and a ReLU keeps a -0.0 sum (v < 0 is false): K = 8 has no padded term after k = 7
  x = np.zeros((1, 8), np.float32)
  w = np.zeros((8, 1), np.float32)
  x[0, 7], w[7, 0] = 2.0 ** -100, -2.0 ** -100
  assert _bits(qnet_emul.dense(x, w, np.array([-0.0], np.float32), True, True))[0, 0] == 0x80000000


def test_head_by_hand():
  z = np.zeros((4, 64), np.float32)
  z[0, :6] = [1, 2, 3, 4, 3, 4]                    # q = 1.5, 3.5, 3.5: the first maximum
  z[1, :6] = [0, 0, np.nan, 0, np.nan, 0]          # the first NaN
  z[2, :6] = [2.0 ** 24, 1, 1, 2.0 ** 24, 0, 0]    # ascending: (2^24 + 1) / 2 = 2^23, (1 + 2^24) / 2 = 2^23: equal, the lower index
  z[3, :6] = [5, 5, 1, 1, 7, 7]
  q, a = qnet_emul.head(z, 2)
  assert a.tolist() == [1, 1, 0, 2]
  assert q[0].tolist() == [1.5, 3.5, 3.5] and np.isnan(q[1, 1:]).all() and q[1, 0] == 0 and q[2, 0] == q[2, 1] == 2.0 ** 23
  # three atoms (2^24, 1, 1): ascending loses both ones, descending keeps them
  z = np.zeros((1, 64), np.float32)
  z[0, :3] = [2.0 ** 24, 1, 1]
  assert qnet_emul.head(z, 3)[0][0, 0] == np.float32(2.0 ** 24) / np.float32(3)
  assert qnet_emul.head(z, 3, order=qnet_emul.ASCENDING)[0][0, 0] == np.float32(2.0 ** 24 + 2) / np.float32(3)


def test_wgrad_by_hand():
  """dW of one weight over rows (2^24, 1, 1): one slab keeps the order; the padded rows add fma(0, 0, acc); db = evens + odds."""
  x = np.array([[2.0 ** 24], [1.0], [1.0]], np.float32)
  dy = np.ones((3, 1), np.float32)
  dw, db = qnet_emul.wgrad(x, dy, 1, 1)
  assert dw[0, 0] == 2.0 ** 24 and db[0] == 3.0
  dw, _ = qnet_emul.wgrad(x[::-1], dy, 1, 1)
  assert dw[0, 0] == 2.0 ** 24 + 2
  # db: rows (2^24, 1, 1, 1): evens 2^24 + 1 = 2^24, odds 1 + 1 = 2, sum 2^24 + 2; one ascending chain would lose all three ones
  dy = np.array([[2.0 ** 24], [1.0], [1.0], [1.0]], np.float32)
  x = np.zeros((4, 1), np.float32)
  assert qnet_emul.wgrad(x, dy, 1, 1)[1][0] == 2.0 ** 24 + 2
  assert qnet_emul.wgrad(x, dy, 1, 1, qnet_emul.EVEN_FIRST)[1][0] == 2.0 ** 24
  assert qnet_emul.wgrad_slabs(511) == (1, 511) and qnet_emul.wgrad_slabs(513) == (2, 257) and qnet_emul.wgrad_slabs(4097) == (16, 257)


# ------------------------------------------------------------------------------------------------------------------------ loss heads
@pytest.mark.parametrize('atoms', [51, 1])
@pytest.mark.parametrize('b', [1, 32, 300])
def test_qr_loss_twin_is_the_float64_function(atoms, b):
  rng = np.random.default_rng(b)
  ld = qnet_emul.round_up(3 * atoms, 64)
  z, zt = (np.zeros((b, ld), np.float32) for _ in range(2))
  z[:, :3 * atoms], zt[:, :3 * atoms] = rng.standard_normal((2, b, 3 * atoms)).astype(np.float32)
  _, _, ret, disc, act = cases.batch(cases.synthetic_rows(), b, seed=b)
  targets, loss, dlog, best, flag = qnet_emul.qr_loss(z, zt, ret, disc, act, atoms)
  t64 = train_host.targets(zt[:, :3 * atoms], ret, disc, atoms)
  assert not flag and np.allclose(targets, t64, rtol=1e-6, atol=1e-6 * np.abs(t64).max())
  assert np.array_equal(best, qnet_emul.head(zt, atoms)[1])
  l64, d64 = train_host.quantile_loss(z[:, :3 * atoms], targets, act, atoms)
  assert np.allclose(loss, l64, rtol=2e-6, atol=1e-7 * l64.max())
  assert np.allclose(dlog[:, :3 * atoms], d64, rtol=2e-6, atol=1e-7 * np.abs(d64).max())
  assert not dlog[:, 3 * atoms:].any() and (dlog[:, :3 * atoms][d64 == 0] == 0).all()


def test_qr_loss_twin_edges():
  """|u| exactly kappa takes the quadratic branch; an action >= 3 zeroes its row and sets the flag."""
  z, zt = np.zeros((2, 64), np.float32), np.zeros((2, 64), np.float32)
  ret, disc = np.array([1.0, 1.0], np.float32), np.zeros(2, np.float32)
  targets, loss, dlog, _, flag = qnet_emul.qr_loss(z, zt, ret, disc, np.array([0, 3], np.uint8), 1)
  # u = 1 = kappa, tau = 1/2: rho = 1/2 * (1/2 * 1 * 1) = 1/4; dL/dtheta = -((1/2 * 1) / 1) / 2
  assert flag and targets.tolist() == [[1.0], [1.0]] and loss.tolist() == [0.25, 0.0]
  assert dlog[0, 0] == -0.25 and not dlog[0, 1:].any() and not dlog[1].any()


@pytest.mark.parametrize('kind', ['mse', 'huber'])
@pytest.mark.parametrize('b', [1, 32, 300])
def test_td_loss_twin_is_the_float64_function(kind, b):
  rng = np.random.default_rng(b)
  z, zt = (np.zeros((b, 64), np.float32) for _ in range(2))
  z[:, :3], zt[:, :3] = rng.standard_normal((2, b, 3)).astype(np.float32)
  _, _, ret, disc, act = cases.batch(cases.synthetic_rows(), b, seed=b)
  targets, loss, dlog, flag = qnet_emul.td_loss(kind, z, zt, ret, disc, act)
  t64 = td_host.dqn_targets(zt[:, :3], ret, disc)
  assert not flag and np.allclose(targets, t64, rtol=1e-6, atol=1e-6 * np.abs(t64).max())
  l64, d64 = td_host.dqn_loss(z[:, :3], targets, act, kind)
  assert np.allclose(loss, l64, rtol=2e-6, atol=1e-7 * np.abs(l64).max())
  assert np.allclose(dlog[:, :3], d64, rtol=2e-6, atol=1e-7 * np.abs(d64).max())
  assert not dlog[:, 3:].any()


def test_td_loss_twin_at_u_exactly_one():
  z, zt = np.zeros((2, 64), np.float32), np.zeros((2, 64), np.float32)
  ret, disc, act = np.array([1.0, -1.0], np.float32), np.zeros(2, np.float32), np.zeros(2, np.uint8)
  _, loss, dlog, _ = qnet_emul.td_loss('huber', z, zt, ret, disc, act)
  assert loss.tolist() == [0.5, 0.5] and dlog[:, 0].tolist() == [-0.5, 0.5]
  _, loss, dlog, _ = qnet_emul.td_loss('mse', z, zt, ret, disc, act)
  assert loss.tolist() == [1.0, 1.0] and dlog[:, 0].tolist() == [-1.0, 1.0]
