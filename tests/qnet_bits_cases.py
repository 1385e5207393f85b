"""The shapes and inputs that tests/test_qnet_emul_host.py (the chain twin against float64, and its mutants' sensitivity) and
tests/test_gpu_qnet_bits.py (the device against the twin, bit for bit) share, so that the condition the host test puts on the inputs
holds for the inputs the device test uses."""
import numpy as np

OBS_DIM = 1099

# (layers, hidden, atoms) of the forward comparison, and why each is there
FORWARD_SHAPES = [
    (1, 0, 1),        # the observation straight to 3 logits: the first layer is also the last
    (2, 7, 1),        # hidden < one chunk: kp = 8, one chunk only
    (2, 8, 2),        # exactly one chunk; M = 6, the actor-critic's head
    (3, 9, 7),        # one column past a chunk
    (3, 37, 7),
    (2, 63, 21),      # M = 63
    (2, 64, 22),      # no padded column in the hidden layer; M = 66: a second column group holding two columns
    (2, 65, 51),      # a second hidden group holding one column
]
REFERENCE_SHAPE, REFERENCE_ROWS = (8, 600, 51), 40

# (layers, hidden, atoms, B) of the backward comparison: either side of the 8-row step, of a 128-row tile, of one slab (B < 512), two
# slabs (513: 257 + 256 rows) and 16 slabs with a ragged last one (4097: 15 x 257 + 242)
BACKWARD_CASES = ([(2, 64, 51, b) for b in (1, 7, 8, 9, 255, 256, 257, 511, 513, 4097)] + [(3, 37, 7, 1), (3, 37, 7, 513)] +
                  [(2, 65, 22, 33), (3, 9, 7, 33), (2, 7, 1, 33)] + [(8, 600, 51, 32)])


def params(layers, hidden, atoms, seed=7, bias=1e-2):
  """The reference's initialisation (QuantileNetwork's variance scaling; num_atoms == 1: MLPNetwork's Glorot) with non-zero biases, as
  agents/qnet.init_params draws it plus test_gpu_train.py's biases -- restated here so that a machine without the library has it."""
  rng = np.random.default_rng(seed)
  dims = [OBS_DIM] + [hidden] * (layers - 1) + [3 * atoms]
  tree = {}
  for i in range(layers):
    fan_in, fan_out = dims[i], dims[i + 1]
    limit = np.sqrt(3.0 / np.sqrt(3.0) / fan_in) if atoms > 1 else np.sqrt(6.0 / (fan_in + fan_out))
    tree[f'Dense_{i}'] = {'kernel': rng.uniform(-limit, limit, (fan_in, fan_out)).astype(np.float32)}
  rng = np.random.default_rng(seed + 1)
  for leaf in tree.values():
    leaf['bias'] = (rng.standard_normal(leaf['kernel'].shape[1]) * bias).astype(np.float32)
  return {'params': tree}


def scaled(tree, factor):
  """Every parameter times `factor`, rounded to float32: a target network other than the online one."""
  f = np.float32(factor)
  return {'params': {name: {k: (np.asarray(v, np.float32) * f).astype(np.float32) for k, v in leaf.items()}
                     for name, leaf in tree['params'].items()}}


def synthetic_rows(seed=1):
  """65 rows a host can make: 48 random rows in [0, 1), 16 rows spanning 1e-6 .. 1e3 with both signs, one all-zero row (the bias
  alone)."""
  rng = np.random.default_rng(seed)
  rnd = rng.random((48, OBS_DIM), dtype=np.float32)
  wide = (10.0 ** rng.uniform(-6.0, 3.0, (16, OBS_DIM)) * rng.choice([-1.0, 1.0], (16, OBS_DIM))).astype(np.float32)
  return np.concatenate([rnd, wide, np.zeros((1, OBS_DIM), np.float32)])


def block(device_rows):
  """The 129-row block: 64 device observations, then synthetic_rows().  Two workgroups, the second with one live row (the zero row)."""
  device_rows = np.asarray(device_rows, np.float32)
  assert device_rows.shape == (64, OBS_DIM)
  return np.concatenate([device_rows, synthetic_rows()])


def reference_rows(rows):
  """REFERENCE_ROWS of a block's rows, spread over its kinds and ending with its last (the zero row)."""
  idx = np.unique(np.round(np.linspace(0, len(rows) - 1, REFERENCE_ROWS)).astype(int))
  assert len(idx) == REFERENCE_ROWS
  return rows[idx]


def special_rows(base):
  """Three copies of row `base` [1099]: one with subnormals (1e-40, both signs) in every fourth column, one with -0.0 in every third
  column, one with a NaN in column 1098."""
  rows = np.repeat(np.asarray(base, np.float32)[None, :], 3, axis=0)
  rows[0, ::4] = np.float32(1e-40)
  rows[0, 2::8] = np.float32(-1e-40)
  rows[1, ::3] = np.float32(-0.0)
  rows[2, 1098] = np.float32('nan')
  return rows


def batch(pool, b, seed, ret_scale=1.0):
  """A training batch drawn from the rows of `pool`, as test_gpu_train.py's _batch draws it: (state, next_state, ret, discount,
  action)."""
  rng = np.random.default_rng(seed)
  i, j = rng.integers(0, len(pool), b), rng.integers(0, len(pool), b)
  disc = np.where(rng.random(b) < 0.2, 0.0, 0.993 ** 5).astype(np.float32)
  ret = (rng.standard_normal(b) * ret_scale).astype(np.float32)
  return pool[i], pool[j], ret, disc, rng.integers(0, 3, b).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ exact by hand
# One MFMA step is fma(a_k1, b_k1, fma(a_k0, b_k0, C)); chunk c, step j takes k = 8c + j then 8c + 4 + j.  A 1-layer one-atom network
# (1099 -> 3 logits, no ReLU) whose weights are zero but for a few columns makes a logit a chain of two or three live terms, every
# other term being fma(0, w, acc) or fma(x, 0, acc).  HAND_TRIPLES: three columns IN THE CONTRACT'S CHAIN ORDER:
#   (0, 1, 5)  columns 0 and 1 (two steps of one chunk); swapping the halves would walk 0, 5, 1;
#   (0, 4, 1)  columns 0 and 4 (the two halves of one step); ascending k would walk 0, 1, 4;
#   (0, 8, 9)  columns 0 and 8 (two chunks).
HAND_TRIPLES = {'adjacent': (0, 1, 5), 'halves': (0, 4, 1), 'chunks': (0, 8, 9)}
_BIG = np.float32(2.0 ** 24)
_TINY = np.float32(2.0 ** -100)
LAST_LIVE = 1098          # the last live term of the chain: after it come only the padded k = 1102, 1099, 1103


def hand_case(triple):
  """(params of a (1, -, 1) network, rows [7, 1099], expected): expected = [(row, logit, bits, why)], worked out by hand below.

  logit 0: w = 1 on the triple, bias -2^24.  logit 1: w = (-1, 1 - 2^-13) on the first two, bias 0.  logit 2: w = (-1, 1 - 2^-12) on
  the first two, -2^-100 on column 1098, bias -0.0."""
  t0, t1, t2 = triple
  w = np.zeros((OBS_DIM, 3), np.float32)
  w[[t0, t1, t2], 0] = 1.0
  w[t0, 1], w[t1, 1] = -1.0, np.float32(1.0 - 2.0 ** -13)
  w[t0, 2], w[t1, 2], w[LAST_LIVE, 2] = -1.0, np.float32(1.0 - 2.0 ** -12), -_TINY
  bias = np.array([-_BIG, 0.0, -0.0], np.float32)
  rows = np.zeros((7, OBS_DIM), np.float32)
  expected = []
  # row 0: 2^24 then 1.  RN(2^24 + 1) = 2^24 (a tie, to even), minus 2^24 = +0.0.  Two terms commute: either order gives this.
  rows[0, t0], rows[0, t1] = _BIG, 1.0
  expected.append((0, 0, 0x00000000, '(2^24 + 1) - 2^24'))
  # row 1: 1, 1, then 2^24: 2 + 2^24 is exact, minus 2^24 = 2.0.  With 2^24 first both ones would be lost.
  rows[1, t0], rows[1, t1], rows[1, t2] = 1.0, 1.0, _BIG
  expected.append((1, 0, 0x40000000, '((1 + 1) + 2^24) - 2^24'))
  # row 2: 2^24, 1, 1: both ones are lost, +0.0.  With the ones first it would be 2.0.
  rows[2, t0], rows[2, t1], rows[2, t2] = _BIG, 1.0, 1.0
  expected.append((2, 0, 0x00000000, '((2^24 + 1) + 1) - 2^24'))
  # row 3: acc = -1, then (1 + 2^-13)(1 - 2^-13) = 1 - 2^-26 exactly: fused, -1 + 1 - 2^-26 = -2^-26; the product rounded alone is 1.0
  # and the sum +0.0.
  rows[3, t0], rows[3, t1] = 1.0, np.float32(1.0 + 2.0 ** -13)
  expected.append((3, 1, 0xB2800000, 'fma(1 + 2^-13, 1 - 2^-13, -1) = -2^-26'))
  # row 4: acc = -1, then (1 + 2^-12)(1 - 2^-12) = 1 - 2^-24, which float32 holds: -2^-24 fused or not.
  rows[4, t0], rows[4, t1] = 1.0, np.float32(1.0 + 2.0 ** -12)
  expected.append((4, 2, 0xB3800000, 'fma(1 + 2^-12, 1 - 2^-12, -1) = -2^-24'))
  # row 5: the only live term is 2^-100 * -2^-100 = -2^-200 at k = 1098, which underflows to -0.0; the padded terms that follow are
  # fma(0, 0, -0.0) = +0.0, and +0.0 + (bias -0.0) = +0.0.  Were the padded terms not walked, -0.0 + -0.0 = -0.0.
  rows[5, LAST_LIVE] = _TINY
  expected.append((5, 2, 0x00000000, 'fma(0, 0, -0.0) + -0.0'))
  # row 6: all zero: every term is fma(0, w, +0.0) = +0.0; the logits are the biases, and +0.0 + -0.0 = +0.0.
  expected += [(6, 0, 0xCB800000, 'bias -2^24'), (6, 1, 0x00000000, 'bias 0'), (6, 2, 0x00000000, '+0.0 + -0.0')]
  return {'params': {'Dense_0': {'kernel': w, 'bias': bias}}}, rows, expected


# ------------------------------------------------------------------------------------------------------------------ one update
def twin_update(tree, target_tree, state, next_state, ret, discount, action, atoms, kind='qr', order=0):
  """One update's chain through the twin (emul/qnet_emul.py), end to end on the twin's own values: the online layers' padded outputs
  on `state`, the target network's logits on `next_state`, the loss head ('qr', or DQN's 'mse' / 'huber'), and the gradient tree.
  `order` is the mutant of dW / db; every other stage is the contract's."""
  from emul import qnet_emul
  layers, tlayers = qnet_emul.layers_of(tree), qnet_emul.layers_of(target_tree)
  acts = qnet_emul.forward(layers, state)
  target_logits = qnet_emul.forward(tlayers, next_state)[-1]
  if kind == 'qr':
    targets, loss, dlogits, best, flag = qnet_emul.qr_loss(acts[-1], target_logits, ret, discount, action, atoms)
  else:
    targets, loss, dlogits, flag = qnet_emul.td_loss(kind, acts[-1], target_logits, ret, discount, action)
    best = None
  grad = qnet_emul.backward(layers, state, acts, dlogits, order)
  return {'acts': acts, 'target_logits': target_logits, 'targets': targets, 'loss': loss, 'dlogits': dlogits, 'best': best, 'flag': flag,
          'grad': grad}


_CASES = {}
# The batch seed of a case is layers + B, except where that batch does not meet test_qnet_emul_host.py's sensitivity condition: the
# last layer of (2, 7, 1) has 21 weights and three live hidden units, and at seed 35 the even-rows-first mutant changes none of them.
_SEEDS = {(2, 7, 1, 33): 38}


def backward_pool():
  """The rows the backward batches draw from: synthetic_rows()'s 48 random rows.  Without the 1e3 rows the TD errors stay around
  kappa, so that dlogits are not all +-tau / B (sums of equal magnitudes would not feel their order)."""
  return synthetic_rows()[:48]


def backward_case(layers, hidden, atoms, b):
  """The QR-DQN update of a BACKWARD_CASES entry on a batch drawn from backward_pool(), target = 1.5 x online: (tree, target tree,
  batch, twin_update's dict).  Computed once and shared; callers leave it unchanged."""
  key = (layers, hidden, atoms, b)
  if key not in _CASES:
    tree = params(layers, hidden, atoms)
    target = scaled(tree, 1.5)
    bt = batch(backward_pool(), b, seed=_SEEDS.get(key, layers + b))
    _CASES[key] = (tree, target, bt, twin_update(tree, target, *bt, atoms))
  return _CASES[key]
