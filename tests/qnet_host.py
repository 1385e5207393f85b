"""Float64 NumPy restatements of the reference's QuantileNetwork.__call__ and MLPNetwork.__call__ (agents/networks.py) and of their
kernel initialisers: the yardstick of the Q-network kernel (ble_qnet_forward_f32)."""
import numpy as np

OBS_DIM, NUM_ACTIONS = 1099, 3


def dense_layers(params):
  tree = params.get('params', params)
  return [(np.asarray(tree[f'Dense_{i}']['kernel'], np.float64), np.asarray(tree[f'Dense_{i}']['bias'], np.float64))
          for i in range(len(tree))]


def forward(params, x, num_atoms, magnitude=False):
  """q-values [N, 3] in float64: Dense -> relu for all layers but the last, logits reshaped to (3, num_atoms), the mean over the atoms
  (QuantileNetwork; num_atoms = 1 is MLPNetwork's q = logits).  magnitude=True runs the same network with |W|, |b| and |x| -- the
  bound S that a float32 evaluation's rounding error is measured against."""
  h = np.asarray(x, np.float64)
  layers = dense_layers(params)
  if magnitude:
    h = np.abs(h)
  for i, (k, b) in enumerate(layers):
    if magnitude:
      k, b = np.abs(k), np.abs(b)
    h = h @ k + b
    if i < len(layers) - 1:
      h = np.maximum(h, 0.0)
  return h.reshape(h.shape[0], NUM_ACTIONS, num_atoms).mean(axis=2)


def variance_scaling_uniform(rng, fan_in, fan_out, scale=1.0 / np.sqrt(3.0)):
  """nn.initializers.variance_scaling(scale, 'fan_in', 'uniform'): U(-l, l), l = sqrt(3 scale / fan_in)."""
  limit = np.sqrt(3.0 * scale / fan_in)
  return rng.uniform(-limit, limit, (fan_in, fan_out))


def glorot_uniform(rng, fan_in, fan_out):
  """jax.nn.initializers.glorot_uniform(): variance_scaling(1, 'fan_avg', 'uniform'), l = sqrt(6 / (fan_in + fan_out))."""
  limit = np.sqrt(6.0 / (fan_in + fan_out))
  return rng.uniform(-limit, limit, (fan_in, fan_out))
