"""Float64 NumPy restatements of one QR-DQN update as Dopamine 4.0.0's JaxQuantileAgent runs it (quantile_agent.train with optax 0.0.9's
adam): the n-step replay sample, the target, the quantile Huber loss, hand-written backprop through the Dense stack and Adam.  The
yardstick of csrc/ble_train.h (ble_replay_sample_f32, ble_qnet_train_step_f32)."""
import numpy as np

import qnet_host

NUM_ACTIONS = 3


def forward_all(params, x):
  """Every layer's output, float64: [h_0, ..., h_{L-1}] (ReLU on all but the last, whose output is the logits)."""
  h = np.asarray(x, np.float64)
  layers = qnet_host.dense_layers(params)
  outs = []
  for i, (k, b) in enumerate(layers):
    h = h @ k + b
    if i < len(layers) - 1:
      h = np.maximum(h, 0.0)
    outs.append(h)
  return outs


def targets(target_logits, ret, discount, num_atoms):
  """T[b, j] = ret + discount * z'[a*, j], a* = argmax_a mean_j z'[a, j] (the first maximum)."""
  z = np.asarray(target_logits, np.float64).reshape(-1, NUM_ACTIONS, num_atoms)
  a = z.mean(axis=2).argmax(axis=1)
  return np.asarray(ret, np.float64)[:, None] + np.asarray(discount, np.float64)[:, None] * z[np.arange(len(a)), a]


def quantile_loss(logits, tgt, action, num_atoms, kappa=1.0):
  """(per-row loss L_b [B], dL/dlogits [B, 3 * atoms] of the objective mean_b L_b).

  u_ij = T_j - theta_i, rho_ij = |tau_i - 1{u_ij < 0}| H(u_ij), L_b = sum_i mean_j rho_ij; the indicator's derivative is 0 (JAX)."""
  z = np.asarray(logits, np.float64).reshape(-1, NUM_ACTIONS, num_atoms)
  b = z.shape[0]
  theta = z[np.arange(b), np.asarray(action)]                       # [B, i]
  u = np.asarray(tgt, np.float64)[:, None, :] - theta[:, :, None]   # [B, i, j]
  tau = (np.arange(num_atoms) + 0.5) / num_atoms
  w = np.abs(tau[None, :, None] - (u < 0))
  au = np.abs(u)
  h = np.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa))
  loss = (w * h).mean(axis=2).sum(axis=1)
  dtheta = -(w * np.clip(u, -kappa, kappa)).mean(axis=2) / b        # d mean_b L_b / d theta
  d = np.zeros_like(z)
  d[np.arange(b), np.asarray(action)] = dtheta
  return loss, d.reshape(b, -1)


def backward(params, x, dlogits, acts=None):
  """Gradients [(dW_l, db_l)] of the objective given dL/dlogits, backpropagated in float64 through the network at inputs x.  acts:
  the layers' outputs to take the ReLU masks and inputs from (default: the float64 forward)."""
  layers = qnet_host.dense_layers(params)
  acts = forward_all(params, x) if acts is None else [np.asarray(a, np.float64) for a in acts]
  dy = np.asarray(dlogits, np.float64)
  grads = [None] * len(layers)
  for l in range(len(layers) - 1, -1, -1):
    xin = np.asarray(x, np.float64) if l == 0 else acts[l - 1]
    grads[l] = (xin.T @ dy, dy.sum(axis=0))
    if l > 0:
      dy = (dy @ layers[l][0].T) * (acts[l - 1] > 0)
  return grads


def backward_magnitude(params, x, dlogits, acts=None):
  """The same chain with |W|, |x|, |dY|: the bound S that a float32 evaluation's rounding error is measured against."""
  layers = qnet_host.dense_layers(params)
  acts = forward_all(params, x) if acts is None else [np.asarray(a, np.float64) for a in acts]
  dy = np.abs(np.asarray(dlogits, np.float64))
  out = [None] * len(layers)
  for l in range(len(layers) - 1, -1, -1):
    xin = np.abs(np.asarray(x, np.float64)) if l == 0 else np.abs(acts[l - 1])
    out[l] = (xin.T @ dy, dy.sum(axis=0))
    if l > 0:
      dy = (dy @ np.abs(layers[l][0]).T) * (acts[l - 1] > 0)
  return out


def loss_of_params(params, x, tgt, action, num_atoms, kappa=1.0):
  """The objective mean_b L_b at params (float64), for finite differences."""
  logits = forward_all(params, x)[-1]
  return quantile_loss(logits, tgt, action, num_atoms, kappa)[0].mean()


def adam(w, g, m, v, t, lr, b1=0.9, b2=0.999, eps=2e-5):
  """optax 0.0.9 adam (scale_by_adam, eps_root = 0, then scale(-lr)) at step t (1-based), float64: (w, m, v) after."""
  w, g, m, v = (np.asarray(a, np.float64) for a in (w, g, m, v))
  m = (1 - b1) * g + b1 * m
  v = (1 - b2) * g * g + b2 * v
  mh = m / (1 - b1 ** t)
  vh = v / (1 - b2 ** t)
  return w - lr * mh / (np.sqrt(vh) + eps), m, v


def nstep(reward, terminal, episode_end, t, env, n, gamma):
  """(m, return, discount, is_terminal) of the n-step window at (t, env), or None if it is invalid (a time-limit end before a terminal).
  The return sums the float32 products gamma^k r in ascending k in float32, as Dopamine's np.sum over float32 arrays does."""
  ret = np.float32(0.0)
  for k in range(n):
    if terminal[t + k, env]:
      m, term = k + 1, True
      break
    if episode_end[t + k, env]:
      return None
  else:
    m, term = n, False
  for k in range(m):
    ret = np.float32(ret + np.float32(np.float32(gamma ** k) * np.float32(reward[t + k, env])))
  disc = np.float32(0.0) if term else np.float32(gamma ** n)
  return m, ret, disc, term
