"""Float64 NumPy restatements of the TD learners of one-atom networks (csrc/ble_train.h's ble_td_loss_kernel and ble_sgd_kernel,
ble_qnet_td_step_f32): Dopamine 4.0.0 JaxDQNAgent's target with its 'mse' and 'huber' losses, the reference MLP agent's SARSA loss with
the gradient through both Q terms, and optax.sgd.  Every gradient is of the objective mean_b L_b, hand-derived; test_td_host.py checks
the derivations against torch.autograd.  The network's forward and backward are train_host's."""
import numpy as np

import train_host

NUM_ACTIONS = 3
KINDS = ('mse', 'huber', 'sarsa')


def dqn_targets(target_q, ret, discount):
  """T[b] = ret + discount * max_a q'(s')[b, a] (the first maximum)."""
  z = np.asarray(target_q, np.float64)
  return np.asarray(ret, np.float64) + np.asarray(discount, np.float64) * z[np.arange(len(z)), z.argmax(axis=1)]


def dqn_loss(q, tgt, action, kind):
  """(L [B], dL/dq [B, 3]) of the objective mean_b L_b; u = T - q(s)[a]: 'mse' u^2, 'huber' u^2 / 2 if |u| <= 1 else |u| - 1/2."""
  q = np.asarray(q, np.float64)
  b = len(q)
  rows, action = np.arange(b), np.asarray(action)
  u = np.asarray(tgt, np.float64) - q[rows, action]
  if kind == 'mse':
    loss, du = u * u, 2.0 * u
  elif kind == 'huber':
    au = np.abs(u)
    loss, du = np.where(au <= 1.0, 0.5 * u * u, au - 0.5), np.clip(u, -1.0, 1.0)
  else:
    raise ValueError(kind)
  d = np.zeros_like(q)
  d[rows, action] = -du / b
  return loss, d


def sarsa_loss(q_state, q_next, reward, action, next_action, gamma, mask=None):
  """(T [B], L [B], dL/dq(s) [B, 3], dL/dq(s') [B, 3]) of mean_b L_b, L_b = delta^2, delta = q(s)[a] - (r + gamma q(s')[a']), both
  terms differentiated; a masked row (mask != 0) has L_b = 0 and zero gradient and still counts in B."""
  qs, qn = np.asarray(q_state, np.float64), np.asarray(q_next, np.float64)
  b = len(qs)
  rows, action, next_action = np.arange(b), np.asarray(action), np.asarray(next_action)
  tgt = np.asarray(reward, np.float64) + gamma * qn[rows, next_action]
  live = np.ones(b) if mask is None else (np.asarray(mask) == 0).astype(np.float64)
  delta = (qs[rows, action] - tgt) * live
  ds, dn = np.zeros_like(qs), np.zeros_like(qn)
  ds[rows, action] = 2.0 * delta / b
  dn[rows, next_action] = -2.0 * gamma * delta / b
  return tgt, delta * delta, ds, dn


def sarsa_backward(params, state, next_state, ds, dn, acts_state=None, acts_next=None, magnitude=False):
  """[(dW_l, db_l)] of both branches summed (the parameters are shared): train_host.backward on each branch.  magnitude: the bound S
  instead, train_host.backward_magnitude summed over the branches."""
  f = train_host.backward_magnitude if magnitude else train_host.backward
  a, c = f(params, state, ds, acts_state), f(params, next_state, dn, acts_next)
  return [(a[l][0] + c[l][0], a[l][1] + c[l][1]) for l in range(len(a))]


def sgd(w, g, lr):
  """optax.sgd(lr), no momentum, float64."""
  return np.asarray(w, np.float64) - lr * np.asarray(g, np.float64)
