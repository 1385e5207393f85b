"""A NumPy restatement of the imitation kernels (csrc/ble_imitate.h), written from their contract: the float64 smoothed
cross-entropy with its aux and dL/dlogits, and the DAgger mixture on the Philox words of the DAGGER stream.  The stream is
ble_explore_kernel's keying under seed ^ "DAGGER", so its words are actor_draws.cpp's epsilon-greedy words of that seed
(ppo_host.build_actor_draws(...).explore).  TEST TOOLING."""
import numpy as np

import ppo_host

DAGGER_STREAM = 0x444147474552          # "DAGGER"
POLICY, VALUE = ppo_host.POLICY, ppo_host.VALUE


def smoothed_target(action, smoothing):
  """q [B, 3] float64: s3 = s / 3 everywhere, (1 - s) + s3 on the label.  s is taken as the float32 the descriptor carries."""
  s = float(np.float32(smoothing))
  act = np.asarray(action).astype(np.int64)
  s3 = s / 3.0
  q = np.full((len(act), 3), s3)
  q[np.arange(len(act)), np.where(act < 3, act, 0)] = (1.0 - s) + s3
  return q


def bc_loss(logits, action, ret=None, smoothing=0.0, value_coef=0.0):
  """float64: (per-row loss [B], aux [B, 2] = (lp_act, agree), dlogits [B, 6] of the objective mean_b L_b).  value_coef == 0: ret is
  not read, L_b = CE and the value column's gradient is exactly 0.  A row whose action is >= 3 is all zeros."""
  z = np.asarray(logits, np.float64)
  act = np.asarray(action).astype(np.int64)
  b = len(act)
  valid = act < 3
  a = np.where(valid, act, 0)
  cv = float(np.float32(value_coef))
  lp, p = ppo_host.log_softmax(z[:, list(POLICY)])
  q = smoothed_target(act, smoothing)
  ce = -((q[:, 0] * lp[:, 0] + q[:, 1] * lp[:, 1]) + q[:, 2] * lp[:, 2])
  d = np.zeros((b, 6))
  for k in range(3):
    d[:, 2 * k] = (p[:, k] - q[:, k]) / b
  loss = ce
  if cv != 0.0:
    dv = z[:, VALUE] - np.asarray(ret, np.float64)
    loss = ce + cv * (dv * dv)
    d[:, VALUE] = (2.0 * cv * dv) / b
  agree = (ppo_host.greedy(np.asarray(logits)[:, :6]).astype(np.int64) == act).astype(np.float64)
  aux = np.stack([lp[np.arange(b), a], agree], axis=1)
  return np.where(valid, loss, 0.0), np.where(valid[:, None], aux, 0.0), np.where(valid[:, None], d, 0.0)


def dagger_words(draw, seed, env_offset, n, step):
  """uint32 [n]: the first Philox word of the DAGGER stream of environments env_offset .. env_offset + n - 1 at `step`.  draw:
  ppo_host.build_actor_draws(...)."""
  return draw.explore((int(seed) ^ DAGGER_STREAM) & (2 ** 64 - 1), env_offset, n, step)


def mix(learner, expert, beta, words):
  """(action, took_expert) uint8 [n]: took = uniform24(w) < float32(beta); action = took ? expert : learner."""
  u = ppo_host.uniform24(words)
  took = u < np.float32(beta)
  return np.where(took, np.asarray(expert, np.uint8), np.asarray(learner, np.uint8)).astype(np.uint8), took.astype(np.uint8)
