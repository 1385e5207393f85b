"""A NumPy restatement of the on-policy kernels (csrc/ble_actor.h), written from their contract: the log-softmax of the
three policy logits, the float32 inverse-CDF draw, generalised advantage estimation in float32 (one rounding per operation, the
kernel's order) and in float64 with the bound float32 arithmetic puts between them, the float64 advantage normalisation, its
restatement in the kernel's summation order and the inputs that tell it from its likely mistakes, the float64 PPO loss with its
dL/dlogits, and the actor stream's Philox words from a g++ build of the generator (actor_draws.cpp).  TEST TOOLING."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ACTOR_STREAM = 0x4143544F52          # "ACTOR"
POLICY, VALUE = (0, 2, 4), 1


def log_softmax(z):
  """(lp, p) [..., 3] of logits [..., 3], in the dtype given (float64 unless float32 comes in): m = max, e = exp(z - m),
  S = (e0 + e1) + e2, lp = (z - m) - log S, p = e / S."""
  z = np.asarray(z)
  z = z if z.dtype == np.float32 else z.astype(np.float64)
  d = z - z.max(axis=-1, keepdims=True)
  e = np.exp(d)
  s = (e[..., 0] + e[..., 1]) + e[..., 2]
  return d - np.log(s)[..., None], e / s[..., None]


def uniform24(words):
  """u = float32(w >> 8) * 2^-24 of uint32 words."""
  return (np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def sample(probs_f32, u):
  """The float32 inverse CDF: c0 = p0, c1 = p0 + p1 (rounded to float32), action = u < c0 ? 0 : (u < c1 ? 1 : 2)."""
  p = np.asarray(probs_f32, np.float32)
  u = np.asarray(u, np.float32)
  c0 = p[..., 0]
  c1 = (p[..., 0] + p[..., 1]).astype(np.float32)
  return np.where(u < c0, 0, np.where(u < c1, 1, 2)).astype(np.uint8)


def greedy(logits):
  """The argmax rule over the policy logits: the lowest index among equal maxima; the first NaN."""
  z = np.asarray(logits)[..., list(POLICY)]
  out = np.zeros(z.shape[:-1], np.uint8)
  for i in np.ndindex(*z.shape[:-1]):
    best, qb = 0, z[i][0]
    for a in (1, 2):
      qa = z[i][a]
      if qb == qb and (qa != qa or qa > qb):
        best, qb = a, qa
    out[i] = best
  return out


def _gae(reward, value, boot_value, terminal, episode_end, gamma, lam, dt):
  reward, value, boot_value = (np.asarray(x, dt) for x in (reward, value, boot_value))
  terminal, episode_end = np.asarray(terminal).astype(bool), np.asarray(episode_end).astype(bool)
  steps, n = reward.shape
  gamma = dt(gamma)
  gl = dt(gamma * dt(lam))
  adv, ret = np.zeros((steps, n), dt), np.zeros((steps, n), dt)
  a_next = np.zeros(n, dt)
  with np.errstate(invalid='ignore', over='ignore'):
    for t in range(steps - 1, -1, -1):
      nv = boot_value if t == steps - 1 else value[t + 1]
      boot = np.where(terminal[t], dt(0), np.where(episode_end[t], value[t], nv)).astype(dt)
      p = (gamma * boot).astype(dt)
      s = (reward[t] + p).astype(dt)
      delta = (s - value[t]).astype(dt)
      carry = np.where(episode_end[t], dt(0), a_next).astype(dt)
      q = (gl * carry).astype(dt)
      a = (delta + q).astype(dt)
      adv[t] = a
      ret[t] = (a + value[t]).astype(dt)
      a_next = a
  return adv, ret


def gae_f32(reward, value, boot_value, terminal, episode_end, gamma, lam):
  """(advantage, ret) float32 [T, N]: the kernel's operations, each rounded to float32 (numpy's float32 arithmetic is correctly
  rounded, as the device's add and multiply are)."""
  return _gae(reward, value, boot_value, terminal, episode_end, np.float32(gamma), np.float32(lam), np.float32)


def gae_f64(reward, value, boot_value, terminal, episode_end, gamma, lam):
  return _gae(reward, value, boot_value, terminal, episode_end, gamma, lam, np.float64)


def gae_f32_error_bound(reward, value, boot_value, terminal, episode_end, gamma, lam):
  """E [T, N] float64 with |gae_f32 - gae_f64| <= E for the advantages, to first order in u = 2^-24.  A step rounds five operations
  (gamma boot, r + ., . - v, gl carry, delta + .), each by at most u times a magnitude that
    M_t = |r_t| + gamma |boot_t| + |v_t| + gamma lambda (end_t ? 0 : M_{t+1})
  bounds, and carries gamma lambda of the error of step t + 1 unless an end cuts the trace:
    E_t = gamma lambda (end_t ? 0 : E_{t+1}) + 5 u M_t."""
  reward, value, boot_value = (np.asarray(x, np.float64) for x in (reward, value, boot_value))
  terminal, episode_end = np.asarray(terminal).astype(bool), np.asarray(episode_end).astype(bool)
  steps, n = reward.shape
  gl = float(gamma) * float(lam)
  u = 2.0 ** -24
  bound = np.zeros((steps, n))
  m_next, e_next = np.zeros(n), np.zeros(n)
  for t in range(steps - 1, -1, -1):
    nv = boot_value if t == steps - 1 else value[t + 1]
    boot = np.where(terminal[t], 0.0, np.where(episode_end[t], value[t], nv))
    m = np.abs(reward[t]) + gamma * np.abs(boot) + np.abs(value[t]) + gl * np.where(episode_end[t], 0.0, m_next)
    e = gl * np.where(episode_end[t], 0.0, e_next) + 5.0 * u * m
    bound[t] = e
    m_next, e_next = m, e
  return bound


def normalize_f64(adv):
  """(A - mean) / (sqrt(var) + 1e-8) in float64 (var / M), any summation order."""
  a = np.asarray(adv, np.float64)
  mean = a.sum() / a.size
  var = ((a - mean) ** 2).sum() / a.size
  return (a - mean) / (np.sqrt(var) + 1e-8)


NORM_BLOCK = 256


def strided_sum(x):
  """ble_adv_normalize_kernel's sum of a float64 vector: thread k adds elements k, k + 256, ... ascending from 0.0, then the 256
  partials are added ascending from 0.0."""
  x = np.asarray(x, np.float64).ravel()
  padded = np.zeros(-(-max(x.size, 1) // NORM_BLOCK) * NORM_BLOCK)
  padded[:x.size] = x                                 # (a trailing + 0.0 changes no partial: none is -0.0)
  part = np.zeros(NORM_BLOCK)
  for row in padded.reshape(-1, NORM_BLOCK):
    part = part + row
  total = 0.0
  for p in part:
    total = total + p
  return total


def normalize_ordered(adv):
  """float32: ble_adv_normalize_kernel's stated order.  mean = strided_sum(A) / M; var = strided_sum((A - mean)^2) / M by a second
  pass; (float)((A - mean) / (sqrt(var) + 1e-8)), all in float64 before the one rounding."""
  a = np.asarray(adv, np.float32).astype(np.float64)
  mean = strided_sum(a) / a.size
  d = a - mean
  den = np.sqrt(strided_sum(d * d) / a.size) + 1e-8
  return (d / den).astype(np.float32)


def normalisation_cases():
  """{name: float32 advantages}: the inputs at which a mistake in the normalisation leaves the one-ulp bound (test_ppo_host.py shows
  that each does, and that the stated order alone stays inside).  'normal_M': the block edges of the 256-thread stride; 'equal': all
  advantages 1.75 (every partial sum exact, so mean == A and the outputs are 0 / 1e-8); 'tiny': sigma = 3e-8, where the 1e-8 is a
  quarter of the denominator; 'offset': 1e4 +- 1e-2, where E[x^2] - mean^2 cancels; 'pair' and 'triple': M - 1 against M."""
  cases = {}
  for m in (1, 2, 255, 256, 257, 511, 513, 65537):
    cases[f'normal_{m}'] = np.random.default_rng(m).standard_normal(m).astype(np.float32)
  cases['equal'] = np.full(300, 1.75, np.float32)
  cases['tiny'] = (np.random.default_rng(11).standard_normal(1025) * 3e-8).astype(np.float32)
  cases['offset'] = (1e4 + np.random.default_rng(12).standard_normal(4097) * 1e-2).astype(np.float32)
  cases['pair'] = np.array([1.0, 3.0], np.float32)
  cases['triple'] = np.array([1.0, 2.0, 4.5], np.float32)
  return cases


def ulps_from(got, want64):
  """|got - want| in float32 ulps of want (float64 array); where want == 0 the ulp is the smallest subnormal."""
  ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
  return np.abs(np.asarray(got, np.float64) - want64) / ulp


def ppo_loss(logits, action, old_logp, advantage, ret, clip=0.2, value_coef=0.5, entropy_coef=0.01):
  """float64: (per-row loss [B], aux [B, 2] = (lp_act, H), dlogits [B, 6] of the objective mean_b L_b).  A row whose action is >= 3
  is all zeros."""
  z = np.asarray(logits, np.float64)
  act = np.asarray(action).astype(np.int64)
  old, adv, r = (np.asarray(x, np.float64) for x in (old_logp, advantage, ret))
  b = len(act)
  valid = act < 3
  a = np.where(valid, act, 0)
  lp, p = log_softmax(z[:, list(POLICY)])
  h = -((p[:, 0] * lp[:, 0] + p[:, 1] * lp[:, 1]) + p[:, 2] * lp[:, 2])
  lpa = lp[np.arange(b), a]
  with np.errstate(over='ignore', invalid='ignore'):
    rho = np.exp(lpa - old)
    s1 = rho * adv
    s2 = np.minimum(np.maximum(rho, 1.0 - clip), 1.0 + clip) * adv
    active = s1 <= s2
    lpi = -np.where(active, s1, s2)
    dv = z[:, VALUE] - r
    loss = (lpi + value_coef * (dv * dv)) - entropy_coef * h
    w = adv * rho
    d = np.zeros((b, 6))
    for k in range(3):
      g = np.where(active, -(w * ((a == k).astype(np.float64) - p[:, k])), 0.0)
      d[:, 2 * k] = (g + entropy_coef * (p[:, k] * (lp[:, k] + h))) / b
    d[:, VALUE] = (2.0 * value_coef * dv) / b
  aux = np.stack([lpa, h], axis=1)
  loss, aux, d = np.where(valid, loss, 0.0), np.where(valid[:, None], aux, 0.0), np.where(valid[:, None], d, 0.0)
  return loss, aux, d


def build_actor_draws(directory):
  """Compiles actor_draws.cpp (g++) into `directory`; returns draw(seed, env_offset, n, step) -> uint32 [n], the first philox_u32 of
  the actor stream of environments env_offset .. env_offset + n - 1 at `step`; draw.explore gives the epsilon-greedy stream's."""
  so = os.path.join(str(directory), 'libactor_draws.so')
  subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-include',
                         os.path.join(_HERE, 'emul', 'ble_intrinsics.h'), '-o', so, os.path.join(_HERE, 'actor_draws.cpp')])
  lib = ctypes.CDLL(so)
  for f in (lib.actor_draws, lib.explore_stream_draws):
    f.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p]
    f.restype = None

  def _draw(f, seed, env_offset, n, step):
    w = np.empty(n, np.uint32)
    f(int(seed) & (2 ** 64 - 1), env_offset, n, int(step) & (2 ** 64 - 1), w.ctypes.data)
    return w

  def draw(seed, env_offset, n, step):
    return _draw(lib.actor_draws, seed, env_offset, n, step)
  draw.explore = lambda seed, env_offset, n, step: _draw(lib.explore_stream_draws, seed, env_offset, n, step)
  return draw
