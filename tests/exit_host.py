"""NumPy twins of expert iteration, written from the definitions there and not from the kernels: the prior counts of
ble_plan_prior_u16, the sampler with a prior of ble_plan_sample_prior_u8 (plan_host's restatement, extended by import), the per-action
values of ble_plan_action_values_f32 and, in float64, the soft cross-entropy of ble_qnet_soft_bc_step_f32.  TEST TOOLING."""
import numpy as np

import plan_host
import ppo_host

POLICY = (0, 2, 4)
VALUE = 1
M32 = plan_host.M32


# ---------------------------------------------------------------------------------------------------------------------- prior counts
def prior_counts(probs, strength, segments):
  """uint16 [n, segments, 3]: c = p > 0 ? min(65535, trunc(float32(p * float32(strength >> s)))) : 0, zero weight from s = 16."""
  p = np.asarray(probs, np.float32).reshape(-1, 1, 3)
  s = np.arange(segments)
  w = np.where(s < 16, int(strength) >> np.minimum(s, 16), 0).astype(np.float32).reshape(1, -1, 1)
  with np.errstate(invalid='ignore', over='ignore'):
    v = (p * w).astype(np.float32)                                      # one float32 product
    c = np.where(v >= np.float32(65535.0), 65535, np.where(v >= np.float32(1.0), np.minimum(v, np.float32(65535.0)), 0.0))
    c = np.where(np.isnan(v), 0.0, c)
  return np.where(p > 0, c, 0.0).astype(np.int64).astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------- sampler with a prior
def words(n, n_plans, segments, iteration, decision, seed=0, env_seed=None, env_offset=0):
  """uint32 [n, K, S]: the 32-bit word of every (environment, plan, segment), from the definition in include/ble_abi.h: key
  (seed_e ^ PLANS, high word ^ the decision counter's high word), counter (block, decision low, key_e low, key_e high), block =
  (iteration 1024 + k) 256 + s / 4, word s % 4."""
  e = np.arange(n, dtype=np.uint64)
  if env_seed is None:
    seeds, keys = np.full(n, int(seed) & (2 ** 64 - 1), np.uint64), e + np.uint64(env_offset)
  else:
    seeds, keys = np.asarray(env_seed).astype(np.uint64), np.zeros(n, np.uint64)
  seeds = seeds ^ np.uint64(plan_host.PLAN_KEY)
  decision = int(decision) & (2 ** 64 - 1)
  out = np.empty((n, n_plans, segments), np.uint32)
  for k in range(n_plans):
    for blk in range(-(-segments // 4)):
      counter = np.stack([np.full(n, (iteration * 1024 + k) * 256 + blk, np.uint64), np.full(n, decision & 0xFFFFFFFF, np.uint64), keys & M32,
                          keys >> np.uint64(32)], -1)
      key = np.stack([seeds & M32, (seeds >> np.uint64(32)) ^ np.uint64(decision >> 32)], -1)
      four = plan_host.philox4x32(counter, key)                          # [n, 4]
      take = min(4, segments - 4 * blk)
      out[:, k, 4 * blk:4 * blk + take] = four[:, :take]
  return out


def sample_prior(n, n_plans, n_entries, segment, iteration, decision, prior, seed=0, env_seed=None, env_offset=0, counts=None,
                 best_plan=None):
  """plans uint8 [H, n, K]: plan_host.sample, except that iteration 0 draws its free plans (k >= 4) from prior [n, segments, 3]."""
  base = plan_host.sample(n, n_plans, n_entries, segment, iteration, decision, seed=seed, env_seed=env_seed, env_offset=env_offset,
                          counts=counts, best_plan=best_plan)
  if iteration > 0 or n_plans <= 4:
    return base
  H, K = int(n_entries), int(n_plans)
  S = -(-H // segment)
  w = words(n, K, S, 0, decision, seed, env_seed, env_offset)
  c = np.asarray(prior).astype(np.int64).reshape(n, 1, S, 3)
  seg_action = plan_host.draw(w, c[..., 0], c[..., 1], c[..., 2])      # [n, K, S]
  drawn = seg_action[:, :, np.arange(H) // segment].transpose(2, 0, 1)
  out = base.copy()
  out[:, :, 4:] = drawn[:, :, 4:]
  return out


# --------------------------------------------------------------------------------------------------------------------- action values
def better(new, old):
  """ble_plan_select_f32's incumbent rule on two float32 values: new is finite and strictly greater, or old is not finite."""
  return bool(np.isfinite(new)) and (not np.isfinite(old) or float(new) > float(old))


def action_values(ret, first, stored=None):
  """ret float32 [n, K], first uint8 [n, K] (an entry >= 2 counts as 2); stored = (q, q_k, visits), each [n, 3], to accumulate into.
  -> (q float32 [n, 3], q_k int32 [n, 3], visits int32 [n, 3])."""
  ret = np.asarray(ret, np.float32)
  first = np.minimum(np.asarray(first).astype(np.int64), 2)
  n = ret.shape[0]
  q = np.full((n, 3), -np.inf, np.float32) if stored is None else np.array(stored[0], np.float32)
  q_k = np.full((n, 3), -1, np.int32)
  visits = np.zeros((n, 3), np.int32) if stored is None else np.array(stored[2], np.int32)
  for e in range(n):
    o = plan_host.order(ret[e])
    for a in range(3):
      visits[e, a] += int((first[e] == a).sum())
      mine = [k for k in o if first[e, k] == a]
      if not mine or not np.isfinite(ret[e, mine[0]]):
        continue                                                         # (no finite plan: -Inf / the stored value, q_k -1)
      k = int(mine[0])
      if stored is None or better(ret[e, k], q[e, a]):
        q[e, a], q_k[e, a] = ret[e, k], k
  return q, q_k, visits


# ------------------------------------------------------------------------------------------------------------------------ soft loss
def best_valid(q):
  """a* [B] of q [B, 3]: the finite entry first in the selection's order (the value descending, -0 == +0, then a ascending); 0 for a
  row without one.  any_valid [B]."""
  q = np.asarray(q, np.float32)
  star = np.array([plan_host.order(row)[0] for row in q], np.int64)
  return star, np.isfinite(q).any(axis=1)


def soft_target(q, beta, smoothing):
  """float64 [B, 3]: t' = (1 - s) softmax(beta q over the finite entries) + s / 3, with beta and s rounded to float32 first and the
  product q beta taken in float32 (the kernel's input rounding); an invalid action: t = 0 exactly."""
  q = np.asarray(q, np.float32)
  valid = np.isfinite(q)
  with np.errstate(invalid='ignore', over='ignore'):
    y = np.where(valid, (q * np.float32(beta)).astype(np.float32), -np.inf).astype(np.float64)
  m = np.where(valid.any(axis=1), np.max(y, axis=1), 0.0)
  e = np.where(valid, np.exp(y - m[:, None]), 0.0)
  s = (e[:, 0] + e[:, 1]) + e[:, 2]
  t = e / np.where(s > 0, s, 1.0)[:, None]
  sm = float(np.float32(smoothing))
  return (1.0 - sm) * t + sm / 3.0


def soft_bc_loss(logits, q, ret=None, beta=1.0, smoothing=0.0, value_coef=0.0):
  """float64: (per-row loss [B], aux [B, 2] = (lp[a*], agree), dlogits [B, 6] of the objective mean_b L_b).  value_coef == 0: ret is
  not read.  A row without a finite q is all zeros."""
  z = np.asarray(logits, np.float64)
  b = len(z)
  cv = float(np.float32(value_coef))
  lp, p = ppo_host.log_softmax(z[:, list(POLICY)])
  t = soft_target(q, beta, smoothing)
  ce = -((t[:, 0] * lp[:, 0] + t[:, 1] * lp[:, 1]) + t[:, 2] * lp[:, 2])
  d = np.zeros((b, 6))
  for k in range(3):
    d[:, 2 * k] = (p[:, k] - t[:, k]) / b
  loss = ce
  if cv != 0.0:
    dv = z[:, VALUE] - np.asarray(ret, np.float64)
    loss = ce + cv * (dv * dv)
    d[:, VALUE] = (2.0 * cv * dv) / b
  star, valid = best_valid(q)
  agree = (ppo_host.greedy(np.asarray(logits)[:, :6]).astype(np.int64) == star).astype(np.float64)
  aux = np.stack([lp[np.arange(b), star], agree], axis=1)
  return np.where(valid, loss, 0.0), np.where(valid[:, None], aux, 0.0), np.where(valid[:, None], d, 0.0)
