"""NumPy twin of the planner's two ends, written from the definition there and not from the kernels: Philox4x32-10, the
plan sampler of ble_plan_sample_u8 and the order, incumbent rule and elite counts of ble_plan_select_f32.  Integers only on the
sampling side, so the device's plans are reproduced bit for bit.  TEST TOOLING."""
import numpy as np

PLAN_KEY = 0x504C414E53
STAY = 1
M32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
  """Philox4x32-10 (Salmon et al. 2011).  counter [..., 4], key [..., 2], any integer arrays of 32-bit values -> uint32 [..., 4]."""
  c = [np.asarray(counter[..., i], np.uint64) & M32 for i in range(4)]
  k0, k1 = (np.asarray(key[..., i], np.uint64) & M32 for i in range(2))
  for _ in range(10):
    p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
    c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
    k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
  return np.stack(c, -1).astype(np.uint32)


def draw(word, c0, c1, c2):
  """The action of one segment from its 32-bit word and its elite counts."""
  r = ((np.asarray(word, np.uint64) * (np.asarray(c0 + c1 + c2, np.uint64) + np.uint64(3))) >> np.uint64(32)).astype(np.int64)
  return np.where(r < c0 + 1, 0, np.where(r < c0 + c1 + 2, 1, 2)).astype(np.uint8)


def sample(n, n_plans, n_entries, segment, iteration, decision, seed=0, env_seed=None, env_offset=0, counts=None, best_plan=None):
  """plans uint8 [H, n, K].  seed: the batch's seed, environments keyed env_offset + e; env_seed (uint64 [n]): a seed per environment,
  every stream keyed 0.  counts: [n, segments, 3] (iteration > 0); best_plan: uint8 [H, n] (the warm start; default all STAY)."""
  H, K = int(n_entries), int(n_plans)
  S = -(-H // segment)
  e = np.arange(n, dtype=np.uint64)
  if env_seed is None:
    seeds, keys = np.full(n, int(seed) & (2 ** 64 - 1), np.uint64), e + np.uint64(env_offset)
  else:
    seeds, keys = np.asarray(env_seed).astype(np.uint64), np.zeros(n, np.uint64)
  seeds = seeds ^ np.uint64(PLAN_KEY)
  decision = int(decision) & (2 ** 64 - 1)
  key = np.stack([seeds & M32, (seeds >> np.uint64(32)) ^ np.uint64(decision >> 32)], -1)                 # [n, 2]
  k = np.arange(K, dtype=np.uint64)
  s = np.arange(S, dtype=np.uint64)
  block = (np.uint64(iteration * 1024) + k)[:, None] * np.uint64(256) + (s // np.uint64(4))[None, :]        # [K, S]
  counter = np.empty((n, K, S, 4), np.uint64)
  counter[..., 0] = block[None]
  counter[..., 1] = decision & 0xFFFFFFFF
  counter[..., 2] = (keys & M32)[:, None, None]
  counter[..., 3] = (keys >> np.uint64(32))[:, None, None]
  out = philox4x32(counter, np.broadcast_to(key[:, None, None, :], (n, K, S, 2)))
  word = np.take_along_axis(out, np.broadcast_to((s % np.uint64(4)).astype(np.int64)[None, None, :, None], (n, K, S, 1)), -1)[..., 0]
  if iteration > 0:
    c = np.asarray(counts).astype(np.int64).reshape(n, 1, S, 3)
    c0, c1, c2 = c[..., 0], c[..., 1], c[..., 2]
  else:
    c0 = c1 = c2 = np.zeros((1, 1, 1), np.int64)
  seg_action = draw(word, c0, c1, c2)                                    # [n, K, S]
  plans = np.ascontiguousarray(seg_action[:, :, np.arange(H) // segment].transpose(2, 0, 1))      # [H, n, K]
  if iteration == 0:
    for slot, a in ((0, STAY), (1, 0), (2, 2)):
      if K > slot:
        plans[:, :, slot] = a
    if K > 3:
      prev = np.full((H, n), STAY, np.uint8) if best_plan is None else np.asarray(best_plan, np.uint8)
      plans[:, :, 3] = prev[np.minimum(np.arange(H) + 1, H - 1)]
  return plans


def order(ret):
  """The plans of one environment, best first: finite before non-finite, the return descending, k ascending (-0 == +0)."""
  ret = np.asarray(ret, np.float32)
  finite = np.isfinite(ret)
  value = np.where(finite, ret, np.float32(0.0)).astype(np.float64) + 0.0
  return np.lexsort((np.arange(len(ret)), -value, ~finite))


def select(ret, plans, iteration, elite, segment, best_return=None, best_plan=None):
  """ret [n, K] float32, plans [H, n, K]; best_return [n] / best_plan [H, n]: the incumbent (iteration > 0).
  -> (best_return [n] f32, best_k [n] i32, best_plan [H, n] u8, action [n] u8, counts [n, segments, 3] u16 or None)."""
  ret = np.asarray(ret, np.float32)
  H, n, K = plans.shape
  S = -(-H // segment)
  out_return = np.empty(n, np.float32) if iteration == 0 else np.array(best_return, np.float32)
  out_plan = np.empty((H, n), np.uint8) if iteration == 0 else np.array(best_plan, np.uint8)
  out_k = np.full(n, -1, np.int32)
  counts = np.zeros((n, S, 3), np.uint16) if elite >= 1 else None
  for e in range(n):
    o = order(ret[e])
    k, new = int(o[0]), ret[e, o[0]]
    if iteration == 0:
      replace = bool(np.isfinite(new))
      if not replace:
        out_return[e], out_plan[:, e] = -np.inf, STAY
    else:
      replace = bool(np.isfinite(new)) and (not np.isfinite(out_return[e]) or new > out_return[e])
    if replace:
      out_return[e], out_k[e], out_plan[:, e] = new, k, plans[:, e, k]
    if elite >= 1:
      first = plans[::segment, e, :][:, o[:elite]]                        # [S, E]
      for a in range(3):
        counts[e, :, a] = (first == a).sum(1) if a < 2 else (first >= 2).sum(1)
  return out_return, out_k, out_plan, out_plan[0].copy(), counts
