"""NumPy twin of the learned terminal value's bootstrap (csrc/ble_plan.h: plan_bootstrap_lane).

score = ret + gamma^steps_flown * value on a live leaf, ret on a dead one.  float64 throughout, in the lane function's order: the
discount is 1.0 multiplied steps_flown times by gamma (one rounding per multiplication: the rollout's own `disc`), the product and the
sum are two roundings, and the sum is rounded to float32 once.  TEST TOOLING: never imported by the package."""
import numpy as np


def discount(steps_flown, gamma):
  """1.0 multiplied steps_flown[i] times by gamma, float64, elementwise."""
  steps = np.asarray(steps_flown, np.int64)
  d = np.ones(steps.shape, np.float64)
  g = np.float64(gamma)
  for t in range(int(steps.max()) if steps.size else 0):
    d = np.where(steps > t, d * g, d)
  return d


def bootstrap(ret, steps_flown, leaf_status, value, gamma):
  """ret float32 [...], steps_flown int32 [...], leaf_status uint8 [...], value float32 [...] -> score float32 [...]."""
  ret = np.asarray(ret, np.float32)
  value = np.asarray(value, np.float32).reshape(ret.shape)
  status = np.asarray(leaf_status, np.uint8).reshape(ret.shape)
  d = discount(np.asarray(steps_flown).reshape(ret.shape), gamma)
  with np.errstate(all='ignore'):
    t = d * value.astype(np.float64)
    s = ret.astype(np.float64) + t
    return np.where(status == 0, s.astype(np.float32), ret)
