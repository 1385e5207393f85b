"""The learned terminal value's bootstrap on the CPU: the NumPy float64 twin (leaves_host.bootstrap) against the host build
of the kernel's own lane function (csrc/ble_plan.h: plan_bootstrap_lane, tests/emul/leaves_emul.cpp), bit for bit, and what the lane
function promises: the rollout's own discount, two roundings, a select on dead leaves."""
import numpy as np
import pytest

import leaves_host
from emul import leaves_emul

STEPS = (0, 1, 24, 960)
GAMMAS = (0.0, 0.993, 1.0)
DENORMAL = np.float32(1e-42)
SPECIAL = np.array([0.0, -0.0, DENORMAL, -DENORMAL, np.inf, -np.inf, np.nan, 1.5, -683.25], np.float32)


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cases(rng, total):
  """ret, steps_flown, leaf_status, value: every (steps, special value, live / dead) combination, then random rows up to `total`."""
  rows = [(np.float32(rng.standard_normal() * 20.0), s, st, v) for s in STEPS for v in SPECIAL for st in (0, 1, 2, 3)]
  rows += [(r, 24, 0, np.float32(2.0)) for r in SPECIAL]                                     # special returns on live leaves
  ret, steps, status, value = (np.array(c) for c in zip(*rows))
  more = max(total - len(rows), 0)
  ret = np.concatenate([ret.astype(np.float32), (rng.standard_normal(more) * 30.0).astype(np.float32)])
  steps = np.concatenate([steps.astype(np.int32), rng.integers(0, 961, more).astype(np.int32)])
  status = np.concatenate([status.astype(np.uint8), (rng.random(more) < 0.2).astype(np.uint8) * rng.integers(1, 4, more).astype(np.uint8)])
  value = np.concatenate([value.astype(np.float32), (rng.standard_normal(more) * 100.0).astype(np.float32)])
  return ret, steps, status, value


@pytest.mark.parametrize('gamma', GAMMAS)
def test_the_twin_equals_the_lane_function(gamma):
  ret, steps, status, value = _cases(np.random.default_rng(7), 4096)
  got = leaves_emul.bootstrap(ret, steps, status, value, gamma)
  want = leaves_host.bootstrap(ret, steps, status, value, gamma)
  assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:4].tolist()


def test_the_discount_is_the_rollouts_own_sequence():
  """disc after t steps of the rollout kernels: 1.0, then `disc *= gamma` once per step flown -- not pow(gamma, t)."""
  gamma = 0.993
  disc, seq = 1.0, []
  for t in range(961):
    seq.append(disc)
    disc *= gamma
  steps = np.arange(961, dtype=np.int32)
  assert np.array_equal(leaves_host.discount(steps, gamma), np.array(seq))
  assert np.any(leaves_host.discount(steps, gamma) != np.power(gamma, steps.astype(np.float64)))      # (the two do differ)
  # through the lane function: ret 0 and value 1 on live leaves give the discount rounded to float32
  one = leaves_emul.bootstrap(np.zeros(961, np.float32), steps, np.zeros(961, np.uint8), np.ones(961, np.float32), gamma)
  assert np.array_equal(_bits(one), _bits(np.array(seq).astype(np.float32)))


def test_a_dead_leaf_keeps_its_return_whatever_its_value():
  ret = np.array([1.25, -0.0, np.nan, np.inf, -3.0], np.float32)
  for status in (1, 2, 3, 255):
    for v in SPECIAL:
      got = leaves_emul.bootstrap(ret, np.full(5, 24, np.int32), np.full(5, status, np.uint8), np.full(5, v, np.float32), 0.993)
      assert np.array_equal(_bits(got), _bits(ret)), (status, v)


def test_live_leaves_two_roundings_and_non_finite_values():
  gamma, steps = 0.993, np.full(3, 24, np.int32)
  live = np.zeros(3, np.uint8)
  got = leaves_emul.bootstrap(np.array([1.0, 1.0, 1.0], np.float32), steps, live, np.array([np.nan, np.inf, -np.inf], np.float32), gamma)
  assert np.isnan(got[0]) and got[1] == np.inf and got[2] == -np.inf
  # gamma 0: the value counts only where no step was flown (0^0 = 1: d starts at 1.0)
  got = leaves_emul.bootstrap(np.array([2.0, 2.0], np.float32), np.array([0, 1], np.int32), np.zeros(2, np.uint8), np.array([5.0, 5.0], np.float32), 0.0)
  assert got.tolist() == [7.0, 2.0]
  # a value of +-0 or a denormal leaves a finite return as it is, to the bit, except that -0 + +0 is +0
  r = np.array([1.5, -2.25, -0.0], np.float32)
  for v in (0.0, -0.0, DENORMAL):
    got = leaves_emul.bootstrap(r, steps, live, np.full(3, v, np.float32), gamma)
    assert np.array_equal(got[:2], r[:2])
  # the sum is formed in float64 and rounded once: not float32(ret) + float32(t)
  rng = np.random.default_rng(3)
  ret, value = (rng.standard_normal(2048) * 50).astype(np.float32), (rng.standard_normal(2048) * 50).astype(np.float32)
  steps = rng.integers(0, 40, 2048).astype(np.int32)
  got = leaves_emul.bootstrap(ret, steps, np.zeros(2048, np.uint8), value, gamma)
  exact = ret.astype(np.float64) + leaves_host.discount(steps, gamma) * value.astype(np.float64)
  assert np.all(np.abs(got.astype(np.float64) - exact) <= 0.5 * np.spacing(np.abs(got)).astype(np.float64) * (1 + 1e-9))
