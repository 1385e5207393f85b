"""The planner's two ends -- ble_plan_sample_u8, ble_plan_select_f32 -- on a machine without a GPU: the entries are declared, exported and
mirrored (their sizes travel in structs: no int64 argument), every invalid argument answers BLE_E_INVALID_ARG before any HIP call, with
n == 0 and with n == 64 (no call below has valid arguments and n > 0: that would launch), and the lane functions of csrc/ble_plan.h,
built for the host (tests/emul/plan_emul.cpp), equal the NumPy twin written from DESIGN 3k (tests/plan_host.py) bit for bit: the
sampler is integer arithmetic, the selection an order on float32 values, so there is no tolerance anywhere in this file."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import plan_host
from balloon_learning_environment_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID_ARG = -1
_FAKE = 0x1000          # a non-NULL address that is never dereferenced (the checks come before any HIP call)
ENTRIES = ('ble_plan_sample_u8', 'ble_plan_select_f32')


def _header():
  return open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()


def _ps(**over):
  f = dict(n=0, n_plans=8, n_plan_steps=6, segment=2, iteration=0, seed=1, env_seed=None, env_offset=0, decision_counter=_FAKE,
           elite_counts=_FAKE, best_plan=_FAKE, plans=_FAKE)
  f.update(over)
  return _abi.BlePlanSample(**f)


def _sel(**over):
  f = dict(n=0, n_plans=8, n_plan_steps=6, segment=2, iteration=0, elite=2, reserved_=0, ret=_FAKE, plans=_FAKE, best_return=_FAKE,
           best_k=_FAKE, best_plan=_FAKE, action=_FAKE, elite_counts=_FAKE, advance_counter=None)
  f.update(over)
  return _abi.BlePlanSelect(**f)


def _sample(ps):
  return _lib.lib().ble_plan_sample_u8(None if ps is None else ctypes.byref(ps), None)


def _select(sel):
  return _lib.lib().ble_plan_select_f32(None if sel is None else ctypes.byref(sel), None)


def test_declared_exported_and_mirrored():
  header = _header()
  assert re.search(r'\bint ble_plan_sample_u8\(const struct ble_plan_sample\* ps, void\* stream\);', header)
  assert re.search(r'\bint ble_plan_select_f32\(const struct ble_plan_select\* sel, void\* stream\);', header)
  assert re.search(r'#define BLE_PLAN_MAX_PLANS 1024\b', header) and _abi.PLAN_MAX_PLANS == 1024
  assert re.search(r'#define BLE_PLAN_MAX_ITERATIONS 16\b', header) and _abi.PLAN_MAX_ITERATIONS == 16
  assert re.search(r'#define BLE_ABI_VERSION 5\b', header) and _lib.ABI_VERSION == 5            # additive: the ABI stays 5
  symbols = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
  for name in ENTRIES:
    assert name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS, name
    assert re.search(r' T ' + name + r'$', symbols, re.M), name
    fn = getattr(_lib.lib(), name)
    assert fn.argtypes is not None and fn.restype is ctypes.c_int
    assert ctypes.c_int64 not in fn.argtypes, name          # sizes travel in the structs
  assert any(s.endswith('ble_plan.h') for s in _lib._SOURCES)
  hip = open(os.path.join(ROOT, 'balloon_learning_environment_amd', 'csrc', 'ble_kernels.hip')).read()
  assert hip.index('#include "ble_gp_belief.h"') < hip.index('#include "ble_plan.h"')


@pytest.mark.parametrize('tag, mirror, size', [('ble_plan_sample', _abi.BlePlanSample, 80), ('ble_plan_select', _abi.BlePlanSelect, 96)])
def test_struct_layout_matches_the_header(tag, mirror, size):
  body = re.search(r'struct ' + tag + r' \{(.*?)\n\};', _header(), re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  declared = [re.search(r'(\w+)\s*$', d).group(1) for d in body.split(';') if d.strip()]
  assert declared == [f[0] for f in mirror._fields_]
  assert ctypes.sizeof(mirror) == size
  # 8-byte members after the int32 block start on an 8-byte boundary with no padding: an even number of int32 fields
  ints = [f for f in mirror._fields_ if f[1] is ctypes.c_int32]
  assert len(ints) % 2 == 0 and mirror.n.offset == 0 and mirror.n_plans.offset == 8


def test_empty_batch_is_ok_without_a_launch():
  assert _sample(_ps()) == _lib.BLE_OK
  assert _sample(_ps(elite_counts=None)) == _lib.BLE_OK                     # iteration 0 reads no counts
  assert _sample(_ps(iteration=15, env_seed=_FAKE, n_plans=1024, n_plan_steps=960, segment=1000)) == _lib.BLE_OK
  assert _select(_sel()) == _lib.BLE_OK
  assert _select(_sel(elite=0, elite_counts=None, advance_counter=_FAKE)) == _lib.BLE_OK
  assert _select(_sel(elite=8, iteration=15, n_plans=1024, n_plan_steps=960)) == _lib.BLE_OK


_SIZES = {                      # what both entries refuse
    'plans_0': dict(n_plans=0), 'plans_negative': dict(n_plans=-1), 'plans_1025': dict(n_plans=1025),
    'steps_0': dict(n_plan_steps=0), 'steps_961': dict(n_plan_steps=961), 'steps_negative': dict(n_plan_steps=-3),
    'segment_0': dict(segment=0), 'segment_negative': dict(segment=-1),
    'iteration_16': dict(iteration=16), 'iteration_negative': dict(iteration=-1),
    'negative_n': dict(n=-1), 'n_2_31': dict(n=2 ** 31, n_plans=1), 'n_times_k_2_31': dict(n=2 ** 21, n_plans=1024),
}

_CASES = {
    'sample_null_struct': lambda n: _sample(None),
    **{f'sample_{k}': (lambda n, k=k: _sample(_ps(**{'n': n, **_SIZES[k]}))) for k in _SIZES},
    **{f'sample_null_{f}': (lambda n, f=f: _sample(_ps(n=n, **{f: None}))) for f in ('plans', 'decision_counter', 'best_plan')},
    'sample_null_counts_in_iteration_1': lambda n: _sample(_ps(n=n, iteration=1, elite_counts=None)),
    'sample_negative_env_offset': lambda n: _sample(_ps(n=n, env_offset=-1)),
    'select_null_struct': lambda n: _select(None),
    **{f'select_{k}': (lambda n, k=k: _select(_sel(**{'n': n, **_SIZES[k]}))) for k in _SIZES},
    **{f'select_null_{f}': (lambda n, f=f: _select(_sel(n=n, **{f: None})))
       for f in ('ret', 'plans', 'best_return', 'best_k', 'best_plan', 'action', 'elite_counts')},
    'select_elite_above_k': lambda n: _select(_sel(n=n, elite=9)),
    'select_elite_negative': lambda n: _select(_sel(n=n, elite=-1)),
}


@pytest.mark.parametrize('n', [0, 64])
@pytest.mark.parametrize('case', sorted(_CASES))
def test_invalid_argument(case, n):
  assert _CASES[case](n) == E_INVALID_ARG


# ---------------------------------------------------------------------------------------------- the lane functions on the host
def test_twin_philox_known_answers():
  """Random123's kat_vectors for Philox4x32-10: the twin's generator is the published one."""
  z = plan_host.philox4x32(np.zeros((1, 4), np.uint64), np.zeros((1, 2), np.uint64))[0]
  assert [int(v) for v in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
  f = plan_host.philox4x32(np.full((1, 4), 0xFFFFFFFF, np.uint64), np.full((1, 2), 0xFFFFFFFF, np.uint64))[0]
  assert [int(v) for v in f] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


_SHAPES = list(itertools.product((1, 3, 4, 5, 67), (1, 2, 7, 9), (1, 3, 4)))          # K, H, segment


@pytest.mark.parametrize('iteration', [0, 1, 15])
def test_sampler_against_the_twin(iteration):
  from emul import plan_emul
  rng = np.random.default_rng(11 + iteration)
  for K, H, segment in _SHAPES:
    S = -(-H // segment)
    for seed, key, decision in ((0, 0, 0), (0x123456789ABCDEF0, 3, 7), (2 ** 64 - 1, 2 ** 33 + 5, 2 ** 32 + 1)):
      counts = rng.integers(0, 9, (1, S, 3)).astype(np.uint16) if iteration else None
      prev = rng.integers(0, 3, (H, 1)).astype(np.uint8)
      want = plan_host.sample(1, K, H, segment, iteration, decision, seed=seed, env_offset=key, counts=counts, best_plan=prev)[:, 0, :]
      got = plan_emul.sample(seed, key, decision, iteration, K, H, segment, None if counts is None else counts[0], prev[:, 0])
      assert np.array_equal(got, want), (K, H, segment, seed, key, decision)
      # a plan is piecewise constant
      if iteration:
        assert all(np.array_equal(got[h], got[h - h % segment]) for h in range(H))


def test_sampler_fixed_slots_and_warm_start():
  from emul import plan_emul
  prev = np.array([2, 0, 1, 2, 0, 0, 1], np.uint8)
  p = plan_emul.sample(9, 0, 4, 0, 5, 7, 3, prev=prev)
  assert (p[:, 0] == 1).all() and (p[:, 1] == 0).all() and (p[:, 2] == 2).all()
  assert np.array_equal(p[:, 3], np.array([0, 1, 2, 0, 0, 1, 1], np.uint8))           # shifted left, the last entry repeated
  assert np.array_equal(plan_emul.sample(9, 0, 4, 0, 3, 7, 3, prev=prev), p[:, :3])        # as far as K reaches
  assert (plan_emul.sample(9, 0, 4, 0, 5, 7, 3)[:, 3] == 1).all()                          # no previous plan: all STAY
  # iteration 1 has no fixed slot: its first plans are draws like the others
  q = plan_emul.sample(9, 0, 4, 1, 64, 7, 1, counts=np.zeros((7, 3), np.uint16))
  assert len({bytes(q[:, k]) for k in range(4)}) > 1


def test_sampler_crosses_philox_blocks_and_depends_on_its_key_only():
  from emul import plan_emul
  H, segment = 23, 1                   # 23 segments: blocks 0 .. 5 of every plan
  a = plan_emul.sample(7, 2, 5, 0, 67, H, segment)
  want = plan_host.sample(3, 67, H, segment, 0, 5, seed=7)[:, 2, :]
  assert np.array_equal(a, want)
  assert np.array_equal(plan_emul.sample(7, 2, 5, 0, 5, H, segment), a[:, :5])              # plan k does not depend on K
  assert np.array_equal(plan_emul.sample(7, 2, 5, 0, 67, 9, segment), a[:9])                # a shorter plan is a prefix (segment 1)
  for other in (plan_emul.sample(8, 2, 5, 0, 67, H, segment), plan_emul.sample(7, 3, 5, 0, 67, H, segment),
                plan_emul.sample(7, 2, 6, 0, 67, H, segment), plan_emul.sample(7, 2, 5 + 2 ** 32, 0, 67, H, segment)):
    assert not np.array_equal(other[:, 4:], a[:, 4:])
  # uniform thirds in iteration 0 (63 x 23 draws: each action 483 +- 3 sigma of 18)
  hist = np.bincount(a[:, 4:].ravel(), minlength=3)
  assert hist.sum() == 63 * 23 and (np.abs(hist - 483) < 60).all(), hist


@pytest.mark.parametrize('action', [0, 1, 2])
def test_sampler_counts_force_an_action(action):
  """E = 8 with all eight on one action: that action has probability 9 / 11 (the histogram, not the bits: those are the twin test's)."""
  from emul import plan_emul
  H, K = 9, 1024
  counts = np.zeros((H, 3), np.uint16)
  counts[:, action] = 8
  p = plan_emul.sample(3, 0, 1, 1, K, H, 1, counts=counts)
  assert np.array_equal(p, plan_host.sample(1, K, H, 1, 1, 1, seed=3, counts=counts[None])[:, 0, :])
  share = np.bincount(p.ravel(), minlength=3) / p.size
  want = np.full(3, 1 / 11)
  want[action] = 9 / 11
  assert (np.abs(share - want) < 5 * np.sqrt(want * (1 - want) / p.size)).all(), share
  # the draw itself at the edges of a word
  assert plan_emul.draw(0, *(int(c) for c in counts[0])) == 0 and plan_emul.draw(2 ** 32 - 1, *(int(c) for c in counts[0])) == 2
  assert plan_emul.draw(0, 0, 0, 0) == 0 and plan_emul.draw(2 ** 32 - 1, 0, 0, 0) == 2 and plan_emul.draw(2 ** 31, 0, 0, 0) == 1


def _crafted(K, rng):
  """Rows of returns with exact ties, +-inf and NaN in some slots and in all, -0 against +0."""
  base = rng.integers(0, 6, K).astype(np.float32) * np.float32(0.25)             # many exact ties
  rows = [base.copy(), np.zeros(K, np.float32), np.full(K, np.nan, np.float32), np.full(K, np.inf, np.float32),
          rng.standard_normal(K).astype(np.float32)]
  r = base.copy(); r[::3] = np.nan; rows.append(r)
  r = base.copy(); r[0] = np.inf; r[-1] = -np.inf; rows.append(r)
  r = base.copy(); r[K // 2] = np.float32(7.0); rows.append(r)                   # one clear best
  r = np.zeros(K, np.float32); r[::2] = np.float32(-0.0); rows.append(r)          # -0 ties with +0: k = 0 wins
  r = -base - np.float32(1.0); r[-1] = np.nan; rows.append(r)                     # all negative
  return rows


@pytest.mark.parametrize('K', [1, 3, 8, 67])
def test_select_against_the_twin(K):
  from emul import plan_emul
  rng = np.random.default_rng(K)
  H, segment = 7, 3
  for row, ret in enumerate(_crafted(K, rng)):
    plans = rng.integers(0, 3, (H, 1, K)).astype(np.uint8)
    for elite in sorted({0, 1, min(8, K), K}):
      # iteration 0: no incumbent
      want = plan_host.select(ret[None], plans, 0, elite, segment)
      got = plan_emul.select(ret, plans[:, 0, :], 0, elite, segment)
      _same(got, want, (K, row, elite, 0))
      # iteration 1 against incumbents below, equal to and above the new best, and a non-finite one
      finite = ret[np.isfinite(ret)]
      top = np.float32(finite.max()) if len(finite) else np.float32(0.0)
      for inc in (np.nextafter(top, np.float32(-np.inf)), top, np.nextafter(top, np.float32(np.inf)), np.float32(-np.inf), np.float32(np.nan)):
        prev = rng.integers(0, 3, (H, 1)).astype(np.uint8)
        want = plan_host.select(ret[None], plans, 1, elite, segment, best_return=np.array([inc], np.float32), best_plan=prev)
        got = plan_emul.select(ret, plans[:, 0, :], 1, elite, segment, best_return=inc, best_plan=prev[:, 0])
        _same(got, want, (K, row, elite, float(inc)))
        if inc == top:
          assert got[1] == -1 and np.array_equal(got[2], prev[:, 0])             # a tie keeps the incumbent


def _same(got, want, what):
  br, bk, bp, act, counts = got
  assert np.array_equal(np.float32(br).view(np.uint32), want[0][0].view(np.uint32)), what
  assert bk == want[1][0] and np.array_equal(bp, want[2][:, 0]) and act == want[3][0], what
  assert (counts is None) == (want[4] is None) and (counts is None or np.array_equal(counts, want[4][0])), what


def test_select_rules_spelled_out():
  from emul import plan_emul
  plans = np.array([[1, 0, 2, 0]] * 4, np.uint8)                                  # H = 4, K = 4: plan k is constant
  nan, inf = np.float32(np.nan), np.float32(np.inf)
  # ties go to the smaller k; a non-finite return comes after every finite one, +inf included
  assert plan_emul.select(np.array([1, 2, 2, 1], np.float32), plans, 0, 0, 2)[1] == 1
  assert plan_emul.select(np.array([inf, -5, nan, -5], np.float32), plans, 0, 0, 2)[1] == 1
  # no finite plan: STAY, -inf, -1
  br, bk, bp, act, _ = plan_emul.select(np.array([nan, inf, -inf, nan], np.float32), plans[:, [1, 1, 2, 2]], 0, 0, 2)
  assert br == -inf and bk == -1 and (bp == 1).all() and act == 1
  # all returns 0 (an environment that is not OK): k = 0, the STAY slot
  br, bk, bp, act, _ = plan_emul.select(np.zeros(4, np.float32), plans, 0, 0, 2)
  assert br == 0 and bk == 0 and (bp == 1).all() and act == 1
  # the elite counts: the first E plans in order, per segment and action
  ret = np.array([3, 9, 9, nan], np.float32)                                     # order: 1, 2, 0, 3
  for elite, want in ((1, [1, 0, 0]), (2, [1, 0, 1]), (3, [1, 1, 1]), (4, [2, 1, 1])):
    counts = plan_emul.select(ret, plans, 0, elite, 2)[4]
    assert counts.shape == (2, 3) and (counts == np.array(want, np.uint16)).all(), (elite, counts)
