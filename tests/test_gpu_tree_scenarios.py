"""The beam search in scenario winds on the device: ble_tree_expand_scenarios_f32 with ble_plan_risk_f32, ble_tree_select_f32
and ble_tree_finish_f32 through VecSimulator.tree_search(scenarios=) and VecScenarioBeamSearchAgent.

The reference of a scenario node is the look-ahead in scenario winds itself: a node of a non-void group reached by (a_1 .. a_d) must
hold, BIT FOR BIT, the return, steps_flown and final words rollout_plans(scenarios=) gives the plan a_1 x segment, .., a_d x segment in
its scenario, and as its full state what scenario_wind + step leave on a copy.  The scores, the selections and the finish are held to
the NumPy twin (tree_scenarios_host.py) on the device's own returns.  No tolerance anywhere: every comparison is on bits or integers."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import scenario_host as sh
import test_gpu_scenarios as tgs
import tree_host
import tree_scenarios_host as twin
from balloon_learning_environment_amd import _abi, _lib, device as dev, vec_state
from balloon_learning_environment_amd.agents import beam_agent
from balloon_learning_environment_amd.env import balloon_env
from balloon_learning_environment_amd.eval import eval_lib, suites

pytestmark = pytest.mark.gpu

DEVICE = 'cuda:0'
GAMMA = 0.993
FINAL_FIELDS = tgs.FINAL_FIELDS
RINGS = (0, 1, 3, 17, 120)
DEAD, BURST = 1, 2
_dev, _bits = tgs._dev, tgs._bits


def _same_words(a, b, what):
  assert a.dtype == b.dtype and a.shape == b.shape, what
  bad = torch.nonzero(a.contiguous().view(torch.uint8) != b.contiguous().view(torch.uint8))
  assert bad.numel() == 0, (what, bad[:4].tolist())


def _five(seed=500):
  """Five environments whose rings hold (0, 1, 3, 17, 120) observations: environment 1 is not OK, environment 2 bursts in its first step
  in every scenario."""
  src, rng = tgs._source(5, seed, RINGS)
  src.state['status'][DEAD] = 1
  src.state['mols_air'][BURST] += 30000.0
  return src, rng


@pytest.fixture(scope='module')
def five():
  src, _ = _five()
  scn = src.fit_wind_scenarios(3, seed=33)
  torch.cuda.synchronize()
  assert scn.n_obs.cpu().numpy().tolist() == list(RINGS)
  return src, scn


def _guard(src, scn):
  """Clones of everything a search must leave alone: the source, its ring, its caches and the slab."""
  torch.cuda.synchronize()
  snap = {name: t.clone() for name, t in src.state.items()}
  snap.update(episode_cache=src.episode_cache.clone(), slab=scn.slab.clone(), n_obs=scn.n_obs.clone(), episode=src.episode.clone(),
              grid=src.grid.clone(), **{'gp_' + key: t.clone() for key, t in src._gp.items()})
  if src._noise_cache is not None:
    snap['noise_cache'] = src._noise_cache.clone()
  return snap


def _assert_guarded(src, scn, before, what):
  torch.cuda.synchronize()
  after = dict(src.state, episode_cache=src.episode_cache, slab=scn.slab, n_obs=scn.n_obs, episode=src.episode, grid=src.grid,
               noise_cache=src._noise_cache, **{'gp_' + key: t for key, t in src._gp.items()})
  for name, t in before.items():
    assert torch.equal(t.view(torch.uint8), after[name].view(torch.uint8)), (what, name)


def _final(leaves, shape):
  return np.stack([leaves.state[f].view(*shape).cpu().numpy() for f in FINAL_FIELDS])


# ------------------------------------------------------------------------------------------------ 1: one level is the rollout
@pytest.mark.parametrize('segment', [1, 3])
def test_one_level_is_the_rollout(five, segment):
  src, scn = five
  n, M = src.n, scn.num
  plans = np.ascontiguousarray(np.broadcast_to(np.arange(3, dtype=np.uint8), (segment, n, 3)))
  want = src.rollout_plans(_dev(plans), gamma=GAMMA, scenarios=scn, want_final=True)
  before = _guard(src, scn)
  got = src.tree_search(1, 1, segment=segment, gamma=GAMMA, scenarios=scn, action_values=True)
  _assert_guarded(src, scn, before, 'the source')
  assert tuple(got.returns.shape) == (n, 3, M) and tuple(got.steps_flown.shape) == (n, 3, M) and tuple(got.score.shape) == (n, 3)
  assert got.leaves.n == n * 3 * M and got.leaves.leaves_per_env == 3 * M
  ret, want_ret = got.returns.cpu().numpy(), want.returns.cpu().numpy()
  void = np.zeros((n, 3), bool)
  void[DEAD, 1:] = True                           # a source that is not OK: its a = 0 group is the carry, the other two are void
  assert np.isnan(ret[void]).all() and not np.isnan(ret[~void]).any()
  assert np.array_equal(_bits(ret[~void]), _bits(want_ret[~void]))
  assert np.array_equal(got.steps_flown.cpu().numpy(), want.steps_flown.cpu().numpy())
  assert np.array_equal(_bits(_final(got.leaves, (n, 3, M))), _bits(want.final.cpu().numpy()))       # (a void node is the same copy)
  flown = want.steps_flown.cpu().numpy()
  assert (flown[DEAD] == 0).all() and (flown[BURST] == 1).all()
  # really flown: the scenarios of a live group end elsewhere than each other, and earn other returns
  live = [e for e in range(n) if e not in (DEAD, BURST)]
  x = got.leaves.state['x'].view(n, 3, M).cpu().numpy()
  differ = 0
  for e in live:
    for a in range(3):
      assert len(set(_bits(x[e, a]).tolist())) == M, (e, a)
      differ += len(set(_bits(ret[e, a]).tolist())) > 1
  print(f'segment {segment}: live groups whose scenario returns differ: {differ} of {3 * len(live)}')
  assert differ > 0
  # the score and the finish: the twin on the device's own returns
  score = sh.risk_scores(ret, M)
  assert np.array_equal(_bits(got.score.cpu().numpy()), _bits(score))
  ok = src.state['status'].cpu().numpy() == 0
  plan, action, best, q, visits = twin.finish(score, [], 1, segment, ok)
  assert np.array_equal(got.best_plan.cpu().numpy(), plan) and np.array_equal(got.action.cpu().numpy(), action)
  assert np.array_equal(_bits(got.best_return.cpu().numpy()), _bits(best))
  assert np.array_equal(_bits(got.q.cpu().numpy()), _bits(q)) and np.array_equal(got.visits.cpu().numpy(), visits)
  assert action[DEAD] == 1 and best[DEAD] == 0.0 and visits[DEAD].tolist() == [1, 0, 0]


VEHICLE = {'payload_mass': 95.0, 'battery_capacity_wh': 2800.0}          # test_gpu_rollout.py's run-time vehicle
VEHICLE_SEED = 526                                # environment 3 flies in the dark, environments 0 and 4 in daylight


@pytest.mark.parametrize('per_env_seeds', [False, True])
def test_one_level_with_a_runtime_vehicle_is_the_rollout_and_a_stepped_copy(per_env_seeds):
  """The VehicleRt instantiations of ble_tree_expand_scenarios_kernel and ble_rollout_scenarios_kernel under a scalar seed and under
  per-environment seeds, 30 lanes: one level of edges of segment 2 x action_repeat 2 against the scenario rollout flown with the same
  vehicle, and every state word of every node against scenario_wind + step on a copy that flies that vehicle."""
  n, M, segment, repeat = 5, 2, 2, 2
  src, _ = tgs._source(n, VEHICLE_SEED, RINGS, vehicle=VEHICLE)
  night = (src.state['solar_charging'] == 0) & (src.state['status'] == 0)
  night[DEAD] = False
  night[BURST] = False
  assert bool(night.any()), 'no environment flies in the dark'
  src.state['battery_charge'][night] = 23.0       # the night load drains it inside the third agent step: inside the edge
  src.state['status'][DEAD] = 1
  src.state['mols_air'][BURST] += 30000.0
  fit = dict(seeds=_dev(np.array([101, 102, 103, 104, 105], np.int64))) if per_env_seeds else dict(seed=33)
  scn = src.fit_wind_scenarios(M, **fit)
  plans = np.ascontiguousarray(np.broadcast_to(np.arange(3, dtype=np.uint8), (segment, n, 3)))
  want = src.rollout_plans(_dev(plans), gamma=GAMMA, action_repeat=repeat, scenarios=scn, want_final=True)
  before = _guard(src, scn)
  got = src.tree_search(1, 1, segment=segment, action_repeat=repeat, gamma=GAMMA, scenarios=scn)
  _assert_guarded(src, scn, before, 'the source')
  ret, want_ret = got.returns.cpu().numpy(), want.returns.cpu().numpy()
  void = np.zeros((n, 3), bool)
  void[DEAD, 1:] = True
  assert np.isnan(ret[void]).all() and not np.isnan(ret[~void]).any()
  assert np.array_equal(_bits(ret[~void]), _bits(want_ret[~void]))
  flown = want.steps_flown.cpu().numpy()
  assert np.array_equal(got.steps_flown.cpu().numpy(), flown)
  assert np.array_equal(_bits(_final(got.leaves, (n, 3, M))), _bits(want.final.cpu().numpy()))       # (a void node is the same copy)
  dark = night.cpu().numpy()
  assert (flown[DEAD] == 0).all() and (flown[BURST] == 1).all()
  assert ((flown[dark] > 0) & (flown[dark] < segment * repeat)).all()
  rest = ~dark
  rest[[DEAD, BURST]] = False
  assert rest.any() and (flown[rest] == segment * repeat).all()
  # every state word of every node, the void ones included: a copy of the source flown in scenario m's wind by the step kernel
  sd = src.state_dict()
  ref = vec_state.VecSimulator(n, DEVICE, env_offset=src.env_offset)
  uv = torch.zeros(n, 2, dtype=torch.float32, device=DEVICE)
  rows = torch.arange(n, device=DEVICE)
  for a in range(3):
    for m in range(M):
      index = torch.full((n,), m, dtype=torch.int32, device=DEVICE)
      ref.load_state_dict(sd)
      for _ in range(segment * repeat):
        ref.scenario_wind(scn, index, out=uv)
        ref.step(torch.full((n,), a, dtype=torch.uint8, device=DEVICE), uv)
      at = (rows * 3 + a) * M + m
      for name, w in ref.state.items():
        _same_words(got.leaves.state[name][at], w, (per_env_seeds, a, m, name))
  # the vehicle is really flown: the default vehicle's nodes are other nodes
  src.set_vehicle()
  default = src.tree_search(1, 1, segment=segment, action_repeat=repeat, gamma=GAMMA, scenarios=scn)
  torch.cuda.synchronize()
  assert not np.array_equal(_bits(default.returns.cpu().numpy()[rest]), _bits(ret[rest]))


# ------------------------------------------------------------------------------------------------ 2: the full node state
def test_every_array_of_every_node_is_a_stepped_copy():
  n, D, segment, B, M = 3, 2, 2, 3, 3
  src, _ = tgs._source(n, 510, (17, 120, 0))
  scn = src.fit_wind_scenarios(M, seed=21)
  got = src.tree_search(D, B, segment=segment, gamma=GAMMA, scenarios=scn)
  torch.cuda.synchronize()
  bf = got.buffers
  choice = bf.choice.cpu().numpy()
  assert sorted(choice[0, 0, :3].tolist()) == [0, 1, 2] and tuple(got.returns.shape) == (n, 9, M)
  assert not np.isnan(got.returns.cpu().numpy()).any()
  level1, level2 = bf.arenas[1], bf.arenas[0]
  sd = src.state_dict()
  ref = vec_state.VecSimulator(n, DEVICE, env_offset=src.env_offset)
  uv = torch.zeros(n, 2, dtype=torch.float32, device=DEVICE)
  rows = torch.arange(n, device=DEVICE)
  checked = 0
  for a1 in range(3):
    for a2 in range(3):
      for m in range(M):
        index = torch.full((n,), m, dtype=torch.int32, device=DEVICE)
        ref.load_state_dict(sd)
        acc, disc = np.zeros(n, np.float64), np.ones(n, np.float64)
        for t in range(D * segment):
          ref.scenario_wind(scn, index, out=uv)
          r, _ = ref.step(torch.full((n,), a1 if t < segment else a2, dtype=torch.uint8, device=DEVICE), uv)
          term = disc * r.cpu().numpy().astype(np.float64)          # the kernel's order: the product and the sum rounded separately
          acc += term
          disc *= GAMMA
          if t + 1 == segment and a2 == 0:                           # level 1: node (e, a1, m)
            at = (rows * 3 + a1) * M + m
            for name, want in ref.state.items():
              _same_words(level1.state[name][at], want, ('level 1', a1, m, name))
            assert np.array_equal(bf.acc[1][at].cpu().numpy().view(np.uint64), acc.view(np.uint64))
            assert np.array_equal(bf.disc[1][at].cpu().numpy().view(np.uint64), disc.view(np.uint64))
        # level 2: the group whose path is (a1, a2) -- child c = 3 r + a2 of the parent of rank r with choice[0][e][r] == a1
        rank = np.array([choice[0, e, :3].tolist().index(a1) for e in range(n)])
        at = (rows * 9 + _dev(3 * rank + a2)) * M + m
        for name, want in ref.state.items():
          _same_words(level2.state[name][at], want, ('level 2', a1, a2, m, name))
        assert np.array_equal(bf.acc[0][at].cpu().numpy().view(np.uint64), acc.view(np.uint64)), (a1, a2, m)
        assert np.array_equal(bf.disc[0][at].cpu().numpy().view(np.uint64), disc.view(np.uint64))
        assert np.array_equal(_bits(bf.ret[0][at].cpu().numpy()), _bits(acc.astype(np.float32)))
        assert (bf.flown[0][at].cpu().numpy() == D * segment).all() and (ref.state['status'].cpu().numpy() == 0).all()
        checked += 1
  assert checked == 27
  src.check_errors()


# ------------------------------------------------------------------------------------------------ 3: the exhaustive tree is the enumeration
def test_the_exhaustive_tree_is_the_enumeration(five):
  src, scn = five
  n, D, segment, B, M = src.n, 3, 2, 9, scn.num
  digits = np.array([[k // 9, (k // 3) % 3, k % 3] for k in range(27)], np.uint8)                 # plan k = 9 a_1 + 3 a_2 + a_3
  plans = np.ascontiguousarray(np.broadcast_to(np.repeat(digits.T, segment, 0)[:, None, :], (D * segment, n, 27)))
  enum = src.rollout_plans(_dev(plans), gamma=GAMMA, scenarios=scn, want_final=True)
  before = _guard(src, scn)
  got = src.tree_search(D, B, segment=segment, gamma=GAMMA, scenarios=scn, risk_tail=2)
  _assert_guarded(src, scn, before, 'the source')
  enum_ret, enum_flown, enum_final = enum.returns.cpu().numpy(), enum.steps_flown.cpu().numpy(), enum.final.cpu().numpy()
  choice = got.buffers.choice.cpu().numpy()
  ret, flown, score = got.returns.cpu().numpy(), got.steps_flown.cpu().numpy(), got.score.cpu().numpy()
  assert ret.shape == (n, 27, M) and score.shape == (n, 27)
  ks = np.array([[int(np.dot(tree_host.path(choice, e, c, D), [9, 3, 1])) for c in range(27)] for e in range(n)])
  void = np.isnan(ret).all(-1)
  assert np.array_equal(np.isnan(ret).any(-1), void)                                              # a group is void in all its nodes or in none
  live = ~void
  pick = ks[..., None]
  assert np.array_equal(_bits(ret[live]), _bits(np.take_along_axis(enum_ret, pick, 1)[live]))
  assert np.array_equal(flown[live], np.take_along_axis(enum_flown, pick, 1)[live])
  final = _final(got.leaves, (n, 27, M))
  assert np.array_equal(_bits(final[:, live]), _bits(np.take_along_axis(enum_final, pick[None], 2)[:, live]))
  enum_score = sh.risk_scores(enum_ret, 2)
  assert np.array_equal(_bits(score[live]), _bits(np.take_along_axis(enum_score, ks, 1)[live])) and np.isnan(score[void]).all()
  for e in range(n):
    assert sorted(set(ks[e].tolist())) == list(range(27))                                         # nothing was cut: every plan has its leaf
  # not on void data: three environments are all live, the dead one keeps its a = 0 chain, the bursting one its three spent chains
  full = [e for e in range(n) if live[e].all()]
  assert full == [0, 3, 4] and all(len(set(_bits(final[0, e, c]).tolist())) == M for e in full for c in (0, 13, 26))      # really flown
  assert live[DEAD].sum() == 1 and ks[DEAD][live[DEAD]].tolist() == [0]
  assert sorted(ks[BURST][live[BURST]].tolist()) == [0, 9, 18] and (flown[BURST][live[BURST]] == 1).all()
  # the best plan is the enumeration's best by the risk score, and flying it earns that score
  best = np.array([enum_score[e, tree_host.order(enum_score[e])[0]] for e in range(n)], np.float32)
  assert np.array_equal(_bits(got.best_return.cpu().numpy()), _bits(best)) and best[DEAD] == 0.0
  assert np.all(got.best_plan.cpu().numpy()[:, DEAD] == 1)
  again = src.rollout_plans(got.best_plan.view(D * segment, n, 1).contiguous(), gamma=GAMMA, scenarios=scn)
  assert np.array_equal(_bits(src.plan_risk(again.returns, 2).cpu().numpy()[:, 0]), _bits(got.best_return.cpu().numpy()))
  assert np.array_equal(got.action.cpu().numpy(), got.best_plan.cpu().numpy()[0])
  print('void groups per environment:', void.sum(1).tolist())


# ------------------------------------------------------------------------------------------------ 4: pruning
@pytest.mark.parametrize('tail', [1, 3, 8])
def test_pruning_equals_the_twin(tail):
  n, D, segment, B, M = 9, 4, 2, 4, 8
  src, _ = tgs._source(n, 520 + tail, (0, 1, 3, 17, 120, 60, 5, 119, 2))
  src.state['status'][DEAD] = 2
  src.state['mols_air'][BURST] += 30000.0
  scn = src.fit_wind_scenarios(M, seed=7)
  trace = []
  got = src.tree_search(D, B, segment=segment, gamma=GAMMA, scenarios=scn, risk_tail=tail, action_values=True, trace=trace)
  torch.cuda.synchronize()
  choice = got.buffers.choice.cpu().numpy()
  sizes = tree_host.level_sizes(D, B)
  assert [c for _, c in sizes] == [3, 9, 12, 12] and len(trace) == D
  lists = []
  for (level, score, parent, ret), (_, C) in zip(trace, sizes):
    assert tuple(score.shape) == (n, C) and tuple(ret.shape) == (n, C, M)
    want_score, want = twin.level(ret.cpu().numpy(), tail, B)
    assert np.array_equal(_bits(score.cpu().numpy()), _bits(want_score)), level
    keep = want.shape[1]
    assert np.array_equal(parent.cpu().numpy()[:, :keep], want), level
    assert np.array_equal(choice[level - 1][:, :keep], want), level
    lists.append(want)
  score = got.score.cpu().numpy()
  assert np.array_equal(_bits(score), _bits(trace[-1][1].cpu().numpy()))
  assert np.array_equal(_bits(got.returns.cpu().numpy()), _bits(trace[-1][3].cpu().numpy()))
  ok = src.state['status'].cpu().numpy() == 0
  plan, action, best, q, visits = twin.finish(score, lists, D, segment, ok)
  assert np.array_equal(got.best_plan.cpu().numpy(), plan) and np.array_equal(got.action.cpu().numpy(), action)
  assert np.array_equal(_bits(got.best_return.cpu().numpy()), _bits(best))
  assert np.array_equal(_bits(got.q.cpu().numpy()), _bits(q)) and np.array_equal(got.visits.cpu().numpy(), visits)
  assert np.isfinite(best).all() and best[DEAD] == 0.0 and np.all(plan[:, DEAD] == 1)
  assert np.array_equal(visits.sum(1), (~np.isnan(score)).sum(1)) and np.isnan(score[BURST]).any() and not np.isnan(score[0]).any()
  again = src.rollout_plans(got.best_plan.view(D * segment, n, 1).contiguous(), gamma=GAMMA, scenarios=scn)
  assert np.array_equal(_bits(src.plan_risk(again.returns, tail).cpu().numpy()[:, 0]), _bits(best))
  print(f'tail {tail}: actions', np.bincount(action, minlength=3), 'void groups at the last level', int(np.isnan(score).sum()))


# ------------------------------------------------------------------------------------------------ 5: stopped inside a live group
def _arena_words(bf, p):
  """Every array of arena p as clones: the state's and acc, disc, flown, ret."""
  out = {name: t.clone() for name, t in bf.arenas[p].state.items()}
  out.update(acc=bf.acc[p].clone(), disc=bf.disc[p].clone(), flown=bf.flown[p].clone(), ret=bf.ret[p].clone())
  return out


def test_stopped_nodes_inside_live_and_spent_groups(five):
  src, scn = five
  n, D, segment, B, M = src.n, 2, 2, 3, scn.num
  got = src.tree_search(D, B, segment=segment, gamma=GAMMA, scenarios=scn)
  torch.cuda.synchronize()
  bf = got.buffers
  plain = _arena_words(bf, 0)                        # the unedited level 2
  parent = bf.choice[0].clone()                      # level 1's selection [n, B]: with C_1 = B = 3 a permutation of its three groups
  ranks = parent.cpu().numpy()
  # the edits of level 1 (arena 1, node (e, c, m) at (3 e + c) M + m): a node of a live group stops; a whole group stops; an acc is NaN
  one, group, nan = (0 * 3 + 0) * M + 1, (0 * 3 + 1) * M, (3 * 3 + 2) * M + 0
  bf.arenas[1].state['status'][one] = 2
  bf.arenas[1].state['status'][group:group + M] = 2
  bf.acc[1][nan] = float('nan')
  torch.cuda.synchronize()
  level1 = _arena_words(bf, 1)
  ex = _abi.BleTreeExpand(n, B, D, 3, 3, segment, 1, vec_state.SUBSTEPS, 0, GAMMA, src.grid.data_ptr(), src.grid_env_stride, parent.data_ptr(),
                          bf.node_struct(1), bf.node_struct(2))
  b, gen = src._scenario_structs(scn)
  src.rollout_flags.zero_()
  with torch.cuda.device(src.device):
    _lib.check(_lib.lib().ble_tree_expand_scenarios_f32(ctypes.byref(src._struct), ctypes.byref(ex), ctypes.byref(b), ctypes.byref(gen),
                                                        src.rollout_flags.data_ptr(), dev.stream_ptr(src.device)), 'ble_tree_expand_scenarios_f32')
  torch.cuda.synchronize()
  edited = {k: v.cpu().numpy() for k, v in _arena_words(bf, 0).items()}
  plain = {k: v.cpu().numpy() for k, v in plain.items()}
  level1 = {k: v.cpu().numpy() for k, v in level1.items()}
  seen = dict(carried=0, void=0, untouched=0)
  for e in range(n):
    for r in range(3):
      c1 = int(ranks[e, r])
      for a in range(3):
        for m in range(M):
          src_at, at = (3 * e + c1) * M + m, (9 * e + 3 * r + a) * M + m
          is_one, in_group, is_nan = src_at == one, group <= src_at < group + M, src_at == nan
          for name in edited:
            here = edited[name][at:at + 1].view(np.uint8)
            if is_one or is_nan or in_group:
              want = level1[name][src_at:src_at + 1]
              if name in ('acc', 'ret') and ((in_group and a != 0) or is_nan):           # void, or the NaN carried on
                assert np.isnan(edited[name][at]), (name, e, c1, a, m)
                continue
              if name == 'ret':
                want = level1['acc'][src_at:src_at + 1].astype(np.float32)
              assert np.array_equal(here, want.view(np.uint8)), ('carried', name, e, c1, a, m)
            else:
              assert np.array_equal(here, plain[name][at:at + 1].view(np.uint8)), ('untouched', name, e, c1, a, m)
          seen['void' if (in_group and a != 0) else 'carried' if (is_one or is_nan or in_group) else 'untouched'] += 1
  assert seen == dict(carried=3 + 3 + M, void=2 * M, untouched=n * 9 * M - 6 - 3 * M), seen
  # the stopped node of the live group keeps a finite acc: its groups still score
  assert np.isfinite(edited['acc'][[(9 * 0 + 3 * int(np.nonzero(ranks[0] == 0)[0][0]) + a) * M + 1 for a in range(3)]]).all()


# ------------------------------------------------------------------------------------------------ 6: housekeeping
def test_flags_go_to_their_own_word_and_nothing_is_written():
  src, _ = _five(530)
  src.wind_noise(7)                                  # (allocates the harmonic cache: it must stay as it is)
  scn = src.fit_wind_scenarios(3, seed=4)
  src.rollout_flags.zero_()
  before = _guard(src, scn)
  flags = int(src.err_flags.item())
  src.tree_search(3, 4, segment=2, gamma=GAMMA, scenarios=scn, action_values=True)
  _assert_guarded(src, scn, before, 'a search')
  assert int(src.err_flags.item()) == flags
  # an upwelling IR outside total_absorptivity's range: the flag of the imagined flights, not the real one's
  src.rollout_flags.zero_()
  src.state['upwelling_infrared'][3] = 1e-3
  src.tree_search(2, 4, segment=1, gamma=GAMMA, scenarios=scn)
  torch.cuda.synchronize()
  assert int(src.rollout_flags.item()) & _lib.FLAG_ABSORPTIVITY and int(src.err_flags.item()) == flags
  src.check_errors()                                 # a flight that never happened raises nothing


@pytest.mark.parametrize('per_env_seeds', [False, True])
def test_batch_invariance(per_env_seeds):
  D, B, segment, M = 3, 4, 2, 3
  src, _ = tgs._source(5, 540, (17, 3, 120, 1, 0), env_offset=3)
  src.episode[2] += 2
  seeds = np.array([101, 102, 103, 104, 105], np.int64)

  def search(sim, which):
    fit = dict(seeds=_dev(seeds[which])) if per_env_seeds else dict(seed=9)
    scn = sim.fit_wind_scenarios(M, **fit)
    out = sim.tree_search(D, B, segment=segment, gamma=GAMMA, scenarios=scn, risk_tail=2, action_values=True)
    torch.cuda.synchronize()
    return out

  batch = search(src, slice(None))
  for e in (0, 2, 4):
    alone = search(tgs._clone_env(src, e), slice(e, e + 1))
    for name in ('action', 'best_plan', 'best_return', 'q', 'visits', 'returns', 'steps_flown', 'score'):
      a, b = getattr(alone, name), getattr(batch, name)
      b = b[:, e:e + 1] if name == 'best_plan' else b[e:e + 1]
      _same_words(a, b, (per_env_seeds, e, name))
    assert np.array_equal(alone.buffers.choice.cpu().numpy()[:, 0], batch.buffers.choice.cpu().numpy()[:, e])
  if per_env_seeds:                                  # its own seed decides: the same plan at another position
    moved = search(tgs._clone_env(src, 2, offset=0), slice(2, 3))
    _same_words(moved.returns, batch.returns[2:3], 'moved')


def test_graph_replay_equals_eager_and_one_scenario_scores_its_return():
  src, _ = _five(550)
  D, B, segment = 3, 4, 2
  scn = src.fit_wind_scenarios(3, seed=2)
  buffers = src.tree_buffers(D, B, segment, action_values=True, num_scenarios=3)

  def body():
    src.fit_wind_scenarios(3, seed=2, out=scn)
    src.tree_search(D, B, segment=segment, gamma=GAMMA, scenarios=scn, risk_tail=2, action_values=True, buffers=buffers)
  body()
  torch.cuda.synchronize()
  names = ('action', 'best_plan', 'best_return', 'q', 'visits', 'score', 'choice')
  eager = {k: getattr(buffers, k).clone() for k in names}
  eager_ret = buffers.ret[D & 1].clone()
  graph = dev.capture(src.device, body)[0]
  for k in names[:-1]:                               # (choice keeps its never-written slots beyond min(C, B))
    getattr(buffers, k).fill_(7)
  graph.replay()
  torch.cuda.synchronize()
  for k in names:
    _same_words(getattr(buffers, k), eager[k], k)
  _same_words(buffers.ret[D & 1], eager_ret, 'returns')
  # M = 1, tail = 1: the score is the return, as floats
  one = src.fit_wind_scenarios(1, seed=2)
  got = src.tree_search(D, B, segment=segment, gamma=GAMMA, scenarios=one)
  torch.cuda.synchronize()
  ret, score = got.returns.cpu().numpy()[..., 0], got.score.cpu().numpy()
  assert np.array_equal(np.isnan(ret), np.isnan(score)) and np.array_equal(ret[~np.isnan(ret)], score[~np.isnan(ret)])
  with pytest.raises(ValueError, match='buffers'):
    src.tree_search(D, B, segment=segment, scenarios=one, buffers=buffers)                          # buffers of another M


# ------------------------------------------------------------------------------------------------ 7: the agent
KW = dict(beam_width=4, depth=3, segment=2, num_scenarios=3, risk_tail=2, seed=5)


def test_act_is_the_public_composition():
  n = 9
  env = tgs._env(n)
  sim = env.arena.sim
  sim.state['status'][2] = 2                         # one environment is not OK: it gets STAY
  agent = env.planner(search='beam', wind='scenarios', action_values=True, **KW)
  assert type(agent) is beam_agent.VecScenarioBeamSearchAgent and agent.get_name() == 'ScenarioBeamSearchAgent'
  rng = np.random.default_rng(1)
  for decision in range(2):
    action = agent.act(None).clone()
    plan, best = (t.clone() for t in agent.plan())
    q, visits = (t.clone() for t in agent.action_values())
    scn = sim.fit_wind_scenarios(3, seed=5)
    want = sim.tree_search(3, 4, segment=2, gamma=agent.gamma, scenarios=scn, risk_tail=2, action_values=True)
    for a, b, name in ((action, want.action, 'action'), (plan, want.best_plan, 'best_plan'), (best, want.best_return, 'best_return'),
                       (q, want.q, 'q'), (visits, want.visits, 'visits')):
      _same_words(a, b, (decision, name))
    assert int(action[2].item()) == 1 and bool(torch.isfinite(best).all())
    env.step(_dev(np.where(rng.random(n) < 0.5, action.cpu().numpy(), 1).astype(np.uint8)))
  env.check_errors()
  # the environment's own pass-through is the same search (its scenario streams are keyed by the env's seed)
  scn = sim.fit_wind_scenarios(3, seed=env.arena._seed)
  want = sim.tree_search(3, 4, segment=2, scenarios=scn, risk_tail=1)
  best = want.best_return.clone()
  tree = env.tree_search(3, 4, segment=2, wind='scenarios', num_scenarios=3, risk_tail=1)
  _same_words(tree.best_return, best, 'env.tree_search')
  assert tuple(tree.returns.shape) == (n, 12, 3) and tuple(tree.score.shape) == (n, 12)


def test_graph_equals_eager_and_resume():
  n, decisions = 9, 3
  runs = {}
  for mode in ('eager', 'graph', 'resume'):
    env = tgs._env(n, seed=9)
    agent = env.planner(search='beam', wind='scenarios', **KW)
    actions = torch.ones(n, dtype=torch.uint8, device=DEVICE)
    obs = torch.empty(n, 1099, dtype=torch.float32, device=DEVICE)

    def body():
      agent.act(None, out=actions)
      env._step_eager(actions, obs_out=obs)
    body()                                               # (lazy allocations happen here, in every mode)
    graph = dev.capture(env.device, body)[0] if mode == 'graph' else None
    log = []
    for d in range(decisions):
      if mode == 'resume' and d == 1:                    # a new agent picks the run up from the old one's state_dict
        saved = agent.state_dict()
        agent = env.planner(search='beam', wind='scenarios', **KW)
        agent.load_state_dict(saved)
      graph.replay() if graph is not None else body()
      torch.cuda.synchronize()
      log.append((actions.cpu().numpy().copy(), _bits(agent.best_return.cpu().numpy()).copy(), obs.cpu().numpy().copy()))
    runs[mode] = log
    env.check_errors()
  for mode in ('graph', 'resume'):
    for d, (a, b) in enumerate(zip(runs['eager'], runs[mode])):
      assert all(np.array_equal(x, y) for x, y in zip(a, b)), (mode, d)
  other = env.planner(search='beam', wind='scenarios', **dict(KW, seed=6))
  with pytest.raises(ValueError, match='checkpoint'):
    other.load_state_dict(saved)


def test_evaluation_is_finite_and_batch_invariant():
  suite = suites.EvaluationSuite([11, 12, 13], 8)
  make = lambda: beam_agent.VecScenarioBeamSearchAgent(beam_width=4, depth=2, segment=2, num_scenarios=3, risk_tail=2)
  alone = eval_lib.eval_agent_vec(make(), suite, batch_size=1)
  batch = eval_lib.eval_agent_vec(make(), suite, batch_size=3)
  for a, b in zip(alone, batch):
    assert dataclasses.asdict(a) == dataclasses.asdict(b), (a, b)
    assert np.isfinite(a.cumulative_reward) and np.isfinite(a.time_within_radius)
  assert [r.seed for r in batch] == [11, 12, 13]


def test_refusals():
  with pytest.raises(ValueError, match='num_scenarios'):
    beam_agent.VecScenarioBeamSearchAgent(num_scenarios=17)
  with pytest.raises(ValueError, match='risk_tail'):
    beam_agent.VecScenarioBeamSearchAgent(num_scenarios=4, risk_tail=5)
  with pytest.raises(ValueError, match='leaf_value'):
    beam_agent.VecScenarioBeamSearchAgent(leaf_value=object())
  with pytest.raises(ValueError, match='bind'):
    beam_agent.VecScenarioBeamSearchAgent().act(None)
  env = tgs._env(3, steps=0)
  sim = env.arena.sim
  scn = sim.fit_wind_scenarios(2)
  with pytest.raises(ValueError, match='three winds'):
    sim.tree_search(2, 4, scenarios=scn, noise_seed=1)
  with pytest.raises(ValueError, match='three winds'):
    sim.tree_search(2, 4, scenarios=scn, belief=sim.fit_wind_belief())
  with pytest.raises(ValueError, match='leaf_score'):
    sim.tree_search(2, 4, scenarios=scn, leaf_score=lambda *a: None)
  with pytest.raises(ValueError, match='risk_tail'):
    sim.tree_search(2, 4, scenarios=scn, risk_tail=3)
  with pytest.raises(ValueError, match='risk_tail'):
    sim.tree_search(2, 4, risk_tail=1)
  with pytest.raises(ValueError, match='buffers'):
    sim.tree_search(2, 4, scenarios=scn, buffers=sim.tree_buffers(2, 4))
  with pytest.raises(ValueError, match='buffers'):
    sim.tree_search(2, 4, buffers=sim.tree_buffers(2, 4, num_scenarios=2))
  with pytest.raises(ValueError, match='num_scenarios'):
    sim.tree_buffers(2, 4, num_scenarios=17)
  with pytest.raises(ValueError, match='wind'):
    env.tree_search(2, 4, wind='gp')
  fleet = balloon_env.VecBalloonEnv(3, seed=1, vehicles=[{}, {'envelope_mass': 75.0}], vehicle_index=[0, 1, 0], auto_reset=False)
  with pytest.raises(ValueError, match='fleet'):
    fleet.planner(search='beam', wind='scenarios')
  with pytest.raises(ValueError, match='fleet'):
    fleet.arena.sim.tree_search(2, 4, scenarios=scn)
  with pytest.raises(ValueError, match='fleet'):
    fleet.arena.sim.tree_buffers(2, 4, num_scenarios=2)
