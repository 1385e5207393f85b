"""Population-based training without a GPU: train_lib.pbt_decide on CPU tensors against the NumPy twin of tests/pbt_host.py
(ties in member order, members without episodes last, truncation 0 / 0.25 / 0.5, P in {1, 2, 8}, the same generator seed the same
decision), and run_pbt_loop_vec on recording fakes: the round schedule, which members are copied from which, the lineage and the stats."""
import math

import numpy as np
import pytest
import torch

import pbt_host
from balloon_learning_environment_amd import train_lib

NAN = float('nan')
FITNESS = {
    1: [[3.0], [NAN]],
    2: [[1.0, 2.0], [2.0, 2.0], [NAN, -5.0], [NAN, NAN]],
    8: [[1.0, 7.0, 3.0, 3.0, 0.0, 5.0, 2.0, 6.0], [2.0] * 8, [1.0, NAN, 3.0, 3.0, NAN, 3.0, 1.0, 1.0], [NAN] * 8,
        [-1.0, -1.0, NAN, 4.0, 4.0, 4.0, -1.0, float('-inf')], [float('inf'), 0.0, 0.0, NAN, 0.0, 0.0, 0.0, 0.0]],
}
CASES = [(p, i, tr) for p in FITNESS for i in range(len(FITNESS[p])) for tr in (0.0, 0.25, 0.5)]


def _draws(seed, k, explored):
  """The draws pbt_decide consumes from a generator of this seed, in its order."""
  g = torch.Generator().manual_seed(seed)
  return torch.randint(0, k, (k,), generator=g).numpy(), torch.randint(0, 2, (k, explored), generator=g).numpy()


@pytest.mark.parametrize('p,i,truncation', CASES)
def test_decide_against_twin(p, i, truncation):
  fitness = FITNESS[p][i]
  k = min(int(math.floor(truncation * p + 1e-9)), p // 2)
  for seed in (0, 1, 2):
    src, dst, fi = train_lib.pbt_decide(torch.tensor(fitness, dtype=torch.float32), truncation, torch.Generator().manual_seed(seed), 2)
    assert src.dtype == dst.dtype == fi.dtype == torch.int64 and src.shape == dst.shape == (k,) and fi.shape == (k, 2)
    if k == 0:
      continue
    want = pbt_host.pbt_decide(fitness, truncation, *_draws(seed, k, 2))
    for got, w in zip((src, dst, fi), want):
      assert np.array_equal(got.numpy(), w), (fitness, truncation, seed, got, w)
    assert len(set(dst.tolist())) == k and not set(dst.tolist()) & set(src.tolist())


def test_decide_spelt_out():
  g = torch.Generator().manual_seed(0)
  # ties: members 2, 3 and 5 share the best fitness -> the top quarter of 8 is (2, 3); members 1 and 4 have no episode -> the bottom
  src, dst, _ = train_lib.pbt_decide(torch.tensor([1.0, NAN, 3.0, 3.0, NAN, 3.0, 1.0, 1.0]), 0.25, g)
  assert dst.tolist() == [1, 4] and set(src.tolist()) <= {2, 3}
  # all equal: the order is the member order -> bottom half (4 .. 7) copies from the top half (0 .. 3)
  src, dst, _ = train_lib.pbt_decide(torch.full((8,), 2.0), 0.5, g)
  assert dst.tolist() == [4, 5, 6, 7] and set(src.tolist()) <= {0, 1, 2, 3}
  # truncation 0 and a population of one decide nothing and draw nothing
  before = g.get_state().clone()
  for f, tr in ((torch.arange(8.0), 0.0), (torch.tensor([1.0]), 0.5)):
    src, dst, fi = train_lib.pbt_decide(f, tr, g)
    assert src.numel() == dst.numel() == fi.numel() == 0
  assert torch.equal(g.get_state(), before)
  a = train_lib.pbt_decide(torch.arange(8.0), 0.5, torch.Generator().manual_seed(7), 3)
  b = train_lib.pbt_decide(torch.arange(8.0), 0.5, torch.Generator().manual_seed(7), 3)
  assert all(torch.equal(x, y) for x, y in zip(a, b))
  with pytest.raises(AssertionError):
    train_lib.pbt_decide(torch.arange(8.0), 0.75, g)


# ---- the loop on fakes -----------------------------------------------------------------------------------------------------------------
P, R, T = pbt_host.P, pbt_host.R, pbt_host.T


def _run(iterations=5, **kw):
  log = pbt_host.Log()
  env, tr, ro = pbt_host.FakePopEnv(log), pbt_host.FakePopTrainer(log), pbt_host.FakePopRollout(log)
  args = dict(num_iterations=iterations, epochs=2, batch_size=2, ready_every=2, truncation=0.25, perturb=(0.5, 2.0), seed=3,
              max_episode_length=pbt_host.LIMIT)
  args.update(kw)
  return log, tr, train_lib.run_pbt_loop_vec(env, tr, ro, **args)


def test_loop_rounds_copies_lineage_and_stats():
  log, tr, stats = _run()
  assert len(stats) == 5
  # the iteration: T acts and steps, the bootstrap act, finish, epochs passes of T R / B grouped updates (the first one captured)
  assert [e[0] for e in log.named('act')] == list(range(5 * (T + 1))) and len(log.named('step')) == 5 * T
  assert len(log.named('finish')) == 5 and [e[:2] for e in log.named('pass')] == [(k, 2) for k in range(10)]
  updates = log.named('update')
  assert [u[0] for u in updates] == ['capture'] + ['train_step'] * 19 and [u[1] for u in updates[:4]] == [(0, 0), (0, 1), (1, 0), (1, 1)]
  for e in log.named('step'):                                       # every environment's episode ends on its LIMIT-th step
    assert e[2].tolist() == [1 if e[0] % 2 else 0] * (P * R)
  # the rounds: after iterations 2 and 4, on the fitness of the two iterations since the last one
  g = torch.Generator().manual_seed(3)
  f1 = (torch.randint(0, 1, (1,), generator=g), torch.randint(0, 2, (1, 2), generator=g))[1][0].tolist()
  f2 = (torch.randint(0, 1, (1,), generator=g), torch.randint(0, 2, (1, 2), generator=g))[1][0].tolist()
  factor = lambda i: [0.5, 2.0][i]
  assert log.named('copy') == [([3], [0]), ([0], [2])]
  assert log.named('scale') == [('lr', [0], [factor(f1[0])]), ('entropy_coef', [0], [factor(f1[1])]),
                                ('lr', [2], [factor(f2[0])]), ('entropy_coef', [2], [factor(f2[1])])]
  assert [s['round'] is not None for s in stats] == [False, True, False, True, False]
  assert stats[1]['round'] == {'fitness': [0.0, 2.0, 4.0, 6.0], 'src': [3], 'dst': [0]}
  assert stats[3]['round'] == {'fitness': [10.0, 2.0, 0.0, 4.0], 'src': [0], 'dst': [2]}
  # the lineage: member 0 became member 3's copy, then member 2 became a copy of that copy
  assert [s['lineage'] for s in stats] == [[0, 1, 2, 3], [3, 1, 2, 3], [3, 1, 2, 3], [3, 1, 3, 3], [3, 1, 3, 3]]
  lr0 = 8.0 * factor(f1[0])
  assert stats[1]['lr'] == [lr0, 2.0, 4.0, 8.0] and stats[4]['lr'] == [lr0, 2.0, lr0 * factor(f2[0]), 8.0]
  assert tr.entropy_coef.tolist() == [0.0625 * factor(f1[1]), 0.25, 0.0625 * factor(f1[1]) * factor(f2[1]), 0.0625]
  # the stats dicts: run_ppo_loop_vec's, and the members' own
  for i, s in enumerate(stats):
    assert s['updates'] == 4 and s['episodes'] == P * R and s['transitions'] == (i + 1) * T * P * R
    assert s['member_episodes'] == [R] * P and s['member_mean_return'] == [2.0 * r for r in pbt_host.REWARD[i]]
    assert s['mean_return'] == pytest.approx(np.mean(s['member_mean_return']))
  assert stats[0]['mean_loss'] == pytest.approx((1.0 + 3 * 3.0) / 4) and stats[1]['mean_loss'] == 3.0
  assert log.named('env_check') and len(log.named('trainer_check')) == 5


def test_loop_without_truncation_is_a_seed_study():
  log, tr, stats = _run(truncation=0.0)
  assert not log.named('copy') and not log.named('scale')
  assert all(s['lineage'] == [0, 1, 2, 3] and s['lr'] == [1.0, 2.0, 4.0, 8.0] for s in stats)
  assert stats[1]['round'] == {'fitness': [0.0, 2.0, 4.0, 6.0], 'src': [], 'dst': []}


def test_controller_resumes_the_schedule():
  """Three iterations, a checkpoint of the controller, two more: the rounds, copies and lineage of five straight iterations."""
  _, _, straight = _run()
  log = pbt_host.Log()
  env, tr, ro = pbt_host.FakePopEnv(log), pbt_host.FakePopTrainer(log), pbt_host.FakePopRollout(log)
  make = lambda: train_lib.PBTController(P, 'cpu', ready_every=2, truncation=0.25, perturb=(0.5, 2.0), seed=3)
  c = make()
  kw = dict(epochs=2, batch_size=2, ready_every=99, max_episode_length=pbt_host.LIMIT)
  first = train_lib.run_pbt_loop_vec(env, tr, ro, num_iterations=3, controller=c, **kw)
  d = make()
  d.load_state_dict(c.state_dict())
  second = train_lib.run_pbt_loop_vec(env, tr, ro, num_iterations=2, controller=d, **kw)
  for a, b in zip(straight, first + second):
    assert a['lineage'] == b['lineage'] and a['round'] == b['round'] and a['lr'] == b['lr']
