"""The planner's rate: one full decision of VecLookaheadAgent next to the parts it is made of.

Every environment holds a full window of 120 observations (profiles/belief_rate.py::source).  Per shape (N, K, H) = (4 096, 64, 24) and
(65 536, 4, 24), wind 'belief' and 'forecast', 1 and 2 iterations:

    decision   agent.act(): [fit] + iterations x (ble_plan_sample_u8 -> rollout_plans -> ble_plan_select_f32)
    rollout    the same decision's rollout_plans call alone, on the plans the decision left
    fit        (belief) fit_wind_belief alone
    outside    the share of a decision spent outside the rollouts and the fit: 1 - (iterations x rollout + fit) / decision

Each leg is timed with HIP events; the median of --reps after --warmup is reported.  One JSON line per leg:

    python profiles/planner_rate.py [--reps 21] [--warmup 5] [--out profiles/planner_rate.jsonl]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from belief_rate import median_of, source  # noqa: E402
from balloon_learning_environment_amd.agents import lookahead_agent  # noqa: E402

SHAPES = ((4096, 64, 24), (65536, 4, 24))


def run(n, k, h, reps, warmup):
  sim, _ = source(n)
  rows = []
  for wind in ('belief', 'forecast'):
    for iterations in (1, 2):
      agent = lookahead_agent.VecLookaheadAgent(num_plans=k, horizon=h, wind=wind, iterations=iterations).bind(sim)
      decision = median_of(lambda: agent.act(None), reps, warmup)
      belief = agent._belief
      out = (agent.returns, agent.steps_flown, None, None)
      rollout = median_of(lambda: sim.rollout_plans(agent.plans, agent.gamma, agent.action_repeat, None, agent.substeps, out=out, belief=belief),
                          reps, warmup)
      fit = median_of(lambda: sim.fit_wind_belief(out=belief), reps, warmup) if wind == 'belief' else None
      sim.check_errors()
      assert bool(torch.isfinite(agent.best_return).all()) and int(agent.counter.item()) == reps + warmup
      inside = iterations * rollout['median_s'] + (fit['median_s'] if fit else 0.0)
      common = {'n': n, 'k': k, 'h': h, 'wind': wind, 'iterations': iterations, 'reps': reps}
      rows.append({**common, 'leg': 'decision', **decision, 'decisions_per_s': n / decision['median_s'],
                   'outside_rollout_and_fit': 1.0 - inside / decision['median_s']})
      rows.append({**common, 'leg': 'rollout', **rollout})
      if fit:
        rows.append({**common, 'leg': 'fit', **fit})
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=21)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  lines = []
  for n, k, h in SHAPES:
    for r in run(n, k, h, args.reps, args.warmup):
      lines.append(json.dumps(r))
      print(lines[-1], flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
