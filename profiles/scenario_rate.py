"""The scenario winds' rates at the same total lane count as the belief look-ahead:

    (a) fit       fit_wind_scenarios(M) against fit_wind_belief, M = 8 and 16, at 4 096 environments (full windows of 120)
    (b) rollout   rollout_plans(scenarios=) at (N, K, M) = (4 096, 8, 8) against rollout_plans(belief=), rollout_plans(noise_seed=) and
                  rollout_plans() at (N, K) = (4 096, 64): 262 144 lanes each, 20 agent steps of 18 substeps per lane, a shared grid
    (c) risk      plan_risk over the scenario returns of (b)

Rings, timing and the report are profiles/belief_rate.py's: every launch timed with HIP events, the median of --reps after --warmup,
one JSON line per leg:

    python profiles/scenario_rate.py [--reps 21] [--warmup 5] [--out profiles/scenario_rate.jsonl]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balloon_learning_environment_amd import vec_state  # noqa: E402
from belief_rate import NOISE_SEED, STEPS, SUBSTEPS, median_of, source  # noqa: E402

N, K, M = 4096, 8, 8
FIT_SCENARIOS = (8, 16)
SCENARIO_SEED = 11


def run_fit(reps, warmup):
  sim, _ = source(N)
  belief = sim.fit_wind_belief()
  fit = median_of(lambda: sim.fit_wind_belief(out=belief), reps, warmup)
  rows = [{'n': N, 'leg': 'fit_belief', 'reps': reps, **fit}]
  for m in FIT_SCENARIOS:
    scn = sim.fit_wind_scenarios(m, seed=SCENARIO_SEED)
    t = median_of(lambda: sim.fit_wind_scenarios(m, seed=SCENARIO_SEED, out=scn), reps, warmup)
    assert bool((scn.n_obs == 120).all()) and bool(torch.isfinite(scn.slab).all())
    rows.append({'n': N, 'm': m, 'leg': 'fit_scenarios', 'reps': reps, **t, 'vs_fit_belief': t['median_s'] / fit['median_s']})
  sim.check_errors()
  return rows


def run_rollout(reps, warmup):
  sim, gen = source(N)
  belief = sim.fit_wind_belief()
  scn = sim.fit_wind_scenarios(M, seed=SCENARIO_SEED)
  wide = torch.randint(0, 3, (STEPS, N, K * M), dtype=torch.uint8, device='cuda', generator=gen)
  narrow = wide[:, :, :K].contiguous()
  out = vec_state.Rollout(torch.empty(N, K * M, device='cuda'), torch.empty(N, K * M, dtype=torch.int32, device='cuda'), None, None)
  out_s = vec_state.Rollout(torch.empty(N, K, M, device='cuda'), torch.empty(N, K, M, dtype=torch.int32, device='cuda'), None, None)
  legs = {'forecast': (wide, out, {}), 'noise': (wide, out, {'noise_seed': NOISE_SEED}), 'belief': (wide, out, {'belief': belief}),
          'scenarios': (narrow, out_s, {'scenarios': scn})}
  t = {name: median_of(lambda p=p, o=o, kw=kw: sim.rollout_plans(p, gamma=0.993, substeps=SUBSTEPS, out=o, **kw), reps, warmup)
       for name, (p, o, kw) in legs.items()}
  score = torch.empty(N, K, device='cuda')
  risk = median_of(lambda: sim.plan_risk(out_s.returns, 2, out=score), reps, warmup)
  sim.check_errors()
  assert int(sim.rollout_flags.item()) == 0 and bool(torch.isfinite(out_s.returns).all()) and bool(torch.isfinite(score).all())
  lane_steps = N * K * M * STEPS
  rows = [{'n': N, 'k': K * M if name != 'scenarios' else K, 'm': M if name == 'scenarios' else 1, 'leg': f'rollout_{name}',
           'agent_steps': STEPS, 'substeps': SUBSTEPS, 'reps': reps, **t[name], 'lane_steps_per_s': lane_steps / t[name]['median_s'],
           'vs_belief': t[name]['median_s'] / t['belief']['median_s'], 'vs_noise': t[name]['median_s'] / t['noise']['median_s']}
          for name in legs]
  rows.append({'n': N, 'k': K, 'm': M, 'tail': 2, 'leg': 'plan_risk', 'reps': reps, **risk})
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=21)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  lines = []
  for r in run_fit(args.reps, args.warmup) + run_rollout(args.reps, args.warmup):
    lines.append(json.dumps(r))
    print(lines[-1], flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
