"""Rates and scores of the beam search in scenario winds, beside the planners it stands next to, in one process:

 * one decision of VecScenarioBeamSearchAgent at N = 4 096, M = 8 scenarios, with (beam_width, depth, segment) = (27, 6, 4) and
   (243, 6, 4) -- the last cuts nothing: the full tree, 4 368 flown steps per environment and scenario --; the scenario fit alone;
 * the same decision beside VecLookaheadAgent(wind='scenarios', num_scenarios=8) at num_plans = 64 and at num_plans = 729, the
   enumeration the full tree replaces (729 x 24 = 17 496 flown steps per environment and scenario);
 * small_eval, one run each, of the scenario beam (risk_tail None and 2), the belief beam and the scenario sampler: NOT a gate.

beam_rate.py's method: device events around every single call, the median of 21 calls after 5 warm-up calls (microseconds); the
evaluations by the host clock around the whole call.  One JSON line per measurement.

  python profiles/beam_scenarios_rate.py [--quick] [--skip-scores] > profiles/beam_scenarios_rate.jsonl
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from beam_rate import GAMMA, _env, _score, timed  # noqa: E402
from balloon_learning_environment_amd import vec_state  # noqa: E402
from balloon_learning_environment_amd.agents import beam_agent, lookahead_agent  # noqa: E402


def decision_rates(n, num, shapes, samplers, steps):
  env, obs = _env(n, steps)
  sim = env.arena.sim
  scn = sim.fit_wind_scenarios(num, seed=0)
  rows = [{'what': 'fit_wind_scenarios alone', 'num_envs': n, 'num_scenarios': num, **timed(lambda: sim.fit_wind_scenarios(num, seed=0, out=scn))}]
  for beam, depth, segment in shapes:
    agent = env.planner(search='beam', wind='scenarios', beam_width=beam, depth=depth, segment=segment, gamma=GAMMA, num_scenarios=num)
    sizes = vec_state.tree_level_sizes(depth, beam)
    flown = sum(c for _, c in sizes) * segment
    row = {'what': 'VecScenarioBeamSearchAgent.act', 'num_envs': n, 'beam_width': beam, 'depth': depth, 'segment': segment,
           'num_scenarios': num, 'flown_steps_per_env_and_scenario': flown, 'children_per_level': [c for _, c in sizes],
           **timed(lambda: agent.act(obs))}
    row['ns_per_flown_step'] = row['median_us'] * 1e3 / (n * flown * num)          # (the whole decision: the fit, risk, select and finish included)
    rows.append(row)
    del agent
  for k, h in samplers:
    agent = env.planner(num_plans=k, horizon=h, segment=4, gamma=GAMMA, wind='scenarios', num_scenarios=num)
    row = {'what': 'VecLookaheadAgent.act', 'num_envs': n, 'num_plans': k, 'horizon': h, 'segment': 4, 'wind': 'scenarios',
           'num_scenarios': num, 'flown_steps_per_env_and_scenario': k * h, **timed(lambda: agent.act(obs))}
    row['ns_per_flown_step'] = row['median_us'] * 1e3 / (n * k * h * num)
    rows.append(row)
    del agent
  env.check_errors()
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='small shapes')
  ap.add_argument('--skip-scores', action='store_true', help='the rates only')
  args = ap.parse_args()
  if args.quick:
    rows = decision_rates(256, 3, ((4, 3, 2),), ((16, 6),), 8)
  else:
    rows = decision_rates(4096, 8, ((27, 6, 4), (243, 6, 4)), ((64, 24), (729, 24)), 60)
  for row in rows:
    print(json.dumps(row), flush=True)
  if not args.skip_scores:
    shape = dict(beam_width=27, depth=6, segment=4)
    sample = dict(num_plans=64, horizon=24, segment=4, wind='scenarios', num_scenarios=8)
    for what, planner, make in (
        ('small_eval, VecScenarioBeamSearchAgent', dict(shape, num_scenarios=8, risk_tail=None), beam_agent.VecScenarioBeamSearchAgent),
        ('small_eval, VecScenarioBeamSearchAgent', dict(shape, num_scenarios=8, risk_tail=2), beam_agent.VecScenarioBeamSearchAgent),
        ('small_eval, VecBeamSearchAgent', dict(shape, wind='belief'), beam_agent.VecBeamSearchAgent),
        ('small_eval, VecLookaheadAgent', sample, lookahead_agent.VecLookaheadAgent)):
      print(json.dumps({'what': what, 'planner': planner, **_score(make(**planner))}), flush=True)


if __name__ == '__main__':
  main()
