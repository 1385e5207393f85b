"""Rates and scores of the beam-search planner, each beside the sampling planner it stands next to, in one process:

 * one decision of VecBeamSearchAgent at N = 4 096, wind='belief', with (beam_width, depth, segment) = (27, 6, 4), (64, 12, 4) and
   (243, 6, 4) -- the last cuts nothing: the full tree --; the belief fit alone; the decision's expand launches alone, and from the two the share of the decision outside them (the fit, the
   selections, the finish);
 * the same decision beside VecLookaheadAgent(num_plans=64, horizon=24) and beside VecLookaheadAgent(num_plans=729, horizon=24): 729
   plans are the enumeration the (27, 6, 4) tree replaces -- by step-lane counts 729 x 24 = 17 496 flown steps per environment against
   (3 + 9 + 27 + 81 + 81 + 81) x 4 = 1 128 for the beam of 27, 4 368 for the full tree;
 * small_eval of both planners, one run each: NOT a gate, recorded like the README's other scores.

Device events around every single call, the median of 21 calls after 5 warm-up calls (microseconds); the evaluations by the host clock
around the whole call.  One JSON line per measurement.

  python profiles/beam_rate.py [--quick] [--skip-scores] > profiles/beam_rate.jsonl
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from balloon_learning_environment_amd import _abi, _lib, device as dev, vec_state  # noqa: E402
from balloon_learning_environment_amd.agents import beam_agent, lookahead_agent  # noqa: E402
from balloon_learning_environment_amd.env import balloon_env  # noqa: E402
from balloon_learning_environment_amd.eval import eval_lib, suites  # noqa: E402

GAMMA = 0.993


def timed(call, iters=21, warmup=5):
  """Microseconds of each of `iters` calls, by a pair of device events around every call: median, min and max."""
  for _ in range(warmup):
    call()
  torch.cuda.synchronize()
  pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
  for a, b in pairs:
    a.record()
    call()
    b.record()
  torch.cuda.synchronize()
  us = np.array([a.elapsed_time(b) * 1e3 for a, b in pairs])
  return {'median_us': float(np.median(us)), 'min_us': float(us.min()), 'max_us': float(us.max()), 'calls': iters}


def _env(n, steps):
  env = balloon_env.VecBalloonEnv(n, seed=0, auto_reset=False)
  obs = env.reset()
  g = torch.Generator(device='cuda').manual_seed(0)
  for _ in range(steps):
    obs, _, _ = env.step(torch.randint(0, 3, (n,), dtype=torch.uint8, device='cuda', generator=g))
  return env, obs


def _expands_only(sim, agent):
  """The depth expand launches of one decision, with tree_search's own descriptors; the parent lists are the last search's."""
  bf, stream = agent.buffers, dev.stream_ptr(agent.device)
  b = sim._belief_struct(agent._belief)
  calls = []
  for level, (parents, _) in enumerate(vec_state.tree_level_sizes(agent.depth, agent.beam_width), 1):
    src = bf.node_struct(level - 1) if level > 1 else _abi.BleTreeArena()
    calls.append(_abi.BleTreeExpand(sim.n, agent.beam_width, agent.depth, parents, 0 if level == 1 else 3 * prev, agent.segment,
                                    agent.action_repeat, agent.substeps, 0, agent.gamma, sim.grid.data_ptr(), sim.grid_env_stride,
                                    bf.parent.data_ptr(), src, bf.node_struct(level)))
    prev = parents

  def run():
    for ex in calls:
      _lib.call('ble_tree_expand_f32', ctypes.byref(sim._struct), ctypes.byref(ex), None, ctypes.byref(b), sim.rollout_flags.data_ptr(), stream)
  return run


def decision_rates(n, shapes, samplers, steps):
  env, obs = _env(n, steps)
  sim = env.arena.sim
  belief = sim.fit_wind_belief()
  rows = [{'what': 'fit_wind_belief alone', 'num_envs': n, **timed(lambda: sim.fit_wind_belief(out=belief))}]
  for beam, depth, segment in shapes:
    agent = env.planner(search='beam', beam_width=beam, depth=depth, segment=segment, gamma=GAMMA, wind='belief')
    sizes = vec_state.tree_level_sizes(depth, beam)
    base = {'num_envs': n, 'beam_width': beam, 'depth': depth, 'segment': segment, 'wind': 'belief',
            'flown_steps_per_env': sum(c for _, c in sizes) * segment, 'children_per_level': [c for _, c in sizes]}
    whole = {'what': 'VecBeamSearchAgent.act', **base, **timed(lambda: agent.act(obs))}
    expands = {'what': 'the expand launches of that decision alone', **base, **timed(_expands_only(sim, agent))}
    whole['share_outside_the_expands'] = 1.0 - expands['median_us'] / whole['median_us']
    whole['ns_per_flown_step'] = expands['median_us'] * 1e3 / (n * base['flown_steps_per_env'])
    rows += [whole, expands, {'what': 'VecBeamSearchAgent.act, again', **base, **timed(lambda: agent.act(obs))}]
    del agent
  for k, h in samplers:
    agent = env.planner(num_plans=k, horizon=h, segment=4, gamma=GAMMA, wind='belief')
    row = {'what': 'VecLookaheadAgent.act', 'num_envs': n, 'num_plans': k, 'horizon': h, 'segment': 4, 'wind': 'belief',
           'flown_steps_per_env': k * h, **timed(lambda: agent.act(obs))}
    row['ns_per_flown_step'] = row['median_us'] * 1e3 / (n * k * h)
    rows.append(row)
    del agent
  env.check_errors()
  return rows


def _score(agent):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  res = eval_lib.eval_agent_vec(agent, suites.get_eval_suite('small_eval'))
  torch.cuda.synchronize()
  return {'mean_cumulative_reward': float(np.mean([r.cumulative_reward for r in res])),
          'mean_time_within_radius': float(np.mean([r.time_within_radius for r in res])), 'flights': len(res),
          'eval_wall_s': time.perf_counter() - t0, 'runs': 1, 'gate': 'not a gate'}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='small shapes')
  ap.add_argument('--skip-scores', action='store_true', help='the rates only')
  args = ap.parse_args()
  if args.quick:
    rows = decision_rates(256, ((4, 3, 2),), ((16, 6),), 8)
  else:
    # (243, 6, 4) cuts nothing: the full tree of 729 leaves, the enumeration itself with every prefix flown once
    rows = decision_rates(4096, ((27, 6, 4), (64, 12, 4), (243, 6, 4)), ((64, 24), (729, 24)), 60)
  for row in rows:
    print(json.dumps(row), flush=True)
  if not args.skip_scores:
    beam = dict(beam_width=27, depth=6, segment=4, wind='belief')
    sample = dict(num_plans=64, horizon=24, segment=4, wind='belief')
    print(json.dumps({'what': 'small_eval, VecBeamSearchAgent', 'planner': beam, **_score(beam_agent.VecBeamSearchAgent(**beam))}), flush=True)
    print(json.dumps({'what': 'small_eval, VecLookaheadAgent', 'planner': sample, **_score(lookahead_agent.VecLookaheadAgent(**sample))}),
          flush=True)


if __name__ == '__main__':
  main()
