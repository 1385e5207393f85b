"""Rates and scores of the guided tree search in scenario winds, beside the two planners it stands between, in one process:

 * one decision of VecScenarioMCTSAgent(16, 8, 6, num_scenarios=8, risk_tail=2) at N = 4 096, segment 4, unguided, and its parts, by
   device events between the launches of one search: the scenario fit, the R selects, the R expands, the R backups (the group step
   included), the finish;
 * in the same process VecMCTSAgent(16, 8, 6, wind='belief') and VecScenarioBeamSearchAgent(27, 6, 4, num_scenarios=8): code this search
   does not touch;
 * one guided decision with a (3, 256, 2) actor-critic of random weights at --guided-envs environments (512, or a size that fits: the
   guide sees M times the imagined states of §3v's guided search);
 * ms per decision and ns per FLOWN edge (the EXPAND slots of the decision x 3 x M, counted on the device after it);
 * small_eval of the unguided scenario search at risk_tail None and 2: one run each, NOT a gate.

Device events around every single call, the median of 21 calls after 5 warm-up calls; the evaluations by the host clock.

  python profiles/mcts_scenarios_rate.py [--quick] [--skip-scores] [--guided-envs N] > profiles/mcts_scenarios_rate.jsonl
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mcts_rate  # noqa: E402  (timed, _env, _guide, _score; it puts the repository on the path)

from balloon_learning_environment_amd import _abi, _lib, device as dev  # noqa: E402
from balloon_learning_environment_amd.agents import mcts_agent  # noqa: E402

GAMMA = mcts_rate.GAMMA
PHASES = ('fit', 'select', 'expand', 'observe_forward', 'backup', 'finish')
ITERS, WARMUP = 21, 5


def phased(sim, agent, iters=ITERS, warmup=WARMUP):
  """One decision launch by launch -- mcts_search's own calls on the agent's buffers -- with a device event between the phases:
  {phase: median microseconds, summed over the rounds}."""
  bf, stream, lib = agent.buffers, dev.stream_ptr(agent.device), sim.lib
  pool, groups, status = ctypes.byref(bf._struct), ctypes.byref(bf._group_struct), sim.state['status'].data_ptr()
  guide, num, tail = agent._guide_fn, agent.num_scenarios, agent.risk_tail

  def mark(events):
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    events.append(e)

  def once(events):
    mark(events)
    scn = sim.fit_wind_scenarios(num, seed=agent.seed, seeds=agent._seeds, out=agent._scenarios)
    b, gen = sim._scenario_structs(scn)
    mark(events)
    for r in range(bf.rounds):
      _lib.check(lib.ble_mcts_select_f32(groups, r, agent.c_puct, status, None, stream), 'select')
      mark(events)
      ex = _abi.BleMctsExpand(r, agent.action_repeat, agent.substeps, 0, agent.gamma, sim.grid.data_ptr(), sim.grid_env_stride)
      _lib.check(lib.ble_mcts_expand_scenarios_f32(ctypes.byref(sim._struct), pool, ctypes.byref(ex), ctypes.byref(b), ctypes.byref(gen),
                                                   sim.rollout_flags.data_ptr(), stream), 'expand')
      mark(events)
      if guide is not None:
        sim.observe_leaves(bf.arenas[r], out=bf.obs)
        guide(bf.obs, out=bf.guide_action, value=bf.value, probs=bf.probs)
      mark(events)
      _lib.check(lib.ble_mcts_backup_scenarios_f32(pool, r, num, tail, dev.ptr(bf.value) if guide else None, dev.ptr(bf.probs) if guide else None,
                                                   bf.group_status.data_ptr(), bf.group_g.data_ptr(), stream), 'backup')
      mark(events)
    fin = _abi.BleMctsFinish(status, bf.best_plan.data_ptr(), bf.action.data_ptr(), bf.best_return.data_ptr(), bf.q.data_ptr(),
                             bf.root_visits.data_ptr(), bf.pv_length.data_ptr())
    _lib.check(lib.ble_mcts_finish_f32(groups, ctypes.byref(fin), stream), 'finish')
    mark(events)

  for _ in range(warmup):
    once([])
  runs = []
  for _ in range(iters):
    events = []
    once(events)
    torch.cuda.synchronize()
    gaps = [a.elapsed_time(b) * 1e3 for a, b in zip(events, events[1:])]
    parts = {'fit': gaps[0], 'finish': gaps[-1]}
    for k, name in enumerate(('select', 'expand', 'observe_forward', 'backup')):
      parts[name] = sum(gaps[1 + k:-1:4])
    runs.append(parts)
  return {name: float(np.median([r[name] for r in runs])) for name in PHASES}


def scenario_rows(env, obs, shape, num, tail, guided):
  sim, n = env.arena.sim, env.num_envs
  rounds, leaves, depth, segment = shape
  agent = env.planner(search='mcts', wind='scenarios', num_rounds=rounds, leaves_per_round=leaves, max_depth=depth, segment=segment,
                      gamma=GAMMA, num_scenarios=num, risk_tail=tail, guide=mcts_rate._guide() if guided else None)
  base = {'num_envs': n, 'num_rounds': rounds, 'leaves_per_round': leaves, 'max_depth': depth, 'segment': segment, 'wind': 'scenarios',
          'num_scenarios': num, 'risk_tail': tail, 'guide': '(3, 256, 2) actor-critic, random weights' if guided else None,
          'observed_states_per_env': 3 * leaves * rounds * num if guided else 0}
  whole = {'what': 'VecScenarioMCTSAgent.act', **base, **mcts_rate.timed(lambda: agent.act(obs), ITERS, WARMUP)}
  parts = phased(sim, agent)
  trace = []
  agent.act(obs, trace=trace)
  torch.cuda.synchronize()
  groups = 3 * sum(int((rec[2] == _abi.MCTS_EXPAND).sum().item()) for rec in trace)
  edges = groups * num
  whole.update({'ms_per_decision': whole['median_us'] / 1e3, 'expanded_groups_per_env': groups / n, 'flown_edges': edges,
                'flown_edges_per_env': edges / n, 'ns_per_flown_edge': 1e3 * parts['expand'] / max(edges, 1),
                'ns_per_flown_edge_whole_decision': 1e3 * whole['median_us'] / max(edges, 1),
                'pv_length_mean': float(agent.buffers.pv_length.float().mean().item())})
  return [whole, {'what': 'the parts of that decision, launch by launch (us, summed over the rounds)', **base, **parts, 'sum_us': sum(parts.values())}]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='small shapes')
  ap.add_argument('--skip-scores', action='store_true', help='the rates only')
  ap.add_argument('--guided-envs', type=int, default=512)
  args = ap.parse_args()
  shape = (4, 2, 3, 2) if args.quick else (16, 8, 6, 4)
  n, steps, num = (256, 8, 3) if args.quick else (4096, 60, 8)
  rounds, leaves, depth, segment = shape
  env, obs = mcts_rate._env(n, steps)
  for row in scenario_rows(env, obs, shape, num, 2, guided=False):
    print(json.dumps(row), flush=True)
  plain = env.planner(search='mcts', num_rounds=rounds, leaves_per_round=leaves, max_depth=depth, segment=segment, gamma=GAMMA, wind='belief')
  row = {'what': 'VecMCTSAgent.act', 'num_envs': n, 'num_rounds': rounds, 'leaves_per_round': leaves, 'max_depth': depth, 'segment': segment,
         'wind': 'belief', **mcts_rate.timed(lambda: plain.act(obs), ITERS, WARMUP)}
  row['ms_per_decision'] = row['median_us'] / 1e3
  print(json.dumps(row), flush=True)
  beam = env.planner(search='beam', wind='scenarios', beam_width=27, depth=6, segment=4, gamma=GAMMA, num_scenarios=num)
  row = {'what': 'VecScenarioBeamSearchAgent.act', 'num_envs': n, 'beam_width': 27, 'depth': 6, 'segment': 4, 'num_scenarios': num,
         'flown_edges_per_env': (3 + 9 + 27 + 81 + 81 + 81) * num, **mcts_rate.timed(lambda: beam.act(obs), ITERS, WARMUP)}
  row.update({'ms_per_decision': row['median_us'] / 1e3, 'ns_per_flown_edge_whole_decision': 1e3 * row['median_us'] / (n * row['flown_edges_per_env'])})
  print(json.dumps(row), flush=True)
  env.check_errors()
  del plain, beam, env
  torch.cuda.empty_cache()
  small, small_obs = mcts_rate._env(min(args.guided_envs, n), steps)
  for row in scenario_rows(small, small_obs, shape, num, 2, guided=True):
    print(json.dumps(row), flush=True)
  small.check_errors()
  del small
  torch.cuda.empty_cache()
  if not args.skip_scores:
    for tail in (None, 2):
      search = dict(num_rounds=rounds, leaves_per_round=leaves, max_depth=depth, segment=segment, num_scenarios=num, risk_tail=tail)
      print(json.dumps({'what': 'small_eval, VecScenarioMCTSAgent without a guide', 'planner': search,
                        **mcts_rate._score(mcts_agent.VecScenarioMCTSAgent(**search))}), flush=True)


if __name__ == '__main__':
  main()
