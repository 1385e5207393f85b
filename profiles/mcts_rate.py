"""Rates and scores of the guided tree search, beside the planners it stands next to, in one process:

 * one decision of VecMCTSAgent at N = 4 096, wind='belief', segment 4, (num_rounds, leaves_per_round, max_depth) = (16, 8, 6) -- at
   most 384 edges = 1 536 flown steps per environment, the 64-plan sampler's count --, without a guide and with a (3, 256, 2)
   actor-critic of random weights as guide; and its parts, by device events between the launches of one search: the belief fit, the R
   selects, the R expands, the R x (observe_leaves + the guide's forward), the R backups, the finish;
 * in the same run the unchanged beam, VecBeamSearchAgent(27, 6, 4), and VecLookaheadAgent(num_plans=64, horizon=24): code this search
   does not touch, so the comparison does not move with it;
 * ms per decision and us per FLOWN edge (the EXPAND slots of the decision x 3, counted on the device after it);
 * small_eval of an unguided search and of one guided by a learner that a short run_exit_loop_vec trained with the search itself as
   its expert (guide=learner): one run each, NOT a gate, recorded like the README's other scores.

--mapping NAME tags every row with the mapping of select, backup and finish that the loaded library has (BLE_HIP_LIB: another build).
The rows of mcts_rate.jsonl tagged 'one wavefront per environment, statistics in LDS' are of the mapping this one replaced, measured
with this script in the same session before it was removed.
Device events around every single call, the median of 11 calls after 3 warm-up calls; the evaluations by the host clock.

  python profiles/mcts_rate.py [--quick] [--skip-scores] [--skip-others] [--mapping NAME] > profiles/mcts_rate.jsonl
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

from balloon_learning_environment_amd import _abi, _lib, device as dev, train_lib  # noqa: E402
from balloon_learning_environment_amd.agents import actor_critic, beam_agent, expert_iteration, lookahead_agent, mcts_agent, qnet  # noqa: E402
from balloon_learning_environment_amd.env import balloon_env  # noqa: E402
from balloon_learning_environment_amd.eval import eval_lib, suites  # noqa: E402

GAMMA = 0.993
PHASES = ('fit', 'select', 'expand', 'observe_forward', 'backup', 'finish')


def timed(call, iters=11, warmup=3):
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


def _guide(layers=3, hidden=256, seed=1):
  net = qnet.QNetwork.from_params(actor_critic.init_params('actor_critic', seed=seed, num_layers=layers, hidden_units=hidden), num_atoms=2)
  return actor_critic.VecActorCriticAgent(net, deterministic=True)


def phased(sim, agent, iters=11, warmup=3):
  """One decision launch by launch -- mcts_search's own calls on the agent's buffers -- with a device event between the phases:
  {phase: median microseconds, summed over the rounds}."""
  bf, stream, lib = agent.buffers, dev.stream_ptr(agent.device), sim.lib
  pool, status = ctypes.byref(bf._struct), sim.state['status'].data_ptr()
  guide = agent._guide_fn

  def mark(events):
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    events.append(e)

  def once(events):
    mark(events)
    belief = sim.fit_wind_belief(out=agent._belief)
    b = sim._belief_struct(belief)
    mark(events)
    for r in range(bf.rounds):
      _lib.check(lib.ble_mcts_select_f32(pool, r, agent.c_puct, status, None, stream), 'select')
      mark(events)
      ex = _abi.BleMctsExpand(r, agent.action_repeat, agent.substeps, 0, agent.gamma, sim.grid.data_ptr(), sim.grid_env_stride)
      _lib.check(lib.ble_mcts_expand_f32(ctypes.byref(sim._struct), pool, ctypes.byref(ex), None, ctypes.byref(b), sim.rollout_flags.data_ptr(),
                                         stream), 'expand')
      mark(events)
      if guide is not None:
        sim.observe_leaves(bf.arenas[r], out=bf.obs)
        guide(bf.obs, out=bf.guide_action, value=bf.value, probs=bf.probs)
      mark(events)
      _lib.check(lib.ble_mcts_backup_f32(pool, r, dev.ptr(bf.value) if guide else None, dev.ptr(bf.probs) if guide else None, stream), 'backup')
      mark(events)
    fin = _abi.BleMctsFinish(status, bf.best_plan.data_ptr(), bf.action.data_ptr(), bf.best_return.data_ptr(), bf.q.data_ptr(),
                             bf.root_visits.data_ptr(), bf.pv_length.data_ptr())
    _lib.check(lib.ble_mcts_finish_f32(pool, ctypes.byref(fin), stream), 'finish')
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


def decision_rates(n, shape, steps, mapping, others):
  env, obs = _env(n, steps)
  sim = env.arena.sim
  rounds, leaves, depth, segment = shape
  rows = []
  for guided in (False, True):
    agent = env.planner(search='mcts', num_rounds=rounds, leaves_per_round=leaves, max_depth=depth, segment=segment, gamma=GAMMA,
                        wind='belief', guide=_guide() if guided else None)
    base = {'mapping': mapping, 'num_envs': n, 'num_rounds': rounds, 'leaves_per_round': leaves, 'max_depth': depth, 'segment': segment,
            'wind': 'belief', 'guide': '(3, 256, 2) actor-critic, random weights' if guided else None}
    whole = {'what': 'VecMCTSAgent.act', **base, **timed(lambda: agent.act(obs))}
    parts = phased(sim, agent)
    # the edges the decision flew: its EXPAND slots are counted round by round on the device, after the timing
    trace = []
    agent.act(obs, trace=trace)
    torch.cuda.synchronize()
    edges = 3 * sum(int((rec[2] == _abi.MCTS_EXPAND).sum().item()) for rec in trace)
    whole.update({'ms_per_decision': whole['median_us'] / 1e3, 'flown_edges': edges, 'flown_edges_per_env': edges / n,
                  'us_per_flown_edge': parts['expand'] / max(edges, 1), 'us_per_flown_edge_whole_decision': whole['median_us'] / max(edges, 1),
                  'pv_length_mean': float(agent.buffers.pv_length.float().mean().item())})
    rows += [whole, {'what': 'the parts of that decision, launch by launch (us, summed over the rounds)', **base, **parts,
                     'sum_us': sum(parts.values())}]
    del agent
  if others:
    beam = env.planner(search='beam', beam_width=27, depth=6, segment=4, gamma=GAMMA, wind='belief')
    row = {'what': 'VecBeamSearchAgent.act', 'num_envs': n, 'beam_width': 27, 'depth': 6, 'segment': 4, 'wind': 'belief',
           'flown_edges_per_env': 3 + 9 + 27 + 81 + 81 + 81, **timed(lambda: beam.act(obs))}
    row.update({'ms_per_decision': row['median_us'] / 1e3, 'us_per_flown_edge_whole_decision': row['median_us'] / (n * row['flown_edges_per_env'])})
    rows.append(row)
    sampler = env.planner(num_plans=64, horizon=24, segment=4, gamma=GAMMA, wind='belief')
    row = {'what': 'VecLookaheadAgent.act', 'num_envs': n, 'num_plans': 64, 'horizon': 24, 'segment': 4, 'wind': 'belief',
           'flown_steps_per_env': 64 * 24, **timed(lambda: sampler.act(obs))}
    row['ms_per_decision'] = row['median_us'] / 1e3
    rows.append(row)
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


def _trained_guide(search, n=256, steps=32, iterations=6):
  """A (2, 64, 2) learner after `iterations` of expert iteration in which the search it guides is its expert."""
  env = balloon_env.VecBalloonEnv(n, seed=1)
  learner = expert_iteration.SoftBCTrainer(qnet.QNetwork.from_params(actor_critic.init_params('actor_critic', 2, 2, 64), num_atoms=2), lr=1e-3,
                                           seed=5, temperature=0.5, value_coef=0.5)
  planner = env.planner(search='mcts', guide=learner, **search)
  buffer = expert_iteration.VecPlanLabelBuffer(n, steps)
  t0 = time.perf_counter()
  stats = train_lib.run_exit_loop_vec(env, learner, planner, buffer, num_iterations=iterations, beta=0.5, epochs=2, batch_size=256,
                                      capture_graph=False)
  return learner, {'iterations': iterations, 'num_envs': n, 'steps_per_iteration': steps, 'train_wall_s': time.perf_counter() - t0,
                   'agreement': [s['agreement'] for s in stats], 'mean_best_return': [s['mean_best_return'] for s in stats]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='small shapes')
  ap.add_argument('--skip-scores', action='store_true', help='the rates only')
  ap.add_argument('--skip-others', action='store_true', help='neither the beam nor the sampler')
  ap.add_argument('--mapping', default='one lane per environment, statistics in global memory')
  args = ap.parse_args()
  shape = (4, 2, 3, 2) if args.quick else (16, 8, 6, 4)
  for row in decision_rates(256 if args.quick else 4096, shape, 8 if args.quick else 60, args.mapping, not args.skip_others):
    print(json.dumps(row), flush=True)
  if not args.skip_scores:
    search = dict(num_rounds=shape[0], leaves_per_round=shape[1], max_depth=shape[2], segment=shape[3], wind='belief')
    print(json.dumps({'what': 'small_eval, VecMCTSAgent without a guide', 'planner': search, **_score(mcts_agent.VecMCTSAgent(**search))}),
          flush=True)
    learner, training = _trained_guide(search, iterations=1 if args.quick else 6)
    print(json.dumps({'what': 'small_eval, VecMCTSAgent guided by its own learner', 'planner': search, 'training': training,
                      **_score(mcts_agent.VecMCTSAgent(guide=learner, **search))}), flush=True)
    if not args.skip_others:
      beam = dict(beam_width=27, depth=6, segment=4, wind='belief')
      sample = dict(num_plans=64, horizon=24, segment=4, wind='belief')
      print(json.dumps({'what': 'small_eval, VecBeamSearchAgent', 'planner': beam, **_score(beam_agent.VecBeamSearchAgent(**beam))}), flush=True)
      print(json.dumps({'what': 'small_eval, VecLookaheadAgent', 'planner': sample, **_score(lookahead_agent.VecLookaheadAgent(**sample))}),
            flush=True)


if __name__ == '__main__':
  main()
