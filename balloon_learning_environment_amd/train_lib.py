"""The training loops of the device learners over a VecBalloonEnv: the reference's train_lib.run_training_loop with Dopamine's
schedule (min_replay_history, update_period, target_update_period counted in transitions) for the replay learners (QNetworkTrainer,
DQNTrainer), the loop of an online learner (VecMLPAgent), the on-policy loop (PPOTrainer), the DAgger loop of an imitation learner
(BCTrainer), the expert-iteration loop of a soft-target learner and a planner (SoftBCTrainer, VecLookaheadAgent) and population-based
training of P on-policy learners in one batch (PopulationPPOTrainer) and of P replay learners in one batch (PopulationQTrainer);
N environments per step.
"""
from typing import Callable, List, Optional, Sequence, Tuple, Union

import torch

from balloon_learning_environment_amd.agents import qnet_train

WITHIN_RADIUS_REWARD = 0.5     # perciatelli_reward_function: 1.0 inside the radius, at most reward_dropoff = 0.4 outside


class _EpisodeBook:
  """The per-environment episode bookkeeping of both loops and the accumulators of one iteration, all on the device: nothing here
  synchronises with the host but finish_iteration()."""

  def __init__(self, num_envs: int, device, max_episode_length: int):
    self.n, self.device, self.max_episode_length = num_envs, device, max_episode_length
    self.ep_steps = torch.zeros(num_envs, dtype=torch.int32, device=device)
    self.ep_return = torch.zeros(num_envs, dtype=torch.float32, device=device)
    self.transitions = 0
    self.begin_iteration()

  def begin_iteration(self) -> None:
    self.loss_sum = torch.zeros((), dtype=torch.float32, device=self.device)
    self.done_returns = torch.zeros((), dtype=torch.float32, device=self.device)
    self.episodes = torch.zeros((), dtype=torch.int64, device=self.device)
    self.within = torch.zeros((), dtype=torch.int64, device=self.device)
    self.updates = 0

  def end_mask(self) -> torch.Tensor:
    """uint8 [N]: the environments whose next step reaches the episode limit."""
    return (self.ep_steps + 1 >= self.max_episode_length).to(torch.uint8)

  def step(self, reward: torch.Tensor, episode_end: torch.Tensor) -> None:
    """One vector step's rewards [N] and episode ends (uint8 [N]: a terminal or the time limit)."""
    self.ep_return += reward
    self.ep_steps += 1
    ended = episode_end.bool()
    self.episodes += ended.sum()
    self.done_returns += torch.where(ended, self.ep_return, torch.zeros_like(self.ep_return)).sum()
    self.ep_return.masked_fill_(ended, 0.0)
    self.ep_steps.masked_fill_(ended, 0)
    self.within += (reward > WITHIN_RADIUS_REWARD).sum()
    self.transitions += self.n

  def update(self, loss: torch.Tensor) -> None:
    """The per-row losses of one update."""
    self.loss_sum += loss.mean()
    self.updates += 1

  def finish_iteration(self, steps: int) -> dict:
    """The iteration's dict (the loop's one host synchronisation), and the accumulators start again."""
    ne = int(self.episodes.item())
    stats = {'mean_loss': float(self.loss_sum.item()) / max(self.updates, 1), 'updates': self.updates, 'episodes': ne,
             'mean_return': float(self.done_returns.item()) / ne if ne else float('nan'),
             'time_within_radius': float(self.within.item()) / (self.n * steps), 'transitions': self.transitions}
    self.begin_iteration()
    return stats


def run_training_loop_vec(env, trainer: qnet_train.QNetworkTrainer, replay: qnet_train.VecReplayBuffer, *, num_iterations: int,
                          steps_per_iteration: int, max_episode_length: int = 960, min_replay_history: int = 500,
                          update_period: int = 4, target_update_period: int = 100,
                          epsilon: Union[float, Callable[[int], float]] = 0.01, updates_per_step: Optional[int] = None,
                          batch_size: int = 32, seed: int = 0, capture_graph: bool = True, exploration=None) -> List[dict]:
  """Trains `trainer` on `env` (auto_reset) for num_iterations x steps_per_iteration vector steps.  Each step: the online network's
  greedy actions, epsilon-greedy (ble_qnet_explore_u8, keyed by (seed, environment, step)), env.step, replay.add, then the updates.

  Dopamine counts agent steps: one update per update_period transitions once min_replay_history transitions are held, and a target
  sync every target_update_period transitions, i.e. every target_update_period / update_period updates.  Here a vector step adds N
  transitions, so it runs N / update_period updates (the fraction carried over); updates_per_step overrides that count.  The
  reference's 960-step episode limit is enforced per environment: a lane reaching it ends its episode (episode_end without terminal)
  and restarts.  epsilon: a float or a function of the transitions added so far.

  exploration: None, or a VecMarcoPoloExploration (configs/quantile.gin: with epsilon=0.0 and a VecPrioritizedReplayBuffer).  Each
  step then runs the greedy actions, epsilon-greedy (skipped when epsilon is 0), then the explorer, whose begin mask is all ones at the
  first step and the previous step's episode_end after; the replay stores the action actually taken.

  Returns one dict per iteration: mean_loss (over the iteration's updates), updates, episodes (finished), mean_return (of the finished
  episodes), time_within_radius (the fraction of the iteration's transitions with reward > 0.5, i.e. inside the radius), transitions."""
  n, dev_ = env.num_envs, env.device
  assert replay.num_envs == n, 'the replay ring has one column per environment'
  sync_every = max(1, target_update_period // update_period)
  obs = env.reset()
  actions = torch.zeros(n, dtype=torch.uint8, device=dev_)
  book = _EpisodeBook(n, dev_, max_episode_length)
  begin = torch.ones(n, dtype=torch.uint8, device=dev_)
  updates, pending, step = 0, 0.0, 0
  captured = False
  stats = []
  for _ in range(num_iterations):
    for _ in range(steps_per_iteration):
      trainer.act(obs, actions)
      eps = epsilon(book.transitions) if callable(epsilon) else epsilon
      if exploration is None:
        qnet_train.explore(actions, eps, seed, step)
      else:
        if eps > 0.0:
          qnet_train.explore(actions, eps, seed, step)
        exploration(obs, actions, begin)
      end_mask = book.end_mask()
      next_obs, reward, terminal = env.step(actions, end_mask=end_mask)
      episode_end = terminal | end_mask
      if exploration is not None:
        begin.copy_(episode_end)
      replay.add(obs, actions, reward, terminal, episode_end)
      book.step(reward, episode_end)
      obs = next_obs
      step += 1
      if book.transitions >= min_replay_history and replay.cursor > replay.update_horizon:
        if updates_per_step is not None:
          todo = int(updates_per_step)
        else:
          pending += n / update_period
          todo = int(pending)
          pending -= todo
        for _ in range(todo):
          if capture_graph and not captured:
            loss = trainer.capture(replay, batch_size)        # (its first, eager update is a real one)
            captured = True
          else:
            loss = trainer.train_step(replay, batch_size)
          book.update(loss)
          updates += 1
          if updates % sync_every == 0:
            trainer.sync_target()
    env.check_errors()
    replay.check_errors()
    trainer.check_errors()
    stats.append(book.finish_iteration(steps_per_iteration))
  return stats


def run_online_loop_vec(env, agent, *, num_iterations: int, steps_per_iteration: int, max_episode_length: int = 960) -> List[dict]:
  """Runs an online learner (VecMLPAgent: begin_episode / step) on `env` (auto_reset) for num_iterations x steps_per_iteration vector
  steps; in train mode every step is one update on the N transitions just made.  The episode limit is run_training_loop_vec's: a lane
  reaching it ends its episode without a terminal and restarts; the agent is told of every episode end, whose row it does not train on.

  Returns run_training_loop_vec's dicts: mean_loss (the objective, i.e. the mean of the N rows' losses, averaged over the iteration's
  updates), updates, episodes, mean_return, time_within_radius, transitions."""
  n, dev_ = env.num_envs, env.device
  assert agent.num_envs == n, 'the agent holds one row per environment'
  training = agent._mode.value == 'train'
  actions = agent.begin_episode(env.reset())
  book = _EpisodeBook(n, dev_, max_episode_length)
  stats = []
  for _ in range(num_iterations):
    for _ in range(steps_per_iteration):
      end_mask = book.end_mask()
      obs, reward, terminal = env.step(actions, end_mask=end_mask)
      episode_end = terminal | end_mask
      actions = agent.step(reward, obs, episode_end)
      if training:
        book.update(agent.loss)
      book.step(reward, episode_end)
    env.check_errors()
    agent.check_errors()
    stats.append(book.finish_iteration(steps_per_iteration))
  return stats


def run_ppo_loop_vec(env, trainer, rollout, *, num_iterations: int, epochs: int = 4, batch_size: int, max_episode_length: int = 960,
                     capture_graph: bool = True) -> List[dict]:
  """Trains an on-policy learner (agents/actor_critic.py: PPOTrainer with a VecRolloutBuffer of T steps) on `env` (auto_reset).  Each
  iteration collects T vector steps with the sampled policy -- the episode limit as in run_training_loop_vec: a lane reaching it ends
  its episode without a terminal and restarts --, takes the bootstrap value from one more act on the last observation (its draw is not
  used), computes the advantages over the [T, N] block (rollout.finish) and runs `epochs` passes of minibatches of batch_size rows, each
  one update; then the block is discarded.

  Returns run_training_loop_vec's dicts (mean_loss over the iteration's updates; transitions counts the collected ones).  The only host
  synchronisation is the end of an iteration."""
  n, dev_ = env.num_envs, env.device
  assert rollout.num_envs == n, 'the rollout block has one column per environment'
  steps = rollout.horizon
  obs = env.reset()
  actions = torch.zeros(n, dtype=torch.uint8, device=dev_)
  logp = torch.zeros(n, dtype=torch.float32, device=dev_)
  value = torch.zeros(n, dtype=torch.float32, device=dev_)
  book = _EpisodeBook(n, dev_, max_episode_length)
  captured = False
  stats = []
  for _ in range(num_iterations):
    for t in range(steps):
      trainer.act(obs, actions, logp, value)
      end_mask = book.end_mask()
      next_obs, reward, terminal = env.step(actions, end_mask=end_mask)
      episode_end = terminal | end_mask
      rollout.add(t, obs, actions, logp, value, reward, terminal, episode_end)
      book.step(reward, episode_end)
      obs = next_obs
    trainer.act(obs, actions, logp, value)
    rollout.finish(value, trainer.gamma, trainer.lam, trainer.normalize_advantage)
    for _ in range(epochs):
      for batch in rollout.minibatches(batch_size):
        if capture_graph and not captured:
          loss = trainer.capture(batch)                     # (its first, eager update is a real one)
          captured = True
        else:
          loss = trainer.train_step(batch)
        book.update(loss)
    env.check_errors()
    trainer.check_errors()
    stats.append(book.finish_iteration(steps))
  return stats


def pbt_decide(fitness: torch.Tensor, truncation: float, generator: Optional[torch.Generator] = None,
               num_explored: int = 1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
  """One round of population-based training (Jaderberg et al. 2017, truncation selection) as a pure function, on fitness's device
  and without a host synchronisation: (src, dst, factor_index).

  fitness [P] float: higher is better; NaN marks a member without a finished episode, which ranks lowest.  The members are ranked best
  first by a stable sort, so ties break by member index.  k = floor(truncation * P), at most P // 2.  dst int64 [k]: the k lowest-ranked
  members, in rank order; src int64 [k]: for each a member of the k highest-ranked drawn uniformly with `generator`; factor_index
  int64 [k, num_explored] in {0, 1}: which of the two perturbation factors each explored hyperparameter of the copy takes.  k == 0
  (truncation 0, or P too small): three empty tensors, nothing drawn."""
  assert fitness.dim() == 1 and fitness.is_floating_point() and 0.0 <= truncation <= 0.5
  p, d = fitness.numel(), fitness.device
  k = min(int(truncation * p + 1e-9), p // 2)
  if k == 0:
    e = torch.zeros(0, dtype=torch.int64, device=d)
    return e, e.clone(), torch.zeros(0, num_explored, dtype=torch.int64, device=d)
  none = torch.isnan(fitness)
  order = torch.sort(torch.where(none, torch.zeros_like(fitness), fitness), descending=True, stable=True).indices
  order = order[torch.sort(none[order].to(torch.int8), stable=True).indices]      # (below every fitness, -inf too; both sorts stable)
  dst = order[p - k:]
  src = order[:k][torch.randint(0, k, (k,), generator=generator, device=d)]
  factor_index = torch.randint(0, 2, (k, num_explored), generator=generator, device=d)
  return src, dst, factor_index


class PBTController:
  """The state of population-based training between iterations, all on the device: the per-member sums of finished episodes' returns
  and their counts since the last round, the lineage (int64 [P]: the initial member each one descends from), the decisions' generator
  and the iteration count.  state_dict / load_state_dict: a resumed run continues to the same bytes."""

  def __init__(self, members: int, device, *, ready_every: int, truncation: float = 0.25, perturb: Sequence[float] = (0.8, 1.25),
               explore: Sequence[str] = ('lr', 'entropy_coef'), seed: int = 0):
    if ready_every < 1 or not 0.0 <= truncation <= 0.5 or len(perturb) != 2:
      raise ValueError('ready_every >= 1, 0 <= truncation <= 0.5 and two perturbation factors')
    self.members, self.device = int(members), torch.device(device)
    self.ready_every, self.truncation, self.explore = int(ready_every), float(truncation), tuple(explore)
    self.perturb = torch.tensor([float(f) for f in perturb], dtype=torch.float32, device=self.device)
    self.generator = torch.Generator(device=self.device)
    self.generator.manual_seed(int(seed))
    self.lineage = torch.arange(self.members, dtype=torch.int64, device=self.device)
    self.return_sum = torch.zeros(self.members, dtype=torch.float32, device=self.device)
    self.episodes = torch.zeros(self.members, dtype=torch.int64, device=self.device)
    self.iteration = 0
    self.rounds = 0

  def step(self, ended_returns: torch.Tensor, ended: torch.Tensor) -> None:
    """One vector step: ended_returns [P, R] float32 (the return of an episode that ended in this step, else 0), ended [P, R] bool."""
    self.return_sum += ended_returns.sum(dim=1)
    self.episodes += ended.sum(dim=1)

  def fitness(self) -> torch.Tensor:
    """[P] float32: the mean return of the episodes each member finished since the last round; NaN without one."""
    return torch.where(self.episodes > 0, self.return_sum / self.episodes.clamp(min=1).to(torch.float32),
                       torch.full_like(self.return_sum, float('nan')))

  def end_iteration(self, trainer) -> Optional[dict]:
    """Counts the iteration; every ready_every-th runs a round on `trainer` (copy_members, scale_hyper) and returns its device
    tensors {'fitness', 'src', 'dst'}, else None."""
    self.iteration += 1
    if self.iteration % self.ready_every:
      return None
    fitness = self.fitness()
    src, dst, factor_index = pbt_decide(fitness, self.truncation, self.generator, len(self.explore))
    if dst.numel():
      trainer.copy_members(src, dst)
      for j, name in enumerate(self.explore):
        trainer.scale_hyper(name, dst, self.perturb[factor_index[:, j]])
      self.lineage.index_copy_(0, dst, self.lineage.index_select(0, src))
    self.return_sum.zero_()
    self.episodes.zero_()
    self.rounds += 1
    return {'fitness': fitness, 'src': src, 'dst': dst}

  def state_dict(self) -> dict:
    return {'members': self.members, 'iteration': self.iteration, 'rounds': self.rounds, 'generator': self.generator.get_state().clone(),
            'lineage': self.lineage.clone(), 'return_sum': self.return_sum.clone(), 'episodes': self.episodes.clone()}

  def load_state_dict(self, d: dict) -> None:
    assert int(d['members']) == self.members
    self.iteration, self.rounds = int(d['iteration']), int(d['rounds'])
    self.generator.set_state(d['generator'])
    for k in ('lineage', 'return_sum', 'episodes'):
      getattr(self, k).copy_(d[k])


def run_pbt_loop_vec(env, trainer, rollout, *, num_iterations: int, epochs: int = 4, batch_size: int, ready_every: int,
                     truncation: float = 0.25, perturb: Sequence[float] = (0.8, 1.25), explore: Sequence[str] = ('lr', 'entropy_coef'),
                     seed: int = 0, max_episode_length: int = 960, capture_graph: bool = True,
                     controller: Optional[PBTController] = None) -> List[dict]:
  """Population-based training of P on-policy learners in one batch (agents/population.py: PopulationPPOTrainer with a
  VecPopulationRolloutBuffer(P, R, T)) on `env` (auto_reset) of P * R environments, environment rows [p R, (p + 1) R) member p's.

  Each iteration is run_ppo_loop_vec's with grouped calls: T vector steps with every member's sampled policy, the bootstrap act,
  rollout.finish (advantages per member), then `epochs` passes of minibatches of batch_size rows PER MEMBER, each one grouped update.
  Every ready_every iterations a round follows (pbt_decide): fitness[p] is the mean return of the episodes member p finished since the
  last round; the members in the bottom `truncation` share each become a copy of a uniformly drawn member of the top share (weights,
  Adam moments and hyperparameters: trainer.copy_members), and each hyperparameter named in `explore` of the copy is multiplied by one of
  the two `perturb` factors (trainer.scale_hyper).  truncation = 0 is a plain P-seed study.  controller: a PBTController to continue
  (its settings then replace ready_every, truncation, perturb, explore and seed).

  Returns run_training_loop_vec's dicts (mean_loss: the mean over the members' rows) plus member_episodes and member_mean_return
  (lists of P, this iteration's), lineage (a list of P: the initial member each one descends from), lr (a list of P) and, on a round's
  iteration, round = {'fitness', 'src', 'dst'} as lists (else None).  One host synchronisation per iteration: its end."""
  n, dev_ = env.num_envs, env.device
  p, r, steps = rollout.members, rollout.rows_per_member, rollout.horizon
  assert trainer.members == p and rollout.num_envs == n == p * r, 'the rollout block has one column per environment, R per member'
  pbt = controller if controller is not None else PBTController(p, dev_, ready_every=ready_every, truncation=truncation, perturb=perturb,
                                                                explore=explore, seed=seed)
  obs = env.reset()
  actions = torch.zeros(n, dtype=torch.uint8, device=dev_)
  logp = torch.zeros(n, dtype=torch.float32, device=dev_)
  value = torch.zeros(n, dtype=torch.float32, device=dev_)
  book = _EpisodeBook(n, dev_, max_episode_length)
  captured = False
  stats = []
  for _ in range(num_iterations):
    it_sum = torch.zeros(p, dtype=torch.float32, device=dev_)
    it_episodes = torch.zeros(p, dtype=torch.int64, device=dev_)
    for t in range(steps):
      trainer.act(obs, actions, logp, value)
      end_mask = book.end_mask()
      next_obs, reward, terminal = env.step(actions, end_mask=end_mask)
      episode_end = terminal | end_mask
      rollout.add(t, obs, actions, logp, value, reward, terminal, episode_end)
      ended = episode_end.bool().view(p, r)
      ended_returns = torch.where(ended, (book.ep_return + reward).view(p, r), torch.zeros((), dtype=torch.float32, device=dev_))
      pbt.step(ended_returns, ended)
      it_sum += ended_returns.sum(dim=1)
      it_episodes += ended.sum(dim=1)
      book.step(reward, episode_end)
      obs = next_obs
    trainer.act(obs, actions, logp, value)
    rollout.finish(value, trainer.gamma, trainer.lam, trainer.normalize_advantage)
    for _ in range(epochs):
      for batch in rollout.minibatches(batch_size):
        if capture_graph and not captured:
          loss = trainer.capture(batch)                     # (its first, eager update is a real one)
          captured = True
        else:
          loss = trainer.train_step(batch)
        book.update(loss)
    rnd = pbt.end_iteration(trainer)
    env.check_errors()
    trainer.check_errors()
    s = book.finish_iteration(steps)
    eps = it_episodes.tolist()
    s['member_episodes'] = eps
    s['member_mean_return'] = [v / e if e else float('nan') for v, e in zip(it_sum.tolist(), eps)]
    s['lineage'] = pbt.lineage.tolist()
    s['lr'] = trainer.lr.tolist()
    s['round'] = None if rnd is None else {k: v.tolist() for k, v in rnd.items()}
    stats.append(s)
  return stats


def run_population_training_loop_vec(env, trainer, replay, *, num_iterations: int, steps_per_iteration: int,
                                     max_episode_length: int = 960, min_replay_history: int = 500, update_period: int = 4,
                                     target_update_period: int = 100,
                                     epsilon: Union[float, Sequence[float], Callable[[int], float]] = 0.01,
                                     updates_per_step: Optional[int] = None, batch_size: int = 32, capture_graph: bool = True,
                                     ready_every: Optional[int] = None, truncation: float = 0.0, perturb: Sequence[float] = (0.8, 1.25),
                                     seed: int = 0, controller: Optional[PBTController] = None, exploration=None) -> List[dict]:
  """Trains P replay learners in one batch (agents/population.py: PopulationQTrainer with a qnet_train.VecPopulationReplayBuffer(P, R,
  ...)) on `env` (auto_reset) of P * R environments, environment rows [p R, (p + 1) R) member p's, for num_iterations x
  steps_per_iteration vector steps.  Each step: every member's greedy actions (trainer.act), epsilon-greedy per member
  (qnet_train.explore_grouped, member p keyed by (trainer.seeds[p], its row, step) at its own rate), env.step, replay.add, then the
  grouped updates -- each one update of every member on batch_size rows of its own columns.

  The schedule is run_training_loop_vec's, applied PER MEMBER: a vector step adds R transitions to each member, so it runs
  R / update_period grouped updates (the fraction carried over; updates_per_step overrides that count) once each member holds
  min_replay_history transitions; every member's target is synced every target_update_period // update_period updates.  The 960-step
  episode limit is enforced per environment.  epsilon: a float, a length-P sequence (an epsilon ladder: member p explores at
  epsilon[p]) or a function of the transitions a member has added so far.  The update is captured into one graph on first use.

  ready_every with truncation > 0 makes it population-based training: every ready_every iterations a round (pbt_decide through a
  PBTController) on the mean return of the episodes each member finished since the last round; each of the bottom `truncation` share
  becomes a copy of a member of the top share (trainer.copy_members: images, targets, Adam moments, lr and kappa -- NOT the replay
  contents, which stay the columns' own, and not the seeds) with its lr multiplied by one of the two `perturb` factors
  (trainer.scale_hyper).  truncation = 0, the default, is a plain P-seed study.  controller: a PBTController to continue.

  exploration: None, or a marco_polo.VecPopulationMarcoPoloExploration(P, R, ...) with run_training_loop_vec's semantics
  (configs/quantile.gin for a population: with epsilon=0.0 and a qnet_train.VecPopulationPrioritizedReplayBuffer).  After the greedy
  actions and the grouped epsilon-greedy (at rate 0 it changes nothing; its draws are addressed, not consumed) the explorer rewrites the
  actions; its begin mask is all ones at the first step and the previous step's episode_end after; the replay stores the action taken.
  Priorities and the explorer's state belong to the columns: a PBT round copies neither.

  Returns run_training_loop_vec's dicts (mean_loss: the mean over all members' rows; transitions: all members') plus, as lists of P,
  member_mean_loss, member_mean_return and member_episodes (this iteration's), lr, and with a controller lineage and round
  ({'fitness', 'src', 'dst'} as lists on a round's iteration, else None).  One host synchronisation per iteration: its end."""
  n, dev_ = env.num_envs, env.device
  p, r = replay.members, replay.rows_per_member
  assert trainer.members == p and replay.num_envs == n == p * r, 'the replay ring has one column per environment, R per member'
  pbt = controller
  if pbt is None and ready_every is not None:
    pbt = PBTController(p, dev_, ready_every=ready_every, truncation=truncation, perturb=perturb, explore=('lr',), seed=seed)
  sync_every = max(1, target_update_period // update_period)
  ladder = None if callable(epsilon) else torch.from_numpy(qnet_train._epsilons(epsilon, p)).to(dev_)
  obs = env.reset()
  actions = torch.zeros(n, dtype=torch.uint8, device=dev_)
  book = _EpisodeBook(n, dev_, max_episode_length)
  zero = torch.zeros((), dtype=torch.float32, device=dev_)
  begin = torch.ones(n, dtype=torch.uint8, device=dev_) if exploration is not None else None
  updates, pending, step, member_transitions = 0, 0.0, 0, 0
  captured = False
  stats = []
  for _ in range(num_iterations):
    it_sum = torch.zeros(p, dtype=torch.float32, device=dev_)
    it_episodes = torch.zeros(p, dtype=torch.int64, device=dev_)
    it_loss = torch.zeros(p, dtype=torch.float32, device=dev_)
    for _ in range(steps_per_iteration):
      trainer.act(obs, actions)
      qnet_train.explore_grouped(actions, epsilon(member_transitions) if ladder is None else ladder, trainer.seeds, step)
      if exploration is not None:
        exploration(obs, actions, begin)
      end_mask = book.end_mask()
      next_obs, reward, terminal = env.step(actions, end_mask=end_mask)
      episode_end = terminal | end_mask
      if exploration is not None:
        begin.copy_(episode_end)
      replay.add(obs, actions, reward, terminal, episode_end)
      ended = episode_end.bool().view(p, r)
      ended_returns = torch.where(ended, (book.ep_return + reward).view(p, r), zero)
      if pbt is not None:
        pbt.step(ended_returns, ended)
      it_sum += ended_returns.sum(dim=1)
      it_episodes += ended.sum(dim=1)
      book.step(reward, episode_end)
      obs = next_obs
      step += 1
      member_transitions += r
      if member_transitions >= min_replay_history and replay.cursor > replay.update_horizon:
        if updates_per_step is not None:
          todo = int(updates_per_step)
        else:
          pending += r / update_period
          todo = int(pending)
          pending -= todo
        for _ in range(todo):
          if capture_graph and not captured:
            loss = trainer.capture(replay, batch_size)        # (its first, eager update is a real one)
            captured = True
          else:
            loss = trainer.train_step(replay, batch_size)
          book.update(loss)
          it_loss += loss.view(p, -1).mean(dim=1)
          updates += 1
          if updates % sync_every == 0:
            trainer.sync_target()
    rnd = pbt.end_iteration(trainer) if pbt is not None else None
    env.check_errors()
    replay.check_errors()
    trainer.check_errors()
    done = book.updates
    s = book.finish_iteration(steps_per_iteration)
    eps = it_episodes.tolist()
    s['member_mean_loss'] = [v / max(done, 1) for v in it_loss.tolist()]
    s['member_episodes'] = eps
    s['member_mean_return'] = [v / e if e else float('nan') for v, e in zip(it_sum.tolist(), eps)]
    s['lr'] = trainer.lr.tolist()
    if pbt is not None:
      s['lineage'] = pbt.lineage.tolist()
      s['round'] = None if rnd is None else {k: v.tolist() for k, v in rnd.items()}
    stats.append(s)
  return stats


def run_dagger_loop_vec(env, trainer, expert, rollout, *, num_iterations: int, beta: Union[float, Callable[[int], float]], epochs: int = 1,
                        batch_size: int, max_episode_length: int = 960, gamma: float = 0.993, lam: float = 0.95,
                        capture_graph: bool = True) -> List[dict]:
  """Clones `expert` into an imitation learner (agents/imitation.py: BCTrainer with a VecRolloutBuffer of T steps) on `env`
  (auto_reset) by DAgger.  expert: anything with act(obs, out) -- VecStationSeekerAgent, a venv.planner(...) bound to env's simulator
  (it plans from the state, so its labels are on the states visited), VecQNetworkAgent, VecActorCriticAgent.  Each step the learner
  samples its action, the expert labels the same observation, and the action flown is the expert's with probability beta_i (drawn per
  environment and step, trainer.mix), else the learner's; the block stores the label, not the action flown.  beta: a float or a
  function of the iteration index (a common choice: lambda i: 0.5 ** i).  The episode limit is run_training_loop_vec's.

  After the T steps one more act gives the bootstrap value, rollout.finish(value, gamma, lam, normalize=False) gives ret, the
  lambda-return of the policy flown (the value target under trainer.value_coef), and `epochs` passes of minibatches of batch_size rows
  follow, each one update; then the block is discarded.

  Returns run_training_loop_vec's dicts plus agreement (the mean over the iteration's updates of the fraction of rows whose greedy
  action is the label) and expert_share (the fraction of the block's actions that were the expert's).  The only host synchronisation is
  the end of an iteration."""
  n, dev_ = env.num_envs, env.device
  assert rollout.num_envs == n, 'the rollout block has one column per environment'
  steps = rollout.horizon
  obs = env.reset()
  learner = torch.zeros(n, dtype=torch.uint8, device=dev_)
  label = torch.zeros(n, dtype=torch.uint8, device=dev_)
  actions = torch.zeros(n, dtype=torch.uint8, device=dev_)
  took = torch.zeros(n, dtype=torch.uint8, device=dev_)
  logp = torch.zeros(n, dtype=torch.float32, device=dev_)
  value = torch.zeros(n, dtype=torch.float32, device=dev_)
  book = _EpisodeBook(n, dev_, max_episode_length)
  captured = False
  stats = []
  for it in range(num_iterations):
    beta_i = float(beta(it) if callable(beta) else beta)
    took_sum = torch.zeros((), dtype=torch.int64, device=dev_)
    agree_sum = torch.zeros((), dtype=torch.float32, device=dev_)
    for t in range(steps):
      trainer.act(obs, learner, logp, value)
      expert.act(obs, label)
      trainer.mix(learner, label, beta_i, actions, took)
      end_mask = book.end_mask()
      next_obs, reward, terminal = env.step(actions, end_mask=end_mask)
      episode_end = terminal | end_mask
      rollout.add(t, obs, label, logp, value, reward, terminal, episode_end)
      book.step(reward, episode_end)
      took_sum += took.sum()
      obs = next_obs
    trainer.act(obs, learner, logp, value)
    rollout.finish(value, gamma, lam, normalize=False)
    for _ in range(epochs):
      for batch in rollout.minibatches(batch_size):
        if capture_graph and not captured:
          loss = trainer.capture(batch)                     # (its first, eager update is a real one)
          captured = True
        else:
          loss = trainer.train_step(batch)
        book.update(loss)
        agree_sum += trainer.views(batch_size)['aux'][:, 1].mean()
    env.check_errors()
    trainer.check_errors()
    if hasattr(expert, 'check_errors'):
      expert.check_errors()
    updates = book.updates
    s = book.finish_iteration(steps)
    s['agreement'] = float(agree_sum.item()) / max(updates, 1)
    s['expert_share'] = float(took_sum.item()) / (n * steps)
    stats.append(s)
  return stats


def run_exit_loop_vec(env, trainer, planner, buffer, *, num_iterations: int, beta: Union[float, Callable[[int], float]], epochs: int,
                      batch_size: int, max_episode_length: int = 960, capture_graph: bool = True) -> List[dict]:
  """Expert iteration of a soft-target learner (agents/expert_iteration.py: SoftBCTrainer with a VecPlanLabelBuffer of T
  steps) and a planner (a venv.planner(prior_strength=..., action_values=True) bound to env's simulator) on `env` (auto_reset).  Each
  step, in this order: the learner samples its action on the observation and gives its probabilities (trainer.act(..., probs=));
  the planner decides on the same observation with those probabilities as its prior (planner.act(obs, label, prior_probs=probs)); the
  action flown is the planner's with probability beta_i, else the learner's (trainer.mix, the DAgger mixture); env.step; the block
  stores the observation acted on, the planner's per-action values and its best return there (buffer.add(t, obs, q, best_return)).
  beta: a float or a function of the iteration index.  The episode limit is run_training_loop_vec's.
  With a bootstrapped planner (VecLookaheadAgent(leaf_value=)) nothing here changes, but the stored best return -- the
  value target under value_coef -- is then an H-step BOOTSTRAPPED return, sum_{t<H} gamma^t r_t + gamma^H V(s_H), and so are the
  per-action values; with leaf_value=trainer the target moves with the learner's own value column.
  A beam-search planner (venv.planner(search='beam', action_values=True)) serves as `planner` as well: the loop uses its
  act, action_values and plan alone; it takes the prior and ignores it.

  After the T steps `epochs` passes of minibatches of batch_size rows follow, each one soft update (epochs x (T N // batch_size) in
  all); then the block is discarded.

  Returns run_training_loop_vec's dicts plus loss (mean_loss under the issue's name), agreement (the mean over the iteration's updates
  of the fraction of rows whose greedy action is the best-valued one), expert_share (the fraction of the block's actions that were the
  planner's) and mean_best_return (the mean over the block of the planner's finite best returns).  The only host synchronisation is the
  end of an iteration."""
  n, dev_ = env.num_envs, env.device
  assert buffer.num_envs == n, 'the label block has one column per environment'
  steps = buffer.horizon
  obs = env.reset()
  learner = torch.zeros(n, dtype=torch.uint8, device=dev_)
  label = torch.zeros(n, dtype=torch.uint8, device=dev_)
  actions = torch.zeros(n, dtype=torch.uint8, device=dev_)
  took = torch.zeros(n, dtype=torch.uint8, device=dev_)
  logp = torch.zeros(n, dtype=torch.float32, device=dev_)
  value = torch.zeros(n, dtype=torch.float32, device=dev_)
  probs = torch.zeros(n, 3, dtype=torch.float32, device=dev_)
  book = _EpisodeBook(n, dev_, max_episode_length)
  captured = False
  stats = []
  for it in range(num_iterations):
    beta_i = float(beta(it) if callable(beta) else beta)
    took_sum = torch.zeros((), dtype=torch.int64, device=dev_)
    agree_sum = torch.zeros((), dtype=torch.float32, device=dev_)
    best_sum = torch.zeros((), dtype=torch.float32, device=dev_)
    best_count = torch.zeros((), dtype=torch.int64, device=dev_)
    for t in range(steps):
      trainer.act(obs, learner, logp, value, probs)
      planner.act(obs, label, prior_probs=probs)
      trainer.mix(learner, label, beta_i, actions, took)
      end_mask = book.end_mask()
      next_obs, reward, terminal = env.step(actions, end_mask=end_mask)
      episode_end = terminal | end_mask
      q, _ = planner.action_values()
      _, best_return = planner.plan()
      buffer.add(t, obs, q, best_return)
      book.step(reward, episode_end)
      took_sum += took.sum()
      finite = torch.isfinite(best_return)
      best_sum += torch.where(finite, best_return, torch.zeros_like(best_return)).sum()
      best_count += finite.sum()
      obs = next_obs
    for _ in range(epochs):
      for batch in buffer.minibatches(batch_size):
        if capture_graph and not captured:
          loss = trainer.capture(batch)                     # (its first, eager update is a real one)
          captured = True
        else:
          loss = trainer.train_step(batch)
        book.update(loss)
        agree_sum += trainer.views(batch_size)['aux'][:, 1].mean()
    env.check_errors()
    trainer.check_errors()
    if hasattr(planner, 'check_errors'):
      planner.check_errors()
    updates = book.updates
    s = book.finish_iteration(steps)
    s['loss'] = s['mean_loss']
    s['agreement'] = float(agree_sum.item()) / max(updates, 1)
    s['expert_share'] = float(took_sum.item()) / (n * steps)
    count = int(best_count.item())
    s['mean_best_return'] = float(best_sum.item()) / count if count else float('nan')
    stats.append(s)
  return stats


def run_es_loop_vec(trainer, *, num_generations: int, seeds_per_member: int, max_episode_length: int = 960, first_seed: int = 0,
                    wind_field=None, wind_noise: bool = True, eval_center_every: int = 0, head: str = 'q') -> List[dict]:
  """The loop of an evolution strategy (agents/evolution.py's ESTrainer) over seeded evaluation flights.  Per generation g: perturb;
  one VecEvaluator flight of P * S rows -- row p S + s flies seed first_seed + g S + s under member p, so every member flies the same
  fresh seeds; fitness[p] = the mean of member p's cumulative rewards (float64 on the device, then float32); update.  The host
  synchronises once per generation, for its dict: mean_fitness, max_fitness, min_fitness, transitions (the steps flown so far) and,
  every eval_center_every generations, center_score: the greedy centre's mean cumulative reward on the generation's seeds; fitness: the
  float32 [P] device tensor the update was given."""
  from balloon_learning_environment_amd.agents import population as population_lib
  from balloon_learning_environment_amd.agents import qnet
  from balloon_learning_environment_amd.eval import eval_lib
  from balloon_learning_environment_amd.eval import suites
  pop = trainer.population
  members, per = pop.members, int(seeds_per_member)
  assert num_generations >= 0 and per >= 1
  agent = population_lib.VecPopulationAgent(pop, per, head=head)
  ev = eval_lib.VecEvaluator(members * per, agent, max_episode_length, wind_field=wind_field, wind_noise=wind_noise,
                             device=trainer.device)
  stats, transitions = [], 0
  for g in range(num_generations):
    seeds = [first_seed + g * per + s for s in range(per)]
    trainer.perturb()
    ev.launch(seeds * members)
    fitness = ev.cumulative_reward.view(members, per).mean(dim=1).to(torch.float32)
    trainer.update(fitness)
    flown = ev.final_timestep.sum()
    row = {'mean_fitness': float(fitness.mean().item()), 'max_fitness': float(fitness.max().item()),
           'min_fitness': float(fitness.min().item())}
    transitions += int(flown.item())
    row['transitions'] = transitions
    ev.sim.check_errors()
    if eval_center_every and (g + 1) % eval_center_every == 0:
      center = trainer.network()
      if head == 'actor':
        from balloon_learning_environment_amd.agents import actor_critic
        center_agent = actor_critic.VecActorCriticAgent(center, deterministic=True)
      else:
        center_agent = qnet.VecQNetworkAgent(center)
      flights = eval_lib.eval_agent_vec(center_agent, suites.EvaluationSuite(seeds, max_episode_length), wind_field=wind_field,
                                        wind_noise=wind_noise, device=trainer.device)
      row['center_score'] = sum(f.cumulative_reward for f in flights) / len(flights)
    row['fitness'] = fitness.clone()
    stats.append(row)
  return stats
