"""Expert iteration on the device: the learner's policy biases where the planner searches, and the planner's per-action
plan returns become the learner's soft targets.

`SoftBCTrainer` fits the two-atom actor-critic of agents/actor_critic.py to per-action values q [B, 3]: one soft cross-entropy update per
minibatch against softmax(q / temperature) over the actions that have a finite value (`ble_qnet_soft_bc_step_f32`: imitation.BCTrainer's
update behind a sixth loss head), capturable as one graph.  `VecPlanLabelBuffer` holds T steps of N environments of (observation, q,
return) and hands out shuffled minibatches.  train_lib.run_exit_loop_vec is the loop; the planner is a
`VecLookaheadAgent(prior_strength=..., action_values=True)`.  With exactly one finite value per row the update is BCTrainer's on that
label, bit for bit.  `VecPriorPlannerAgent` is a policy and a planner as one device agent: the policy's probabilities are the planner's
prior at every decision (eval_lib.eval_agent_vec takes it).

There is no agent_registry entry: the reference has no such agent.  No floating-point atomics and every reduction in an order fixed by
the shapes: a run is a pure function of (initial parameters, data, seeds).
"""
import ctypes
from typing import Dict, Iterator, Optional

import numpy as np
import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd.agents import actor_critic
from balloon_learning_environment_amd.agents import imitation
from balloon_learning_environment_amd.agents import qnet
from balloon_learning_environment_amd.agents import qnet_train

ROW_FLOATS = qnet_train.ROW_FLOATS
NUM_ACTIONS = qnet.NUM_ACTIONS


class SoftBatch(qnet_train.TrainBatch):
  """One minibatch of B rows with soft targets (static device buffers): TrainBatch's state and ret (the value target R), and target_q
  [B, 3]; no action, next_state, discount or index."""

  def __init__(self, batch_size: int, device):      # pylint: disable=super-init-not-called
    b = int(batch_size)
    self.batch_size = b
    self.state = torch.zeros(b, ROW_FLOATS, dtype=torch.float32, device=device)
    self.ret = torch.zeros(b, dtype=torch.float32, device=device)
    self.target_q = torch.zeros(b, NUM_ACTIONS, dtype=torch.float32, device=device)
    self.action = self.next_state = self.discount = self.index = self.priority = self.weighted_loss = None
    self.struct = _abi.BleTrainBatchF32(b, ROW_FLOATS, self.state.data_ptr(), None, self.ret.data_ptr(), None, None, None)

  @classmethod
  def from_tensors(cls, state, target_q, ret, device) -> 'SoftBatch':      # pylint: disable=arguments-differ
    """A batch given on the host or device (state rows of 1099 features); for tests and offline data."""
    bt = cls(len(target_q), device)
    bt.state[:, :_lib.OBS_DIM].copy_(torch.as_tensor(np.asarray(state, np.float32)))
    bt.target_q.copy_(torch.as_tensor(np.asarray(target_q, np.float32)))
    bt.ret.copy_(torch.as_tensor(np.asarray(ret, np.float32)))
    return bt


class SoftBCTrainer(imitation.BCTrainer):
  """Soft-target cloning of an actor-critic's parameters on its device.

    trainer = SoftBCTrainer(qnet.QNetwork.from_params(actor_critic.init_params('actor_critic'), num_atoms=2), temperature=0.5)
    planner = env.planner(num_plans=16, prior_strength=64, action_values=True)
    train_lib.run_exit_loop_vec(env, trainer, planner, VecPlanLabelBuffer(env.num_envs, 32), num_iterations=..., beta=0.5, epochs=1,
                                batch_size=4096)
    policy = trainer.network()                     # a QNetwork: VecActorCriticAgent, eval_agent_vec, PPOTrainer, save_npz

  temperature > 0: the target is softmax(q / temperature) over the actions whose q is finite (an action no plan took has none and gets
  probability 0; a row without any finite q trains nothing).  label_smoothing s in [0, 1): the target becomes (1 - s) of that plus
  s / 3 on every action.  value_coef: the weight of (value - batch.ret)^2; 0 (the default) leaves the value column untrained and reads
  no ret.  act, act_greedy, mix, views, capture, train_step, network and state_dict are BCTrainer's."""

  def __init__(self, network: qnet.QNetwork, *, temperature: float = 1.0, label_smoothing: float = 0.0, value_coef: float = 0.0, **kw):
    if not (float(temperature) > 0.0 and np.isfinite(float(temperature))):
      raise ValueError('temperature is finite and above 0')
    super().__init__(network, label_smoothing=label_smoothing, value_coef=value_coef, **kw)
    self.temperature = float(temperature)

  def views(self, batch_size: int) -> dict:
    """BCTrainer.views' layout; 'aux' [B, 2] holds the log-probability of the row's best-valued action a* and agree: 1.0 where the
    greedy action is a*."""
    return super().views(batch_size)

  def _soft(self, batch: SoftBatch) -> _abi.BleSoftBcF32:
    return _abi.BleSoftBcF32(1.0 / self.temperature, self.label_smoothing, self.value_coef, 0, batch.target_q.data_ptr())

  @dev.on_own_device
  def train_on_batch(self, batch: SoftBatch, apply_update: bool = True) -> torch.Tensor:
    """One update on a minibatch with target_q [B, 3]: the per-row losses [B] (a view of a buffer the next update at this size
    overwrites)."""
    ws, _, loss = self.workspace(batch.batch_size)
    tr, soft = self._struct(ws, apply_update), self._soft(batch)
    _lib.call('ble_qnet_soft_bc_step_f32', ctypes.byref(tr), ctypes.byref(soft), ctypes.byref(batch.struct), loss.data_ptr(),
              self.err_flags.data_ptr(), dev.stream_ptr(self.device))
    return loss[:batch.batch_size]

  # ---- checkpoints
  def _hyper(self) -> tuple:
    return (self.lr, self.eps, self.b1, self.b2, self.label_smoothing, self.value_coef, self.temperature)

  def load_state_dict(self, d: dict) -> None:
    hyper = tuple(d['hyper'])
    if int(d['seed']) != self.seed or hyper != self._hyper():
      self._graphs.clear()                     # (the seed and hyperparameters are arguments of the captured launches)
    self.lr, self.eps, self.b1, self.b2, self.label_smoothing, self.value_coef, self.temperature = hyper
    qnet_train.QNetworkLearner.load_state_dict(self, d)


class VecPlanLabelBuffer:
  """T steps of N environments stepped in lockstep, on the device: obs [T, N, ROW_FLOATS], target_q [T, N, 3] (the planner's per-action
  values on that observation) and ret [T, N] (the planner's best return there: the value target under value_coef).

  add(t, obs, target_q, ret) copies one vector step; minibatches(B, generator) follows VecRolloutBuffer.minibatches' contract: one
  SoftBatch object refilled for every minibatch by index_select over a torch.randperm of the T N rows (distinct rows per pass, a trailing
  partial minibatch dropped), drawn from the buffer's generator or the one given, whose state a state_dict restores.  No call
  synchronises with the host."""

  _TENSORS = ('obs', 'target_q', 'ret')

  def __init__(self, num_envs: int, horizon: int, device='cuda:0'):
    self.device = d = dev.require_gpu(device)
    self.num_envs, self.horizon = int(num_envs), int(horizon)
    if self.num_envs < 1 or self.horizon < 1:
      raise ValueError('num_envs and horizon must be at least 1')
    t, n = self.horizon, self.num_envs
    with torch.cuda.device(d):
      self.obs = torch.zeros(t, n, ROW_FLOATS, dtype=torch.float32, device=d)
      self.target_q = torch.zeros(t, n, NUM_ACTIONS, dtype=torch.float32, device=d)
      self.ret = torch.zeros(t, n, dtype=torch.float32, device=d)
      self.generator = torch.Generator(device=d)
    self.generator.manual_seed(0)
    self._batches: Dict[int, SoftBatch] = {}

  @dev.on_own_device
  def add(self, t: int, obs: torch.Tensor, target_q: torch.Tensor, ret: torch.Tensor) -> None:
    """Step t of the block: obs is the observation the planner decided on, target_q [N, 3] and ret [N] what it found there."""
    self.obs[t, :, :_lib.OBS_DIM].copy_(obs[:, :_lib.OBS_DIM])
    self.target_q[t].copy_(target_q)
    self.ret[t].copy_(ret)

  def batch_buffers(self, batch_size: int) -> SoftBatch:
    return dev.first_use(self._batches, batch_size, lambda: SoftBatch(batch_size, self.device),
                         f'VecPlanLabelBuffer: draw minibatches once at batch size {batch_size} before capturing an update')

  @dev.on_own_device
  def minibatches(self, batch_size: int, generator: Optional[torch.Generator] = None) -> Iterator[SoftBatch]:
    """One pass over the block in a random order: the same SoftBatch buffers, refilled for every minibatch."""
    b, m = int(batch_size), self.horizon * self.num_envs
    bt = self.batch_buffers(b)
    perm = torch.randperm(m, device=self.device, generator=self.generator if generator is None else generator)
    flat = {'state': self.obs.view(m, ROW_FLOATS), 'target_q': self.target_q.view(m, NUM_ACTIONS), 'ret': self.ret.view(m)}
    for k in range(m // b):
      idx = perm[k * b:(k + 1) * b]
      for name, src in flat.items():
        torch.index_select(src, 0, idx, out=getattr(bt, name))
      yield bt

  def state_dict(self) -> dict:
    return {'num_envs': self.num_envs, 'horizon': self.horizon, 'generator': self.generator.get_state().clone(),
            **{k: getattr(self, k).clone() for k in self._TENSORS}}

  def load_state_dict(self, d: dict) -> None:
    assert (d['num_envs'], d['horizon']) == (self.num_envs, self.horizon)
    for k in self._TENSORS:
      getattr(self, k).copy_(d[k])
    self.generator.set_state(d['generator'])


class VecPriorPlannerAgent:
  """A planner that searches where a policy points: act(obs) runs the actor-critic `policy` (a VecActorCriticAgent, or a trainer with
  act_greedy) for its probabilities and hands them to `planner` (a VecLookaheadAgent built with prior_strength > 0) as its prior.  An
  agent like any other device agent: eval_lib.VecEvaluator binds it to its simulator and may capture it in a graph.  The same network
  can serve twice: as `policy` here and as the planner's leaf_value (VecLookaheadAgent(leaf_value=policy)) -- its policy head
  biases where the planner searches, its value head scores where the plans end.  A VecBeamSearchAgent is accepted as
  `planner` too: it takes prior_probs and ignores them (a beam search has no prior), so the pair then acts as the beam search alone."""

  def __init__(self, policy, planner):
    self.policy, self.planner = policy, planner
    self.device = planner.device
    self._probs: Optional[torch.Tensor] = None

  def bind(self, sim, seeds: Optional[torch.Tensor] = None, noise_seed=None) -> 'VecPriorPlannerAgent':
    self.planner.bind(sim, seeds=seeds, noise_seed=noise_seed)
    if self._probs is None or self._probs.shape[0] != sim.n:
      self._probs = torch.zeros(sim.n, NUM_ACTIONS, dtype=torch.float32, device=self.device)
    return self

  @dev.on_own_device
  def act(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if self._probs is None:
      raise ValueError('VecPriorPlannerAgent.act before bind(sim)')
    policy_act = getattr(self.policy, 'act_greedy', None) or self.policy.act
    policy_act(obs, probs=self._probs)
    return self.planner.act(obs, out, prior_probs=self._probs)

  __call__ = act

  def check_errors(self) -> None:
    self.planner.check_errors()

  def get_name(self) -> str:
    return 'PriorLookaheadAgent'
