"""Imitation on the device: behaviour cloning of an actor-critic and the DAgger mixture (csrc/ble_imitate.h).

`BCTrainer` fits the two-atom actor-critic of agents/actor_critic.py to an expert's labels: one smoothed cross-entropy update per
minibatch (`ble_qnet_bc_step_f32`: the forward, backward and Adam of the other learners behind a fifth loss head), capturable as one
graph.  Its `mix` draws, per environment and step, whether the expert's or the learner's action is flown (`ble_dagger_mix_u8`), so that
the labels are gathered on the states the learner itself reaches; train_lib.run_dagger_loop_vec is the loop.  The expert is anything
with act(obs, out): VecStationSeekerAgent, a venv.planner(...), VecQNetworkAgent, VecActorCriticAgent.  What comes out is a QNetwork:
`PPOTrainer(bc_trainer.network())` fine-tunes it on-policy, eval_agent_vec evaluates it.

There is no agent_registry entry: the reference has no imitation agent, as it has no on-policy one (agents/actor_critic.py).  No
floating-point atomics and every reduction in an order fixed by the shapes: a run is a pure function of (initial parameters, data,
seeds).
"""
import ctypes
from typing import Dict, Optional

import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd.agents import actor_critic
from balloon_learning_environment_amd.agents import qnet
from balloon_learning_environment_amd.agents import qnet_train

NUM_ATOMS = actor_critic.NUM_ATOMS


class BCTrainer(qnet_train.QNetworkLearner):
  """Behaviour cloning of an actor-critic's parameters on its device.

    trainer = BCTrainer(qnet.QNetwork.from_params(actor_critic.init_params('actor_critic'), num_atoms=2))
    train_lib.run_dagger_loop_vec(env, trainer, expert, VecRolloutBuffer(env.num_envs, 32), num_iterations=..., beta=lambda i: 0.5 ** i,
                                  batch_size=4096)
    policy = trainer.network()                     # a QNetwork: VecActorCriticAgent, eval_agent_vec, PPOTrainer, save_npz

  label_smoothing s in [0, 1): the target is (1 - s) on the label plus s / 3 on every action.  value_coef: the weight of
  (value - batch.ret)^2; 0 (the default) leaves the value column untrained and reads no ret."""

  _TENSORS = ('weights', 'adam_m', 'adam_v', 'adam_step', 'act_step', 'mix_step')

  def __init__(self, network: qnet.QNetwork, *, lr: float = 3e-4, eps: float = 1e-5, label_smoothing: float = 0.0,
               value_coef: float = 0.0, seed: int = 0, b1: float = 0.9, b2: float = 0.999):
    actor_critic._require_actor_critic(network, 'BCTrainer')      # pylint: disable=protected-access
    if not 0.0 <= float(label_smoothing) < 1.0:
      raise ValueError('label_smoothing lies in [0, 1)')
    super().__init__(network)
    self.lr, self.eps, self.b1, self.b2 = float(lr), float(eps), float(b1), float(b2)
    self.label_smoothing, self.value_coef, self.seed = float(label_smoothing), float(value_coef), int(seed)
    d = self.device
    with torch.cuda.device(d):
      self.adam_m = torch.zeros_like(self.weights)
      self.adam_v = torch.zeros_like(self.weights)
      self.adam_step = torch.zeros(1, dtype=torch.int64, device=d)
      self.mix_step = torch.zeros(1, dtype=torch.int64, device=d)      # (read as uint64 by the kernel)
    self._sampler = actor_critic._Sampler(self.seed, d)      # pylint: disable=protected-access
    self.act_step = self._sampler.step
    self._actor = actor_critic.ActorForward(self._net, d, 'BCTrainer')
    self._ws: Dict[int, tuple] = {}

  workspace = qnet_train.QNetworkTrainer.workspace

  def views(self, batch_size: int) -> dict:
    """The workspace's tensors of the last update at this batch size (PPOTrainer.views' layout): 'acts', 'logits' [B, 6], 'aux'
    [B, 2] (the label's log-probability; agree: 1.0 where the greedy action is the label), 'dlogits' [B, ld], 'loss' [B]."""
    return actor_critic.PPOTrainer.views(self, batch_size)

  # ---- acting
  @dev.on_own_device
  def act(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None, logp: Optional[torch.Tensor] = None,
          value: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sampled actions of the live image (VecActorCriticAgent.act's contract); the device step counter advances after each call."""
    self._sampler.seed = self.seed
    out = self._actor(obs, out, logp, value, probs, self._sampler.struct())
    if obs.shape[0]:
      self.act_step.add_(1)
    return out

  @dev.on_own_device
  def act_greedy(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None, logp: Optional[torch.Tensor] = None,
                 value: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Greedy actions of the live image; the step counter stays."""
    return self._actor(obs, out, logp, value, probs, None)

  # ---- the DAgger mixture
  @dev.on_own_device
  def mix(self, learner_actions: torch.Tensor, expert_actions: torch.Tensor, beta: float, out: Optional[torch.Tensor] = None,
          took_expert: Optional[torch.Tensor] = None, env_offset: int = 0) -> torch.Tensor:
    """out[i] = the expert's action with probability beta, else the learner's, drawn per (seed, environment env_offset + i, mix_step);
    took_expert (optional uint8 [N]) records the draw.  out may be learner_actions.  mix_step, a device counter, advances after each
    call (a device add: part of the captured work).  No host synchronisation."""
    n = learner_actions.numel()
    if out is None:
      out = torch.empty(n, dtype=torch.uint8, device=self.device)
    for t in (learner_actions, expert_actions, out, took_expert):
      if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() != n or t.device != self.device):
        raise ValueError('mix: learner, expert, out and took_expert are contiguous uint8 tensors of one length on the trainer\'s device')
    if not 0.0 <= float(beta) <= 1.0:
      raise ValueError('mix: beta lies in [0, 1]')
    m = _abi.BleDaggerMixF32(n, float(beta), 0, self.seed & (2 ** 64 - 1), int(env_offset), self.mix_step.data_ptr(),
                             learner_actions.data_ptr(), expert_actions.data_ptr(), out.data_ptr(), dev.ptr(took_expert))
    _lib.call('ble_dagger_mix_u8', ctypes.byref(m), dev.stream_ptr(self.device))
    if n:
      self.mix_step.add_(1)
    return out

  # ---- the update
  def _bc(self) -> _abi.BleBcF32:
    return _abi.BleBcF32(self.label_smoothing, self.value_coef, 0)

  @dev.on_own_device
  def train_on_batch(self, batch, apply_update: bool = True) -> torch.Tensor:
    """One update on a minibatch whose action column holds the expert's labels: the per-row losses [B] (a view of a buffer the next
    update at this size overwrites).  batch: a PPOBatch (old_logp and advantage are ignored; ret is the value target under
    value_coef), or a TrainBatch a VecReplayBuffer of update_horizon 1 sampled (its ret is a reward: value_coef must be 0)."""
    if self.value_coef != 0.0 and getattr(batch, 'next_state', None) is not None:
      raise ValueError('BCTrainer: a replay batch carries rewards, not value targets, in ret: value_coef must be 0 with it')
    ws, _, loss = self.workspace(batch.batch_size)
    tr, bc = self._struct(ws, apply_update), self._bc()
    _lib.call('ble_qnet_bc_step_f32', ctypes.byref(tr), ctypes.byref(bc), ctypes.byref(batch.struct), loss.data_ptr(),
              self.err_flags.data_ptr(), dev.stream_ptr(self.device))
    return loss[:batch.batch_size]

  def train_step(self, batch) -> torch.Tensor:
    """train_on_batch, by the captured graph of this batch's buffers when there is one (capture())."""
    g = self._graphs.get(batch.batch_size)
    if g is not None and g[1] is batch:
      g[0].replay()
      return g[2]
    return self.train_on_batch(batch)

  def capture(self, batch) -> torch.Tensor:
    """Records one minibatch update on `batch`'s static buffers into a HIP graph that train_step(batch) replays from then on.  Runs
    one eager update first (the lazy allocations) -- that is a real update; returns its per-row losses."""
    first = self.train_on_batch(batch)
    graph, loss = dev.capture(self.device, lambda: self.train_on_batch(batch))
    self._graphs[batch.batch_size] = (graph, batch, loss)
    return first

  # ---- checkpoints
  def _hyper(self) -> tuple:
    return (self.lr, self.eps, self.b1, self.b2, self.label_smoothing, self.value_coef)

  def state_dict(self) -> dict:
    return {**super().state_dict(), 'hyper': self._hyper()}

  def load_state_dict(self, d: dict) -> None:
    hyper = tuple(d['hyper'])
    if int(d['seed']) != self.seed or hyper != self._hyper():
      self._graphs.clear()                     # (the seed and hyperparameters are arguments of the captured launches)
    self.lr, self.eps, self.b1, self.b2, self.label_smoothing, self.value_coef = hyper
    super().load_state_dict(d)
