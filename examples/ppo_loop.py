#!/usr/bin/env python3
"""The loop of the reference's trainer (rl/train.py:58-130: act -> envs.step -> bookkeeping -> insert ->
compute_returns -> PPO epochs) with every environment-side piece on the device:

    envs     SFVecNormalize(SFVecEnv(...))       <- VecNormalize(SubprocVecEnv([...]))     rl/train.py:30-36
    rollouts DeviceRollout(envs, T)              <- RolloutStorage + the per-step bookkeeping rl/train.py:41,79-98

The actor-critic below is a stand-in (two tanh layers, like rl/model.py's MLP branch) so that the script is
self-contained; the point is the data path: nothing crosses PCIe inside an iteration.

    python examples/ppo_loop.py --envs 4096 --iters 20

--obs image runs the same loop on 84x84 frames, four to a stack (rl/train.py:38-41), over FrameRollout: every frame is kept
once, the actor reads the current stack that step() returns and the minibatches are gathered as float32 by one launch each.

    python examples/ppo_loop.py --obs image --envs 1024 --steps 32 --iters 5

--time-limit-bootstrap: every episode of this game ends by the clock, so `done` is a truncation; the rollout keeps each env's
final observation (image: its final stack of frames, include/sfmi_final.h) and the returns bootstrap with the critic's value of
it instead of 0 -- one more critic forward per update (DeviceRollout / FrameRollout(time_limit_bootstrap=True), INTEGRATION.md
"Episodes end by the clock").  Not with --frame-skip > 1 on images.

    python examples/ppo_loop.py --time-limit-bootstrap --envs 256 --steps 16 --iters 2
    python examples/ppo_loop.py --obs image --time-limit-bootstrap --envs 256 --steps 16 --iters 2

--frame-skip K: every action is played for K ticks by one launch (SFVecEnv(frame_skip=K), include/sfmi_repeat.h); rewards are
summed over the window, an env that finishes inside it stops there, an image batch draws one frame per action.  Default 1.

    python examples/ppo_loop.py --obs image --frame-skip 4 --envs 1024 --steps 32 --iters 5

--device-policy-head: the step between the network and the env -- Categorical(logits).sample(), log_prob, unsqueeze and two
copies into the rollout, about ten small launches -- becomes ONE launch (PolicyHead, include/sfmi_policy.h): the loop hands the
network's logits to rollout.step_logits, which draws the actions on the device, writes their log-probabilities straight into the
rollout and keeps the rows' entropies (the log line prints their mean).  The PPO update then runs its loss head on the device
as well: ppo_loss (include/sfmi_ppo.h) evaluates the minibatch's actions with the sampling head's own arithmetic, builds the
clipped surrogate, the value loss and the entropy bonus in two launches and their gradients in one, and the log line prints the
last minibatch's losses.  Off by default: without the flag the loop is torch.distributions all the way.

    python examples/ppo_loop.py --device-policy-head --envs 4096 --iters 20

--device-minibatches: the stretch between compute_returns and the loss on the device as well (include/sfmi_minibatch.h): the
normalised advantages are rollout.advantages() -- three launches with a fixed arithmetic instead of six of torch's -- and every
minibatch is ONE gather launch into buffers that are made once (rollout.minibatches(..., reuse=True)) instead of seven indexing
launches into fresh tensors.

    python examples/ppo_loop.py --device-policy-head --device-minibatches --envs 4096 --iters 20

--graph-update (features only; implies the two flags above): one minibatch update -- MiniBatcher.next() -> the network ->
ppo_loss -> backward -> Adam(capturable=True) -- is captured in a graph once and replayed ppo_epochs x mini_batches times per
iteration, with a shuffle() between epochs.  The batcher's cursor lives on the device, so every replay of the one captured
gather yields the next minibatch.

    python examples/ppo_loop.py --graph-update --envs 4096 --iters 20

--max-grad-norm X: the reference's clip_grad_norm_(parameters, X) between backward() and the optimiser's step (rl/train.py:131)
on every path.  Default 0: no clipping, as before.

--device-optimizer: DeviceAdam (include/sfmi_optim.h) in place of torch.optim.Adam on every path: the norm, the clipping and
the Adam step for all parameters in three launches, the step count and a skipped step kept on the device; --max-grad-norm goes
to it instead of clip_grad_norm_.  Its step() is capturable as it is, so --graph-update takes it unchanged.  The log line prints
the last gradient norm and the count of steps skipped for a non-finite gradient.

    python examples/ppo_loop.py --graph-update --device-optimizer --max-grad-norm 0.5 --envs 4096 --iters 20
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spacefortress_amd import DeviceAdam, DeviceRollout, FrameRollout, SFVecEnv, SFVecNormalize, ppo_loss  # noqa: E402
from spacefortress_amd.stats import summarize  # noqa: E402


def reward_line(venv, log):
    """The reward part of the trainer's log line (rl/train.py:158-165) from the device's own bookkeeping: the episode statistics
    and the episode log's histogram, over the episodes finished so far (stats.py says how that differs from final_rewards)."""
    s = summarize(venv.episode_stats(), log.histogram(), log.hist_lo)
    if not s["episodes"]:
        return "no episode finished yet"
    return "mean/median reward %.1f/%.1f, min/max reward %.1f/%.1f over %d episodes" % (
        s["mean_return"], s["median_return"], s["min_return"], s["max_return"], s["episodes"])


def make_optimizer(a, net, capturable=False):
    """torch.optim.Adam, or with --device-optimizer DeviceAdam, which clips inside its step."""
    if a.device_optimizer:
        return DeviceAdam(net.parameters(), lr=7e-4, max_grad_norm=a.max_grad_norm if a.max_grad_norm > 0 else None)
    return torch.optim.Adam(net.parameters(), lr=7e-4, capturable=capturable)


def optimizer_step(opt, max_grad_norm):
    """rl/train.py:131-132: clip_grad_norm_ where asked for (DeviceAdam has it inside), then the step."""
    if max_grad_norm > 0 and not isinstance(opt, DeviceAdam):
        torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], max_grad_norm)
    opt.step()


def optimizer_line(opt):
    return "          device optimizer: last grad norm %.4f, coef %.4f, skipped steps %d" % (opt.last_norm(), opt.last_coef(), opt.check())


def device_update(net, opt, obs, act, ret, old_logp, adv_t, max_grad_norm=0.0):
    """One minibatch of the PPO update with the loss head on the device (--device-policy-head): the network's logits and values
    go to ppo_loss -- evaluate the actions, the clipped surrogate, the three means and the weighted sum in two launches, their
    gradients in one (include/sfmi_ppo.h) -- where the default path below runs torch.distributions and a dozen small kernels
    each way.  -> (loss, policy loss, value loss, entropy), on the device."""
    logits, value = net.logits_value(obs)
    losses = ppo_loss(logits, value, act, old_logp, adv_t, ret, 0.1, 0.5, 0.01)
    opt.zero_grad()
    losses[0].backward()
    optimizer_step(opt, max_grad_norm)
    return losses


class GraphUpdate:
    """--graph-update: one minibatch update as a captured graph.  The first three updates run eagerly on a side stream (torch's
    warm-up recipe: the optimiser's state and ppo_loss's workspace come to exist there), the fourth call captures one update
    and every call from then on replays it.  `losses` are the four 0-dim tensors the graph writes."""

    def __init__(self, net, opt, batcher, warmup=3, max_grad_norm=0.0):
        self.net, self.opt, self.batcher, self.warmup, self.max_grad_norm = net, opt, batcher, warmup, max_grad_norm
        self.graph, self.losses, self.calls = None, None, 0

    def _update(self):
        obs, _, act, ret, _, old_logp, adv_t = self.batcher.next()
        logits, value = self.net.logits_value(obs)
        losses = ppo_loss(logits, value, act, old_logp, adv_t, ret, 0.1, 0.5, 0.01)
        self.opt.zero_grad(set_to_none=True)
        losses[0].backward()
        optimizer_step(self.opt, self.max_grad_norm)
        return losses

    def step(self):
        self.calls += 1
        if self.graph is not None:
            self.graph.replay()
        elif self.calls <= self.warmup:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self.losses = self._update()
            torch.cuda.current_stream().wait_stream(side)
        else:
            self.opt.zero_grad(set_to_none=True)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.losses = self._update()
            self.graph.replay()  # (capturing launched nothing: this is the update itself)
        return self.losses


class ActorCritic(nn.Module):
    def __init__(self, obs_dim, n_actions, hidden=64):
        super().__init__()
        self.body = nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh())
        self.pi, self.v = nn.Linear(hidden, n_actions), nn.Linear(hidden, 1)

    def forward(self, obs):
        h = self.body(obs)
        return torch.distributions.Categorical(logits=self.pi(h)), self.v(h)

    def logits_value(self, obs):
        """The policy's logits and the value, for rollout.step_logits (--device-policy-head)."""
        h = self.body(obs)
        return self.pi(h), self.v(h)


class ConvActorCritic(nn.Module):
    """A small stand-in for rl/model.py's CNN branch: [B, 4, 84, 84] float (0 .. 255) -> policy, value."""

    def __init__(self, num_stack, n_actions):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(num_stack, 16, 8, stride=4), nn.ReLU(), nn.Conv2d(16, 32, 4, stride=2), nn.ReLU(),
                                  nn.Flatten(), nn.Linear(32 * 9 * 9, 128), nn.ReLU())
        self.pi, self.v = nn.Linear(128, n_actions), nn.Linear(128, 1)

    def forward(self, obs):
        h = self.body(obs * (1.0 / 255.0))
        return torch.distributions.Categorical(logits=self.pi(h)), self.v(h)

    def logits_value(self, obs):
        h = self.body(obs * (1.0 / 255.0))
        return self.pi(h), self.v(h)


def main_image(a):
    """The image path: FrameRollout instead of DeviceRollout(env, T, num_stack=4); no `observations` tensor anywhere."""
    env = SFVecEnv(a.envs, gametype=a.gametype, obs_type="image", spawn_stride=1, frame_skip=a.frame_skip)
    ro = FrameRollout(env, a.steps, num_stack=4, time_limit_bootstrap=a.time_limit_bootstrap)
    net = ConvActorCritic(4, env.n_actions).to(env.device)
    opt = make_optimizer(a, net)
    cur = ro.reset()
    print("observation storage: %.1f MB (stacked: %.1f MB)" % (ro.nbytes() / 1e6, (a.steps + 1) * a.envs * 4 * 7056 / 1e6))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(a.iters):
        for t in range(a.steps):
            if a.device_policy_head:
                with torch.no_grad():
                    logits, value = net.logits_value(cur.float())
                cur, _, _ = ro.step_logits(t, logits, value_pred=value)
                continue
            with torch.no_grad():
                dist, value = net(cur.float())
                action = dist.sample()
            cur, _, _ = ro.step(t, action, value_pred=value, action_log_prob=dist.log_prob(action).unsqueeze(1))
        with torch.no_grad():
            next_value = net(cur.float())[1]
            # the critic's value of every env's final stack: used where masks == 0 only
            final_value = net(ro.final_obs().float())[1] if a.time_limit_bootstrap else None
        ro.compute_returns(next_value, True, 0.99, 0.95, final_value=final_value)
        if a.device_minibatches:
            adv = ro.advantages()
        else:
            adv = ro.returns[:-1] - ro.value_preds[:-1]
            adv = (adv - adv.mean()) / (adv.std() + 1e-5)
        for _ in range(a.ppo_epochs):
            if a.device_minibatches:
                batches = ro.minibatches(adv, a.mini_batches, reuse=True, obs_dtype=torch.float32)
            else:
                batches = ro.feed_forward_generator(adv, a.mini_batches, obs_dtype=torch.float32)
            for obs, _, act, ret, _, old_logp, adv_t in batches:
                if a.device_policy_head:
                    losses = device_update(net, opt, obs, act, ret, old_logp, adv_t, a.max_grad_norm)
                    continue
                dist, value = net(obs)
                ratio = torch.exp(dist.log_prob(act.squeeze(1)).unsqueeze(1) - old_logp)
                loss = (-torch.min(ratio * adv_t, torch.clamp(ratio, 0.9, 1.1) * adv_t).mean()
                        + 0.5 * (value - ret).pow(2).mean() - 0.01 * dist.entropy().mean())
                opt.zero_grad()
                loss.backward()
                optimizer_step(opt, a.max_grad_norm)
        ro.after_update()  # (the current stack is stack_at(0) of the next rollout: `cur` stays valid)
        if (it + 1) % 5 == 0 or it == a.iters - 1:
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print("iter %3d  env-steps %9d  %.3g env-steps/s (whole loop)  mean final reward %.3f  kills %d" % (
                it + 1, (it + 1) * a.steps * a.envs, (it + 1) * a.steps * a.envs / dt, float(ro.final_rewards.mean()),
                ro.num_destruction))
            if a.device_policy_head:
                print("          policy head: mean entropy %.4f over the last step's rows, bad rows %d" % (
                    float(ro.policy_entropy.mean()), ro.policy.check()))
                print("          last minibatch: loss %.5f, policy loss %.5f, value loss %.5f, entropy %.5f, bad rows %d" % (
                    *(float(x) for x in losses), ppo_loss.check()))
            if a.device_minibatches and not a.device_policy_head:
                print("          last minibatch: loss %.5f" % float(loss))
            if a.device_optimizer:
                print(optimizer_line(opt))
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", choices=["features", "image"], default="features",
                    help="features: normalised 1-D observations over DeviceRollout; image: frame stacks over FrameRollout")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20, help="num_fwd_steps")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--gametype", default="autoturn")
    ap.add_argument("--ppo-epochs", type=int, default=4)
    ap.add_argument("--mini-batches", type=int, default=4)
    ap.add_argument("--time-limit-bootstrap", action="store_true",
                    help="bootstrap the returns at an episode's end with V(final observation / final frame stack) instead of 0")
    ap.add_argument("--frame-skip", type=int, default=1, metavar="K",
                    help="ticks every action is played for, in one launch (1: a tick per step)")
    ap.add_argument("--device-policy-head", action="store_true",
                    help="draw the actions from the network's logits in one launch on the device (rollout.step_logits)")
    ap.add_argument("--device-minibatches", action="store_true",
                    help="normalised advantages in three launches, every minibatch one gather launch into reused buffers")
    ap.add_argument("--graph-update", action="store_true",
                    help="capture one minibatch update (gather, network, ppo_loss, backward, Adam) once and replay it; features "
                         "only; implies --device-policy-head --device-minibatches")
    ap.add_argument("--max-grad-norm", type=float, default=0.0, metavar="X",
                    help="clip_grad_norm_(parameters, X) in front of every optimiser step, as the reference does (0: off)")
    ap.add_argument("--device-optimizer", action="store_true",
                    help="DeviceAdam in place of torch.optim.Adam: norm, clipping and the Adam step in three launches")
    a = ap.parse_args()
    if a.graph_update:
        if a.obs == "image":
            ap.error("--graph-update is for --obs features")
        if (a.steps * a.envs) % a.mini_batches:
            ap.error("--graph-update needs minibatches of equal size: steps * envs must be a multiple of --mini-batches")
        a.device_policy_head = a.device_minibatches = True
    torch.manual_seed(0)
    if a.obs == "image":
        if a.time_limit_bootstrap and a.frame_skip > 1:
            ap.error("--time-limit-bootstrap with --obs image needs --frame-skip 1 (the action repeat has no final frames yet)")
        return main_image(a)
    envs = SFVecNormalize(SFVecEnv(a.envs, gametype=a.gametype, spawn_stride=1, frame_skip=a.frame_skip))
    log = envs.venv.enable_episode_log()
    ro = DeviceRollout(envs, a.steps, time_limit_bootstrap=a.time_limit_bootstrap)
    net = ActorCritic(envs.venv.obs_dim, envs.venv.n_actions).to(envs.device)
    opt = make_optimizer(a, net, capturable=a.graph_update)
    ro.reset()
    adv_buf = torch.zeros(a.steps, a.envs, 1, device=envs.device) if a.device_minibatches else None  # filled in place per update
    graph = GraphUpdate(net, opt, ro.batcher(adv_buf, a.mini_batches), max_grad_norm=a.max_grad_norm) if a.graph_update else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(a.iters):
        for t in range(a.steps):
            if a.device_policy_head:
                with torch.no_grad():
                    logits, value = net.logits_value(ro.observations[t])
                ro.step_logits(t, logits, value_pred=value)
                continue
            with torch.no_grad():
                dist, value = net(ro.observations[t])
                action = dist.sample()
            ro.step(t, action, value_pred=value, action_log_prob=dist.log_prob(action).unsqueeze(1))
        with torch.no_grad():
            next_value = net(ro.observations[-1])[1]
            # the critic's value of every env's final observation (normalised like the rest): used where masks == 0 only
            final_value = net(ro.final_obs())[1] if a.time_limit_bootstrap else None
        ro.compute_returns(next_value, True, 0.99, 0.95, final_value=final_value)
        if a.device_minibatches:
            adv = ro.advantages(out=adv_buf)
        else:
            adv = ro.returns[:-1] - ro.value_preds[:-1]
            adv = (adv - adv.mean()) / (adv.std() + 1e-5)
        for _ in range(a.ppo_epochs):
            if graph is not None:  # the captured update, once per minibatch; the cursor moves on the device
                graph.batcher.shuffle()
                for _ in range(a.mini_batches):
                    losses = graph.step()
                continue
            if a.device_minibatches:
                batches = ro.minibatches(adv, a.mini_batches, reuse=True)
            else:
                batches = ro.feed_forward_generator(adv, a.mini_batches)
            for obs, _, act, ret, _, old_logp, adv_t in batches:
                if a.device_policy_head:
                    losses = device_update(net, opt, obs, act, ret, old_logp, adv_t, a.max_grad_norm)
                    continue
                dist, value = net(obs)
                ratio = torch.exp(dist.log_prob(act.squeeze(1)).unsqueeze(1) - old_logp)
                loss = (-torch.min(ratio * adv_t, torch.clamp(ratio, 0.9, 1.1) * adv_t).mean()
                        + 0.5 * (value - ret).pow(2).mean() - 0.01 * dist.entropy().mean())
                opt.zero_grad()
                loss.backward()
                optimizer_step(opt, a.max_grad_norm)
        ro.after_update()
        if (it + 1) % 5 == 0 or it == a.iters - 1:
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print("iter %3d  env-steps %9d  %.3g env-steps/s (whole loop)  mean final reward %.3f  kills %d" % (
                it + 1, (it + 1) * a.steps * a.envs, (it + 1) * a.steps * a.envs / dt, float(ro.final_rewards.mean()),
                ro.num_destruction))
            if a.device_policy_head:
                print("          policy head: mean entropy %.4f over the last step's rows, bad rows %d" % (
                    float(ro.policy_entropy.mean()), ro.policy.check()))
                print("          last minibatch: loss %.5f, policy loss %.5f, value loss %.5f, entropy %.5f, bad rows %d" % (
                    *(float(x) for x in losses), ppo_loss.check()))
            if a.device_minibatches and not a.device_policy_head:
                print("          last minibatch: loss %.5f" % float(loss))
            if graph is not None:
                print("          graph update: %d minibatch updates, %d of them replays of the one captured update" % (
                    graph.calls, max(0, graph.calls - graph.warmup)))
            if a.device_optimizer:
                print(optimizer_line(opt))
            print("          " + reward_line(envs.venv, log))
    envs.close()


if __name__ == "__main__":
    main()
