#!/usr/bin/env python3
"""Evaluate a policy for whole episodes on the device: the reference's train/rllib/rollout.py:8-26 (compute_action, env.step until
done, "Episode reward"), and the ``model.predict(obs, deterministic=True)`` loop Stable-Baselines users write, against this package.

    python train/evaluate_native.py --envs 4096 --episodes 4 [--checkpoint net.pt] [--sampled] [--separate-value] [--seed 0]
                                     [--obs-filter FILE]

Builds train/ppo_torch.py's ActorCritic — loaded from ``--checkpoint`` (a ``state_dict`` saved by ``torch.save``) or with seeded random
weights — and runs it on ``--envs`` envs until every env has finished ``--episodes`` episodes (ship_sim_gym_amd/evaluate.py: one
policy launch, one step and one accounting launch per step, enqueued from C).  The action is the arg-max by default, a draw with
``--sampled``.  Every env contributes exactly its first ``--episodes`` episodes, so short episodes are not over-weighted.  Prints one
row per policy: episodes, mean return and length, how the episodes ended (collision, out of bounds, time-out, no goals left; not
exclusive of each other) and goals per episode.

``--obs-filter FILE``: normalise the observations with the running mean / std statistics a training run saved (train/ppo_torch.py
``--save-obs-filter``), frozen — an evaluation never updates them — instead of the fixed division by the largest bound.

Out of scope here: recording trajectories (rollout.py --out) and rendering during evaluation.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _positive(text):
    v = int(text)
    if v < 1:
        raise argparse.ArgumentTypeError("must be >= 1 (got %s)" % text)
    return v


def make_arg_parser():
    ap = argparse.ArgumentParser(description="Evaluate an ActorCritic for whole episodes on the device (the reference's rollout.py).")
    ap.add_argument("--checkpoint", default=None, help="a state_dict saved by torch.save; random weights otherwise")
    ap.add_argument("--envs", type=_positive, default=4096)
    ap.add_argument("--episodes", type=_positive, default=4, help="episodes counted per env")
    ap.add_argument("--sampled", action="store_true", help="draw the actions (Philox keyed by --seed) instead of the arg-max")
    ap.add_argument("--separate-value", action="store_true", help="the ActorCritic has a value network of its own (pi_body, pi, vf_body, v)")
    ap.add_argument("--seed", type=int, default=0, help="of the random weights and of the sampled actions")
    ap.add_argument("--obs-filter", default=None, metavar="FILE",
                    help="observation filter statistics saved by train/ppo_torch.py --save-obs-filter (applied frozen); default: obs / max bound")
    ap.add_argument("--device", default="cuda:0")
    return ap


def parse_args(argv=None):
    return make_arg_parser().parse_args(argv)


def evaluate(envs=4096, episodes=4, checkpoint=None, sampled=False, separate_value=False, seed=0, device="cuda:0", log=print, obs_filter=None):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from ppo_torch import ActorCritic
    from ship_gym.config import EnvConfig, GameConfig
    from ship_sim_gym_amd.evaluate import NativeEvaluator, format_table
    from ship_sim_gym_amd.policy import NativePolicy
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    torch.manual_seed(seed)
    env = ShipVecEnv(envs, GameConfig, EnvConfig, device=device)
    net = ActorCritic(env.states_history, env.action_space.n, separate_value=separate_value)
    if checkpoint is not None:
        net.load_state_dict(torch.load(checkpoint, map_location="cpu"))
    net = net.to(env.device)
    scale = torch.full((env.states_history,), float(max(env.bounds)), dtype=torch.float64, device=env.device)
    policy = NativePolicy.from_actor_critic(net, scale)
    if obs_filter is not None:
        from ship_sim_gym_amd.obs_filter import ObsFilter
        sd = torch.load(obs_filter, map_location="cpu")
        flt = ObsFilter(env, n_members=int(sd["n_members"]), update=False).load_state_dict(sd)
        env.set_obs_filter(flt)
    result = NativeEvaluator(env).evaluate(policy, episodes, greedy=not sampled, seed=seed)
    log(format_table(result))
    if not result["complete"]:
        log("(some env did not finish %d episodes within %d steps)" % (episodes, result["steps"]))
    out = {k: v for k, v in result.items() if k not in ("per_env", "per_member")}
    out["per_member"] = result["per_member"].cpu().numpy().copy()
    env.close()
    return out


if __name__ == "__main__":
    a = parse_args()
    evaluate(envs=a.envs, episodes=a.episodes, checkpoint=a.checkpoint, sampled=a.sampled, separate_value=a.separate_value, seed=a.seed,
             device=a.device, obs_filter=a.obs_filter)
