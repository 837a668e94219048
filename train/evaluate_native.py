#!/usr/bin/env python3
"""Evaluate a policy for whole episodes on the device: the reference's train/rllib/rollout.py:8-26 (compute_action, env.step until
done, "Episode reward"), and the ``model.predict(obs, deterministic=True)`` loop Stable-Baselines users write, against this package.

    python train/evaluate_native.py --envs 4096 --episodes 4 [--checkpoint FILE [--member M]] [--sampled] [--separate-value] [--seed 0]
                                     [--obs-filter FILE]
                                     [--record-envs 0,5,17 [--out FILE] [--frames FILE.npz [--frame-size WxH] [--frame-every S]]
                                      [--record-steps C]]

``--checkpoint FILE`` is a checkpoint of train/ppo_torch.py or train/pbt_native.py (``--save`` / ``--save-best``;
ship_sim_gym_amd/checkpoint.py): the architecture comes from the file (``--separate-value`` is unnecessary, and refused when it
contradicts the file), the beam count follows the policy's observation width, and the file's observation filter is applied frozen
unless ``--obs-filter FILE`` overrides it.  A population file evaluates every member, one table row each, on ``--envs`` / P envs per
member; ``--member M`` evaluates that member alone on all of them.  A plain module ``state_dict`` saved by ``torch.save`` works as
before: it is loaded into train/ppo_torch.py's ActorCritic.  Without ``--checkpoint`` the weights are seeded random ones.

The policy runs on ``--envs`` envs until every env has finished ``--episodes`` episodes (ship_sim_gym_amd/evaluate.py: one
policy launch, one step and one accounting launch per step, enqueued from C).  The action is the arg-max by default, a draw with
``--sampled``.  Every env contributes exactly its first ``--episodes`` episodes, so short episodes are not over-weighted.  Prints one
row per policy: episodes, mean return and length, how the episodes ended (collision, out of bounds, time-out, no goals left; not
exclusive of each other) and goals per episode.

``--obs-filter FILE``: normalise the observations with the running mean / std statistics a training run saved (train/ppo_torch.py
``--save-obs-filter``), frozen — an evaluation never updates them — instead of the fixed division by the largest bound.

``--record-envs 0,5,17`` records those envs' counted steps on the device while the evaluation runs (ship_sim_gym_amd/evaluate.py,
EvalRecorder) and prints one ``Episode reward`` line per recorded episode, as rollout.py:26 does.  ``--out FILE`` pickles
[state, action, next_state, reward, done] per step, a list per episode, as rollout.py --out writes it (rollout.py:20-28); next_state
of a done step is the episode's terminal observation.  ``--frames FILE.npz`` saves one uint8 array [T', H, W, 3] per recorded episode
(``episode_0000`` ...), a frame for every ``--frame-every``-th kept step of ``--frame-size`` pixels (default 128x128), each drawn
before its step: what the agent saw when it acted.  ``--record-steps C`` bounds the steps kept per env (default episodes *
max_steps, which always suffices); a slot that ran full is reported.

Out of scope here: the frame after a crash (a done env is reset inside the step, so the next frame shows the new episode), a video
encoder, and recording during training rollouts.
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


def _env_list(text):
    try:
        ids = [int(t) for t in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("a comma-separated list of env indices (got %s)" % text)
    if not ids or min(ids) < 0 or len(set(ids)) != len(ids):
        raise argparse.ArgumentTypeError("distinct env indices >= 0 (got %s)" % text)
    return ids


def _size(text):
    try:
        w, h = (int(t) for t in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError("WxH, e.g. 128x128 (got %s)" % text)
    if not (1 <= w <= 8192 and 1 <= h <= 8192):
        raise argparse.ArgumentTypeError("width and height must be in 1..8192 (got %s)" % text)
    return w, h


def make_arg_parser():
    ap = argparse.ArgumentParser(description="Evaluate an ActorCritic for whole episodes on the device (the reference's rollout.py).")
    ap.add_argument("--checkpoint", default=None, metavar="FILE",
                    help="a checkpoint written by the trainers' --save / --save-best, or a module state_dict saved by torch.save; random "
                         "weights otherwise")
    ap.add_argument("--member", type=int, default=None, metavar="M",
                    help="of a population checkpoint: evaluate this member alone (default: every member, one row each)")
    ap.add_argument("--envs", type=_positive, default=4096)
    ap.add_argument("--episodes", type=_positive, default=4, help="episodes counted per env")
    ap.add_argument("--sampled", action="store_true", help="draw the actions (Philox keyed by --seed) instead of the arg-max")
    ap.add_argument("--separate-value", action="store_true", help="the ActorCritic has a value network of its own (pi_body, pi, vf_body, v)")
    ap.add_argument("--seed", type=int, default=0, help="of the random weights and of the sampled actions")
    ap.add_argument("--obs-filter", default=None, metavar="FILE",
                    help="observation filter statistics saved by train/ppo_torch.py --save-obs-filter (applied frozen); default: obs / max bound")
    ap.add_argument("--record-envs", type=_env_list, default=None, metavar="0,5,17", help="record these envs' trajectories on the device")
    ap.add_argument("--out", default=None, metavar="FILE", help="pickle the recorded episodes as rollout.py --out does (needs --record-envs)")
    ap.add_argument("--frames", default=None, metavar="FILE.npz", help="save one uint8 [T', H, W, 3] array per recorded episode (needs --record-envs)")
    ap.add_argument("--frame-size", type=_size, default=(128, 128), metavar="WxH")
    ap.add_argument("--frame-every", type=_positive, default=1, metavar="S", help="a frame for every S-th kept step")
    ap.add_argument("--record-steps", type=_positive, default=None, metavar="C", help="steps kept per recorded env (default episodes * max_steps)")
    ap.add_argument("--device", default="cuda:0")
    return ap


def parse_args(argv=None):
    return make_arg_parser().parse_args(argv)


def evaluate(envs=4096, episodes=4, checkpoint=None, sampled=False, separate_value=False, seed=0, device="cuda:0", log=print, obs_filter=None,
             member=None, env_kw=None, record_envs=None, out=None, frames=None, frame_size=(128, 128), frame_every=1, record_steps=None):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from ppo_torch import ActorCritic
    from ship_gym.config import EnvConfig, GameConfig
    from ship_sim_gym_amd import checkpoint as ckpt_mod
    from ship_sim_gym_amd.evaluate import EvalRecorder, NativeEvaluator, format_table
    from ship_sim_gym_amd.obs_filter import ObsFilter
    from ship_sim_gym_amd.policy import NativePolicy
    from ship_sim_gym_amd.population import NativePopulation
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    torch.manual_seed(seed)
    env_kw = dict(env_kw or {})
    if (out is not None or frames is not None) and not record_envs:
        raise ValueError("evaluate: out and frames save what record_envs records; no env was named")
    if record_envs and max(record_envs) >= envs:
        raise ValueError("evaluate: record_envs names env %d of %d" % (max(record_envs), envs))
    ckpt = None
    if checkpoint is not None:
        content = ckpt_mod.read(checkpoint)  # (a checkpoint and a module's state_dict both load without running any code of the file's)
        if ckpt_mod.is_checkpoint(content):
            ckpt = ckpt_mod.validate(content, (), str(checkpoint))
    if member is not None and (ckpt is None or "population" not in ckpt):
        raise ValueError("evaluate: member picks a member of a population checkpoint; %s" % (
            "no checkpoint was given" if checkpoint is None else "%s holds one policy" % checkpoint))
    filter_sd = None
    if ckpt is not None:
        arch = ckpt["population"] if "population" in ckpt else ckpt["policy"]
        if separate_value and not arch["separate_value"]:
            raise ValueError("evaluate: separate_value contradicts %s, whose policy has a shared body" % checkpoint)
        if "n_beams" not in env_kw:  # (the observation width is history * (6 + beams): the env must produce what the policy reads)
            hist = int(EnvConfig.HISTORY_SIZE)
            if arch["obs_dim"] % hist or arch["obs_dim"] // hist <= 6:
                raise ValueError("evaluate: the file's obs_dim %d is no history %d x (6 + beams)" % (arch["obs_dim"], hist))
            env_kw["n_beams"] = arch["obs_dim"] // hist - 6
        filter_sd = ckpt.get("obs_filter")
        if "population" in ckpt:
            P = int(ckpt["population"]["n_members"])
            if member is not None and not 0 <= int(member) < P:
                raise ValueError("evaluate: member %d of a population of %d" % (member, P))
            if member is None and envs % P:
                raise ValueError("evaluate: %d envs do not split into the file's %d members" % (envs, P))
    env = ShipVecEnv(envs, GameConfig, EnvConfig, device=device, **env_kw)
    if ckpt is None:
        net = ActorCritic(env.states_history, env.action_space.n, separate_value=separate_value)
        if checkpoint is not None:
            net.load_state_dict(content)
        net = net.to(env.device)
        scale = torch.full((env.states_history,), float(max(env.bounds)), dtype=torch.float64, device=env.device)
        policy = NativePolicy.from_actor_critic(net, scale)
    elif "population" in ckpt:
        if member is not None:
            policy = NativePolicy.from_state_dict(ckpt["population"], env.device, row=int(member))
            if filter_sd is not None:  # that member's statistics, as a filter of one member
                filter_sd = dict(filter_sd, state=filter_sd["state"][int(member): int(member) + 1].clone(), n_members=1)
        else:
            policy = NativePopulation.from_state_dict(ckpt["population"], env.device)
    else:
        policy = NativePolicy.from_state_dict(ckpt["policy"], env.device)
    if obs_filter is not None:  # (overrides the checkpoint's)
        filter_sd = torch.load(obs_filter, map_location="cpu")
    if filter_sd is not None:
        flt = ObsFilter(env, n_members=int(filter_sd["n_members"]), update=False).load_state_dict(filter_sd)
        env.set_obs_filter(flt)
    recorder = None
    if record_envs:
        recorder = EvalRecorder(env, record_envs, record_steps or episodes * int(env.cfg.max_steps),
                                frames=frame_size if frames is not None else None, frame_every=frame_every)
    result = NativeEvaluator(env).evaluate(policy, episodes, greedy=not sampled, seed=seed, recorder=recorder)
    log(format_table(result))
    if not result["complete"]:
        log("(some env did not finish %d episodes within %d steps)" % (episodes, result["steps"]))
    res = {k: v for k, v in result.items() if k not in ("per_env", "per_member")}
    res["per_member"] = result["per_member"].cpu().numpy().copy()
    if recorder is not None:
        save_recording(recorder, out, frames, log)
    env.close()
    return res


def save_recording(recorder, out, frames, log):
    """One "Episode reward" line per recorded episode (rollout.py:26), a warning per slot that ran full, the pickle and the frames."""
    import pickle
    import numpy as np
    per_slot = recorder.episodes()
    for e, eps in zip(recorder.env_ids, per_slot):
        for ep in eps:
            total = 0.0
            for r in ep["reward"]:  # (summed in order, as rollout.py:17 does)
                total += float(r)
            log("Episode reward %r (env %d, %d steps%s)" % (total, e, len(ep["reward"]), "" if ep["complete"] else ", incomplete"))
    for e, lost in zip(recorder.env_ids, recorder.overflow):
        if lost:
            log("warning: env %d counted %d steps past the %d kept (--record-steps)" % (e, lost, recorder.capacity))
    if out is not None:
        with open(out, "wb") as f:
            pickle.dump(recorder.as_rollouts(), f)
    if frames is not None:
        arrays = {"episode_%04d" % i: ep["frames"] for i, ep in enumerate(ep for eps in per_slot for ep in eps)}
        np.savez(frames, **arrays)


if __name__ == "__main__":
    a = parse_args()
    evaluate(envs=a.envs, episodes=a.episodes, checkpoint=a.checkpoint, sampled=a.sampled, separate_value=a.separate_value, seed=a.seed,
             device=a.device, obs_filter=a.obs_filter, member=a.member, record_envs=a.record_envs, out=a.out, frames=a.frames,
             frame_size=a.frame_size, frame_every=a.frame_every, record_steps=a.record_steps)
