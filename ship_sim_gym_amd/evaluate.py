"""Evaluate a trained policy on the device: NativeEvaluator (ssg_evaluate / ssg_pop_evaluate / ssg_eval_account / ssg_eval_reduce) and
eval_walk.

The reference's evaluation script (train/rllib/rollout.py:8-26) acts, steps until done and prints the episode's reward, one env at a
time; Stable-Baselines users call ``model.predict(obs, deterministic=True)`` in the same loop.  ``NativeEvaluator`` runs that loop for
every env of a ``ShipVecEnv`` at once, enqueued from C: per step one policy launch (the arg-max action by default, or a draw), the
step, and one small accounting launch.  Every env contributes exactly its first ``episodes`` episodes, so an env that crashes early
does not weigh more than one that sails on, and every counted episode's ending is tallied from the step's event bits.

The stats columns (``COLUMNS``; include/shipsim.h): episodes, llrint(100 * return), length, endings with SSG_EV_COLLIDING /
OUT_OF_BOUNDS / MAX_STEPS / NO_GOALS_LEFT set on the done step (not exclusive of each other), goal events.

``eval_walk`` is a plain numpy restatement of the accounting over ``[T, N]`` arrays, for tests.
"""
import ctypes as C

import numpy as np

from . import _native as N

COLUMNS = ("episodes", "return100", "length", "collided", "out_of_bounds", "max_steps", "no_goals_left", "goals")


def _torch():
    import torch
    return torch


def new_carry(n_envs):
    """A zero carry for eval_walk: (return f64 [N], int32 [N, 4] = length, goal events, episodes counted, 0)."""
    return np.zeros(n_envs, dtype=np.float64), np.zeros((n_envs, 4), dtype=np.int32)


def eval_walk(rew, done, flags, episodes, carry=None):
    """The accounting of ssg_evaluate over recorded steps: rew f64 / done u8 / flags u8 arrays [T, N] -> (rows int64 [N, 8], carry).
    `carry` (from new_carry or an earlier call) is continued, not modified; the rows are THIS call's additions."""
    rew, done, flags = np.asarray(rew, dtype=np.float64), np.asarray(done), np.asarray(flags)
    if rew.ndim != 2 or done.shape != rew.shape or flags.shape != rew.shape:
        raise ValueError("eval_walk: rew, done and flags must be [T, N] arrays of one shape")
    E = int(episodes)
    if E < 1:
        raise ValueError("eval_walk: episodes must be >= 1")
    T, n = rew.shape
    ret, ci = new_carry(n) if carry is None else (carry[0].copy(), carry[1].copy())
    rows = np.zeros((n, N.EVAL_STATS), dtype=np.int64)
    bits = (N.EV_COLLIDING, N.EV_OUT_OF_BOUNDS, N.EV_MAX_STEPS, N.EV_NO_GOALS_LEFT)
    for t in range(T):
        for e in range(n):
            if ci[e, 2] >= E:
                continue
            f = int(flags[t, e])
            ret[e] += rew[t, e]
            ci[e, 0] += 1
            ci[e, 1] += 1 if f & N.EV_GOAL_REACHED else 0
            if done[t, e]:
                rows[e, 0] += 1
                rows[e, 1] += int(np.rint(ret[e] * 100.0))  # (llrint: round to nearest, ties to even)
                rows[e, 2] += ci[e, 0]
                for c, b in enumerate(bits):
                    rows[e, 3 + c] += 1 if f & b else 0
                rows[e, 7] += ci[e, 1]
                ret[e] = 0.0
                ci[e, 0] = ci[e, 1] = 0
                ci[e, 2] += 1
    return rows, (ret, ci)


def derive(per_member):
    """Per-member floats from stats rows int64 [P, 8] (numpy): means over the counted episodes; NaN where a member counted none."""
    s = np.asarray(per_member, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        eps = s[:, 0]
        return {
            "return_mean": s[:, 1] / 100.0 / eps, "length_mean": s[:, 2] / eps,
            "collision_rate": s[:, 3] / eps, "out_of_bounds_rate": s[:, 4] / eps, "max_steps_rate": s[:, 5] / eps,
            "no_goals_left_rate": s[:, 6] / eps, "goals_per_episode": s[:, 7] / eps,
        }


class NativeEvaluator(object):
    """Owns the one-row scratch buffers, the carries and the stats tensors of evaluations on `env` (allocated once).  An observation
    filter bound to `env` (``env.set_obs_filter``; usually a trainer's ``ObsFilter.frozen(env)``) normalises the observations of every
    policy launch and is never updated by an evaluation, whatever its record says."""

    def __init__(self, env):
        torch = _torch()
        self.env = env
        n, dev = env.num_envs, env.device
        with torch.cuda.device(dev):
            self.act = torch.zeros(n, dtype=torch.int32, device=dev)
            self.logp = torch.zeros(n, dtype=torch.float32, device=dev)
            self.value = torch.zeros(n, dtype=torch.float32, device=dev)
            self.reward = torch.zeros(n, dtype=torch.float64, device=dev)
            self.done = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.flags = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.carry_return = torch.zeros(n, dtype=torch.float64, device=dev)
            self.carry = torch.zeros((n, 4), dtype=torch.int32, device=dev)
            self.env_stats = torch.zeros((n, N.EVAL_STATS), dtype=torch.int64, device=dev)
            self.member_stats = torch.zeros((N.POP_MAX_MEMBERS, N.EVAL_STATS), dtype=torch.int64, device=dev)
        self.steps = 0  # steps run since the carries were last zeroed

    def reset_carry(self):
        """Zero the carries and the stats rows (after an env reset: no episode is running)."""
        self.carry_return.zero_()
        self.carry.zero_()
        self.env_stats.zero_()
        self.steps = 0

    def _record(self, episodes, n_steps, greedy, seed, step0, uniforms):
        env = self.env
        ev = N.Eval()
        ev.struct_size = C.sizeof(N.Eval)
        ev.flags = N.EVAL_GREEDY if greedy else 0
        ev.episodes_per_env, ev.n_steps = int(episodes), int(n_steps)
        ev.seed, ev.step0 = int(seed), int(step0)
        ev.dev_uniform_TN = uniforms.data_ptr() if uniforms is not None else None
        ev.dev_obs = env.obs.data_ptr()
        ev.dev_act, ev.dev_logp, ev.dev_value = self.act.data_ptr(), self.logp.data_ptr(), self.value.data_ptr()
        ev.dev_reward, ev.dev_done, ev.dev_flags = self.reward.data_ptr(), self.done.data_ptr(), self.flags.data_ptr()
        ev.dev_carry_return, ev.dev_carry, ev.dev_env_stats = self.carry_return.data_ptr(), self.carry.data_ptr(), self.env_stats.data_ptr()
        return ev

    def run(self, policy_or_population, episodes, n_steps, greedy=True, seed=0, step0=0, uniforms=None):
        """One ssg_evaluate / ssg_pop_evaluate call: n_steps iterations enqueued on the current stream, no synchronisation.  uniforms:
        float32 [n_steps, N] rows for the sampled mode.  Continues the carries as they stand."""
        torch = _torch()
        env, pol = self.env, policy_or_population
        population = hasattr(pol, "member")
        what = "evaluate"
        if greedy and uniforms is not None:
            raise ValueError("evaluate: greedy=True reads no uniforms (pass one or the other)")
        if int(episodes) < 1 or int(n_steps) < 1:
            raise ValueError("evaluate: episodes and the number of steps must be >= 1")
        (env._check_population if population else env._check_policy)(pol, what)
        if uniforms is not None:
            env._f32_rows(uniforms, (int(n_steps), env.num_envs), "evaluate uniforms")
        ev = self._record(episodes, n_steps, greedy, seed, step0, uniforms)
        rec = pol.to_native()
        with torch.cuda.device(env.device):
            fn = N.lib().ssg_pop_evaluate if population else N.lib().ssg_evaluate
            N.check(fn(env._h, C.byref(rec), C.byref(ev), env._stream()), env._h, "ssg_pop_evaluate" if population else "ssg_evaluate")
        self.steps += int(n_steps)

    def account(self, episodes, reward=None, done=None, flags=None):
        """ssg_eval_account: the accounting launch alone, for a caller that steps the env itself — on one step's reward f64 / done u8 /
        flags u8 rows [N] (default: the env's own output tensors, as step_tensor leaves them)."""
        torch = _torch()
        env = self.env
        if int(episodes) < 1:
            raise ValueError("evaluate: episodes must be >= 1")
        reward = env.reward if reward is None else reward
        done = env.done if done is None else done
        flags = env.flags if flags is None else flags
        for t, dt, what in ((reward, torch.float64, "reward"), (done, torch.uint8, "done"), (flags, torch.uint8, "flags")):
            if t.dtype != dt or t.device != env.device or not t.is_contiguous() or t.numel() != env.num_envs:
                raise ValueError("evaluate: %s must be a contiguous %s tensor of %d elements on %s" % (what, dt, env.num_envs, env.device))
        with torch.cuda.device(env.device):
            N.check(N.lib().ssg_eval_account(env._h, int(episodes), C.c_void_p(reward.data_ptr()), C.c_void_p(done.data_ptr()),
                                             C.c_void_p(flags.data_ptr()), C.c_void_p(self.carry_return.data_ptr()),
                                             C.c_void_p(self.carry.data_ptr()), C.c_void_p(self.env_stats.data_ptr()), env._stream()),
                    env._h, "ssg_eval_account")
        self.steps += 1

    def reduce(self, n_members=1):
        """ssg_eval_reduce: int64 [n_members, 8] column sums of each member's rows of env_stats (a view of this object's buffer); a
        member's rows are its slice of the env's set_population_slices when one is bound."""
        torch = _torch()
        env = self.env
        P = int(n_members)
        sizes = env.population_slices if P > 1 else None  # (one policy's reduce is over the whole handle)
        if P < 1 or P > N.POP_MAX_MEMBERS or (len(sizes) != P if sizes is not None else env.num_envs % P):
            raise ValueError("evaluate: %d envs do not split into %d member slices" % (env.num_envs, P))
        with torch.cuda.device(env.device):
            N.check(N.lib().ssg_eval_reduce(env._h, P, C.c_void_p(self.env_stats.data_ptr()), C.c_void_p(self.member_stats.data_ptr()),
                                            env._stream()), env._h, "ssg_eval_reduce")
        return self.member_stats[:P]

    def evaluate(self, policy_or_population, episodes, greedy=True, max_steps=None, seed=0, step0=0, uniforms=None, reset=True, chunk=128):
        """Run until every env has counted `episodes` episodes, or for max_steps steps (default episodes * env.cfg.max_steps, which
        always suffices: an episode cannot outlive max_steps).  Steps are enqueued in chunks of `chunk`; after each chunk ONE device
        scalar is read, the minimum over the envs of the episodes counted.  reset=True resets the env and zeroes the carries first;
        reset=False continues both.  uniforms: float32 [>= max_steps, N] for the sampled mode (row k drives step k of this call).
        Returns a dict: per_env int64 [N, 8], per_member int64 [P, 8] (device tensors), the derived per-member floats (numpy [P]:
        return_mean, length_mean, collision_rate, out_of_bounds_rate, max_steps_rate, no_goals_left_rate, goals_per_episode),
        complete (every env reached `episodes`) and steps (run by this call)."""
        env, pol = self.env, policy_or_population
        E, chunk = int(episodes), int(chunk)
        if E < 1:
            raise ValueError("evaluate: episodes must be >= 1")
        if chunk < 1:
            raise ValueError("evaluate: chunk must be >= 1")
        if max_steps is None:
            max_steps = E * int(env.cfg.max_steps)
        max_steps = int(max_steps)
        if max_steps < 1:
            raise ValueError("evaluate: max_steps must be >= 1")
        if greedy and uniforms is not None:
            raise ValueError("evaluate: greedy=True reads no uniforms (pass one or the other)")
        if uniforms is not None and (uniforms.dim() != 2 or uniforms.shape[0] < max_steps):
            raise ValueError("evaluate: uniforms must hold max_steps = %d rows (got %s)" % (max_steps, tuple(uniforms.shape)))
        P = len(pol) if hasattr(pol, "member") else 1
        if reset:
            env.reset_tensor()
            self.reset_carry()
        done_steps, complete = 0, False
        while done_steps < max_steps and not complete:
            k = min(chunk, max_steps - done_steps)
            self.run(pol, E, k, greedy=greedy, seed=seed, step0=int(step0) + done_steps,
                     uniforms=uniforms[done_steps: done_steps + k] if uniforms is not None else None)
            done_steps += k
            complete = int(self.carry[:, 2].min().item()) >= E
        per_member = self.reduce(P)
        out = {"per_env": self.env_stats, "per_member": per_member, "complete": complete, "steps": done_steps}
        out.update(derive(per_member.cpu().numpy()))
        return out


def format_table(result, names=None):
    """The result of NativeEvaluator.evaluate as text: a header line and one row per policy / member."""
    pm = result["per_member"].cpu().numpy()
    keys = ("return_mean", "length_mean", "collision_rate", "out_of_bounds_rate", "max_steps_rate", "no_goals_left_rate", "goals_per_episode")
    lines = ["%-10s %9s " % ("policy", "episodes") + " ".join("%18s" % k for k in keys)]
    for m in range(pm.shape[0]):
        name = names[m] if names else ("member %d" % m if pm.shape[0] > 1 else "policy")
        lines.append("%-10s %9d " % (name, pm[m, 0]) + " ".join("%18.4f" % result[k][m] for k in keys))
    return "\n".join(lines)
