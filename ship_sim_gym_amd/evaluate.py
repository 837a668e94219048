"""Evaluate a trained policy on the device: NativeEvaluator (ssg_evaluate / ssg_pop_evaluate / ssg_eval_account / ssg_eval_reduce),
EvalRecorder (ssg_set_eval_recorder: the trajectories and frames of a few envs of a run), eval_walk and record_walk.

The reference's evaluation script (train/rllib/rollout.py:8-26) acts, steps until done and prints the episode's reward, one env at a
time; Stable-Baselines users call ``model.predict(obs, deterministic=True)`` in the same loop.  ``NativeEvaluator`` runs that loop for
every env of a ``ShipVecEnv`` at once, enqueued from C: per step one policy launch (the arg-max action by default, or a draw), the
step, and one small accounting launch.  Every env contributes exactly its first ``episodes`` episodes, so an env that crashes early
does not weigh more than one that sails on, and every counted episode's ending is tallied from the step's event bits.

The stats columns (``COLUMNS``; include/shipsim.h): episodes, llrint(100 * return), length, endings with SSG_EV_COLLIDING /
OUT_OF_BOUNDS / MAX_STEPS / NO_GOALS_LEFT set on the done step (not exclusive of each other), goal events.

``EvalRecorder`` keeps what the reference's loop keeps with ``--out`` and shows with ``env.render()`` (train/rllib/rollout.py:18-28)
for a few tracked envs: [state, action, next_state, reward, done] of every counted step, and optionally a frame per step.

``eval_walk`` and ``record_walk`` are plain numpy restatements of the accounting and of the recorder over ``[T, N]`` arrays, for tests.
"""
import ctypes as C

import numpy as np

from . import _native as N
from ._native import _torch

COLUMNS = ("episodes", "return100", "length", "collided", "out_of_bounds", "max_steps", "no_goals_left", "goals")


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


RECORD_ROWS = ("obs", "act", "logp", "value", "reward", "done", "flags", "next_obs")


def next_observations(obs_after, term_obs, done):
    """What rollout.py's loop calls next_state, from what a step with terminal observations on leaves ([..., N, D] rows and done
    [..., N]): the TERMINAL observation row where done is set (the in-kernel reset has already replaced that env's row of obs_after),
    the row of obs_after elsewhere.  Rows of term_obs of envs that were not done hold stale memory and are never taken."""
    obs_after, term_obs, done = np.asarray(obs_after), np.asarray(term_obs), np.asarray(done)
    return np.where((done != 0)[..., None], term_obs, obs_after)


def record_walk(obs, act, logp, value, rew, done, flags, next_obs, env_ids, episodes, capacity, state=None):
    """The evaluation recorder (ssg_set_eval_recorder) over recorded steps, in plain numpy: arrays [T, N, ...] of every env — obs (what
    the policy read at step k), the policy's act / logp / value, the step's rew / done / flags and next_obs (next_observations) —
    -> a dict with obs / next_obs [R, C, D], act / logp / value / reward / done / flags [R, C], cursor / overflow int32 [R],
    iteration int64 [R, C] (the k of this walk's numbering that filled row t, -1 where unwritten) and counted int32 [N] (the episodes
    each env has counted, the accounting's carry).  Rows at and past the cursor are zero.  `state` (the dict an earlier call returned)
    is continued, not modified; its iteration numbers go on from where it stopped."""
    obs, next_obs = np.asarray(obs, dtype=np.float64), np.asarray(next_obs, dtype=np.float64)
    cols = {"act": (act, np.int32), "logp": (logp, np.float32), "value": (value, np.float32), "reward": (rew, np.float64),
            "done": (done, np.uint8), "flags": (flags, np.uint8)}
    cols = {k: np.asarray(a, dtype=dt) for k, (a, dt) in cols.items()}
    if obs.ndim != 3 or next_obs.shape != obs.shape or any(a.shape != obs.shape[:2] for a in cols.values()):
        raise ValueError("record_walk: obs and next_obs must be [T, N, D], the other arrays [T, N]")
    T, n, D = obs.shape
    ids = [int(e) for e in env_ids]
    E, cap, R = int(episodes), int(capacity), len(ids)
    if E < 1 or cap < 1 or R < 1:
        raise ValueError("record_walk: episodes, capacity and the number of tracked envs must be >= 1")
    if len(set(ids)) != R or min(ids) < 0 or max(ids) >= n:
        raise ValueError("record_walk: env_ids must be distinct and in [0, N)")
    if state is None:
        out = {"obs": np.zeros((R, cap, D)), "next_obs": np.zeros((R, cap, D)), "cursor": np.zeros(R, dtype=np.int32),
               "overflow": np.zeros(R, dtype=np.int32), "iteration": np.full((R, cap), -1, dtype=np.int64),
               "counted": np.zeros(n, dtype=np.int32), "iterations": 0}
        out.update({k: np.zeros((R, cap), dtype=a.dtype) for k, a in cols.items()})
    else:
        out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
        if out["obs"].shape != (R, cap, D) or out["counted"].shape != (n,):
            raise ValueError("record_walk: state belongs to another shape")
    k0 = out["iterations"]
    for k in range(T):
        before = out["counted"].copy()  # (read BEFORE this iteration's accounting)
        for r, e in enumerate(ids):
            if before[e] >= E:
                continue
            t = int(out["cursor"][r])
            if t >= cap:
                out["overflow"][r] += 1
                continue
            out["obs"][r, t], out["next_obs"][r, t] = obs[k, e], next_obs[k, e]
            for name, a in cols.items():
                out[name][r, t] = a[k, e]
            out["iteration"][r, t] = k0 + k
            out["cursor"][r] = t + 1
        out["counted"] += ((before < E) & (cols["done"][k] != 0)).astype(np.int32)
    out["iterations"] = k0 + T
    return out


def split_episodes(rec, frame_every=1):
    """Cut the kept steps of every slot where done is set.  rec: a dict of numpy arrays as record_walk returns or EvalRecorder.numpy()
    (obs ... next_obs, cursor; optionally frames [R, ceil(C / S), W, H, 3]).  Returns, per slot, a list of episodes: dicts of the rows
    of RECORD_ROWS for the episode's steps, `frames` [T', H, W, 3] (the orientation render('rgb_array') returns; the frames of the
    episode's steps t with t % S == 0) when rec has frames, and `complete`: False for a trailing episode cut by the capacity or by
    the end of the run."""
    S = int(frame_every)
    out = []
    for r in range(len(rec["cursor"])):
        n = int(rec["cursor"][r])
        ends = [t for t in range(n) if rec["done"][r, t]]
        bounds = [0] + [t + 1 for t in ends]
        if bounds[-1] < n:
            bounds.append(n)
        eps = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            ep = {k: rec[k][r, a:b].copy() for k in RECORD_ROWS}
            ep["complete"] = bool(rec["done"][r, b - 1])
            if rec.get("frames") is not None:
                ts = [t for t in range(a, b) if t % S == 0]
                ep["frames"] = np.transpose(rec["frames"][r, [t // S for t in ts]], (0, 2, 1, 3)).copy()
            eps.append(ep)
        out.append(eps)
    return out


def rollouts_of(episodes_per_slot):
    """rollout.py's --out structure (train/rllib/rollout.py:20-28) from split_episodes' result: a list of episodes, slot after slot,
    each a list of [state, action, next_state, reward, done] per step."""
    return [[[ep["obs"][t], int(ep["act"][t]), ep["next_obs"][t], float(ep["reward"][t]), bool(ep["done"][t])]
             for t in range(len(ep["act"]))] for eps in episodes_per_slot for ep in eps]


class EvalRecorder(object):
    """Owns the buffers of an evaluation recorder (ssg_set_eval_recorder) on `env`: the trajectories of the envs `env_ids` (distinct,
    any order, at most EVAL_REC_MAX_ENVS), `capacity` steps each across all of an env's episodes, and with frames=(W, H) a frame for
    every frame_every-th kept step, drawn BEFORE the step: what the agent saw when it chose the action.  The frame after a done step
    shows the next episode's first state: the post-crash state is never drawn (the env is reset inside the step).  Pass it to
    NativeEvaluator.run / evaluate as `recorder`; they bind it around their library calls, so the handle never keeps it."""

    def __init__(self, env, env_ids, capacity, frames=None, frame_every=1, debug=True):
        torch = _torch()
        self.env = env
        self.env_ids = [int(e) for e in env_ids]
        self.capacity, self.frame_every, self.debug = int(capacity), int(frame_every), bool(debug)
        self.frame_size = None if frames is None else (int(frames[0]), int(frames[1]))
        R, Cp, D, dev = len(self.env_ids), self.capacity, env.states_history, env.device
        if R < 1 or R > N.EVAL_REC_MAX_ENVS or Cp < 1 or self.frame_every < 1:
            raise ValueError("EvalRecorder: 1..%d tracked envs, capacity >= 1 and frame_every >= 1" % N.EVAL_REC_MAX_ENVS)
        self._ids = (C.c_int32 * R)(*self.env_ids)
        with torch.cuda.device(dev):
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
            self.obs, self.next_obs = z((R, Cp, D), torch.float64), z((R, Cp, D), torch.float64)
            self.act, self.logp, self.value = z((R, Cp), torch.int32), z((R, Cp), torch.float32), z((R, Cp), torch.float32)
            self.reward, self.done, self.flags = z((R, Cp), torch.float64), z((R, Cp), torch.uint8), z((R, Cp), torch.uint8)
            self.cursor, self.overflow_count = z((R,), torch.int32), z((R,), torch.int32)
            self.term_obs = z((env.num_envs, D), torch.float64)
            self.frames = None
            if self.frame_size is not None:
                W, H = self.frame_size
                self.frames = z((R, (Cp + self.frame_every - 1) // self.frame_every, W, H, 3), torch.uint8)

    def record(self):
        """The ssg_eval_recorder record of these buffers."""
        rec = N.EvalRecorderRecord()
        rec.struct_size, rec.n_tracked, rec.capacity = C.sizeof(N.EvalRecorderRecord), len(self.env_ids), self.capacity
        rec.env_ids = C.cast(self._ids, C.POINTER(C.c_int32))
        rec.dev_obs, rec.dev_next_obs = self.obs.data_ptr(), self.next_obs.data_ptr()
        rec.dev_act, rec.dev_logp, rec.dev_value = self.act.data_ptr(), self.logp.data_ptr(), self.value.data_ptr()
        rec.dev_reward, rec.dev_done, rec.dev_flags = self.reward.data_ptr(), self.done.data_ptr(), self.flags.data_ptr()
        rec.dev_cursor, rec.dev_overflow, rec.dev_term_obs = self.cursor.data_ptr(), self.overflow_count.data_ptr(), self.term_obs.data_ptr()
        if self.frames is not None:
            rec.dev_frames = self.frames.data_ptr()
            rec.frame_width, rec.frame_height = self.frame_size
            rec.frame_every, rec.frame_flags = self.frame_every, 1 if self.debug else 0
        return rec

    def bind(self):
        rec = self.record()
        self.env.call("ssg_set_eval_recorder", C.byref(rec))

    def unbind(self):
        self.env.call("ssg_set_eval_recorder", None)

    def reset(self):
        """Zero the cursors and the overflow counts: the next evaluation records from row 0."""
        self.cursor.zero_()
        self.overflow_count.zero_()

    @property
    def steps(self):
        """numpy int32 [R]: the steps kept per slot."""
        return self.cursor.cpu().numpy()

    @property
    def overflow(self):
        """numpy int32 [R]: the counted steps per slot that found it full."""
        return self.overflow_count.cpu().numpy()

    def numpy(self):
        """Every buffer as a numpy array, keyed as record_walk keys them (plus `frames` [R, ceil(C / S), W, H, 3], or None)."""
        out = {k: getattr(self, k).cpu().numpy() for k in RECORD_ROWS}
        out.update(cursor=self.steps, overflow=self.overflow, frames=None if self.frames is None else self.frames.cpu().numpy())
        return out

    def episodes(self):
        """Per slot, the list of its recorded episodes (split_episodes)."""
        return split_episodes(self.numpy(), self.frame_every)

    def as_rollouts(self):
        """rollout.py's structure: a list of episodes, each a list of [state, action, next_state, reward, done]."""
        return rollouts_of(self.episodes())


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

    def run(self, policy_or_population, episodes, n_steps, greedy=True, seed=0, step0=0, uniforms=None, recorder=None):
        """One ssg_evaluate / ssg_pop_evaluate call: n_steps iterations enqueued on the current stream, no synchronisation.  uniforms:
        float32 [n_steps, N] rows for the sampled mode.  Continues the carries as they stand.  recorder: an EvalRecorder on this env,
        bound for the duration of the library call (it continues at its cursors) and unbound on every way out."""
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
        if recorder is not None:
            if recorder.env is not env:
                raise ValueError("evaluate: the recorder belongs to another env")
            recorder.bind()
        try:
            env.enqueue("ssg_pop_evaluate" if population else "ssg_evaluate", C.byref(rec), C.byref(ev))
        finally:
            if recorder is not None:
                recorder.unbind()
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
        p = [env._arg(t, dt, env.num_envs, "evaluate: " + what) for t, dt, what in
             ((reward, torch.float64, "reward"), (done, torch.uint8, "done"), (flags, torch.uint8, "flags"))]
        env.enqueue("ssg_eval_account", int(episodes), *p, self.carry_return.data_ptr(), self.carry.data_ptr(), self.env_stats.data_ptr())
        self.steps += 1

    def reduce(self, n_members=1):
        """ssg_eval_reduce: int64 [n_members, 8] column sums of each member's rows of env_stats (a view of this object's buffer); a
        member's rows are its slice of the env's set_population_slices when one is bound."""
        env = self.env
        P = int(n_members)
        sizes = env.population_slices if P > 1 else None  # (one policy's reduce is over the whole handle)
        if P < 1 or P > N.POP_MAX_MEMBERS or (len(sizes) != P if sizes is not None else env.num_envs % P):
            raise ValueError("evaluate: %d envs do not split into %d member slices" % (env.num_envs, P))
        env.enqueue("ssg_eval_reduce", P, self.env_stats.data_ptr(), self.member_stats.data_ptr())
        return self.member_stats[:P]

    def evaluate(self, policy_or_population, episodes, greedy=True, max_steps=None, seed=0, step0=0, uniforms=None, reset=True, chunk=128,
                 recorder=None):
        """Run until every env has counted `episodes` episodes, or for max_steps steps (default episodes * env.cfg.max_steps, which
        always suffices: an episode cannot outlive max_steps).  Steps are enqueued in chunks of `chunk`; after each chunk ONE device
        scalar is read, the minimum over the envs of the episodes counted.  reset=True resets the env and zeroes the carries first;
        reset=False continues both.  uniforms: float32 [>= max_steps, N] for the sampled mode (row k drives step k of this call).
        Returns a dict: per_env int64 [N, 8], per_member int64 [P, 8] (device tensors), the derived per-member floats (numpy [P]:
        return_mean, length_mean, collision_rate, out_of_bounds_rate, max_steps_rate, no_goals_left_rate, goals_per_episode),
        complete (every env reached `episodes`) and steps (run by this call).  recorder: an EvalRecorder that records its envs
        during the run (reset=True also zeroes its cursors); nothing else in the result changes."""
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
            if recorder is not None:
                recorder.reset()
        done_steps, complete = 0, False
        while done_steps < max_steps and not complete:
            k = min(chunk, max_steps - done_steps)
            self.run(pol, E, k, greedy=greedy, seed=seed, step0=int(step0) + done_steps,
                     uniforms=uniforms[done_steps: done_steps + k] if uniforms is not None else None, recorder=recorder)
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
