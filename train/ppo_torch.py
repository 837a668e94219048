#!/usr/bin/env python3
"""Trainer glue demo: a minimal PPO loop in plain PyTorch driving ShipVecEnv with zero-copy
device tensors — the role SubprocVecEnv + PPO2 play in the reference's train/stable_baselines/ppo.py:84-123, without
stable-baselines (absent from this image).  The env side is the only point: observations, rewards and dones never
leave the GPU; the policy is a small MLP in fp32.

    python train/ppo_torch.py --envs 4096 --updates 20 [--mode eager|graph|pingpong|native] [--update torch|native] [--separate-value]
                              [--eval-every U --eval-episodes E] [--obs-filter [--save-obs-filter FILE]]
                              [--norm-reward [--reward-clip C]]
                              [--save FILE [--save-every U]] [--save-best FILE] [--resume FILE] [--gpus W]
                              [--report [--report-kl]] [--progress FILE] [--job-obs-filter] [--job-norm-reward [--reward-clip C]]
                              [--job-report [--job-report-kl] [--job-report-shards]] [--job-progress FILE]
                              [--lr-schedule SPEC] [--clip-schedule SPEC] [--ent-schedule SPEC] [--total-timesteps T]

Four ways to run the rollout loop (the reference's `model.learn` -> runner.run(): one `env.step(actions)` per policy
forward, train/stable_baselines/ppo.py:84-100,122-123) — same arithmetic, same results bit for bit:

* ``eager``    — every rollout step launches the policy forward, the action sampling, ``ssg_step`` and the buffer writes one
                 kernel at a time from Python (a dozen launches and their host overhead per step);
* ``graph``    — that whole step — policy forward + sampling + ``ssg_step`` + buffer writes — is captured ONCE as a HIP graph
                 (a 1-ship handle on a shared bank launches with constant arguments, include/shipsim.h) and replayed per step:
                 one host call per rollout step;
* ``pingpong`` — the batch is split into two halves (two ShipVecEnv shards, global env ids and so results unchanged), each
                 with its own graph on its own stream: half A's env step runs while half B's policy forward does;
* ``native``   — the policy forward + sampling run on the device inside the library (ship_sim_gym_amd/policy.py, ABI 9): the
                 whole rollout is ONE ``env.rollout_policy`` call that enqueues {policy kernel, ``ssg_step``} per step from C, then the
                 buffers' dtype conversions once per rollout; ``policy.refresh()`` re-packs the parameters after each PPO update.
                 Same uniforms, same formulas; the MLP's f32 sums are the kernel's own fmaf chains, so logp / value agree with the
                 PyTorch modes to rounding and an action differs only where a uniform lies within rounding of a CDF boundary.

Two ways to run the update after each rollout (GAE, advantage normalisation, epochs x minibatches of loss + backward + Adam):

* ``torch``  — eager PyTorch: the GAE loop below, autograd and torch.optim.Adam on the module (the default);
* ``native`` — (``--mode native`` only) ship_sim_gym_amd/ppo.py's NativePPO: GAE and the whole update on the device from two library
               calls, on the packed parameters the native rollout reads (no refresh); the minibatches are the same randperm chunks,
               drawn from the same generator.  Same loss, same conventions; the parameters agree with the torch update's to f32
               rounding (the module is loaded from the packed buffer at the end, NativePPO.load_into).

``--eval-every U`` (``--mode native`` only; default off): every U updates the current policy is evaluated greedily for
``--eval-episodes`` episodes per env on a second ShipVecEnv of its own (ship_sim_gym_amd/evaluate.py; the reference's
train/rllib/rollout.py:8-26), so the training envs are not disturbed, and the result is printed.

``--obs-filter`` (``--mode native`` only; default off): observations are normalised by a running mean / std filter on the device
(ship_sim_gym_amd/obs_filter.py — RLlib's default MeanStdFilter, Stable-Baselines' VecNormalize) instead of the fixed division by the
largest bound: every rollout step first merges its observations into the statistics, then normalises them; the ``--eval-every`` env
gets a frozen view of the same statistics.  With ``--update native`` the per-update loss terms are printed as well.
``--save-obs-filter FILE`` saves the statistics (``ObsFilter.state_dict``) for train/evaluate_native.py ``--obs-filter FILE``.

``--norm-reward`` (``--mode native --update native`` only; default off): the rewards GAE sees are divided by a running standard deviation
of the per-env discounted return, kept on the device (ship_sim_gym_amd/ret_filter.py — the reward half of Stable-Baselines'
VecNormalize, its default): one library call per rollout between ``rollout_policy`` and GAE; the raw rewards, which the logged
statistics read, stay as they are.  ``--reward-clip C`` clamps the normalised rewards to +-C (default 10, VecNormalize's; 0: none).

``--save FILE`` writes a checkpoint at the end (ship_sim_gym_amd/checkpoint.py; the reference's ``model.save``,
train/stable_baselines/ppo.py:100), ``--save-every U`` also after every U updates, ``--save-best FILE`` after every update whose
episode_reward_mean — the mean return of the episodes that ended during it — exceeds the best so far (the reference callback's
best_model.pkl, :25-52; an update in which no episode ended never writes).  With ``--mode native --update native`` a file holds the
policy, the trainer (Adam moments, step and update counts), both filters, the env's snapshot, this loop's state (the generator, the
history, the best score) and the run's arguments, and ``--resume FILE`` continues that run bit for bit: repeat the original command
line and add ``--resume``; ``--updates`` stays the TOTAL and may be raised, the ``--save*`` and ``--eval-*`` options may change, any
other argument that differs from the file's is refused.  In the other modes ``--save`` writes the policy alone (the torch optimiser's
state is out of scope), which train/evaluate_native.py ``--checkpoint FILE`` reads and ``--resume`` refuses.

``--report`` (``--mode native --update native`` only; default off): after every update one line with the explained variance of the value
network over the rollout and the means of the policy loss, value loss, entropy and clip fraction over the update's minibatches —
what PPO2's verbose=1 prints per update (train/stable_baselines/ppo.py:88-90) — reduced on the device by two launches and read with
one copy (ship_sim_gym_amd/report.py, ssg_ppo_report).  ``--report-kl`` adds how far the update moved the policy (the approximate KL,
PPO2's approxkl and the clip fraction over the whole batch under the new parameters) for one more policy forward over the batch;
``--progress FILE`` writes every update's record as a CSV row (PPO2's progress.csv) and, with ``--resume``, cuts the file back to the
checkpoint's update first.  The three may change between a run and its resumption; without them nothing is computed or printed.
More than one rank refuses them: a job reports through ``--job-report``.

``--gpus W`` (``--mode native --update native`` only): ONE policy trained data-parallel on W ranks, one per GPU, as the RLlib scripts
train one policy from the experience of their workers (train/rllib/ppo.py:34-35, train/rllib/pbt.py:57-58).  The script starts the W
rank processes itself and waits for them; under a launcher's environment (``RANK`` / ``WORLD_SIZE`` > 1) it is a rank itself.
``--envs`` is the job's total: rank r owns the global envs of ``sharding.shard_range``, every rank builds the same policy from the
seed and draws the whole job's uniforms, and the update goes through ship_sim_gym_amd/dp.py's ``DataParallelPPO`` (local gradients,
an all-gather of the rows, the same apply on every rank: no parameter broadcast).  Rank 0 logs the job-wide episode statistics,
evaluates and writes ``--save`` (the policy and the trainer); every rank prints a checksum of its parameters, and the lines agree.
``--resume``, ``--save-every``, ``--obs-filter``, ``--norm-reward`` and ``--adv-norm minibatch`` are refused with more than one rank
(the last three have job-wide forms: ``--job-obs-filter``, ``--job-norm-reward``, ``--job-adv-norm minibatch``).
``SSG_TRAIN_SHARE_DEVICE=1`` (tests on a one-GPU box) puts every rank on device 0 over gloo.

``--job-obs-filter`` (``--mode native --update native`` only, one rank or more; not together with ``--obs-filter``): the running
observation filter for a job, synchronised as RLlib synchronises its workers' filters (``ObsFilter(job=True)``,
ship_sim_gym_amd/obs_filter.py).  During a rollout a rank normalises with its own state, the job's statistics as of the last
synchronisation plus its own rows since; after every rollout, before GAE, the ranks all-gather what they added and every rank merges
the rows with the same arithmetic, so the states agree bit for bit.  Rank 0 evaluates through a frozen view, ``--save`` gains the
``obs_filter`` section, which train/evaluate_native.py ``--checkpoint FILE`` applies, and every rank prints a checksum of the filter's
state beside the parameters'.

``--job-norm-reward`` (``--mode native --update native`` only, one rank or more; not together with ``--norm-reward``; ``--reward-clip``
applies): return normalisation for a job, the ``VecNormalize(norm_reward=True)`` a Stable-Baselines user gets around the whole
SubprocVecEnv (``ReturnFilter(job=True)``, ship_sim_gym_amd/ret_filter.py).  Between the rollout and GAE every rank reduces its shard
to one statistics row per step, the ranks all-gather the [horizon, 4] rows once, and every rank chains the same rows in the same
order: the state is that of one filter over all the job's envs, bit-identical on every rank, and with one rank it is ``--norm-reward``'s
bit for bit.  ``--save`` holds the ``ret_filter`` section (rank 0's: the job's state and rank 0's returns in flight), with one rank
``--resume`` continues from it, and every rank prints a checksum of the filter's state beside the parameters'.

``--job-report`` (``--mode native --update native`` only, one rank or more; not together with ``--report`` / ``--report-kl`` /
``--progress``: one report per update): the update report of a job, taken over the experience of all ranks as RLlib takes
vf_explained_var and kl over its workers' (train/rllib/ppo.py:34-35).  After the update every rank reduces its shard to one row of f64
sums, the ranks all-gather the rows once, and every rank forms the same record from them in rank order (``job_report``,
ship_sim_gym_amd/report.py; ssg_ppo_report_sums / ssg_ppo_report_rows); rank 0 prints the line.  ``--job-report-kl`` adds the
post-update group, ``--job-report-shards`` one line per rank with its shard's samples and explained variance, and ``--job-progress
FILE`` has rank 0 write the job's record as ``--progress`` writes a rank's (``timesteps`` counts the job's ``--envs``); each implies
``--job-report``.  With one rank the record is ``--report``'s bit for bit, and ``--resume`` cuts the file back likewise.
Populations across ranks and multi-rank resume stay out of scope.

``--job-adv-norm minibatch`` (``--mode native --update native`` only, one rank or more; not together with ``--adv-norm minibatch``):
PPO2's per-minibatch advantage normalisation for a job, over the minibatch of all workers' samples as PPO2 over a SubprocVecEnv takes
it (train/stable_baselines/ppo.py:88-90,122-123).  Before the first gradient of an update every rank sums adv, adv^2 and 1 over each
of its epochs x chunks minibatches in one pass, the ranks all-gather the blocks once, and every rank forms the same table of
{mean, std + eps} rows in rank order (``DataParallelPPO(job_adv_norm="minibatch")``, ship_sim_gym_amd/dp.py;
ssg_ppo_minibatch_adv_sums / ssg_ppo_set_minibatch_adv_rows); the per-minibatch loop exchanges nothing more than it did.  With one
rank the parameters are ``--adv-norm minibatch``'s bit for bit; every rank prints the parameter checksum, one rank too.

``--job-episode-log FILE`` (``--mode native --update native`` only, one rank or more; not together with ``--episode-log``;
``--episode-log-capacity`` sizes its ring): the episode log of a job, over the episodes of all ranks as SubprocVecEnv + Monitor +
load_results give them to the reference (train/stable_baselines/ppo.py:7-8,25-52,122-123).  After every rollout each rank packs its
shard's finished episodes into one fixed-size block, the ranks all-gather the blocks once, and every rank merges them into the same
ring in the order one log over all the job's envs would keep (``EpisodeLog(job=True)``, ship_sim_gym_amd/episode_log.py;
ssg_job_episode_log_shard / ssg_job_episode_log_merge_blocks).  Every rank holds the same ring, so ``--job-best-window W`` scores ``--save-best``
alike on every rank without a broadcast; rank 0 alone attaches the MonitorWriter, prints the line and writes FILE (``timesteps`` counts
the job's ``--envs``).  ``--save`` holds rank 0's ``episode_log`` section (the job's ring, rank 0's carries); with one rank the file is
``--episode-log``'s in every column but ``t`` and ``--resume`` continues from the section.  ``--episode-log`` and ``--best-window`` stay
refused with more than one rank.

``--lr-schedule SPEC``, ``--clip-schedule SPEC``, ``--ent-schedule SPEC`` (every ``--mode``, either ``--update``, any number of ranks;
default: constants): hyper-parameter schedules of the learning rate, the clip range and the entropy coefficient, piecewise linear in
the timesteps collected (ship_sim_gym_amd/hparam_schedule.py).  SPEC is ``linear:STOP`` — from ``--lr`` / ``--clip`` / the entropy
coefficient's constant 0.01 down to STOP over ``--total-timesteps T``, whose default is ``--updates`` x ``--envs`` x ``--horizon``, the run's
own length: PPO2's rule, so ``--lr-schedule linear:0`` is train/stable_baselines/ppo.py:111-119's ``make_lr_func(s, 0)`` — or absolute
points ``T0:V0,T1:V1,...`` as RLlib writes them (``--lr-schedule 0:1e-3,5000000:1e-4,10000000:1e-5`` is train/rllib/ppo.py:39's).  Before
update u (0-based) the clock is set to u x envs x horizon, envs being the job's total: the timesteps collected before this update's
rollout, PPO2's ``frac = 1 - (update - 1) / nupdates`` in other words; no step parity with RLlib's own timestep counter is claimed.  Both
update paths apply the same values, and an update's log line names them.  The specs are part of a run's configuration: ``--resume`` with
another spec is refused, and the resumed trainer's schedule is the file's, so raising ``--updates`` past a defaulted span continues at the
stop value instead of stretching the decay.  ``--total-timesteps`` is a span, not a stop criterion: ``--updates`` stays the only one.

The sampling noise of a whole rollout is drawn in one call before it (uniforms [horizon, envs], inverse-CDF sampling inside
the step), so a captured step holds no random-number generator state and replays exactly what the eager loop computes.

This is NOT a re-implementation of the reference's trainers (out of scope); it exists to show the batched env plugs
into a GPU-resident training loop and to give `tests/` and `bench.py` an end-to-end caller.
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ship_gym.config import EnvConfig, GameConfig  # noqa: E402  (the reference's import lines, via the alias package)
from ship_sim_gym_amd.vec_env import ShipVecEnv  # noqa: E402
from ship_sim_gym_amd.policy import NativePolicy  # noqa: E402
from ship_sim_gym_amd.ppo import NativePPO  # noqa: E402
from train import loop  # noqa: E402


class ActorCritic(nn.Module):
    """separate_value=False: one body under both heads.  True: the reference trainers' own shape — Stable-Baselines' MlpPolicy
    (train/stable_baselines/ppo.py: net_arch [dict(vf=[64, 64], pi=[64, 64])], tanh) and RLlib's default vf_share_layers=False
    (train/rllib/pbt.py) — a pi tower under the logits and a vf tower under the value, declared in the packed order
    pi_body, pi, vf_body, v (ship_sim_gym_amd/policy.py)."""

    def __init__(self, obs_dim, n_actions, hidden=64, separate_value=False):
        super().__init__()
        tower = lambda: nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh())  # noqa: E731
        self.separate_value = bool(separate_value)
        if not self.separate_value:
            self.body = tower()
            self.pi = nn.Linear(hidden, n_actions)
            self.v = nn.Linear(hidden, 1)
        else:
            self.pi_body = tower()
            self.pi = nn.Linear(hidden, n_actions)
            self.vf_body = tower()
            self.v = nn.Linear(hidden, 1)

    def forward(self, x):
        if self.separate_value:
            return self.pi(self.pi_body(x)), self.v(self.vf_body(x)).squeeze(-1)
        h = self.body(x)
        return self.pi(h), self.v(h).squeeze(-1)


def normalise(obs, scale):
    """obs is float64 with -1 for "nothing yet"; positions/lidar in map units, rudder in degrees, angle in rad."""
    return (obs / scale).float()


class Shard(object):
    """One env shard of the rollout and everything a rollout step of it reads or writes, at fixed addresses (what a captured
    step needs): the env's own output tensors, the rollout buffers [horizon, n, ...] and a device-side step index."""

    def __init__(self, env, net, scale, horizon):
        self.env, self.net, self.scale, self.horizon = env, net, scale, horizon
        n, D, dev = env.num_envs, env.states_history, env.device
        self.n = n
        f32 = dict(dtype=torch.float32, device=dev)
        self.buf_obs = torch.zeros((horizon, n, D), **f32)
        self.buf_act = torch.zeros((horizon, n), dtype=torch.int64, device=dev)
        self.buf_logp, self.buf_val = torch.zeros((horizon, n), **f32), torch.zeros((horizon, n), **f32)
        self.buf_rew, self.buf_done = torch.zeros((horizon, n), **f32), torch.zeros((horizon, n), **f32)
        self.noise = torch.zeros((horizon, n), **f32)           # uniforms of the whole rollout, drawn before it
        self.t = torch.zeros(1, dtype=torch.int64, device=dev)  # the step index, advanced by the step itself
        self.act_i32 = torch.zeros(n, dtype=torch.int32, device=dev)
        self.graph = None
        self.stream = None

    def step(self):
        """ONE rollout step of this shard: policy forward on the env's current observation, inverse-CDF sampling with this
        step's uniforms, ssg_step (the env rewrites its obs / reward / done in place; done envs are reset in-kernel), and the
        rollout buffers' rows of this step.  Every address it touches is fixed, so it can run eagerly or be captured."""
        env, t = self.env, self.t
        x = normalise(env.obs, self.scale)
        with torch.no_grad():
            logits, val = self.net(x)
            logp_all = torch.log_softmax(logits, dim=-1)
            cdf = logp_all.exp().cumsum(dim=-1)
            u = self.noise.index_select(0, t)[0]
            act = (u.unsqueeze(-1) > cdf[:, :-1]).sum(dim=-1)                 # in 0 .. n_actions - 1
            logp = logp_all.gather(-1, act.unsqueeze(-1)).squeeze(-1)
        self.act_i32.copy_(act)
        self.buf_obs.index_copy_(0, t, x.unsqueeze(0))
        self.buf_act.index_copy_(0, t, act.unsqueeze(0))
        self.buf_logp.index_copy_(0, t, logp.unsqueeze(0))
        self.buf_val.index_copy_(0, t, val.unsqueeze(0))
        _, rew, done, _ = env.step_tensor(self.act_i32)
        self.buf_rew.index_copy_(0, t, rew.float().unsqueeze(0))
        self.buf_done.index_copy_(0, t, done.float().unsqueeze(0))
        t.add_(1)

    def capture(self, stream):
        """Capture step() as a HIP graph on `stream` (after one eager step on a scratch copy of nothing: the library's kernels are
        prepared by the env's reset + the warm-up step the caller ran).  The capture itself executes nothing."""
        self.stream = stream
        g = torch.cuda.CUDAGraph()
        stream.wait_stream(torch.cuda.current_stream(self.env.device))
        with torch.cuda.stream(stream):
            with torch.cuda.graph(g, stream=stream):
                self.step()
        torch.cuda.current_stream(self.env.device).wait_stream(stream)
        self.graph = g


def env_columns(env):
    """The env's body / episode state columns (clones): what two runs that stepped the same envs the same way must agree on.  (Not the
    whole state blob: its reset counters also count the extra reset a graph run does after its warm-up step.)"""
    from ship_sim_gym_amd import _native as N
    return {name: env.field(getattr(N, name)).clone() for name in
            ("F_X", "F_Y", "F_VX", "F_VY", "F_ANGLE", "F_W", "F_LIDAR", "F_RUDDER", "F_STEP_COUNT", "F_MAP_ID", "F_GOAL_MASK", "F_CUM_REWARD")}


def job_ranks():
    """(rank, world) of the process group this process has joined; (0, 1) without one: the single-process run."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def make_shards(envs, mode, net, device, horizon, n_maps=64, env_kw=None, env_range=None):
    """The rollout's env shards: one ShipVecEnv, or (pingpong) two halves that together are the same batch — global env ids,
    map assignment and therefore every result are those of the unsplit batch (ship_sim_gym_amd/sharding.py).  env_range = (lo, hi):
    this rank's shard of a data-parallel job's envs, global ids [lo, hi), instead of all of them."""
    env_kw = dict(env_kw or {})
    sizes = [envs] if mode != "pingpong" else [envs - envs // 2, envs // 2]
    shards, base = [], 0
    if env_range is not None:
        sizes, base = [env_range[1] - env_range[0]], env_range[0]
    for n in sizes:
        env = ShipVecEnv(n, GameConfig, EnvConfig, device=device, n_maps=n_maps, env_id_base=base, **env_kw)  # was: SubprocVecEnv([make_env()]*n)
        scale = torch.full((env.states_history,), float(max(env.bounds)), dtype=torch.float64, device=device)
        shards.append(Shard(env, net, scale, horizon))
        base += n
    return shards


def rollout(shards, horizon, mode, gen, policy=None, job=None):
    """`horizon` policy-in-the-loop steps of every shard; returns the rollout buffers concatenated over the shards (env axis).
    mode "native" (one shard, `policy` = its NativePolicy) also returns "last_val", the device's bootstrap value.  job = (lo, hi, total):
    a rank of a data-parallel job draws the WHOLE job's uniforms (every rank the same, from the same generator) and samples with its
    own columns [lo, hi), so the job's rollout is the single process's over `total` envs."""
    full = torch.rand((horizon, sum(sh.n for sh in shards) if job is None else job[2]), generator=gen, device=shards[0].noise.device)
    if job is not None:
        full = full[:, job[0]: job[1]].contiguous()
    if mode == "native":
        sh = shards[0]
        o = sh.env.rollout_policy(policy, horizon, uniforms=full, out=getattr(sh, "native_out", None))
        sh.native_out = o
        return {"obs": o["obs"], "act": o["act"].long(), "logp": o["logp"], "val": o["val"], "rew": o["rew"].float(),
                "done": o["done"].float(), "last_val": o["last_val"]}
    base = 0
    for sh in shards:  # (one draw for the whole batch, split by env: a split batch samples with the unsplit batch's uniforms)
        sh.noise.copy_(full[:, base: base + sh.n])
        sh.t.zero_()
        base += sh.n
    if mode == "eager":
        for _ in range(horizon):
            shards[0].step()
    elif mode == "graph":
        g = shards[0].graph
        for _ in range(horizon):
            g.replay()
    else:  # pingpong: both graphs every step, each on its own stream — A's env step overlaps B's policy forward
        cur = torch.cuda.current_stream(shards[0].env.device)
        for sh in shards:
            sh.stream.wait_stream(cur)
        for _ in range(horizon):
            for sh in shards:
                with torch.cuda.stream(sh.stream):
                    sh.graph.replay()
        for sh in shards:
            cur.wait_stream(sh.stream)
    cat = (lambda name: torch.cat([getattr(sh, name) for sh in shards], dim=1)) if len(shards) > 1 else (lambda name: getattr(shards[0], name))
    return {k: cat("buf_" + k) for k in ("obs", "act", "logp", "val", "rew", "done")}


# what a resumed run may change: everything else in train()'s arguments is the run's configuration (the checkpoint's "config" section)
CONFIG_EXEMPT = ("updates", "save", "save_every", "save_best", "save_obs_filter", "resume", "eval_every", "eval_episodes", "eval_envs", "log",
                 "return_details", "report", "report_kl", "progress", "job_report", "job_report_kl", "job_progress", "job_report_shards")
RESUME_SECTIONS = ("policy", "trainer", "env", "loop", "config")
open_resume = loop.open_resume  # (importable from here, as it was)


def run_config(**kwargs):
    """The "config" section of a run of train(**kwargs): its effective arguments without CONFIG_EXEMPT, as plain data."""
    return loop.run_config(train, CONFIG_EXEMPT, kwargs)


# What needs what, once, for parse_args (ap.error) and train() (ValueError).  NEEDS: a need's flag, its spelling in train(), when it is met.
# A row of REQUIREMENTS: the name in train() ("ranks": the job's size), the flag, when it is on, its needs, refused with > 1 rank?, why.
NEEDS = {"mode": ("--mode native", "mode='native'", lambda a: a.mode == "native"),
         "update": ("--update native", "update='native'", lambda a: a.update == "native"),
         "obs_filter": ("--obs-filter", "obs_filter=True", lambda a: bool(a.obs_filter)),
         "save": ("--save", "save", lambda a: bool(a.save)),
         "episode_log": ("--episode-log", "episode_log", lambda a: bool(a.episode_log)),
         "job_episode_log": ("--job-episode-log", "job_episode_log", lambda a: bool(getattr(a, "job_episode_log", None)))}
REQUIREMENTS = (  # (a row that needs more stands before the row of what it needs: the refusal then names the flag that asks for most)
    ("save_obs_filter", "--save-obs-filter", lambda a: bool(a.save_obs_filter), ("mode", "obs_filter"), True, "it saves that filter's statistics"),
    ("obs_filter", "--obs-filter", lambda a: bool(a.obs_filter), ("mode",), True, "the filter runs inside the native policy launch"),
    ("norm_reward", "--norm-reward", lambda a: bool(a.norm_reward), ("mode", "update"), True, "it runs between the native rollout and the device's GAE"),
    ("timeout_bootstrap", "--timeout-bootstrap", lambda a: bool(a.timeout_bootstrap), ("mode", "update"), False,
     "the native rollout hands the terminal observation's value to the device's GAE; the torch update has no time-out bootstrap"),
    ("eval_every", "--eval-every", lambda a: bool(a.eval_every), ("mode",), False, "the evaluation runs the native policy on the device"),
    ("perm", "--perm native", lambda a: a.perm == "native", ("update",), False, "the library draws the permutations of the device update"),
    ("resume", "--resume", lambda a: bool(a.resume), ("mode", "update"), True, "it restores the device trainer's state"),
    ("save_every", "--save-every", lambda a: bool(a.save_every), ("save",), True, "the file it rewrites"),
    ("adv_norm", "--adv-norm minibatch", lambda a: a.adv_norm == "minibatch", (), True, "a rank's minibatch statistics are not the job's"),
    ("ranks", "more than one rank (--gpus / WORLD_SIZE)", lambda a: a.ranks > 1, ("mode", "update"), False, "the ranks train through the device update"),
    ("update", "--update native", lambda a: a.update == "native", ("mode",), False, "the update runs on the native policy's packed parameters"),
)


# The episode log's rows, in the same form and walked by the same function, ahead of the rows above.
EPISODE_LOG_REQUIREMENTS = (
    ("best_window", "--best-window", lambda a: bool(a.best_window), ("episode_log",), True, "the window is over the log's last episodes"),
    ("episode_log", "--episode-log", lambda a: bool(a.episode_log), ("mode", "update"), True,
     "it reads the native rollout's reward / done / flags rows; a job's ranks would each hold a log of their own envs (the job's log: "
     "--job-episode-log)"),
)


# The job-wide episode log's rows, likewise: any number of ranks; not together with the handle's own log (JOB_EXCLUDES below).
JOB_EPISODE_LOG_REQUIREMENTS = (
    ("job_best_window", "--job-best-window", lambda a: bool(getattr(a, "job_best_window", 0)), ("job_episode_log",), False,
     "the window is over the job log's last episodes"),
    ("job_episode_log", "--job-episode-log", lambda a: bool(getattr(a, "job_episode_log", None)), ("mode", "update"), False,
     "the ranks' blocks of finished episodes are gathered once per rollout, from the native rollout's reward / done / flags rows"),
)


# The update report's rows, likewise (a: getattr, since callers from before the flags pass argument sets without them).
REPORT_REQUIREMENTS = tuple(
    (name, flag, (lambda a, name=name: bool(getattr(a, name, None))), ("mode", "update"), True,
     "the record is reduced from the device update's buffers and stats rows; a job's ranks would each report their own shard")
    for name, flag in (("progress", "--progress"), ("report_kl", "--report-kl"), ("report", "--report")))


# The job-wide observation filter's row, likewise: any number of ranks.  What it cannot be combined with is asked after its needs.
JOB_OBS_FILTER_REQUIREMENTS = (
    ("job_obs_filter", "--job-obs-filter", lambda a: bool(getattr(a, "job_obs_filter", None)), ("mode", "update"), False,
     "the ranks' filters are synchronised between the native rollout and the device's GAE"),
)


# The job-wide return filter's row, likewise: any number of ranks; not together with the plain one.
JOB_NORM_REWARD_REQUIREMENTS = (
    ("job_norm_reward", "--job-norm-reward", lambda a: bool(getattr(a, "job_norm_reward", None)), ("mode", "update"), False,
     "the ranks' rows are gathered between the native rollout and the device's GAE"),
)
# The job-wide per-minibatch advantage normalisation's row, likewise: any number of ranks; not together with the single-handle mode.
JOB_ADV_NORM_REQUIREMENTS = (
    ("job_adv_norm", "--job-adv-norm minibatch", lambda a: getattr(a, "job_adv_norm", "batch") == "minibatch", ("mode", "update"), False,
     "the ranks' sums of every minibatch are gathered once per update, ahead of the device update's gradient calls"),
)
# (what a job-wide filter's or the job-wide episode log's row is not supported together with — the handle's own counterpart —, asked
# after its needs: the argument, its flag, why)
JOB_EXCLUDES = {"job_obs_filter": ("obs_filter", "--obs-filter", "one filter is bound to the env"),
                       "job_norm_reward": ("norm_reward", "--norm-reward", "one filter normalises the rewards"),
                       "job_episode_log": ("episode_log", "--episode-log", "one log records the run's episodes")}
JOB_ADV_NORM_EXCLUDES = ("adv_norm", "--adv-norm minibatch", "a handle has one source of per-minibatch statistics")


# The job's update report's rows, likewise: any number of ranks; not together with the rank's own report (one report per update).
JOB_REPORT_REQUIREMENTS = tuple(
    (name, flag, (lambda a, name=name: bool(getattr(a, name, None))), ("mode", "update"), False,
     "the ranks' sum rows are reduced from the device update's buffers and gathered once per update")
    for name, flag in (("job_progress", "--job-progress"), ("job_report_shards", "--job-report-shards"), ("job_report_kl", "--job-report-kl"),
                       ("job_report", "--job-report")))
JOB_REPORT_EXCLUDES = tuple((name, flag, "one report per update")  # (the flag that implies another stands before it, as above)
                            for name, flag in (("progress", "--progress"), ("report_kl", "--report-kl"), ("report", "--report")))


def excluded_with(name, a):
    """What the row `name` is on together with and is not supported with: (the argument, its flag, why), or three Nones."""
    if name == "job_adv_norm":
        return JOB_ADV_NORM_EXCLUDES if a.adv_norm == "minibatch" else (None, None, None)
    if name in JOB_EXCLUDES:
        other = JOB_EXCLUDES[name]
        return other if getattr(a, other[0]) else (None, None, None)
    if name in (row[0] for row in JOB_REPORT_REQUIREMENTS):
        for other in JOB_REPORT_EXCLUDES:
            if getattr(a, other[0], None):
                return other
    return None, None, None


def check_requirements(args, ranks, error=None):
    """Walk EPISODE_LOG_REQUIREMENTS, JOB_EPISODE_LOG_REQUIREMENTS, JOB_REPORT_REQUIREMENTS, REPORT_REQUIREMENTS, JOB_OBS_FILTER_REQUIREMENTS, JOB_NORM_REWARD_REQUIREMENTS, JOB_ADV_NORM_REQUIREMENTS and REQUIREMENTS over the arguments `args` (a dict) of a run of `ranks` ranks.  The first row that is on and misses a need, or is
    refused with more than one rank, goes to the parser's `error` with the flags in the text, or is a ValueError with train()'s names."""
    a = argparse.Namespace(**dict(args, ranks=ranks))
    rows = EPISODE_LOG_REQUIREMENTS + JOB_EPISODE_LOG_REQUIREMENTS + JOB_REPORT_REQUIREMENTS + REPORT_REQUIREMENTS + JOB_OBS_FILTER_REQUIREMENTS + JOB_NORM_REWARD_REQUIREMENTS + JOB_ADV_NORM_REQUIREMENTS + REQUIREMENTS
    for name, flag, on, needs, one_rank_only, why in rows:
        text = None
        other, other_flag, other_why = excluded_with(name, a) if on(a) else (None, None, None)
        if other and all(NEEDS[k][2](a) for k in needs):
            text = ("%s is not supported together with %s: %s" % (flag, other_flag, other_why) if error else
                    "%s (%s): it is not supported together with %s: %s" % (
                        name, flag, "adv_norm='minibatch'" if name == "job_adv_norm" else "%s=True" % other, other_why))
        elif on(a) and not all(NEEDS[k][2](a) for k in needs):
            text = ("%s needs %s (%s)" % (flag, " ".join(NEEDS[k][0] for k in needs), why) if error else
                    "%s: it needs %s (%s; got mode=%r, update=%r)" % (name, " and ".join(NEEDS[k][1] for k in needs), why, a.mode, a.update))
        elif on(a) and one_rank_only and ranks > 1:
            text = "%s is not supported with more than one rank (%d ranks): %s" % (flag if error else "%s (%s)" % (name, flag), ranks, why)
        if text and error:
            error(text)
        if text:
            raise ValueError(text)


def check_train_arguments(a, ranks):
    """Every host-side refusal of train(**vars(a)), before the first env is built: the values, then REQUIREMENTS."""
    assert a.mode in ("eager", "graph", "pingpong", "native")
    for name, allowed in (("perm", ("torch", "native")), ("adv_norm", ("batch", "minibatch")), ("job_adv_norm", ("batch", "minibatch")),
                          ("update", ("torch", "native"))):
        if getattr(a, name) not in allowed:
            raise ValueError("%s must be %r or %r (got %r)" % ((name,) + allowed + (getattr(a, name),)))
    if a.save_every < 0 or a.eval_every < 0 or a.eval_episodes < 1:
        raise ValueError("save_every and eval_every must be >= 0 and eval_episodes >= 1")
    if a.episode_log_capacity < 1 or a.best_window < 0 or getattr(a, "job_best_window", 0) < 0:
        raise ValueError("episode_log_capacity must be >= 1, best_window and job_best_window >= 0")
    make_hparam_schedules(a)  # (a malformed spec is refused here)
    check_requirements(vars(a), ranks)


ENT_COEF = 0.01  # the entropy coefficient's constant: torch_update's and NativePPO's default
HPARAM_SCHEDULE_FLAGS = (("lr", "lr_schedule", "--lr-schedule"), ("clip", "clip_schedule", "--clip-schedule"),
                         ("ent_coef", "ent_schedule", "--ent-schedule"))


def make_hparam_schedules(a):
    """(the hyper-parameter schedules of a run, {"lr" | "clip" | "ent_coef": HparamSchedule or None}, their span) from its arguments
    (train()'s, or the parsed command line's): a "linear:" spec starts from lr / clip / ENT_COEF and spans total_timesteps, by default the
    run's own length updates * envs * horizon (envs: the job's total).  ValueError for a malformed spec, a span < 1, a clip <= 0."""
    from ship_sim_gym_amd.hparam_schedule import HparamSchedule, check_schedulable
    total = getattr(a, "total_timesteps", None)
    if total is not None and (isinstance(total, bool) or not isinstance(total, int) or total < 1):
        raise ValueError("total_timesteps (--total-timesteps) must be an int >= 1 (got %r)" % (total,))
    span = int(a.updates) * int(a.envs) * int(a.horizon) if total is None else total
    start = {"lr": a.lr, "clip": a.clip, "ent_coef": ENT_COEF}
    out = {}
    for name, arg, flag in HPARAM_SCHEDULE_FLAGS:
        spec = getattr(a, arg, None)
        out[name] = None if spec is None else check_schedulable("%s (%s)" % (arg, flag), name, HparamSchedule.parse(spec, start[name], span))
    return out, span


class LoopState(object):
    """What the loop carries from one update to the next — with the generator's state, the checkpoint's "loop" section: the last update
    done, the history rows, every update's score (the mean return of the episodes that ended during it, -inf when none did), the best
    score and its update (the reference callback's best_model.pkl, train/stable_baselines/ppo.py:25-52) and the env counters so far."""
    KINDS = (("update", int), ("gen_state", torch.Tensor), ("history", list), ("scores", list), ("best", float), ("best_update", int),
             ("episodes", int), ("sum_return", float))

    def __init__(self, episodes=0, sum_return=0.0):
        self.update, self.history, self.scores, self.best, self.best_update, self.episodes, self.sum_return = -1, [], [], float("-inf"), -1, episodes, sum_return

    def state_dict(self, gen):
        return {"update": int(self.update), "gen_state": gen.get_state().cpu().clone(), "history": [list(r) for r in self.history],
                "scores": list(self.scores), "best": float(self.best), "best_update": int(self.best_update),
                "episodes": int(self.episodes), "sum_return": float(self.sum_return)}

    def load_state_dict(self, sd, gen):
        from ship_sim_gym_amd.checkpoint import check_values
        check_values("train: the checkpoint's loop section", sd, self.KINDS)
        gen.set_state(sd["gen_state"])
        self.update, self.history, self.scores = sd["update"], [tuple(r) for r in sd["history"]], list(sd["scores"])
        self.best, self.best_update, self.episodes, self.sum_return = sd["best"], sd["best_update"], sd["episodes"], sd["sum_return"]


def build_run(run, rank, world):
    """Add the run's objects to train()'s arguments, in the order that decides the bits: the global seed, the device generator (seed + 1),
    the probe env, the module (it draws from the global generator), the shards — a rank's own of the job's `envs` —, policy and trainer."""
    from ship_sim_gym_amd import sharding
    env_range = sharding.shard_range(run.envs, rank, world) if world > 1 else None
    torch.manual_seed(run.seed)
    run.rank, run.world, run.dev = rank, world, torch.device(run.device)
    run.gen = torch.Generator(device=run.dev)
    run.gen.manual_seed(run.seed + 1)
    probe = ShipVecEnv(1, GameConfig, EnvConfig, device=run.device, n_maps=1,  # (the observation width follows the beam count)
                       **{k: v for k, v in dict(run.env_kw or {}).items() if k == "n_beams"})
    D, A = probe.states_history, probe.action_space.n
    probe.close()
    run.net = ActorCritic(D, A, hidden=run.hidden, separate_value=run.separate_value).to(run.dev)
    run.opt = torch.optim.Adam(run.net.parameters(), lr=run.lr)
    run.shards = make_shards(run.envs, run.mode, run.net, run.device, run.horizon, env_kw=run.env_kw, env_range=env_range)
    run.env = run.shards[0].env
    if world > 1:
        sharding.broadcast_bank(run.env, src=0)
    for sh in run.shards:
        sh.env.reset_tensor()
    run.policy = NativePolicy.from_actor_critic(run.net, run.shards[0].scale) if run.mode == "native" else None
    perm_seed, run.ppo = run.seed if run.perm == "native" else None, None
    run.schedules, run.span = make_hparam_schedules(run)
    run.now = {"lr": run.lr, "clip": run.clip, "ent_coef": ENT_COEF}  # the current values (the torch update reads them)
    hparams = {k: run.schedules[k] if run.schedules[k] is not None else run.now[k] for k in run.now}  # a float, or its schedule
    if world > 1 or run.job_adv_norm == "minibatch":  # (refuses, on every rank alike, shards that would make different numbers of minibatches)
        from ship_sim_gym_amd.dp import DataParallelPPO
        run.ppo = DataParallelPPO(run.policy, run.env, plan=(run.horizon, run.minibatches), perm_seed=perm_seed,
                                  job_adv_norm=run.job_adv_norm, **hparams)
    elif run.update == "native":
        run.ppo = NativePPO(run.policy, run.env, adv_norm=run.adv_norm, perm_seed=perm_seed, **hparams)
    run.job = None if world == 1 else (env_range[0], env_range[1], run.envs)
    run.n_local = run.envs if world == 1 else env_range[1] - env_range[0]


def capture_graphs(run):
    """One eager warm-up step per shard OUTSIDE the capture (it prepares the library's kernels and hipBLASLt's workspaces), then the envs
    start over; the capture itself runs nothing."""
    for sh in run.shards:
        sh.step()
        sh.env.reset_tensor()
        sh.t.zero_()
    torch.cuda.synchronize()
    for sh in run.shards:
        sh.capture(torch.cuda.Stream(device=run.dev))
    torch.cuda.synchronize()


def episode_stats(run):
    """The episode counters so far: this process's envs', or (every rank calls it: an all-reduce) the whole job's."""
    if run.world > 1:
        from ship_sim_gym_amd import sharding
        return sharding.global_stats(run.env)
    return {k: sum(sh.env.stats()[k] for sh in run.shards) for k in ("sum_return", "episodes", "goals_hit")}


def load_run(run, state, ckpt):
    """Everything is built and bound as the configuration says; now take the saved state over."""
    run.policy.load_state_dict(ckpt["policy"])
    run.ppo.load_state_dict(ckpt["trainer"])
    loop.load_filters(ckpt, run.flt, run.rflt)
    loop.load_episode_log(ckpt, run.eplog)
    run.env.restore(ckpt["env"])
    state.load_state_dict(ckpt["loop"], run.gen)


def write_checkpoint(path, run, state):
    """The checkpoint after update state.update: everything a resumed run needs with the device update, else the policy (for evaluation)."""
    from ship_sim_gym_amd import checkpoint
    sections = dict(loop.filter_sections(run.flt, run.rflt), config=run.config, loop=state.state_dict(run.gen))
    sections.update(loop.episode_log_section(run.eplog))
    if run.ppo is not None:  # (a job's file is rank 0's: the policy and the trainer; per-rank env snapshots are out of scope)
        sections.update(policy=run.policy.state_dict(), trainer=run.ppo.state_dict(), **({"env": run.env.snapshot()} if run.world == 1 else {}))
    else:  # (the torch update trains the module: pack it as evaluation reads it)
        sections["policy"] = (run.policy if run.policy is not None else NativePolicy.from_actor_critic(run.net, run.shards[0].scale)).state_dict()
    checkpoint.save(path, sections)


def native_update(run, u, log):
    """GAE + the whole update on the device, on the rollout's own buffers; perm "native": the library shuffles (a row per epoch, keyed
    by the seed and the update's number), else torch's generator does (the same randperm draws as the torch update)."""
    nb = dict(run.shards[0].native_out)
    run.ppo.gae(nb, run.gamma, run.lam, return_filter=run.rflt)
    n = run.horizon * run.n_local  # (a rank shuffles its own samples)
    rows = None if run.perm == "native" else torch.stack([torch.randperm(n, device=run.dev, generator=run.gen) for _ in range(run.epochs)])
    filters = run.flt is not None or run.rflt is not None
    st_upd = run.ppo.update(nb, rows, run.epochs, run.minibatches, stats=filters or run.report or run.job_report)
    if run.report:
        report_update(run, u, nb, st_upd, log)
    if run.job_report:  # (every rank: the call gathers the ranks' sum rows)
        job_report_update(run, u, nb, st_upd, log)
    if filters:
        pg, vf, ent = (float(v) for v in st_upd[-1, :3])
        notes = []
        if run.flt is not None:
            notes.append("(obs filter: %d rows merged)" % int(run.flt.count[0].item()))
        if run.rflt is not None:
            notes.append("(return filter: %d returns merged, std %.5f)" % (int(run.rflt.count[0].item()), float(run.rflt.denom[0].item())))
        log("update %3d  last minibatch: policy loss %+.5f  value loss %.5f  entropy %.5f  %s" % (u, pg, vf, ent, "  ".join(notes)))


def report_line(rec, extended):
    """The update report's line (rec: one member's record as floats): explained variance, the update's minibatch means and, when they
    were computed, the extended terms and the post-update group."""
    text = "explained variance %+.4f  policy loss %+.5f  value loss %.5f  entropy %.5f  clip fraction %.4f" % (
        rec["explained_variance"], rec["policy_loss"], rec["value_loss"], rec["entropy"], rec["clip_fraction_minibatch"])
    if extended:
        text += "  kl %.6f  grad norm %.4f  kl coef %.4f" % (rec["kl"], rec["grad_norm"], rec["kl_coef"])
    if rec["post"]:
        text += "  after the update: approx kl %.6f  approxkl %.6f  clip fraction %.4f" % (rec["approx_kl"], rec["approxkl_ppo2"], rec["clip_fraction"])
    return text


def report_update(run, u, nb, st_upd, log):
    """--report: one line per update from ssg_ppo_report's record (one copy to the host), and the --progress row."""
    rec = run.ppo.report(nb, stats=st_upd, post=run.report_kl)
    log("update %3d  report: %s" % (u, report_line(rec, st_upd.shape[1] == 8)))
    if run.progress_writer is not None:
        run.progress_writer.write(u, (u + 1) * run.envs * run.horizon, rec, rec["lr"], rec["clip"])


def job_report_update(run, u, nb, st_upd, log):
    """--job-report: the record over the experience of all ranks (every rank calls it: one all-gather of the sum rows, one copy to the
    host); rank 0 logs the line, the shards' own lines and the --job-progress row (log and the writer are rank 0's alone)."""
    rec = run.ppo.job_report(nb, stats=st_upd, post=run.job_report_kl, per_shard=run.job_report_shards)
    log("update %3d  job report (%d ranks, %d samples): %s" % (u, rec["shards"], int(rec["n"]), report_line(rec, st_upd.shape[1] == 8)))
    for r, shard in enumerate(rec.get("shard_records", ())):
        log("update %3d  job report, shard %d: %d samples  explained variance %+.4f" % (u, r, int(shard["n"]), shard["explained_variance"]))
    if run.job_progress_writer is not None:
        run.job_progress_writer.write(u, (u + 1) * run.envs * run.horizon, rec, rec["lr"], rec["clip"])


def torch_update(net, opt, b, last_val, epochs, minibatches, gen, gamma=0.99, lam=0.95, clip=0.2, adv_norm="batch", ent_coef=ENT_COEF):
    """The eager update on a rollout b (obs [horizon, envs, D]; act int64, the rest float32 [horizon, envs]) and the values after its
    last step, on whatever device they are: GAE, then epochs x minibatches of loss, backward, Adam.  One randperm from `gen` per epoch."""
    horizon, envs, D = b["obs"].shape
    dev = b["obs"].device
    adv = torch.zeros(envs, device=dev)
    advs, rets = [None] * horizon, [None] * horizon
    nxt = last_val
    for t in reversed(range(horizon)):           # GAE; a done env's next obs belongs to a fresh episode (auto-reset)
        nonterm = 1.0 - b["done"][t]
        delta = b["rew"][t] + gamma * nxt * nonterm - b["val"][t]
        adv = delta + gamma * lam * nonterm * adv
        advs[t], rets[t] = adv, adv + b["val"][t]
        nxt = b["val"][t]
    b_obs, b_act = b["obs"].reshape(horizon * envs, D), b["act"].reshape(-1)
    b_logp, b_adv, b_ret = b["logp"].reshape(-1), torch.cat(advs), torch.cat(rets)
    if adv_norm == "batch":
        b_adv = (b_adv - b_adv.mean()) / (b_adv.std() + 1e-8)
    n = b_obs.shape[0]
    for _ in range(epochs):
        perm = torch.randperm(n, device=dev, generator=gen)
        for mb in perm.chunk(minibatches):
            logits, val = net(b_obs[mb])
            dist = torch.distributions.Categorical(logits=logits)
            ratio = torch.exp(dist.log_prob(b_act[mb]) - b_logp[mb])
            mb_adv = b_adv[mb]
            if adv_norm == "minibatch":  # PPO2's rule, as the device update applies it: the minibatch's own mean / unbiased std
                mb_std = mb_adv.std() if mb_adv.numel() > 1 else mb_adv.new_zeros(())  # (one sample: a std of 0, not NaN)
                mb_adv = (mb_adv - mb_adv.mean()) / (mb_std + 1e-8)
            pg = -torch.min(ratio * mb_adv, torch.clamp(ratio, 1 - clip, 1 + clip) * mb_adv).mean()
            loss = pg + 0.5 * (val - b_ret[mb]).pow(2).mean() - ent_coef * dist.entropy().mean()
            opt.zero_grad(); loss.backward(); opt.step()


def eager_update(run, b, last_val):
    """torch_update on the module, from the native rollout's last value or a forward on the envs' current observations; then re-pack."""
    if last_val is None:
        with torch.no_grad():
            last_val = torch.cat([run.net(normalise(sh.env.obs, sh.scale))[1] for sh in run.shards])
    for group in run.opt.param_groups:  # (the schedules' current values, set_hparam_clock's; without schedules the constants)
        group["lr"] = run.now["lr"]
    torch_update(run.net, run.opt, b, last_val, run.epochs, run.minibatches, run.gen, run.gamma, run.lam, run.now["clip"], run.adv_norm,
                 ent_coef=run.now["ent_coef"])
    if run.policy is not None:
        run.policy.refresh()


def set_hparam_clock(run, u, log):
    """Before update u (0-based): the hyper-parameter schedules' clock is the timesteps collected so far, u * envs * horizon over the
    job's envs (the same integer on every rank).  The device trainer evaluates its own schedules (a resumed one's are the file's); the
    torch update reads run.now.  With a schedule on, one log line names the current values."""
    t = u * run.envs * run.horizon
    if run.ppo is not None:
        run.ppo.set_timesteps(t)
        run.now = {k: float(getattr(run.ppo.hp, k)) for k in run.now}
        on = any(s is not None for s in run.ppo.schedules.values())
    else:
        run.now = {k: (s.value(t) if s is not None else run.now[k]) for k, s in run.schedules.items()}
        on = any(s is not None for s in run.schedules.values())
    if on:
        log("update %3d  hyper-parameter schedules at %d timesteps: lr %.6g  clip %.6g  entropy coefficient %.6g" % (
            u, t, run.now["lr"], run.now["clip"], run.now["ent_coef"]))


def log_hparam_schedules(run, log):
    """Once per run: the schedules in use and the span a "linear:" spec was given (a resumed device trainer's are the file's)."""
    scheds = run.ppo.schedules if run.ppo is not None else run.schedules
    for name, sched in sorted(scheds.items()):
        if sched is not None:
            log("hyper-parameter schedule of %s: points %s (timesteps, value); this run's span for a linear spec: %d timesteps" % (
                name, sched.state(), run.span))


def account(run, state, u, b, log):
    """After update u: the history row and the update's score (-inf: no episode ended, never a best).  Returns how many ended."""
    st = episode_stats(run)
    mean_ret = st["sum_return"] / max(st["episodes"], 1)
    goals_per_ep = st["goals_hit"] / max(st["episodes"], 1)
    state.update = u
    state.history.append((u, mean_ret, goals_per_ep, float(b["rew"].mean())))
    log("update %3d  episodes %8d  mean return so far %+.3f  goals/episode %.3f  mean step reward %+.4f" % (
        u, st["episodes"], mean_ret, goals_per_ep, state.history[-1][3]))
    ended = st["episodes"] - state.episodes
    state.scores.append((st["sum_return"] - state.sum_return) / ended if ended > 0 else float("-inf"))
    state.episodes, state.sum_return = st["episodes"], st["sum_return"]
    if run.eplog is not None:  # the cycle's one copy of the ring to the host; then the window's score in place of the update's own
        written = run.epwriter.flush() if run.epwriter is not None else 0  # (a job's file is rank 0's; the ring is every rank's, the same bits)
        if run.best_window > 0 and ended > 0:
            state.scores[-1] = run.eplog.mean_last(run.best_window)
        log("update %3d  episode log: %d rows written, %d in all%s" % (u, written, run.eplog.rows_written, (
            "  mean return of the last %d at most: %+.3f" % (run.best_window, state.scores[-1]) if run.best_window > 0 and ended > 0 else "")))
    return ended


def evaluate(run, u, episodes, log):
    """One greedy evaluation on the evaluator's own env: the (update, results) entry of details["evaluations"]."""
    r = run.evaluator.evaluate(run.policy, episodes, greedy=True)
    log("update %3d  greedy evaluation (%d envs x %d episodes): mean return %+.3f  length %.1f  goals/episode %.3f  "
        "collided %.2f  out of bounds %.2f  timed out %.2f" % (
            u, run.evaluator.env.num_envs, episodes, r["return_mean"][0], r["length_mean"][0], r["goals_per_episode"][0],
            r["collision_rate"][0], r["out_of_bounds_rate"][0], r["max_steps_rate"][0]))
    return (u, {k: (v[0] if hasattr(v, "__len__") else v) for k, v in r.items() if k not in ("per_env", "per_member")})


def train(envs=4096, updates=20, horizon=64, epochs=2, minibatches=4, lr=3e-4, gamma=0.99, lam=0.95, clip=0.2,
          device="cuda:0", seed=0, log=print, mode="eager", return_details=False, env_kw=None, update="torch", separate_value=False,
          eval_every=0, eval_episodes=1, eval_envs=None, obs_filter=False, save_obs_filter=None,
          norm_reward=False, reward_clip=10.0, adv_norm="batch", perm="torch", timeout_bootstrap=False, hidden=64,
          save=None, save_every=0, save_best=None, resume=None, episode_log=None, episode_log_capacity=65536, best_window=0,
          report=False, report_kl=False, progress=None, job_obs_filter=False, job_norm_reward=False,
          job_report=False, job_report_kl=False, job_progress=None, job_report_shards=False, job_episode_log=None, job_best_window=0,
          job_adv_norm="batch", lr_schedule=None, clip_schedule=None, ent_schedule=None, total_timesteps=None):
    config = run_config(**dict(locals()))  # (first statement: the arguments, nothing else)
    run = argparse.Namespace(**locals())  # the run record: the arguments and the config; build_run() and the bind step add the objects
    run.report = bool(report or report_kl or progress)  # (--report-kl and --progress imply --report)
    run.job_report = bool(job_report or job_report_kl or job_progress or job_report_shards)  # (likewise)
    # check: every refusal on the host, then the file a run resumes from, before any device work (a wrong command line costs nothing)
    rank, world = job_ranks()
    check_train_arguments(run, world)
    run.best_window = best_window or job_best_window  # (one window: over the handle's log, or over the job's)
    if rank != 0:  # (a data-parallel job trains ONE policy, ship_sim_gym_amd/dp.py: only rank 0 logs, evaluates and saves)
        log = lambda *_, **__: None  # noqa: E731
    ckpt = open_resume(resume, config, loop.resume_sections(RESUME_SECTIONS, obs_filter or job_obs_filter, norm_reward or job_norm_reward, episode_log or job_episode_log), exempt=CONFIG_EXEMPT) if resume else None
    # build, bind, resume
    build_run(run, rank, world)
    eval_env = (ShipVecEnv(int(eval_envs or min(envs, 1024)), GameConfig, EnvConfig, device=device, n_maps=64, **dict(env_kw or {}))
                if eval_every and rank == 0 else None)
    run.flt, run.rflt, run.evaluator = loop.bind_env(run.env, horizon, 1, obs_filter, norm_reward, gamma, reward_clip, timeout_bootstrap, eval_env,
                                                     job_obs_filter=job_obs_filter, job_norm_reward=job_norm_reward)
    if job_episode_log:  # every rank: the ring is the job's, the same bits everywhere; the file is rank 0's
        run.eplog, run.epwriter = loop.bind_episode_log(run.env, job_episode_log, episode_log_capacity, 1, resume, job_rows=horizon, writer=rank == 0)
    else:
        run.eplog, run.epwriter = loop.bind_episode_log(run.env, episode_log, episode_log_capacity, 1, resume)
    run.progress_writer = loop.open_progress(progress, resume)
    run.job_progress_writer = loop.open_progress(job_progress, resume) if rank == 0 else None  # (the job's file is rank 0's)
    if mode in ("graph", "pingpong"):
        capture_graphs(run)
    snapshots, evals, t_roll, t_upd, t_all0 = [], [], 0.0, 0.0, time.perf_counter()
    if (save or save_best) and run.ppo is not None and world == 1:
        run.env.check_snapshot_supported("snapshot")  # (refuse now, not after the training, a handle that cannot be saved)
    st0 = episode_stats(run)
    state = LoopState(st0["episodes"], st0["sum_return"])
    if ckpt is not None:
        load_run(run, state, ckpt)
        for writer in (run.progress_writer, run.job_progress_writer):
            if writer is not None:
                writer.cut_back(state.update)  # (the rows of updates the checkpoint has not seen are written again)
        log("resumed from %s: %d updates done, continuing at update %d of %d" % (resume, state.update + 1, state.update + 1, updates))
    start = state.update + 1
    log_hparam_schedules(run, log)
    for u in range(start, updates):
        set_hparam_clock(run, u, log)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b = rollout(run.shards, horizon, mode, run.gen, run.policy, job=run.job)
        torch.cuda.synchronize()
        t_roll += time.perf_counter() - t0
        native_last_val = b.pop("last_val", None)
        if job_obs_filter:  # every rank: gather what the ranks' rollouts added, merge it alike (the x rows were formed rank-locally)
            run.flt.sync()
        if run.eplog is not None and run.eplog.job:  # every rank: one all-gather of the ranks' blocks, merged alike
            run.eplog.job_append(run.shards[0].native_out)
        elif run.eplog is not None:
            run.eplog.append(run.shards[0].native_out)  # (the rollout's own f64 / u8 rows; no host synchronisation)
        if return_details is True:
            snapshots.append({k: v.clone() for k, v in b.items()})
        t1 = time.perf_counter()
        if run.ppo is not None:
            native_update(run, u, log)
        else:
            eager_update(run, b, native_last_val)
        torch.cuda.synchronize()
        t_upd += time.perf_counter() - t1
        ended = account(run, state, u, b, log)
        if state.scores[-1] > state.best:  # save-best: written at once (an update in which no episode ended scores -inf: never here; --best-window: the score is the log's window mean)
            state.best, state.best_update = state.scores[-1], u
            if save_best and rank == 0:
                write_checkpoint(save_best, run, state)
                log("update %3d  episode_reward_mean %+.3f over %d episodes: the best so far, saved to %s" % (u, state.best, ended, save_best))
        if save and save_every and (u + 1) % save_every == 0:
            write_checkpoint(save, run, state)
        if run.evaluator is not None and (u + 1) % eval_every == 0:
            evals.append(evaluate(run, u, eval_episodes, log))
    # finish
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t_all0
    if save and rank == 0:
        write_checkpoint(save, run, state)
        log("checkpoint after update %d saved to %s" % (state.update, save))
    if run.ppo is not None:
        run.ppo.load_into(run.net)  # the module gets the device-trained parameters (details["params"])
    if world > 1 or job_adv_norm == "minibatch":  # every rank prints it: the ranks hold the same bits, so the lines are the same
        import hashlib
        print("parameter checksum after %d Adam steps: %s" % (
            run.ppo.step, hashlib.sha256(run.policy.params.detach().cpu().numpy().tobytes()).hexdigest()), flush=True)
        if job_obs_filter:
            print("observation filter checksum after %d rows merged: %s" % (
                int(run.flt.count[0].item()), hashlib.sha256(run.flt.state.detach().cpu().numpy().tobytes()).hexdigest()), flush=True)
        if job_norm_reward:
            print("return filter checksum after %d returns merged: %s" % (
                int(run.rflt.count[0].item()), hashlib.sha256(run.rflt.state.detach().cpu().numpy().tobytes()).hexdigest()), flush=True)
    steps = envs * horizon * max(0, updates - start)  # (this process's own; a resumed run did not step the updates it loaded)
    log("rollout (%s): %.1f M env-steps/s with the policy in the loop; whole training loop (rollout + PPO update): %.1f M env-steps/s" % (
        mode, steps / max(t_roll, 1e-9) / 1e6, steps / max(t_all, 1e-9) / 1e6))
    full = return_details is True
    details = {"mode": mode, "rollout_env_steps_per_s": steps / max(t_roll, 1e-9), "training_env_steps_per_s": steps / max(t_all, 1e-9),
               "rollout_us_per_step": t_roll * 1e6 / (horizon * max(1, updates - start)), "rollout_seconds": t_roll, "update_seconds": t_upd, "total_seconds": t_all,
               "snapshots": snapshots, "final_state": [env_columns(sh.env) for sh in run.shards] if full else None,
               "params": [p.detach().clone() for p in run.net.parameters()] if full else None, "evaluations": evals,
               "episode_reward_mean": list(state.scores), "best": state.best, "best_update": state.best_update,
               "env_state": run.env.state.detach().cpu().clone() if full else None}
    details.update(loop.filter_sections(run.flt, run.rflt))
    if run.flt is not None and save_obs_filter:
        torch.save(details["obs_filter"], save_obs_filter)
        log("observation filter statistics (%d rows merged) saved to %s" % (int(details["obs_filter"]["state"][0, 3, 0]), save_obs_filter))
    if run.evaluator is not None:
        run.evaluator.env.close()
    for sh in run.shards:
        sh.graph = None
        sh.env.close()
    return (state.history, details) if return_details else state.history


def make_arg_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--mode", choices=("eager", "graph", "pingpong", "native"), default="graph")
    ap.add_argument("--update", choices=("torch", "native"), default="torch",
                    help="where GAE and the PPO update run: eager PyTorch, or on the device (needs --mode native)")
    ap.add_argument("--separate-value", action="store_true",
                    help="a value network of its own (SB's MlpPolicy, RLlib's vf_share_layers=False) instead of a shared body; every --mode")
    ap.add_argument("--eval-every", type=int, default=0, metavar="U",
                    help="every U updates evaluate the policy greedily on a second env of its own (needs --mode native); 0 = off")
    ap.add_argument("--eval-episodes", type=int, default=1, metavar="E", help="episodes counted per env by each evaluation")
    ap.add_argument("--obs-filter", action="store_true",
                    help="normalise observations with a running mean / std filter on the device (needs --mode native); default: obs / max bound")
    ap.add_argument("--save-obs-filter", default=None, metavar="FILE", help="save the filter's statistics at the end (needs --obs-filter)")
    ap.add_argument("--norm-reward", action="store_true",
                    help="divide the rewards GAE sees by a running std of the discounted return, on the device (needs --mode native "
                         "--update native); default: raw rewards")
    ap.add_argument("--reward-clip", type=float, default=10.0, metavar="C",
                    help="clamp the normalised rewards to +-C (needs --norm-reward or --job-norm-reward; 0: no clamp)")
    ap.add_argument("--adv-norm", choices=("batch", "minibatch"), default="batch",
                    help="normalise the advantages once per rollout, or inside every minibatch as Stable-Baselines' PPO2 does (either --update)")
    ap.add_argument("--perm", choices=("torch", "native"), default="torch",
                    help="who shuffles the update's minibatches: torch.randperm, or the library on the device (needs --update native)")
    ap.add_argument("--timeout-bootstrap", action="store_true",
                    help="GAE bootstraps an episode the clock ended from the value of its terminal observation instead of scoring it as a "
                         "return of 0 (needs --mode native --update native); default: every done alike")
    ap.add_argument("--hidden", type=int, default=64, help="width of the hidden layers (the native policy: a multiple of 16 up to 128)")
    ap.add_argument("--gpus", type=int, default=1, metavar="W",
                    help="train ONE policy data-parallel on W ranks, one per GPU (needs --mode native --update native): this process "
                         "starts the W rank processes and waits for them; --envs is the job's total.  Under a launcher's environment "
                         "(RANK / WORLD_SIZE) the process is a rank itself")
    ap.add_argument("--save", default=None, metavar="FILE",
                    help="write a checkpoint at the end (ship_sim_gym_amd/checkpoint.py): with --mode native --update native everything a "
                         "--resume needs, else the policy alone, for train/evaluate_native.py --checkpoint")
    ap.add_argument("--save-every", type=int, default=0, metavar="U", help="also rewrite --save after every U updates (atomically); 0 = off")
    ap.add_argument("--save-best", default=None, metavar="FILE",
                    help="write a checkpoint after every update whose episode_reward_mean (the mean return of the episodes that ended "
                         "during it) exceeds the best so far")
    loop.add_episode_log_flags(ap)
    ap.add_argument("--best-window", type=int, default=0, metavar="W",
                    help="--save-best compares the mean return of the last W finished episodes (the reference callback's "
                         "np.mean(y[-100:]); needs --episode-log) instead of the mean over the episodes of one update; 0 = off")
    ap.add_argument("--job-episode-log", default=None, metavar="FILE",
                    help="--episode-log for a data-parallel job, one rank or more: the log of the episodes of ALL ranks, in the order one "
                         "log over all the job's envs would keep; the ranks gather one block of records once per rollout and merge them "
                         "alike, bit-identically; rank 0 writes FILE (needs --mode native --update native; not together with "
                         "--episode-log; --episode-log-capacity sizes its ring)")
    ap.add_argument("--job-best-window", type=int, default=0, metavar="W",
                    help="--best-window over the job's log (needs --job-episode-log): every rank computes the same score; 0 = off")
    loop.add_report_flags(ap)
    ap.add_argument("--job-obs-filter", action="store_true",
                    help="the running observation filter for a data-parallel job, one rank or more: every rank normalises with its own "
                         "statistics during a rollout, and after it the ranks merge what they added, bit-identically (needs --mode native "
                         "--update native; not together with --obs-filter)")
    ap.add_argument("--job-norm-reward", action="store_true",
                    help="--norm-reward for a data-parallel job, one rank or more: the running std is that of the returns of all the "
                         "job's envs; the ranks gather one row of statistics per step once per rollout and chain them alike, "
                         "bit-identically (needs --mode native --update native; not together with --norm-reward)")
    ap.add_argument("--job-adv-norm", choices=("batch", "minibatch"), default="batch",
                    help="--adv-norm for a data-parallel job, one rank or more: minibatch normalises the advantages of every minibatch "
                         "by the mean / std over the whole job's minibatch (PPO2's rule over all workers' samples); the ranks gather "
                         "one block of sums once per update and form the same statistics, bit-identically (needs --mode native --update "
                         "native; not together with --adv-norm minibatch)")
    ap.add_argument("--job-report", action="store_true",
                    help="--report for a data-parallel job, one rank or more: the record over the experience of all ranks, from one "
                         "gathered row of sums per rank, bit-identical on every rank; rank 0 prints it (needs --mode native --update "
                         "native; not together with --report / --report-kl / --progress)")
    ap.add_argument("--job-report-kl", action="store_true",
                    help="--report-kl for the job's record: one more policy forward over each rank's batch per update; implies --job-report")
    ap.add_argument("--job-progress", default=None, metavar="FILE",
                    help="rank 0 writes the job's record of every update to FILE as CSV (--progress's format); implies --job-report")
    ap.add_argument("--job-report-shards", action="store_true",
                    help="also print one line per rank: its shard's samples and explained variance; implies --job-report")
    ap.add_argument("--lr", type=float, default=3e-4, help="Adam's learning rate (either --update); the start of --lr-schedule linear:STOP")
    ap.add_argument("--clip", type=float, default=0.2, help="the PPO clip range (either --update); the start of --clip-schedule linear:STOP")
    loop.add_hparam_schedule_flags(ap, "--lr / --clip / the entropy coefficient's 0.01", "--updates x --envs x --horizon")
    ap.add_argument("--resume", default=None, metavar="FILE",
                    help="continue the run a checkpoint was saved from, bit for bit (needs --mode native --update native): repeat the "
                         "original command line; --updates stays the TOTAL and may be raised")
    return ap


def parse_args(argv=None):
    """make_arg_parser().parse_args, then the shared value checks and REQUIREMENTS for the job's size (--gpus, or a launcher's WORLD_SIZE)."""
    ap = make_arg_parser()
    a = ap.parse_args(argv)
    loop.check_flag_values(a, ap.error)
    if a.best_window < 0 or a.job_best_window < 0:
        ap.error("--best-window and --job-best-window must be >= 0")
    if a.gpus < 1 or a.gpus > 64:
        ap.error("--gpus must be in 1..64")
    try:
        make_hparam_schedules(a)
    except ValueError as ex:
        ap.error(str(ex))
    check_requirements(vars(a), max(a.gpus, int(os.environ.get("WORLD_SIZE", "1"))), ap.error)
    return a


def launch_ranks(world, argv):
    """Start `world` fresh rank processes of this script with the same arguments (RANK / LOCAL_RANK / WORLD_SIZE and a free local
    port in their environment), wait for them, and return the first non-zero exit code (0: all succeeded).  When a rank fails the
    others are ended: a rank waiting in a collective for a dead peer would wait for ever."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    rc, left = 0, list(procs)
    while left and rc == 0:
        for p in list(left):
            try:
                code = p.wait(timeout=0.2)
            except subprocess.TimeoutExpired:
                continue
            left.remove(p)
            rc = rc or code
    for p in left:  # (only after a failure)
        p.terminate()
    for p in left:
        try:
            p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
    return rc


def join_job():
    """Join the launcher's process group (RANK / WORLD_SIZE / MASTER_* in the environment) and return this rank's device: nccl
    (RCCL) with one GPU per rank, or — SSG_TRAIN_SHARE_DEVICE=1, for tests on a one-GPU box — gloo with every rank on device 0."""
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    share = os.environ.get("SSG_TRAIN_SHARE_DEVICE") == "1"
    local = 0 if share else int(os.environ.get("LOCAL_RANK", str(rank)))
    if torch.cuda.device_count() <= local:
        sys.exit("train/ppo_torch.py: rank %d needs device %d, the node shows %d (SSG_TRAIN_SHARE_DEVICE=1 shares device 0 over gloo)"
                 % (rank, local, torch.cuda.device_count()))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if share:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    else:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    return dev


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    a = parse_args(argv)
    in_job = "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1
    if a.gpus > 1 and not in_job:
        return launch_ranks(a.gpus, argv)
    device = "cuda:0"
    if in_job:
        if a.gpus > 1 and a.gpus != int(os.environ["WORLD_SIZE"]):
            sys.exit("train/ppo_torch.py: --gpus %d but WORLD_SIZE=%s" % (a.gpus, os.environ["WORLD_SIZE"]))
        device = str(join_job())
    train(device=device, **{k: v for k, v in vars(a).items() if k != "gpus"})  # (every other flag is an argument of train() of the same name)
    if in_job:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
