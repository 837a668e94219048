#!/usr/bin/env python3
"""Population-based training of PPO on the MI355X batched env, entirely on the device: the counterpart of the reference's
train/rllib/pbt.py (:29-43 the scheduler, :47-74 the experiment) that runs without ray — train/rllib_pbt.py is that script with its env
line changed and needs ray; this one needs only the library.

    python train/pbt_native.py --members 16 --envs-per-member 512 --updates 40 --horizon 32 --perturb-every 5 --seed 0
    python train/pbt_native.py --lrs 1e-3,1e-4,1e-5 --no-pbt        # the learning-rate sweep of train/stable_baselines/ppo.py:118-137
    python train/pbt_native.py --mutate-schedule                    # num_sgd_iter and sgd_minibatch_size per member too (pbt.py:40-41)
    python train/pbt_native.py --members 3 --epochs 1,2,4 --minibatches 4,4,8 --no-pbt   # a sweep over schedules
    python train/pbt_native.py --members 4 --envs 256 --mutate-batch --mutate-schedule   # train_batch_size per member too (pbt.py:42)
    python train/pbt_native.py --members 3 --batch-shares 1,2,4 --no-pbt                 # a sweep over batch sizes
    python train/pbt_native.py --lrs 1e-3,1e-4,1e-5 --no-pbt --lr-schedule linear:0      # that sweep with its linear decay to 0 (:111-119)

One ShipVecEnv of members x envs-per-member envs; member m owns the contiguous slice [m*n, (m+1)*n).  Every update is one
``rollout_population`` (one policy launch per step for the whole population), then ``PopulationPPO.gae`` and ``.update`` (two launches
per minibatch for the whole population), with per-member lambda / clip / learning rate.  Same game configuration as the reference's PBT
(FPS 1000, SPEED 30, DEBUG off, BOUNDS 1000x1000), same initial lambda 0.95, clip 0.2, lr 5e-4, same scheduler semantics
(ship_sim_gym_amd/population.py's PBTScheduler: bottom quarter exploits a random top-quarter member, resample probability 0.33, x1.2 /
x0.8 or a neighbouring list entry otherwise) ranked by episode_reward_mean.

What differs from the reference, on purpose:
* --perturb-every counts UPDATES, not seconds of wall time (the reference perturbs every 600 s of a trial's own clock; a population
  that trains in lockstep has no per-trial clock, and a count makes runs reproducible);
* of the six mutated hyper-parameters lambda, clip_param and lr always vary per member; num_sgd_iter and sgd_minibatch_size do with
  --mutate-schedule (initial draws from the reference's {10, 20, 30} and {128, 512, 2048}, train/rllib/pbt.py:65-68; mutated as
  :40-41; the source's schedule travels with an exploit) and are otherwise set by --epochs / --minibatches, which also take
  comma-separated per-member lists;
* train_batch_size, the sixth, is a member's SHARE of the handle's envs (--mutate-batch: initial draws from the reference's {10000,
  20000, 40000}, train/rllib/pbt.py:69-70, mutated as :42, travelling with an exploit; --batch-shares a,b,c: fixed shares for a sweep).
  The handle's horizon x envs samples per update are fixed, so the values are turned into contiguous env slices of unequal size by
  ``slices_for_batch_sizes`` (multiples of --quantum envs, at least one quantum each) and member m trains on horizon x n_m samples.
  After every perturbation the handle is re-sliced from the members' current values and the new sizes are logged.  Envs are fungible:
  a re-slice touches no env state; the episode carries are per env and are kept, so an episode in flight is credited to whichever
  member owns the env when it ends.  Without either flag train_batch_size is common to the population (--horizon x --envs-per-member);
* a schedule is clamped before use: num_sgd_iter to [1, --max-epochs] (the permutations are drawn as [P, max-epochs, samples]) and the
  minibatch size to [min(128, samples), samples], samples being the member's own (horizon x its slice).  ray clamps nothing: there a trial whose sgd_minibatch_size exceeds its
  train_batch_size simply fails.  A minibatch size becomes a minibatch count (ceil(samples / size)), and the chunks are torch.chunk's:
  at most `size` long, not RLlib's exact slices;
* one handle on one GPU, one architecture.

The loss terms of the reference trainers' own PPO are opt-in: --kl-coeff 1.0 is the reference's setting (train/rllib/pbt.py:55-62; the
coefficient then adapts per member against --kl-target, as RLlib's update_kl does, and travels with the weights on an exploit),
--vf-clip is RLlib's vf_clip_param / PPO2's cliprange_vf, --max-grad-norm PPO2's 0.5.  Without them a run is the plain clipped loss.

Logged per update: every member's episode_reward_mean (over the episodes that ended since the last perturbation); per perturbation:
each exploit (member <- source) and each mutation (key, resample / perturb, old -> new).

--eval-every U --eval-episodes E (default off): every U updates every member is evaluated greedily (the arg-max action) for E episodes
per env on a second ShipVecEnv of its own (ship_sim_gym_amd/evaluate.py; the reference's train/rllib/rollout.py:8-26), so the training
envs are not disturbed, and the table is printed.  The ranking stays by training episodes, the reference's reward_attr.

--obs-filter (default off): observations are normalised by a running mean / std filter on the device, one set of statistics per member
(ship_sim_gym_amd/obs_filter.py; RLlib's "PPO" default MeanStdFilter behind train/rllib/pbt.py:50, where every trial has its own
filter), instead of the fixed division by the largest bound.  Every rollout step merges each member's own rows into its statistics
before the policy launch; the statistics stay with the member through a re-slice, travel with the weights on an exploit, and the
--eval-every env reads them frozen.

--norm-reward (default off): the rewards each member's GAE sees are divided by a running standard deviation of its envs' discounted
returns, kept on the device per member (ship_sim_gym_amd/ret_filter.py; the reward half of Stable-Baselines' VecNormalize, with the
member's own gamma): one library call per rollout between the rollout and GAE.  The raw rewards, which episode_reward_mean reads, stay
as they are; a member's statistics travel with its weights on an exploit, the per-env returns in flight stay with their envs.
--reward-clip C clamps the normalised rewards to +-C (default 10; 0: none).

--report prints, after every update, one table row per member: the explained variance of its value network over its slice of the
rollout and the means of its policy loss, value loss, entropy and clip fraction over ITS steps of the update (with an extended term on
also the KL, the gradient norm and the coefficient) — what RLlib reports per trial and iteration (train/rllib/pbt.py:47-74:
vf_explained_var, policy_loss, vf_loss, entropy, kl) — from two launches for the whole population and one copy
(ship_sim_gym_amd/report.py, ssg_pop_report).  --report-kl adds how far the update moved each member's policy (approximate KL, PPO2's
approxkl, the clip fraction over its whole batch under its own clip) for one more ssg_pop_dist launch; --progress FILE writes the
records as CSV, one row per member per update, and with --resume cuts the file back to the checkpoint's update first.  The records are
taken before a perturbation that is due.  Off by default; the three may change between a run and its resumption.

--lr-schedule SPEC, --clip-schedule SPEC, --ent-schedule SPEC (default: constants): hyper-parameter schedules of every member's learning
rate, clip range and entropy coefficient (ship_sim_gym_amd/hparam_schedule.py; not the update schedule of --mutate-schedule), piecewise
linear in the member's own timesteps.  SPEC is linear:STOP — from the member's OWN constant (its --lrs entry, clip 0.2, entropy
coefficient 0.01) down to STOP over --total-timesteps T, by default the member's own run, --updates x --horizon x its envs — or absolute
points T0:V0,T1:V1,..., the same for every member.  Member m's clock before update u (1, 2, ...) is (u - 1) x horizon x n_m, the samples
it has collected.  --lr-schedule and --clip-schedule need --no-pbt: PBT mutates those two, and a schedule would overwrite the mutation
at the next update (as RLlib's lr_schedule overrides a mutated lr); --ent-schedule goes with PBT.  None of the three goes with
--mutate-batch: a member's clock would depend on the history of re-slices.  The specs are part of the run's configuration, and a
resumed trainer's schedules are the file's.

--save FILE writes a checkpoint at the end (ship_sim_gym_amd/checkpoint.py; the reference's checkpoint_at_end, train/rllib/pbt.py:53),
--save-every U also after every U updates (its checkpoint_freq, :54), --save-best FILE after every update in which the best member's
episode_reward_mean exceeds the best so far (never after an update in which no episode ended; the file holds the whole population and
names the member).  A file holds the population, the trainer, both filters, the env's snapshot, the scheduler with its generator, this
loop's state (the torch generator, the score window and history, the exploit and re-slice logs, the current schedules, batch sizes and
slices) and the run's arguments; it is written at the end of an update's iteration, after a perturbation that was due.  --resume FILE
continues that run bit for bit: repeat the original command line and add --resume; --updates stays the TOTAL and may be raised, the
--save* and --eval-* options may change, any other argument that differs from the file's is refused.  train/evaluate_native.py
--checkpoint FILE evaluates such a file, every member or --member M.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from train import loop  # noqa: E402  (host only: no torch)

INITIAL = {"lambda": 0.95, "clip_param": 0.2, "lr": 5e-4}  # train/rllib/pbt.py:60-62
INITIAL_SCHEDULE = {"num_sgd_iter": [10, 20, 30], "sgd_minibatch_size": [128, 512, 2048]}  # train/rllib/pbt.py:65-68
INITIAL_BATCH = [10000, 20000, 40000]  # train_batch_size, train/rllib/pbt.py:69-70


def default_quantum(n_envs, members):
    """The slice quantum when none is given: 64 envs (the policy kernel's tile) where that leaves at least four quanta per member,
    else the largest smaller power of two that does and divides n_envs (at least 1)."""
    q = 64
    while q > 1 and (n_envs % q or n_envs // q < 4 * members):
        q //= 2
    return q


def initial_batch_sizes(sched, members):
    """The members' initial train_batch_size draws (from the scheduler's generator, after the schedule's draws when there are any)."""
    return [sched.rng.choice(INITIAL_BATCH) for _ in range(members)]


def clamp_schedule(num_sgd_iter, sgd_minibatch_size, samples, max_epochs):
    """The schedule as it is used: num_sgd_iter in [1, max_epochs], the minibatch size in [min(128, samples), samples]; ints."""
    return (max(1, min(int(max_epochs), int(num_sgd_iter))), max(min(128, int(samples)), min(int(samples), int(sgd_minibatch_size))))


# what a resumed run may change: everything else in train()'s arguments is the run's configuration (the checkpoint's "config" section)
CONFIG_EXEMPT = ("updates", "save", "save_every", "save_best", "resume", "eval_every", "eval_episodes", "log", "return_details", "report",
                 "report_kl", "progress")
RESUME_SECTIONS = ("population", "trainer", "env", "scheduler", "loop", "config")


def run_config(**kwargs):
    """The "config" section of a run of train(**kwargs): its effective arguments without CONFIG_EXEMPT, as plain data."""
    return loop.run_config(train, CONFIG_EXEMPT, kwargs)


def plain_events(events):
    """Exploit events as a checkpoint holds them: the mutation tuples as lists."""
    return [dict(ev, mutations=[list(mu) for mu in ev["mutations"]]) for ev in events]


def events_from_plain(events):
    """plain_events undone: the events as perturb() returned them."""
    return [dict(ev, mutations=[tuple(mu) for mu in ev["mutations"]]) for ev in events]


def make_arg_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--members", type=int, default=16, help="population size (the reference: 120 samples)")
    ap.add_argument("--envs-per-member", type=int, default=512)
    ap.add_argument("--envs", type=int, default=None, help="the handle's envs in all (overrides --envs-per-member: envs / members each)")
    ap.add_argument("--mutate-batch", action="store_true",
                    help="train_batch_size per member as its share of the envs: drawn from the reference's set, mutated and exploited; "
                         "the handle is re-sliced after every perturbation")
    ap.add_argument("--batch-shares", default=None, help="comma-separated fixed batch shares, one member each (unequal env slices; overrides --members)")
    ap.add_argument("--quantum", type=int, default=None, help="slice sizes are multiples of this many envs (default: 64, less on a small handle)")
    ap.add_argument("--updates", type=int, default=40)
    ap.add_argument("--horizon", type=int, default=32, help="rollout steps per update (common to the population)")
    ap.add_argument("--perturb-every", type=int, default=5, help="perturbation interval in UPDATES (the reference: 600 s of wall time)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--epochs", default="2", help="epochs per update, or a comma-separated list, one member each")
    ap.add_argument("--minibatches", default="4", help="minibatches per epoch, or a comma-separated list, one member each")
    ap.add_argument("--mutate-schedule", action="store_true",
                    help="num_sgd_iter and sgd_minibatch_size per member: drawn from the reference's sets, mutated and exploited "
                         "(overrides --epochs / --minibatches)")
    ap.add_argument("--max-epochs", type=int, default=30, help="upper clamp of a mutated num_sgd_iter")
    ap.add_argument("--lrs", default=None, help="comma-separated learning rates, one member each (overrides --members)")
    ap.add_argument("--no-pbt", dest="pbt", action="store_false", help="no exploit / explore: a plain sweep")
    ap.add_argument("--kl-coeff", type=float, default=0.0, help="initial KL penalty coefficient (the reference: 1.0; 0 = no KL term)")
    ap.add_argument("--kl-target", type=float, default=0.01, help="the coefficient adapts against this mean KL (RLlib's default)")
    ap.add_argument("--vf-clip", type=float, default=0.0, help="value-loss clip range (0 = off)")
    ap.add_argument("--max-grad-norm", type=float, default=0.0, help="global gradient-norm clip (PPO2: 0.5; 0 = off)")
    ap.add_argument("--separate-value", action="store_true",
                    help="every member has a value network of its own (RLlib's default vf_share_layers=False) instead of a shared body")
    ap.add_argument("--eval-every", type=int, default=0, metavar="U",
                    help="every U UPDATES evaluate every member greedily on a second env of its own and print it; 0 = off "
                         "(the ranking stays by training episodes, the reference's reward_attr)")
    ap.add_argument("--eval-episodes", type=int, default=1, metavar="E", help="episodes counted per env by each evaluation")
    ap.add_argument("--obs-filter", action="store_true",
                    help="normalise observations with a running mean / std filter per member on the device; default: obs / max bound")
    ap.add_argument("--norm-reward", action="store_true",
                    help="divide the rewards GAE sees by a running std of the discounted return, per member on the device; default: raw rewards")
    ap.add_argument("--reward-clip", type=float, default=10.0, metavar="C",
                    help="clamp the normalised rewards to +-C (needs --norm-reward; 0: no clamp)")
    ap.add_argument("--adv-norm", choices=("batch", "minibatch"), default="batch",
                    help="normalise every member's advantages once per rollout, or inside every minibatch as Stable-Baselines' PPO2 does")
    ap.add_argument("--perm", choices=("torch", "native"), default="torch",
                    help="who shuffles every member's minibatches: torch (rand + argsort), or the library on the device, one launch")
    ap.add_argument("--timeout-bootstrap", action="store_true",
                    help="GAE bootstraps an episode the clock ended from the value of its terminal observation instead of scoring it as a "
                         "return of 0; default: every done alike")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--hidden", type=int, default=64, help="width of the hidden layers (a multiple of 16 up to 128)")
    ap.add_argument("--save", default=None, metavar="FILE",
                    help="write a checkpoint at the end (ship_sim_gym_amd/checkpoint.py): the population, the trainer, both filters, the "
                         "env, the scheduler and this loop's state — what --resume and train/evaluate_native.py --checkpoint read")
    ap.add_argument("--save-every", type=int, default=0, metavar="U", help="also rewrite --save after every U updates (atomically); 0 = off")
    ap.add_argument("--save-best", default=None, metavar="FILE",
                    help="write a checkpoint after every update in which the best member's episode_reward_mean exceeds the best so far "
                         "(the whole population; the file names the member)")
    loop.add_episode_log_flags(ap)
    loop.add_report_flags(ap)
    loop.add_hparam_schedule_flags(ap, "each member's own constant", "--updates x --horizon x the member's envs")
    ap.add_argument("--resume", default=None, metavar="FILE",
                    help="continue the run a checkpoint was saved from, bit for bit: repeat the original command line; --updates stays "
                         "the TOTAL and may be raised")
    return ap


def parse_args(argv=None):
    ap = make_arg_parser()
    a = ap.parse_args(argv)
    a.lrs = [float(x) for x in a.lrs.split(",")] if a.lrs else None
    if a.lrs is not None:
        a.members = len(a.lrs)
    for key in ("epochs", "minibatches"):
        try:
            vals = [int(x) for x in str(getattr(a, key)).split(",")]
        except ValueError:
            ap.error("--%s takes an integer or a comma-separated list of integers" % key)
        if min(vals) < 1:
            ap.error("--%s must be >= 1" % key)
        setattr(a, key, vals[0] if len(vals) == 1 else vals)
    lists = [len(v) for v in (a.epochs, a.minibatches) if isinstance(v, list)]
    if lists:
        if a.lrs is None:
            a.members = lists[0]
        if any(n != a.members for n in lists):
            ap.error("--epochs / --minibatches list %s entries for %d members" % (lists, a.members))
    if a.batch_shares is not None:
        try:
            a.batch_shares = [float(x) for x in a.batch_shares.split(",")]
        except ValueError:
            ap.error("--batch-shares takes a comma-separated list of numbers")
        if min(a.batch_shares) <= 0:
            ap.error("--batch-shares must be > 0")
        if a.mutate_batch:
            ap.error("--batch-shares and --mutate-batch exclude each other")
        if a.lrs is None and not lists:
            a.members = len(a.batch_shares)
        if len(a.batch_shares) != a.members:
            ap.error("--batch-shares lists %d entries for %d members" % (len(a.batch_shares), a.members))
    if a.envs is not None:
        if a.envs < a.members:
            ap.error("--envs must hold at least one env per member")
        a.envs_per_member = max(1, a.envs // a.members)
        if not (a.mutate_batch or a.batch_shares) and a.envs % a.members:
            ap.error("--envs must be a multiple of --members (equal slices)")
    if a.quantum is not None and a.quantum < 1:
        ap.error("--quantum must be >= 1")
    if a.max_epochs < 1:
        ap.error("--max-epochs must be >= 1")
    if a.members < 1 or a.envs_per_member < 1 or a.updates < 1 or a.horizon < 1 or a.perturb_every < 1:
        ap.error("--members, --envs-per-member, --updates, --horizon and --perturb-every must be >= 1")
    if a.kl_coeff < 0 or a.kl_target < 0 or a.vf_clip < 0 or a.max_grad_norm < 0:
        ap.error("--kl-coeff, --kl-target, --vf-clip and --max-grad-norm must be >= 0")
    loop.check_flag_values(a, ap.error)
    try:
        check_hparam_schedules(a)
    except ValueError as ex:
        ap.error(str(ex))
    return a


class LoopState(object):
    """What the loop carries from one update to the next — with the generator's state, the checkpoint's "loop" section: the last update
    done, the scores and their history, the episode window they come from (a device tensor: episodes since the last perturbation), the
    exploit and re-slice logs, the schedule as used (iters, sizes, counts when it is swept; empty when it is common), the layout (batch
    sizes and slices; empty when equal), the best score, its update and member, the episodes ended per update.  member_samples is not saved."""
    KINDS = tuple((k, int) for k in ("update", "best_update", "best_member")) + (("best", float),) + tuple((k, list) for k in (
        "history", "scores", "exploits", "reslices", "iters", "sizes", "counts", "batch_sizes", "slices", "episodes_ended"))

    def __init__(self, members, window, samples):
        self.update, self.history, self.scores, self.window, self.member_samples = 0, [], [float("-inf")] * members, window, [samples] * members
        self.exploits, self.reslices, self.iters, self.sizes, self.counts, self.batch_sizes, self.slices = [], [], [], [], [], [], []
        self.best, self.best_update, self.best_member, self.episodes_ended = float("-inf"), 0, -1, []

    def state_dict(self, gen):
        return {"update": int(self.update), "gen_state": gen.get_state().cpu().clone(), "history": [list(r) for r in self.history],
                "scores": list(self.scores), "window": self.window.detach().cpu().clone(), "exploits": plain_events(self.exploits),
                "reslices": [[int(r[0]), list(r[1])] for r in self.reslices], "iters": list(self.iters), "sizes": list(self.sizes),
                "counts": list(self.counts), "batch_sizes": list(self.batch_sizes), "slices": list(self.slices), "best": float(self.best),
                "best_update": int(self.best_update), "best_member": int(self.best_member), "episodes_ended": list(self.episodes_ended)}

    def load_state_dict(self, sd, gen):
        import torch
        from ship_sim_gym_amd.checkpoint import check_values
        check_values("train: the checkpoint's loop section", sd, self.KINDS + (("gen_state", torch.Tensor), ("window", torch.Tensor)))
        gen.set_state(sd["gen_state"])
        self.window.copy_(sd["window"])
        for k, _ in self.KINDS:  # (plain data of the kinds just checked, as state_dict wrote it)
            setattr(self, k, sd[k])
        self.exploits, self.reslices = events_from_plain(sd["exploits"]), [(r[0], r[1]) for r in sd["reslices"]]


HPARAM_SCHEDULE_FLAGS = (("lr", "lr_schedule", "--lr-schedule"), ("clip", "clip_schedule", "--clip-schedule"),
                         ("ent_coef", "ent_schedule", "--ent-schedule"))
ENT_COEF = 0.01  # PopulationPPO's default entropy coefficient


def check_hparam_schedules(a):
    """The host-side refusals of the hyper-parameter schedule flags (a: train()'s arguments or the parsed command line's): what PBT
    would overwrite, what re-slicing would make history-dependent, a bad span, a malformed spec or a clip <= 0 (parsed here from the
    common starts; a learning rate's start, the member's own, does not decide whether its spec is well-formed)."""
    from ship_sim_gym_amd.hparam_schedule import HparamSchedule, check_schedulable
    on = [(name, arg, flag) for name, arg, flag in HPARAM_SCHEDULE_FLAGS if getattr(a, arg, None) is not None]
    for name, arg, flag in on:
        if a.pbt and name in ("lr", "clip"):
            raise ValueError("%s (%s) needs --no-pbt (pbt=False): PBT mutates %s, and the schedule would overwrite the mutation at the "
                             "next update" % (arg, flag, name))
        if a.mutate_batch:
            raise ValueError("%s (%s) is not supported together with --mutate-batch (mutate_batch=True): a member's clock would depend on "
                             "the history of re-slices" % (arg, flag))
    total = getattr(a, "total_timesteps", None)
    if total is not None and (isinstance(total, bool) or not isinstance(total, int) or total < 1):
        raise ValueError("total_timesteps (--total-timesteps) must be an int >= 1 (got %r)" % (total,))
    start = {"lr": INITIAL["lr"], "clip": INITIAL["clip_param"], "ent_coef": ENT_COEF}
    for name, arg, flag in on:
        check_schedulable("%s (%s)" % (arg, flag), name, HparamSchedule.parse(getattr(a, arg), start[name], 1 if total is None else total))


def member_hparam_schedules(run, sizes, lrs):
    """Every member's lr / clip / ent_coef as PopulationPPO takes them: lists of P floats, or of P HparamSchedules where a flag is on —
    a "linear:" spec from the member's own constant over total_timesteps, by default its own run of updates * horizon * sizes[m]."""
    from ship_sim_gym_amd.hparam_schedule import HparamSchedule
    out = {"lr": list(lrs), "clip": [INITIAL["clip_param"]] * run.P, "ent_coef": [ENT_COEF] * run.P}
    for name, arg, _ in HPARAM_SCHEDULE_FLAGS:
        spec = getattr(run, arg)
        if spec is not None:
            spans = [run.updates * run.horizon * n if run.total_timesteps is None else run.total_timesteps for n in sizes]
            out[name] = [HparamSchedule.parse(spec, out[name][m], spans[m]) for m in range(run.P)]
    return out


def plan(run):
    """The host side of a run (run: train()'s arguments), before the first env is built: refuse what does not fit, then add what follows
    from the arguments: P members on n_total envs, sliced or n each, the schedule per member or common, the permutation rows drawn."""
    if run.save_every < 0 or (run.save_every and not run.save):
        raise ValueError("train: save_every must be >= 0 and needs save (the file it rewrites)")
    if run.episode_log_capacity < 1:
        raise ValueError("train: episode_log_capacity must be >= 1")
    if run.perm not in ("torch", "native"):
        raise ValueError("train: perm must be 'torch' or 'native' (got %r)" % (run.perm,))
    check_hparam_schedules(run)
    run.scheduled = any(getattr(run, arg, None) is not None for _, arg, _ in HPARAM_SCHEDULE_FLAGS)
    P = run.P = int(run.members)
    run.n_total = int(run.envs) if run.envs is not None else P * int(run.envs_per_member)
    run.sliced = bool(run.mutate_batch) or run.batch_shares is not None
    if run.mutate_batch and run.batch_shares is not None:
        raise ValueError("train: mutate_batch and batch_shares exclude each other")
    if not run.sliced and run.n_total % P:
        raise ValueError("train: %d envs do not split into %d equal member slices" % (run.n_total, P))
    for name, what in (("lrs", "learning rates"), ("batch_shares", "batch shares")):
        if getattr(run, name) is not None and len(getattr(run, name)) != P:
            raise ValueError("train: %d %s for %d members" % (len(getattr(run, name)), what, P))
    run.n, run.native_perm = max(1, run.n_total // P), run.perm == "native"
    run.quantum = default_quantum(run.n_total, P) if run.quantum is None else int(run.quantum)
    # the schedule: common ints (one launch shape for everyone) or one entry per member
    swept = [isinstance(x, (list, tuple)) for x in (run.epochs, run.minibatches)]
    run.per_member = run.sliced or bool(run.mutate_schedule) or any(swept)
    if run.per_member and not run.mutate_schedule:
        run.iters0 = [int(e) for e in run.epochs] if swept[0] else [int(run.epochs)] * P
        run.counts0 = [int(b) for b in run.minibatches] if swept[1] else [int(run.minibatches)] * P
        if len(run.iters0) != P or len(run.counts0) != P:
            raise ValueError("train: %d epochs and %d minibatches for %d members" % (len(run.iters0), len(run.counts0), P))
    run.perm_epochs = run.max_epochs if run.mutate_schedule else (max(run.iters0) if run.per_member else run.epochs)


def bind_layout(run, state, log, u=None, batch_sizes=None):
    """From batch sizes to bound slices: the members' values become env slices, logged under update u (0: the initial layout), the env
    is bound to them and member_samples follows.  Without batch_sizes the record's own layout is bound: a resumed run's, as it was
    saved, whose log is the file's.  Env state and the episode carries stay as they are."""
    from ship_sim_gym_amd.population import slices_for_batch_sizes
    if batch_sizes is not None:
        state.batch_sizes = list(batch_sizes)
        state.slices = slices_for_batch_sizes(state.batch_sizes, run.n_total, run.quantum)
        state.reslices.append((u, list(state.slices)))
        log("slices: train_batch_size %s -> envs %s (quantum %d)" % (state.batch_sizes, state.slices, run.quantum) if u == 0 else
            "update %d  re-slice: train_batch_size %s -> envs %s" % (u, state.batch_sizes, state.slices))
    run.env.set_population_slices(state.slices)
    state.member_samples = [run.horizon * s for s in state.slices]


def set_schedule(state, max_epochs, raw=None, iters=None, counts=None):
    """The schedule as it is used, from the members' own samples: a mutated one (raw: (num_sgd_iter, sgd_minibatch_size) per member)
    clamped, or a swept one (iters, counts) with the minibatch sizes its counts make."""
    from ship_sim_gym_amd.ppo import chunk_split
    if raw is not None:
        used = [clamp_schedule(i, s, state.member_samples[m], max_epochs) for m, (i, s) in enumerate(raw)]
        state.iters, state.sizes = [c[0] for c in used], [c[1] for c in used]
    else:
        state.iters, state.counts = list(iters), list(counts)
        state.sizes = [chunk_split(state.member_samples[m], c)[0] for m, c in enumerate(state.counts)]


def build(run, log):
    """The run's objects, in the order that decides the bits: the global seed, the device generator (seed + 1), the envs, the nets in
    member order, the scheduler, whose generator draws the schedules before the batch sizes, the layout, the trainer, what the
    configuration binds, the reset.  Returns the loop-state record."""
    import torch
    from ship_gym.config import EnvConfig, GameConfig
    from ship_sim_gym_amd.population import NativePopulation, PBTScheduler, PopulationPPO, reference_mutations
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    from train.ppo_torch import ActorCritic
    from train.rllib_ppo import game_configuration
    P, env_kw = run.P, dict(run.env_kw or {})
    torch.manual_seed(run.seed)
    run.dev = torch.device(run.device)
    run.gen = torch.Generator(device=run.dev)
    run.gen.manual_seed(run.seed + 1)
    saved = {k: getattr(GameConfig, k) for k in ("FPS", "SPEED", "DEBUG", "BOUNDS")}
    try:  # (game_configuration writes the GameConfig class, as the reference's does; the env reads it once, here)
        run.env = ShipVecEnv(run.n_total, game_configuration(speed=30, fps=1000, debug=False), EnvConfig, device=run.device, n_maps=64, **env_kw)
        # the held-out run's env (train/rllib/rollout.py:8-26): evaluation resets and steps it, the training envs keep their episodes
        run.eval_env = ShipVecEnv(P * min(run.n, 256), GameConfig, EnvConfig, device=run.device, n_maps=64, **env_kw) if run.eval_every else None
    finally:
        for k, v in saved.items():
            setattr(GameConfig, k, v)
    D, A = run.env.states_history, run.env.action_space.n
    run.nets = [ActorCritic(D, A, hidden=run.hidden, separate_value=run.separate_value).to(run.dev) for _ in range(P)]
    run.pop = NativePopulation.from_actor_critics(run.nets, torch.full((D,), float(max(run.env.bounds)), dtype=torch.float64, device=run.dev))
    mutations = reference_mutations(schedule=run.mutate_schedule, batch=run.mutate_batch) if run.mutate_schedule or run.mutate_batch else None
    run.sched = PBTScheduler(P, seed=run.seed, perturbation_interval=run.perturb_every, mutations=mutations)
    state = LoopState(P, torch.zeros((P, 3), dtype=torch.int64, device=run.dev), run.horizon * run.n)
    if run.mutate_schedule:  # (drawn first: a seed's schedule does not depend on whether the batch is mutated too)
        raw = [(run.sched.rng.choice(INITIAL_SCHEDULE["num_sgd_iter"]), run.sched.rng.choice(INITIAL_SCHEDULE["sgd_minibatch_size"])) for _ in range(P)]
    if run.sliced:
        bind_layout(run, state, log, 0, initial_batch_sizes(run.sched, P) if run.mutate_batch else run.batch_shares)
    if run.mutate_schedule:
        set_schedule(state, run.max_epochs, raw=raw)
        log("schedule: num_sgd_iter %s  sgd_minibatch_size %s" % (state.iters, state.sizes))
    elif run.per_member:
        set_schedule(state, run.max_epochs, iters=run.iters0, counts=run.counts0)
    hparams = member_hparam_schedules(run, state.slices if run.sliced else [run.n] * P, run.lrs if run.lrs is not None else [INITIAL["lr"]] * P)
    run.ppo = PopulationPPO(run.pop, run.env, lam=INITIAL["lambda"], clip=hparams["clip"], lr=hparams["lr"], ent_coef=hparams["ent_coef"],
                            vf_clip=run.vf_clip, max_grad_norm=run.max_grad_norm, kl_coef=run.kl_coeff, kl_target=run.kl_target if run.kl_coeff > 0 else 0.0,
                            adv_norm=run.adv_norm, perm_seed=run.seed if run.native_perm else None)
    # per-member statistics: a member's rows are its slice, whatever the slices currently are
    run.flt, run.rflt, run.evaluator = loop.bind_env(run.env, run.horizon, P, run.obs_filter, run.norm_reward, run.ppo.gamma, run.reward_clip,
                                                     run.timeout_bootstrap, run.eval_env)
    if run.rflt is not None:
        run.ppo.set_return_filter(run.rflt)  # (an exploit copies the source's state rows with its weights)
    # the episode log: a record names the member that owns the env when its episode ends, whatever the slices currently are
    run.eplog, run.epwriter = loop.bind_episode_log(run.env, run.episode_log, run.episode_log_capacity, P, run.resume)
    run.env.reset_tensor()
    if run.save or run.save_best:
        run.env.check_snapshot_supported("snapshot")  # (refuse now, not after the training, a handle that cannot be saved)
    return state


def load_run(run, state, ckpt, log):
    """Everything is built and bound as the configuration says; now the saved layout, then the saved states."""
    state.load_state_dict(ckpt["loop"], run.gen)
    if run.sliced:
        bind_layout(run, state, log)
    run.pop.load_state_dict(ckpt["population"])
    run.ppo.load_state_dict(ckpt["trainer"])
    loop.load_filters(ckpt, run.flt, run.rflt)
    loop.load_episode_log(ckpt, run.eplog)
    run.sched.load_state_dict(ckpt["scheduler"])
    run.env.restore(ckpt["env"])


def write_checkpoint(path, run, state):
    """The checkpoint after update state.update (and after its perturbation, when one was due): everything a resumed run needs."""
    from ship_sim_gym_amd import checkpoint
    checkpoint.save(path, dict(loop.filter_sections(run.flt, run.rflt), **loop.episode_log_section(run.eplog), config=run.config, population=run.pop.state_dict(),
                               trainer=run.ppo.state_dict(), env=run.env.snapshot(), scheduler=run.sched.state_dict(), loop=state.state_dict(run.gen)))


def draw_permutations(run, state):
    """One update's permutations from the generator: None with perm "native" (update() draws its own, keyed by its count); sliced, member
    m's own rows [perm_epochs, horizon * n_m] in member order; else one draw [P, perm_epochs, samples].  Always perm_epochs rows."""
    import torch
    if run.native_perm:
        return None
    if run.sliced:
        return [torch.rand((run.perm_epochs, s), generator=run.gen, device=run.dev).argsort(dim=-1) for s in state.member_samples]
    return torch.rand((run.P, run.perm_epochs, state.member_samples[0]), generator=run.gen, device=run.dev).argsort(dim=-1)


def update_population(run, state, batch, perm):
    """The population's PPO update on one rollout: the common schedule, or every member's own, on max(iters) of the drawn rows."""
    if not run.per_member:
        return run.ppo.update(batch, perm, run.epochs, run.minibatches, stats=run.report)
    mbs = [run.ppo.minibatches_for_size(s, state.member_samples[m]) for m, s in enumerate(state.sizes)] if run.mutate_schedule else state.counts
    if perm is not None:
        perm = [q[:max(state.iters)].contiguous() for q in perm] if run.sliced else perm[:, :max(state.iters)].contiguous()
    return run.ppo.update(batch, perm, state.iters, mbs, stats=run.report)


def report_table(rec, extended):
    """The update report's table, one row per member (rec: PopulationPPO.report's arrays): explained variance, the update's minibatch
    means over the member's own steps and, when they were computed, the extended terms and the post-update group."""
    cols = [("expl.var", "explained_variance", "%+.4f"), ("policy loss", "policy_loss", "%+.5f"), ("value loss", "value_loss", "%.5f"),
            ("entropy", "entropy", "%.5f"), ("clip frac", "clip_fraction_minibatch", "%.4f")]
    if extended:
        cols += [("kl", "kl", "%.6f"), ("grad norm", "grad_norm", "%.4f"), ("kl coef", "kl_coef", "%.4f")]
    if rec["post"].any():
        cols += [("approx kl", "approx_kl", "%.6f"), ("approxkl", "approxkl_ppo2", "%.6f"), ("clip frac after", "clip_fraction", "%.4f")]
    lines = ["%6s  %s" % ("member", "  ".join("%15s" % c[0] for c in cols))]
    for m in range(len(rec["n"])):
        lines.append("%6d  %s" % (m, "  ".join("%15s" % (c[2] % rec[c[1]][m]) for c in cols)))
    return "\n".join(lines)


def report_update(run, u, batch, st, log):
    """--report: one table per update from ssg_pop_report's records (one copy to the host), and the --progress rows."""
    rec = run.ppo.report(batch, stats=st, post=run.report_kl)
    log("update %d  report\n%s" % (u, report_table(rec, st.shape[2] == 8)))
    if run.progress_writer is not None:
        run.progress_writer.write(u, u * run.horizon * run.n_total, rec, rec["lr"], rec["clip"])


def account(state, u, ep, log):
    """After update u: every member's episode_reward_mean over its window (none ended: it keeps its score), the history row, and how
    many episodes ended during the update, which is returned."""
    w, P = state.window.cpu().tolist(), len(state.scores)
    state.update, state.scores = u, [w[m][0] / 100.0 / w[m][2] if w[m][2] else state.scores[m] for m in range(P)]
    state.history.append(list(state.scores))
    log("update %d  episode_reward_mean %s" % (u, " ".join("%d:%.3f" % (m, s) for m, s in enumerate(state.scores))))
    state.episodes_ended.append(int(ep[:, 2].sum().item()))
    return state.episodes_ended[-1]


def evaluate(run, u, episodes, log):
    """One greedy evaluation of every member (printed only: PBT ranks by training episodes, as the reference does)."""
    from ship_sim_gym_amd.evaluate import format_table
    r = run.evaluator.evaluate(run.pop, episodes, greedy=True)
    log("update %d  greedy evaluation (%d envs x %d episodes per member)\n%s" % (u, run.eval_env.num_envs // run.P, episodes, format_table(r)))
    return (u, r["per_member"].cpu().tolist())


def perturb(run, state, u, log):
    """One perturbation, on the loop-state record: the members' hyper-parameters -> sched.perturb -> the exploit -> the new values taken
    over -> the handle re-sliced -> the schedule re-made from the members' own samples -> the events logged -> the window reset."""
    ppo = run.ppo
    hp = {"lambda": ppo.lam, "clip_param": ppo.clip, "lr": ppo.lr}
    if run.sliced:  # (fixed shares are the member's configuration: they travel with an exploit, unmutated)
        hp["train_batch_size" if run.mutate_batch else "batch_share"] = state.batch_sizes
    if run.per_member:  # (a swept schedule is not mutated either, and travels with an exploit too)
        hp.update({"num_sgd_iter": state.iters, "sgd_minibatch_size": state.sizes} if run.mutate_schedule else
                  {"num_sgd_iter": state.iters, "minibatches": state.counts})
    src, new, events = run.sched.perturb(state.scores, hp)
    ppo.exploit(src)
    ppo.lam, ppo.clip, ppo.lr = new["lambda"], new["clip_param"], new["lr"]
    if run.sliced:
        bind_layout(run, state, log, u, new["train_batch_size" if run.mutate_batch else "batch_share"])
    if run.mutate_schedule:  # (the minibatch-size clamp uses the member's own samples)
        set_schedule(state, run.max_epochs, raw=list(zip(new["num_sgd_iter"], new["sgd_minibatch_size"])))
    elif run.per_member:
        set_schedule(state, run.max_epochs, iters=new["num_sgd_iter"], counts=new["minibatches"])
    for ev in events:
        m = ev["member"]
        log("update %d  exploit: member %d <- member %d" % (u, m, ev["source"]))
        for key, kind, old, val in ev["mutations"]:
            log("update %d  mutation: member %d %s %s %.6g -> %.6g" % (u, m, key, kind, old, val))
        if run.per_member:
            ev["schedule"] = {"num_sgd_iter": state.iters[m], "sgd_minibatch_size": state.sizes[m]}
            log("update %d  schedule: member %d num_sgd_iter %d sgd_minibatch_size %d (as used)" % (u, m, state.iters[m], state.sizes[m]))
        state.scores[m] = state.scores[ev["source"]]
    state.exploits += events
    state.window.zero_()


def train(members=16, envs_per_member=512, updates=40, horizon=32, perturb_every=5, seed=0, epochs=2, minibatches=4, lrs=None,
          pbt=True, device="cuda:0", log=print, return_details=False, kl_coeff=0.0, kl_target=0.01, vf_clip=0.0, max_grad_norm=0.0,
          separate_value=False, mutate_schedule=False, max_epochs=30, eval_every=0, eval_episodes=1, envs=None, mutate_batch=False,
          batch_shares=None, quantum=None, obs_filter=False, norm_reward=False, reward_clip=10.0, adv_norm="batch", perm="torch",
          timeout_bootstrap=False, hidden=64, env_kw=None, save=None, save_every=0, save_best=None, resume=None, episode_log=None,
          episode_log_capacity=65536, report=False, report_kl=False, progress=None, lr_schedule=None, clip_schedule=None, ent_schedule=None,
          total_timesteps=None):
    config = run_config(**dict(locals()))  # (first statement: the arguments, nothing else)
    run = argparse.Namespace(**locals())  # the run record: the arguments and the config; plan() and build() add to it
    run.report = bool(report or report_kl or progress)  # (--report-kl and --progress imply --report)
    import torch
    from ship_sim_gym_amd.ppo import chunk_split
    # check (every refusal on the host, then the file a run resumes from, before any device work), build and bind, resume
    plan(run)
    ckpt = loop.open_resume(resume, config, loop.resume_sections(RESUME_SECTIONS, obs_filter, norm_reward, episode_log), exempt=CONFIG_EXEMPT) if resume else None
    state = build(run, log)
    run.progress_writer = loop.open_progress(progress, resume)
    if ckpt is not None:
        load_run(run, state, ckpt, log)
        if run.progress_writer is not None:
            run.progress_writer.cut_back(state.update)  # (the rows of updates the checkpoint has not seen are written again)
        log("resumed from %s: %d updates done, continuing at update %d of %d" % (resume, state.update, state.update + 1, updates))
    out, evals = None, []
    for name in sorted(run.ppo.schedules) if run.scheduled else ():  # (once: a resumed trainer's schedules are the file's)
        log("hyper-parameter schedules of %s: %s" % (name, ["constant" if s is None else s.state() for s in run.ppo.schedules[name]]))
    for u in range(state.update + 1, updates + 1):
        # the hyper-parameter schedules' clocks: the samples each member has collected before this update (without --mutate-batch the
        # slices never change, so a clock is a function of u alone)
        run.ppo.set_timesteps([(u - 1) * s for s in state.member_samples])
        if run.scheduled:
            log("update %d  lr %s  clip %s  entropy coefficient %s" % (u, *(" ".join("%d:%.6g" % (m, v) for m, v in enumerate(getattr(run.ppo, k)))
                                                                            for k in ("lr", "clip", "ent_coef"))))
        uniforms = torch.rand((horizon, run.n_total), generator=run.gen, device=run.dev)
        batch = run.env.rollout_population(run.pop, horizon, uniforms=uniforms, out=out)
        out = {k: v for k, v in batch.items() if k not in ("adv", "ret", "logp_all", "rew_norm", "rew_denom")}
        ep = run.ppo.episode_stats(batch)
        state.window += ep
        if run.eplog is not None:
            run.eplog.append(batch)  # (no host synchronisation; flushed below, next to the update's log line)
        if run.rflt is not None:
            run.rflt.set_gamma(run.ppo.gamma)  # (the members' own discounts, whatever they currently are)
        run.ppo.gae(batch, return_filter=run.rflt)
        st_upd = update_population(run, state, batch, draw_permutations(run, state))
        if run.report:
            report_update(run, u, batch, st_upd, log)
        ended = account(state, u, ep, log)
        if run.eplog is not None:  # the cycle's one copy of the ring to the host
            log("update %d  episode log: %d rows written, %d in all" % (u, run.epwriter.flush(), run.eplog.rows_written))
        # save-best: the best member's episode_reward_mean so far (an update in which no episode ended never is one) ...
        new_best = ended > 0 and max(state.scores) > state.best
        if new_best:
            state.best, state.best_update, state.best_member = max(state.scores), u, state.scores.index(max(state.scores))
        if run.evaluator is not None and u % eval_every == 0:
            evals.append(evaluate(run, u, eval_episodes, log))
        if pbt and run.sched.due(u):
            perturb(run, state, u, log)
        if new_best and save_best:  # ... written after the perturbation, so that the file resumes like any other (the best member ranks top: a source, not a destination)
            write_checkpoint(save_best, run, state)
            log("update %d  member %d's episode_reward_mean %.3f is the best so far: saved to %s" % (u, state.best_member, state.best, save_best))
        if save and save_every and u % save_every == 0:
            write_checkpoint(save, run, state)
    # finish
    torch.cuda.synchronize(run.dev)
    if save:
        write_checkpoint(save, run, state)
        log("checkpoint after update %d saved to %s" % (state.update, save))
    run.pop.load_into(run.nets)
    P, samples, ppo = run.P, horizon * run.n, run.ppo
    details = {"params": run.pop.params.detach().clone(), "exploits": state.exploits, "nets": run.nets,
               "hparams": {"lambda": list(ppo.lam), "clip_param": list(ppo.clip), "lr": list(ppo.lr),
                           "num_sgd_iter": list(state.iters) if run.per_member else [int(epochs)] * P,
                           "sgd_minibatch_size": list(state.sizes) if run.per_member else [chunk_split(samples, minibatches)[0]] * P},
               "member_steps": list(ppo.member_steps), "kl_coef": ppo.kl_coef.detach().cpu().tolist(), "evaluations": evals,
               "slices": list(run.env.population_slices) if run.sliced else [run.n] * P, "reslices": state.reslices,
               "train_batch_size": list(state.batch_sizes) if run.sliced else [samples] * P,
               "best": state.best, "best_update": state.best_update, "best_member": state.best_member, "episodes_ended": list(state.episodes_ended),
               "env_state": run.env.state.detach().cpu().clone() if return_details else None}
    details.update(loop.filter_sections(run.flt, run.rflt))
    if run.flt is not None:
        log("observation filter: rows merged per member %s" % [int(c) for c in details["obs_filter"]["state"][:, 3, 0].tolist()])
    if run.rflt is not None:
        log("return filter: returns merged per member %s  std %s" % ([int(c) for c in details["ret_filter"]["state"][:, 3].tolist()],
                                                                     ["%.5f" % d for d in details["ret_filter"]["state"][:, 2].tolist()]))
    if run.eval_env is not None:
        run.eval_env.close()
    run.env.close()
    return (state.history, details) if return_details else state.history


def main(argv=None):
    train(**vars(parse_args(argv)))  # (every flag is an argument of train() of the same name)


if __name__ == "__main__":
    main()
