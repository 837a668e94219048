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
CONFIG_EXEMPT = ("updates", "save", "save_every", "save_best", "resume", "eval_every", "eval_episodes", "log", "return_details")
RESUME_SECTIONS = ("population", "trainer", "env", "scheduler", "loop", "config")


def run_config(**kwargs):
    """The "config" section of a run of train(**kwargs): its effective arguments (defaults filled in) without CONFIG_EXEMPT, as
    plain data."""
    import inspect
    from ship_sim_gym_amd.checkpoint import plain_config
    args = {k: p.default for k, p in inspect.signature(train).parameters.items()}
    unknown = sorted(set(kwargs) - set(args))
    if unknown:
        raise TypeError("train() has no argument %s" % ", ".join(unknown))
    args.update(kwargs)
    return plain_config({k: v for k, v in args.items() if k not in CONFIG_EXEMPT})


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
    if a.eval_every < 0 or a.eval_episodes < 1:
        ap.error("--eval-every must be >= 0 and --eval-episodes >= 1")
    if a.reward_clip != 10.0 and not a.norm_reward:
        ap.error("--reward-clip needs --norm-reward")
    if not a.reward_clip >= 0.0:
        ap.error("--reward-clip must be >= 0")
    if a.save_every < 0:
        ap.error("--save-every must be >= 0")
    if a.save_every and not a.save:
        ap.error("--save-every needs --save (the file it rewrites)")
    return a


def train(members=16, envs_per_member=512, updates=40, horizon=32, perturb_every=5, seed=0, epochs=2, minibatches=4, lrs=None,
          pbt=True, device="cuda:0", log=print, return_details=False, kl_coeff=0.0, kl_target=0.01, vf_clip=0.0, max_grad_norm=0.0,
          separate_value=False, mutate_schedule=False, max_epochs=30, eval_every=0, eval_episodes=1, envs=None, mutate_batch=False,
          batch_shares=None, quantum=None, obs_filter=False, norm_reward=False, reward_clip=10.0, adv_norm="batch", perm="torch",
          timeout_bootstrap=False, hidden=64, env_kw=None, save=None, save_every=0, save_best=None, resume=None):
    config = run_config(**dict(locals()))  # (first statement: the arguments, nothing else)
    import torch
    from ship_gym.config import EnvConfig, GameConfig
    from ship_sim_gym_amd import checkpoint
    from ship_sim_gym_amd.population import NativePopulation, PBTScheduler, PopulationPPO, reference_mutations, slices_for_batch_sizes
    from ship_sim_gym_amd.ppo import chunk_split
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    from train.ppo_torch import ActorCritic, open_resume
    from train.rllib_ppo import game_configuration

    if save_every < 0 or (save_every and not save):
        raise ValueError("train: save_every must be >= 0 and needs save (the file it rewrites)")
    ckpt = None
    if resume:  # (read and compared before any device work: a wrong command line costs nothing)
        ckpt = open_resume(resume, config, RESUME_SECTIONS + (("obs_filter",) if obs_filter else ()) + (("ret_filter",) if norm_reward else ()),
                           exempt=CONFIG_EXEMPT)
    env_kw = dict(env_kw or {})

    if perm not in ("torch", "native"):
        raise ValueError("train: perm must be 'torch' or 'native' (got %r)" % (perm,))
    native_perm = perm == "native"
    P, n = int(members), int(envs_per_member)
    n_total = int(envs) if envs is not None else P * n
    sliced = bool(mutate_batch) or batch_shares is not None
    if mutate_batch and batch_shares is not None:
        raise ValueError("train: mutate_batch and batch_shares exclude each other")
    if not sliced and n_total % P:
        raise ValueError("train: %d envs do not split into %d equal member slices" % (n_total, P))
    n = max(1, n_total // P)
    if lrs is not None and len(lrs) != P:
        raise ValueError("train: %d learning rates for %d members" % (len(lrs), P))
    if batch_shares is not None and len(batch_shares) != P:
        raise ValueError("train: %d batch shares for %d members" % (len(batch_shares), P))
    quantum = default_quantum(n_total, P) if quantum is None else int(quantum)
    torch.manual_seed(seed)
    dev = torch.device(device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed + 1)
    saved = {k: getattr(GameConfig, k) for k in ("FPS", "SPEED", "DEBUG", "BOUNDS")}
    try:  # (game_configuration writes the GameConfig class, as the reference's does; the env reads it once, here)
        env = ShipVecEnv(n_total, game_configuration(speed=30, fps=1000, debug=False), EnvConfig, device=device, n_maps=64, **env_kw)
        # the held-out run's env (train/rllib/rollout.py:8-26): evaluation resets and steps it, the training envs keep their episodes
        eval_env = ShipVecEnv(P * min(n, 256), GameConfig, EnvConfig, device=device, n_maps=64, **env_kw) if eval_every else None
    finally:
        for k, v in saved.items():
            setattr(GameConfig, k, v)
    D, A = env.states_history, env.action_space.n
    nets = [ActorCritic(D, A, hidden=hidden, separate_value=separate_value).to(dev) for _ in range(P)]
    scale = torch.full((D,), float(max(env.bounds)), dtype=torch.float64, device=dev)
    pop = NativePopulation.from_actor_critics(nets, scale)
    sched = PBTScheduler(P, seed=seed, perturbation_interval=perturb_every,
                         mutations=reference_mutations(schedule=mutate_schedule, batch=mutate_batch) if mutate_schedule or mutate_batch else None)
    samples = horizon * n
    member_samples = [samples] * P  # a member's own samples per update (unequal once the handle is sliced)
    reslices = []
    raw = None
    if mutate_schedule:  # (drawn first: a seed's schedule does not depend on whether the batch is mutated too)
        raw = [(sched.rng.choice(INITIAL_SCHEDULE["num_sgd_iter"]), sched.rng.choice(INITIAL_SCHEDULE["sgd_minibatch_size"])) for _ in range(P)]
    batch_sizes = None
    if sliced:
        batch_sizes = initial_batch_sizes(sched, P) if mutate_batch else list(batch_shares)
        slices = slices_for_batch_sizes(batch_sizes, n_total, quantum)
        env.set_population_slices(slices)
        member_samples = [horizon * s for s in slices]
        reslices.append((0, list(slices)))
        log("slices: train_batch_size %s -> envs %s (quantum %d)" % (batch_sizes, slices, quantum))
    ppo = PopulationPPO(pop, env, lam=INITIAL["lambda"], clip=INITIAL["clip_param"], lr=list(lrs) if lrs is not None else INITIAL["lr"],
                        vf_clip=vf_clip, max_grad_norm=max_grad_norm, kl_coef=kl_coeff, kl_target=kl_target if kl_coeff > 0 else 0.0, adv_norm=adv_norm,
                        perm_seed=seed if native_perm else None)
    flt = None
    if obs_filter:  # per-member statistics; a member's rows are its slice, whatever the slices currently are
        from ship_sim_gym_amd.obs_filter import ObsFilter
        flt = ObsFilter(env, n_members=P)
        env.set_obs_filter(flt)
        if eval_env is not None:
            eval_env.set_obs_filter(flt.frozen(eval_env))
    rflt = None
    if norm_reward:  # per-member statistics of the discounted returns; applied between the rollout and GAE, nothing is bound to the env
        from ship_sim_gym_amd.ret_filter import ReturnFilter
        rflt = ReturnFilter(env, n_members=P, gamma=ppo.gamma, clip=reward_clip)
        ppo.set_return_filter(rflt)  # (an exploit copies the source's state rows with its weights)
    if timeout_bootstrap:  # (the rollout then also returns "boot", which gae() reads: a time-out is no longer scored as a return of 0)
        env.set_timeout_bootstrap(True, rows=horizon)
    env.reset_tensor()
    window = torch.zeros((P, 3), dtype=torch.int64, device=dev)  # episodes since the last perturbation
    scores = [float("-inf")] * P
    out, history, exploits, evals = None, [], [], []
    evaluator = None
    if eval_env is not None:
        from ship_sim_gym_amd.evaluate import NativeEvaluator, format_table
        evaluator = NativeEvaluator(eval_env)
    # the schedule: common ints (one launch shape for everyone, as before) or one entry per member
    per_member = sliced or mutate_schedule or isinstance(epochs, (list, tuple)) or isinstance(minibatches, (list, tuple))
    if mutate_schedule:
        draws = [clamp_schedule(i, s, member_samples[m], max_epochs) for m, (i, s) in enumerate(raw)]
        iters, sizes = [d[0] for d in draws], [d[1] for d in draws]
        log("schedule: num_sgd_iter %s  sgd_minibatch_size %s" % (iters, sizes))
    elif per_member:
        iters = [int(e) for e in epochs] if isinstance(epochs, (list, tuple)) else [int(epochs)] * P
        counts = [int(b) for b in minibatches] if isinstance(minibatches, (list, tuple)) else [int(minibatches)] * P
        if len(iters) != P or len(counts) != P:
            raise ValueError("train: %d epochs and %d minibatches for %d members" % (len(iters), len(counts), P))
        sizes = [chunk_split(member_samples[m], c)[0] for m, c in enumerate(counts)]
    perm_epochs = max_epochs if mutate_schedule else (max(iters) if per_member else epochs)
    if save or save_best:
        env.check_snapshot_supported("snapshot")  # (refuse now, not after the training, a handle that cannot be saved)
    # --save-best: the best member's episode_reward_mean so far, the update and the member it belongs to; episodes ended per update
    best, best_update, best_member, ended_log = float("-inf"), 0, -1, []
    start = 1
    if ckpt is not None:  # everything is built and bound as the configuration says; now the saved layout, then the saved state
        loop = ckpt["loop"]
        if sliced:  # (the layout the run had when it was saved, not the initial one)
            batch_sizes, slices = list(loop["batch_sizes"]), [int(x) for x in loop["slices"]]
            env.set_population_slices(slices)
            member_samples = [horizon * x for x in slices]
        if per_member:
            iters, sizes = [int(x) for x in loop["iters"]], [int(x) for x in loop["sizes"]]
            if not mutate_schedule:
                counts = [int(x) for x in loop["counts"]]
        pop.load_state_dict(ckpt["population"])
        ppo.load_state_dict(ckpt["trainer"])
        if flt is not None:
            flt.load_state_dict(ckpt["obs_filter"])
        if rflt is not None:
            rflt.load_state_dict(ckpt["ret_filter"])
        sched.load_state_dict(ckpt["scheduler"])
        env.restore(ckpt["env"])
        gen.set_state(loop["gen_state"])
        window.copy_(loop["window"])
        scores, history = [float(x) for x in loop["scores"]], [list(r) for r in loop["history"]]
        exploits, reslices = events_from_plain(loop["exploits"]), [(int(r[0]), list(r[1])) for r in loop["reslices"]]
        best, best_update, best_member = float(loop["best"]), int(loop["best_update"]), int(loop["best_member"])
        ended_log = [int(x) for x in loop["episodes_ended"]]
        start = int(loop["update"]) + 1
        log("resumed from %s: %d updates done, continuing at update %d of %d" % (resume, start - 1, start, updates))

    def write(path, u):
        """The checkpoint after update u (and after its perturbation, when one was due): everything a resumed run needs."""
        sections = {"config": config, "population": pop.state_dict(), "trainer": ppo.state_dict(), "env": env.snapshot(),
                    "scheduler": sched.state_dict(),
                    "loop": {"update": int(u), "gen_state": gen.get_state().cpu().clone(), "history": [list(r) for r in history],
                             "scores": list(scores), "window": window.detach().cpu().clone(), "exploits": plain_events(exploits),
                             "reslices": [[int(r[0]), list(r[1])] for r in reslices],
                             "iters": list(iters) if per_member else [], "sizes": list(sizes) if per_member else [],
                             "counts": list(counts) if per_member and not mutate_schedule else [],
                             "batch_sizes": list(batch_sizes) if sliced else [], "slices": list(env.population_slices) if sliced else [],
                             "best": float(best), "best_update": int(best_update), "best_member": int(best_member),
                             "episodes_ended": list(ended_log)}}
        if flt is not None:
            sections["obs_filter"] = flt.state_dict()
        if rflt is not None:
            sections["ret_filter"] = rflt.state_dict()
        checkpoint.save(path, sections)

    for u in range(start, updates + 1):
        uniforms = torch.rand((horizon, n_total), generator=gen, device=dev)
        batch = env.rollout_population(pop, horizon, uniforms=uniforms, out=out)
        out = {k: v for k, v in batch.items() if k not in ("adv", "ret", "logp_all", "rew_norm", "rew_denom")}
        ep = ppo.episode_stats(batch)
        window += ep
        if rflt is not None:
            rflt.set_gamma(ppo.gamma)  # (the members' own discounts, whatever they currently are)
        ppo.gae(batch, return_filter=rflt)
        if native_perm:  # update() draws what it needs itself: max(iters) rows per member, in the bound layout, keyed by its count
            perm = None
        elif sliced:  # member m's own rows: [perm_epochs, horizon * n_m], nothing padded to the widest member
            perm = [torch.rand((perm_epochs, s), generator=gen, device=dev).argsort(dim=-1) for s in member_samples]
        else:
            perm = torch.rand((P, perm_epochs, samples), generator=gen, device=dev).argsort(dim=-1)
        if per_member:
            mbs = [ppo.minibatches_for_size(s, member_samples[m]) for m, s in enumerate(sizes)] if mutate_schedule else counts
            if native_perm:
                ppo.update(batch, None, iters, mbs)
            elif sliced:
                ppo.update(batch, [q[:max(iters)].contiguous() for q in perm], iters, mbs)
            else:
                ppo.update(batch, perm[:, :max(iters)].contiguous(), iters, mbs)
        else:
            ppo.update(batch, perm, epochs, minibatches)
        w = window.cpu().tolist()
        scores = [w[m][0] / 100.0 / w[m][2] if w[m][2] else scores[m] for m in range(P)]
        history.append(list(scores))
        log("update %d  episode_reward_mean %s" % (u, " ".join("%d:%.3f" % (m, s) for m, s in enumerate(scores))))
        ended_log.append(int(ep[:, 2].sum().item()))
        new_best = ended_log[-1] > 0 and max(scores) > best  # (an update in which no episode ended never is one)
        if new_best:
            best, best_update, best_member = max(scores), u, scores.index(max(scores))
        if evaluator is not None and u % eval_every == 0:  # (printed only: PBT ranks by training episodes, as the reference does)
            r = evaluator.evaluate(pop, eval_episodes, greedy=True)
            evals.append((u, r["per_member"].cpu().tolist()))
            log("update %d  greedy evaluation (%d envs x %d episodes per member)\n%s" % (u, eval_env.num_envs // P, eval_episodes, format_table(r)))
        if pbt and sched.due(u):
            hp = {"lambda": ppo.lam, "clip_param": ppo.clip, "lr": ppo.lr}
            if mutate_batch:
                hp["train_batch_size"] = batch_sizes
            elif sliced:  # (fixed shares are the member's configuration: they travel with an exploit, unmutated)
                hp["batch_share"] = batch_sizes
            if mutate_schedule:
                hp.update({"num_sgd_iter": iters, "sgd_minibatch_size": sizes})
            elif per_member:  # a swept schedule is not mutated, but it is its member's configuration: it travels with an exploit
                hp.update({"num_sgd_iter": iters, "minibatches": counts})
            src, new, events = sched.perturb(scores, hp)
            ppo.exploit(src)
            ppo.lam, ppo.clip, ppo.lr = new["lambda"], new["clip_param"], new["lr"]
            if sliced:  # re-slice the handle from the members' current values; env state and the episode carries stay as they are
                batch_sizes = new["train_batch_size"] if mutate_batch else new["batch_share"]
                slices = slices_for_batch_sizes(batch_sizes, n_total, quantum)
                env.set_population_slices(slices)
                member_samples = [horizon * s for s in slices]
                reslices.append((u, list(slices)))
                log("update %d  re-slice: train_batch_size %s -> envs %s" % (u, batch_sizes, slices))
            if mutate_schedule:  # (the minibatch-size clamp uses the member's own samples)
                used = [clamp_schedule(i, s, member_samples[m], max_epochs)
                        for m, (i, s) in enumerate(zip(new["num_sgd_iter"], new["sgd_minibatch_size"]))]
                iters, sizes = [c[0] for c in used], [c[1] for c in used]
            elif per_member:
                iters, counts = new["num_sgd_iter"], new["minibatches"]
                sizes = [chunk_split(member_samples[m], c)[0] for m, c in enumerate(counts)]
            for ev in events:
                log("update %d  exploit: member %d <- member %d" % (u, ev["member"], ev["source"]))
                for key, kind, old, val in ev["mutations"]:
                    log("update %d  mutation: member %d %s %s %.6g -> %.6g" % (u, ev["member"], key, kind, old, val))
                if per_member:
                    ev["schedule"] = {"num_sgd_iter": iters[ev["member"]], "sgd_minibatch_size": sizes[ev["member"]]}
                    log("update %d  schedule: member %d num_sgd_iter %d sgd_minibatch_size %d (as used)"
                        % (u, ev["member"], iters[ev["member"]], sizes[ev["member"]]))
                scores[ev["member"]] = scores[ev["source"]]
            exploits += events
            window.zero_()
        if new_best and save_best:  # (after the perturbation, so that the file resumes like any other; the best member ranks top: a source, not a destination)
            write(save_best, u)
            log("update %d  member %d's episode_reward_mean %.3f is the best so far: saved to %s" % (u, best_member, best, save_best))
        if save and save_every and u % save_every == 0:
            write(save, u)
    torch.cuda.synchronize(dev)
    if save:
        write(save, max(updates, start - 1))
        log("checkpoint after update %d saved to %s" % (max(updates, start - 1), save))
    pop.load_into(nets)
    details = {"params": pop.params.detach().clone(), "exploits": exploits, "nets": nets,
               "hparams": {"lambda": list(ppo.lam), "clip_param": list(ppo.clip), "lr": list(ppo.lr),
                           "num_sgd_iter": list(iters) if per_member else [int(epochs)] * P,
                           "sgd_minibatch_size": list(sizes) if per_member else [chunk_split(samples, minibatches)[0]] * P},
               "member_steps": list(ppo.member_steps), "kl_coef": ppo.kl_coef.detach().cpu().tolist(), "evaluations": evals,
               "slices": list(env.population_slices) if sliced else [n] * P, "reslices": reslices,
               "train_batch_size": list(batch_sizes) if sliced else [samples] * P,
               "best": best, "best_update": best_update, "best_member": best_member, "episodes_ended": list(ended_log),
               "env_state": env.state.detach().cpu().clone() if return_details else None}
    if flt is not None:
        details["obs_filter"] = flt.state_dict()
        log("observation filter: rows merged per member %s" % [int(c) for c in details["obs_filter"]["state"][:, 3, 0].tolist()])
    if rflt is not None:
        details["ret_filter"] = rflt.state_dict()
        log("return filter: returns merged per member %s  std %s" % ([int(c) for c in details["ret_filter"]["state"][:, 3].tolist()],
                                                                     ["%.5f" % d for d in details["ret_filter"]["state"][:, 2].tolist()]))
    if eval_env is not None:
        eval_env.close()
    env.close()
    return (history, details) if return_details else history


def main(argv=None):
    a = parse_args(argv)
    train(members=a.members, envs_per_member=a.envs_per_member, updates=a.updates, horizon=a.horizon, perturb_every=a.perturb_every,
          seed=a.seed, epochs=a.epochs, minibatches=a.minibatches, lrs=a.lrs, pbt=a.pbt, device=a.device, kl_coeff=a.kl_coeff,
          kl_target=a.kl_target, vf_clip=a.vf_clip, max_grad_norm=a.max_grad_norm, separate_value=a.separate_value,
          mutate_schedule=a.mutate_schedule, max_epochs=a.max_epochs, eval_every=a.eval_every, eval_episodes=a.eval_episodes, envs=a.envs,
          mutate_batch=a.mutate_batch, batch_shares=a.batch_shares, quantum=a.quantum, obs_filter=a.obs_filter,
          norm_reward=a.norm_reward, reward_clip=a.reward_clip, adv_norm=a.adv_norm, perm=a.perm, timeout_bootstrap=a.timeout_bootstrap,
          hidden=a.hidden, save=a.save, save_every=a.save_every, save_best=a.save_best, resume=a.resume)


if __name__ == "__main__":
    main()
