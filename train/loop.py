"""What train/ppo_torch.py and train/pbt_native.py do alike, once: a run's "config" section, opening the checkpoint it resumes from, the
value checks of both command lines, and binding the filters, the time-out bootstrap and the evaluator to the envs.  Host only: importing
it imports no torch.  What merely looks alike — the loop-state records, the save-best rules — differs in substance and stays apart."""


def run_config(train_fn, exempt, kwargs):
    """The "config" section of a run of train_fn(**kwargs): its effective arguments (defaults filled in) without `exempt`, as plain data."""
    import inspect
    from ship_sim_gym_amd.checkpoint import plain_config
    args = {k: p.default for k, p in inspect.signature(train_fn).parameters.items()}
    unknown = sorted(set(kwargs) - set(args))
    if unknown:
        raise TypeError("train() has no argument %s" % ", ".join(unknown))
    args.update(kwargs)
    return plain_config({k: v for k, v in args.items() if k not in exempt})


def open_resume(path, config, require, who="train", exempt=()):
    """Read the checkpoint a run resumes from and compare its configuration with this run's (host only, before any device work):
    ValueError for a file without trainer state, for a missing section, and for arguments that differ — every key, with both values."""
    from ship_sim_gym_amd import checkpoint
    ckpt = checkpoint.load(path)
    if "trainer" not in ckpt:
        raise ValueError("%s: %s holds no trainer section: it was saved by a run whose update is not the device's (--mode native --update "
                         "native), so it can be evaluated but not resumed" % (who, path))
    checkpoint.validate(ckpt, require, str(path))
    diff = checkpoint.config_differences(ckpt["config"], config)
    if diff:
        raise ValueError("%s: cannot resume from %s: the arguments differ from the file's config in %s (only %s may change)" % (
            who, path, "; ".join("%s (the file has %r, this run %r)" % (k, ckpt["config"].get(k, "nothing"), config.get(k, "nothing")) for k in diff),
            ", ".join(exempt)))
    return ckpt


# the checkpoint sections that depend on the configuration: the section, and the train() argument that switches it on
OPTIONAL_SECTIONS = (("obs_filter", "obs_filter"), ("ret_filter", "norm_reward"), ("episode_log", "episode_log"))


def resume_sections(base, obs_filter, norm_reward, episode_log=None):
    """The sections a resumed run needs: the script's own and one per row of OPTIONAL_SECTIONS that is on."""
    on = {"obs_filter": obs_filter, "norm_reward": norm_reward, "episode_log": episode_log}
    return tuple(base) + tuple(section for section, arg in OPTIONAL_SECTIONS if on[arg])


def check_flag_values(a, error):
    """The value checks both command lines share (a: the parsed arguments; error: the parser's, which exits)."""
    if a.eval_every < 0 or a.eval_episodes < 1:
        error("--eval-every must be >= 0 and --eval-episodes >= 1")
    if a.reward_clip != 10.0 and not (a.norm_reward or getattr(a, "job_norm_reward", False)):
        error("--reward-clip needs --norm-reward" + (" or --job-norm-reward" if hasattr(a, "job_norm_reward") else ""))
    if not a.reward_clip >= 0.0:
        error("--reward-clip must be >= 0")
    if a.save_every < 0:
        error("--save-every must be >= 0")
    if a.save_every and not a.save:
        error("--save-every needs --save (the file it rewrites)")
    if a.episode_log_capacity < 1:
        error("--episode-log-capacity must be >= 1")
    if a.episode_log_capacity != 65536 and not (a.episode_log or getattr(a, "job_episode_log", None)):
        error("--episode-log-capacity needs --episode-log" + (" or --job-episode-log" if hasattr(a, "job_episode_log") else ""))


def bind_env(env, horizon, n_members=1, obs_filter=False, norm_reward=False, gamma=0.99, reward_clip=10.0, timeout_bootstrap=False,
             eval_env=None, job_obs_filter=False, job_norm_reward=False):
    """Bind what the configuration asks for to a training env of n_members members; returns (obs filter, return filter, evaluator), None
    where off.  The obs filter is bound to the env (the rollout merges each step's rows, then normalises) and, frozen, to eval_env —
    job_obs_filter: the job-wide one, with its buffer, which the caller synchronises after every rollout; the
    bootstrap makes the rollout return "boot", which gae() reads; the return filter is applied per rollout, between the rollout and GAE —
    job_norm_reward: the job-wide one, whose rows gae() gathers over the ranks."""
    flt = rflt = evaluator = None
    if obs_filter or job_obs_filter:
        from ship_sim_gym_amd.obs_filter import ObsFilter
        flt = ObsFilter(env, n_members=n_members, job=bool(job_obs_filter))
        env.set_obs_filter(flt)
    if timeout_bootstrap:
        env.set_timeout_bootstrap(True, rows=horizon)
    if norm_reward or job_norm_reward:
        from ship_sim_gym_amd.ret_filter import ReturnFilter
        rflt = ReturnFilter(env, n_members=n_members, gamma=gamma, clip=reward_clip, job=bool(job_norm_reward))
    if eval_env is not None:  # an env of its own: evaluation resets and steps it, the training envs keep their episodes
        from ship_sim_gym_amd.evaluate import NativeEvaluator
        evaluator = NativeEvaluator(eval_env)
        if flt is not None:
            eval_env.set_obs_filter(flt.frozen(eval_env))  # the training statistics, never updated by an evaluation
    return flt, rflt, evaluator


def filter_sections(flt, rflt):
    """The checkpoint sections of the filters that are on."""
    return {k: f.state_dict() for k, f in (("obs_filter", flt), ("ret_filter", rflt)) if f is not None}


def load_filters(ckpt, flt, rflt):
    for k, f in (("obs_filter", flt), ("ret_filter", rflt)):
        if f is not None:
            f.load_state_dict(ckpt[k])


def add_episode_log_flags(ap):
    """The flags both command lines share for the episode log."""
    ap.add_argument("--episode-log", default=None, metavar="FILE",
                    help="record every finished training episode on the device and write them to FILE in Stable-Baselines' monitor "
                         "format (r,l,t and more), flushed once per update; default: off")
    ap.add_argument("--episode-log-capacity", type=int, default=65536, metavar="C",
                    help="episodes the device ring holds between two flushes (needs --episode-log); older ones are dropped with a warning")


def bind_episode_log(env, path, capacity, n_members=1, resume=False, job_rows=None, writer=True):
    """(EpisodeLog, MonitorWriter) of a run that asks for one, else (None, None).  A resumed run keeps the file: loading the log's
    state cuts it back to the rows the checkpoint had written.  job_rows (the rollout length): the job-wide log of a data-parallel
    job — every rank calls this (the ranks' env counts are gathered once), and only the rank with `writer` attaches the file."""
    if not path:
        return None, None
    from ship_sim_gym_amd.episode_log import EpisodeLog, MonitorWriter
    if job_rows is None:
        eplog = EpisodeLog(env, capacity=capacity, n_members=n_members)
    else:
        eplog = EpisodeLog(env, capacity=capacity, job=True, rows=job_rows)
    return eplog, (MonitorWriter(path, eplog, resume=bool(resume)) if writer else None)


def episode_log_section(eplog):
    """The checkpoint section of the episode log when it is on."""
    return {"episode_log": eplog.state_dict()} if eplog is not None else {}


def load_episode_log(ckpt, eplog):
    if eplog is not None:
        eplog.load_state_dict(ckpt["episode_log"])


def add_report_flags(ap):
    """The flags both command lines share for the update report."""
    ap.add_argument("--report", action="store_true",
                    help="after every update print the explained variance of the value network and the means of the policy loss, value "
                         "loss, entropy and clip fraction over the update's minibatches, reduced on the device (needs --mode native "
                         "--update native where there is a choice); default: off")
    ap.add_argument("--report-kl", action="store_true",
                    help="also measure how far the update moved the policy (approximate KL, PPO2's approxkl, the clip fraction over the "
                         "whole batch): one more policy forward over the batch per update; implies --report")
    ap.add_argument("--progress", default=None, metavar="FILE",
                    help="write the report of every update to FILE as CSV, one row per policy (Stable-Baselines' progress.csv); implies --report")


def add_hparam_schedule_flags(ap, starts, span):
    """The flags both command lines share for the hyper-parameter schedules (ship_sim_gym_amd/hparam_schedule.py); starts / span: what
    a "linear:" spec starts from and spans by default, in the command line's words."""
    for flag, what in (("--lr-schedule", "learning rate"), ("--clip-schedule", "clip range"), ("--ent-schedule", "entropy coefficient")):
        ap.add_argument(flag, default=None, metavar="SPEC",
                        help="a hyper-parameter schedule of the %s, piecewise linear in the timesteps collected and evaluated once per "
                             "update: linear:STOP (from %s down to STOP over --total-timesteps) or absolute points T0:V0,T1:V1,... "
                             "(held at the last value afterwards); default: a constant" % (what, starts))
    ap.add_argument("--total-timesteps", type=int, default=None, metavar="T",
                    help="the span of a linear: spec (default: %s, the run's own length); not a stop criterion" % span)


def open_progress(path, resume=False):
    """The ProgressWriter of a run that asks for one, else None.  A resumed run keeps the file and cuts it back to the checkpoint's update."""
    if not path:
        return None
    from ship_sim_gym_amd.report import ProgressWriter
    return ProgressWriter(path, resume=bool(resume))
