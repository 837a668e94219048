"""Hyper-parameter schedules on the host (ship_sim_gym_amd/hparam_schedule.py): the values at, between and beyond the points, PPO2's and
RLlib's rules bit for bit, the command lines' specs, every refusal, and the two trainer scripts' flags before any env is built.

Every comparison of a value is ==: the module fixes its expression, v_i + ((t - t_i) / (t_{i+1} - t_i)) * (v_{i+1} - v_i) in Python
floats with the true division of the two ints, and the tests restate it."""
import math

import pytest

from gpu_support import load_script
from ship_sim_gym_amd.hparam_schedule import HparamSchedule, check_schedulable, entry_from_state, entry_state

ONE = [(0, 0.25)]
TWO = [(0, 1e-3), (2688, 0.0)]
THREE = [(0, 1e-3), (5_000_000, 1e-4), (10_000_000, 1e-5)]  # train/rllib/ppo.py:39's lr_schedule


def _expr(points, t):
    """The module's expression, restated."""
    if t >= points[-1][0]:
        return points[-1][1]
    for (t0, v0), (t1, v1) in zip(points, points[1:]):
        if t0 <= t < t1:
            return v0 + ((t - t0) / (t1 - t0)) * (v1 - v0)
    raise AssertionError(t)


@pytest.mark.parametrize("points", [ONE, TWO, THREE], ids=["one", "two", "three"])
def test_values_at_between_and_beyond_the_points(points):
    s = HparamSchedule(points)
    for t, v in points:
        assert s.value(t) == v
    last_t, last_v = points[-1]
    for t in (last_t, last_t + 1, last_t * 3 + 7, 10 ** 12):
        assert s.value(t) == last_v
    for (t0, v0), (t1, v1) in zip(points, points[1:]):
        for t in (t0 + 1, (t0 + t1) // 2, (t0 + 2 * t1) // 3, t1 - 1):
            got = s.value(t)
            assert got == _expr(points, t) and isinstance(got, float)
            assert min(v0, v1) <= got <= max(v0, v1) and got != v0
    assert s.values() == [v for _, v in points]
    for bad in (-1, 0.5, 1.0, True, None, "3"):
        with pytest.raises(ValueError, match="int >= 0"):
            s.value(bad)


@pytest.mark.parametrize("start", [1e-3, 1e-4, 1e-5])
def test_ppo2s_linear_decay_bit_for_bit(start):
    """train/stable_baselines/ppo.py:111-119,137: make_lr_func(s, 0) under PPO2's frac = 1 - (update - 1) / nupdates, update = 1 ..."""
    nupdates, n_batch, stop = 7, 384, 0.0
    s = HparamSchedule.linear(start, stop, nupdates * n_batch)
    assert s == HparamSchedule([(0, start), (nupdates * n_batch, stop)])
    for u in range(nupdates):
        assert s.value(u * n_batch) == start + ((u) / nupdates) * (stop - start)
    assert s.value(0) == start and s.value(nupdates * n_batch) == 0.0 and s.value(nupdates * n_batch * 2) == 0.0
    assert [s.value(u * n_batch) for u in range(nupdates)] == sorted((s.value(u * n_batch) for u in range(nupdates)), reverse=True)


def test_the_rllib_experiments_points():
    s = HparamSchedule(THREE)
    assert s.value(0) == 1e-3
    assert s.value(2_500_000) == 1e-3 + ((2_500_000 - 0) / (5_000_000 - 0)) * (1e-4 - 1e-3)
    assert s.value(7_500_000) == 1e-4 + ((7_500_000 - 5_000_000) / (10_000_000 - 5_000_000)) * (1e-5 - 1e-4)
    assert s.value(10 ** 7) == s.value(10 ** 9) == 1e-5


def test_constructors_state_and_equality():
    c = HparamSchedule.constant(0.2)
    assert c.state() == [[0, 0.2]] and c.value(0) == c.value(10 ** 9) == 0.2
    s = HparamSchedule(THREE)
    st = s.state()
    assert st == [[0, 1e-3], [5_000_000, 1e-4], [10_000_000, 1e-5]]
    assert all(type(p) is list and type(p[0]) is int and type(p[1]) is float for p in st)  # (plain data: no tuple, no None)
    from ship_sim_gym_amd.checkpoint import check_plain
    check_plain(st)
    assert HparamSchedule.from_state(st) == s and HparamSchedule.from_state(st) is not s
    assert s != HparamSchedule(TWO) and s != st and HparamSchedule([(0, 1)]) == HparamSchedule.constant(1.0)
    assert entry_state(None) == [] and entry_from_state("t", "lr", []) is None and entry_from_state("t", "lr", st) == s


def test_parse_both_forms_round_trip():
    lin = HparamSchedule.parse("linear:1e-5", 3e-4, 2048)
    assert lin == HparamSchedule.linear(3e-4, 1e-5, 2048) and lin.state() == [[0, 3e-4], [2048, 1e-5]]
    assert HparamSchedule.from_state(lin.state()) == lin
    pts = HparamSchedule.parse("0:1e-3,5000000:1e-4,10000000:1e-5", 123.0, 1)  # (absolute points: start and total do not enter)
    assert pts == HparamSchedule(THREE) and HparamSchedule.from_state(pts.state()) == pts
    assert HparamSchedule.parse(" 0:0.2, 1024:0.1 ", 0.0, 1) == HparamSchedule([(0, 0.2), (1024, 0.1)])
    assert HparamSchedule.parse("0:0.5", 0.0, 1) == HparamSchedule.constant(0.5)


@pytest.mark.parametrize("points,names", [
    ([], "non-empty"), (None, "non-empty"), ("0:1", "non-empty"),
    ([(1, 0.5)], r"points\[0\]"), ([(0, 0.5), (0, 0.4)], r"points\[1\]"), ([(0, 0.5), (8, 0.4), (4, 0.3)], r"points\[2\]"),
    ([(0.0, 0.5)], r"points\[0\]"), ([(0, 0.5), (True, 0.4)], r"points\[1\]"), ([(0, float("nan"))], r"points\[0\]"),
    ([(0, 0.5), (3, float("inf"))], r"points\[1\]"), ([(0, 0.5), (3, None)], r"points\[1\]"), ([(0, 0.5), (3, "x")], r"points\[1\]"),
    ([(0, 0.5), 3], r"points\[1\]"), ([(0, 0.5, 1)], r"points\[0\]"),
])
def test_points_that_are_refused_name_the_entry(points, names):
    with pytest.raises(ValueError, match=names):
        HparamSchedule(points)


@pytest.mark.parametrize("spec", ["", "linear", "linear:", "linear:x", "0", "0:1,", "0:1;5:2", "1:0.5", "0:1,0:2", "0:nan", "0.5:1", "a:b", None, 3])
def test_malformed_specs_quote_the_spec(spec):
    with pytest.raises(ValueError) as ex:
        HparamSchedule.parse(spec, 1.0, 100)
    assert repr(spec) in str(ex.value)


def test_a_linear_spec_needs_a_span():
    for total in (0, -5, 2.5, None):
        with pytest.raises(ValueError) as ex:
            HparamSchedule.parse("linear:0", 1.0, total)
        assert "'linear:0'" in str(ex.value)


def test_the_trainers_refusals():
    """A clip schedule must be > 0 at every point; lr and ent_coef need only be finite; a malformed state entry names its field."""
    for pts in ([(0, 0.2), (10, 0.0)], [(0, -0.1)], [(0, 0.2), (5, 0.1), (9, -1e-9)]):
        with pytest.raises(ValueError, match=r"clip schedule's points\[%d\]" % (len(pts) - 1)):
            check_schedulable("who", "clip", HparamSchedule(pts))
    neg = HparamSchedule([(0, 0.0), (4, -1.0)])
    assert check_schedulable("who", "lr", neg) is neg and check_schedulable("who", "ent_coef", neg) is neg
    for entry in ([[1, 0.5]], [[0, 0.5], [0, 0.4]], "x", [[0]], {"a": 1}):
        with pytest.raises(ValueError, match=r"schedules\['lr'\]"):
            entry_from_state("who", "lr", entry)
    with pytest.raises(ValueError, match=r"schedules\['clip'\].*not > 0"):
        entry_from_state("who", "clip", [[0, 0.2], [8, 0.0]])
    assert math.isfinite(neg.value(3))


# ------------------------------------------------------------------------------------------------------------------------------------
# the scripts, before any env is built
# ------------------------------------------------------------------------------------------------------------------------------------
FLAGS = ["--lr-schedule", "linear:0", "--clip-schedule", "0:0.2,1024:0.1", "--ent-schedule", "linear:0.001", "--total-timesteps", "2048"]
NAMES = ("lr_schedule", "clip_schedule", "ent_schedule", "total_timesteps")


def _no_env(*a, **k):
    pytest.fail("an env was built before the refusal")


@pytest.fixture(scope="module")
def single():
    return load_script("train/ppo_torch.py")


@pytest.fixture(scope="module")
def pbt():
    return load_script("train/pbt_native.py")


def test_the_single_trainers_flags_and_config(single, monkeypatch, capsys):
    import inspect
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = single.parse_args(FLAGS + ["--lr", "1e-3", "--clip", "0.3"])
    assert (a.lr_schedule, a.clip_schedule, a.ent_schedule, a.total_timesteps) == ("linear:0", "0:0.2,1024:0.1", "linear:0.001", 2048)
    assert all(n in inspect.signature(single.train).parameters for n in NAMES)  # (main() hands every flag to train() by name)
    scheds, span = single.make_hparam_schedules(a)
    assert span == 2048 and scheds["lr"] == HparamSchedule.linear(1e-3, 0.0, 2048)
    assert scheds["clip"] == HparamSchedule([(0, 0.2), (1024, 0.1)]) and scheds["ent_coef"] == HparamSchedule.linear(0.01, 0.001, 2048)
    d = single.parse_args(["--lr-schedule", "linear:0", "--updates", "7", "--envs", "96", "--horizon", "4"])  # the span's default: the run's length
    scheds, span = single.make_hparam_schedules(d)
    assert span == 7 * 96 * 4 and scheds["lr"] == HparamSchedule.linear(3e-4, 0.0, 7 * 96 * 4) and scheds["clip"] is None
    assert single.make_hparam_schedules(single.parse_args([]))[0] == {"lr": None, "clip": None, "ent_coef": None}
    assert single.run_config(lr_schedule="linear:0") != single.run_config()
    assert single.run_config(lr_schedule="linear:0")["lr_schedule"] == "linear:0" and single.run_config()["total_timesteps"] == "None"
    assert not set(NAMES) & set(single.CONFIG_EXEMPT)
    # refusals: on the command line, and from train() before an env exists
    monkeypatch.setattr(single, "ShipVecEnv", _no_env)
    for argv, kw, text in ((["--lr-schedule", "0:1,0:2"], dict(lr_schedule="0:1,0:2"), "'0:1,0:2'"),
                           (["--clip-schedule", "linear:0"], dict(clip_schedule="linear:0"), "not > 0"),
                           (["--ent-schedule", "linear:0", "--total-timesteps", "0"], dict(ent_schedule="linear:0", total_timesteps=0), "total"),):
        with pytest.raises(SystemExit) as ex:
            single.parse_args(argv)
        assert ex.value.code not in (0, None) and text in capsys.readouterr().err
        for mode, update in (("eager", "torch"), ("native", "native")):
            with pytest.raises(ValueError, match=text):
                single.train(envs=8, updates=1, log=None, mode=mode, update=update, **kw)


def test_the_population_scripts_flags_refusals_and_config(pbt, monkeypatch, capsys):
    import inspect
    from ship_sim_gym_amd import vec_env
    monkeypatch.setattr(vec_env, "ShipVecEnv", _no_env)
    a = pbt.parse_args(["--lrs", "1e-3,1e-4,1e-5", "--no-pbt"] + FLAGS)  # the Stable-Baselines script's sweep in one population
    assert (a.lr_schedule, a.clip_schedule, a.ent_schedule, a.total_timesteps) == ("linear:0", "0:0.2,1024:0.1", "linear:0.001", 2048)
    assert all(n in inspect.signature(pbt.train).parameters for n in NAMES)
    assert pbt.parse_args(["--ent-schedule", "linear:0"]).ent_schedule == "linear:0"  # (the entropy coefficient's goes with PBT)
    assert pbt.run_config(lr_schedule="linear:0") != pbt.run_config() and not set(NAMES) & set(pbt.CONFIG_EXEMPT)
    refused = ((["--lr-schedule", "linear:0"], dict(lr_schedule="linear:0"), "needs --no-pbt"),
               (["--clip-schedule", "0:0.2,9:0.1"], dict(clip_schedule="0:0.2,9:0.1"), "needs --no-pbt"),
               (["--no-pbt", "--mutate-batch", "--lr-schedule", "linear:0"], dict(pbt=False, mutate_batch=True, lr_schedule="linear:0"), "--mutate-batch"),
               (["--no-pbt", "--mutate-batch", "--clip-schedule", "linear:0.1"], dict(pbt=False, mutate_batch=True, clip_schedule="linear:0.1"), "--mutate-batch"),
               (["--mutate-batch", "--ent-schedule", "linear:0"], dict(mutate_batch=True, ent_schedule="linear:0"), "--mutate-batch"),
               (["--no-pbt", "--lr-schedule", "zz"], dict(pbt=False, lr_schedule="zz"), "'zz'"),
               (["--no-pbt", "--clip-schedule", "linear:0"], dict(pbt=False, clip_schedule="linear:0"), "not > 0"))
    for argv, kw, text in refused:
        with pytest.raises(SystemExit) as ex:
            pbt.parse_args(argv)
        assert ex.value.code not in (0, None) and text in capsys.readouterr().err, argv
        with pytest.raises(ValueError, match=text):
            pbt.train(members=2, envs_per_member=8, updates=1, log=None, **kw)


def test_each_member_decays_from_its_own_constant_over_its_own_run(pbt):
    """--lrs 1e-3,1e-4,1e-5 --no-pbt --lr-schedule linear:0: member m's schedule is linear(lrs[m], 0, updates * horizon * n_m)."""
    import argparse
    run = argparse.Namespace(P=3, updates=5, horizon=4, total_timesteps=None, lr_schedule="linear:0", clip_schedule=None, ent_schedule="0:0.01,64:0.0")
    hp = pbt.member_hparam_schedules(run, [64, 128, 64], [1e-3, 1e-4, 1e-5])
    assert hp["lr"] == [HparamSchedule.linear(lr, 0.0, 5 * 4 * n) for lr, n in zip([1e-3, 1e-4, 1e-5], [64, 128, 64])]
    assert hp["clip"] == [0.2] * 3 and hp["ent_coef"] == [HparamSchedule([(0, 0.01), (64, 0.0)])] * 3
    run.total_timesteps = 999
    assert pbt.member_hparam_schedules(run, [64, 128, 64], [1e-3, 1e-4, 1e-5])["lr"][1] == HparamSchedule.linear(1e-4, 0.0, 999)
