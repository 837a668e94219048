"""The trainer scripts' parts on the host: the loop-state records and their checkpoint form, the one requirements table of
train/ppo_torch.py from both sides, torch_update on CPU tensors, and train/pbt_native.py's layout and schedule helpers on a fake env."""
import argparse
import copy

import pytest
import torch

from gpu_support import load_script

SINGLE_KEYS = {"update", "gen_state", "history", "scores", "best", "best_update", "episodes", "sum_return"}
PBT_KEYS = {"update", "gen_state", "history", "scores", "window", "exploits", "reslices", "iters", "sizes", "counts", "batch_sizes", "slices",
            "best", "best_update", "best_member", "episodes_ended"}
INF = float("inf")


@pytest.fixture(scope="module")
def single():
    return load_script("train/ppo_torch.py")


@pytest.fixture(scope="module")
def pbt():
    return load_script("train/pbt_native.py")


def _gen(draws=3):
    g = torch.Generator()
    g.manual_seed(11)
    for _ in range(draws):
        torch.rand(5, generator=g)
    return g


def _same(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def _single_record(mod):
    st = mod.LoopState(40, 12.5)
    st.update, st.history = 2, [(0, -1.5, 0.0, -0.01), (1, -1.25, 0.125, -0.02), (2, -1.0, 0.25, 0.03)]
    st.scores, st.best, st.best_update, st.episodes, st.sum_return = [-INF, -2.5, -0.75], -0.75, 2, 97, -130.25
    return st


def _pbt_record(mod):
    st = mod.LoopState(2, torch.tensor([[-250, 1, 3], [0, 0, 0]]), 128)
    st.update, st.history, st.scores = 3, [[-INF, -INF], [-1.5, -INF], [-0.75, -INF]], [-0.75, -INF]
    st.exploits = [{"member": 1, "source": 0, "mutations": [("lr", "perturb", 5e-4, 6e-4), ("num_sgd_iter", "resample", 10, 20)],
                    "schedule": {"num_sgd_iter": 3, "sgd_minibatch_size": 128}}]
    st.reslices, st.iters, st.sizes, st.counts = [(0, [16, 48]), (2, [32, 32])], [3, 3], [128, 256], []
    st.batch_sizes, st.slices, st.member_samples = [20000, 20000], [32, 32], [256, 256]
    st.best, st.best_update, st.best_member, st.episodes_ended = -0.75, 3, 0, [0, 1, 2]
    return st


def _fresh(mod, which):
    return mod.LoopState() if which == "single" else mod.LoopState(2, torch.zeros((2, 3), dtype=torch.int64), 128)


@pytest.mark.parametrize("which", ["single", "pbt"])
def test_loop_state_round_trip(which, single, pbt):
    from ship_sim_gym_amd import checkpoint
    mod, make, keys = (single, _single_record, SINGLE_KEYS) if which == "single" else (pbt, _pbt_record, PBT_KEYS)
    gen = _gen()
    sd = make(mod).state_dict(gen)
    checkpoint.check_plain(sd)
    assert set(sd) == keys
    assert all(isinstance(r, list) for r in sd["history"])  # (tuples are lists in the file)
    if which == "pbt":
        assert sd["exploits"][0]["mutations"][0] == ["lr", "perturb", 5e-4, 6e-4] and sd["reslices"][1] == [2, [32, 32]]
    fresh, gen2 = _fresh(mod, which), torch.Generator()
    fresh.load_state_dict(copy.deepcopy(sd), gen2)
    assert _same(fresh.state_dict(gen2), sd)
    assert torch.equal(torch.rand(7, generator=gen2), torch.rand(7, generator=gen))
    if which == "single":
        assert fresh.history[1] == (1, -1.25, 0.125, -0.02) and fresh.scores[0] == -INF
    else:
        assert fresh.exploits[0]["mutations"][1] == ("num_sgd_iter", "resample", 10, 20) and fresh.reslices[0] == (0, [16, 48])


@pytest.mark.parametrize("which", ["single", "pbt"])
def test_loop_state_refuses_a_bad_section_and_stays_as_it_was(which, single, pbt):
    mod, make, keys = (single, _single_record, SINGLE_KEYS) if which == "single" else (pbt, _pbt_record, PBT_KEYS)
    good = make(mod).state_dict(_gen())
    rec, gen = _fresh(mod, which), _gen(1)
    before, gen_before = rec.state_dict(gen), gen.get_state().clone()
    missing = [(key, {k: v for k, v in good.items() if k != key}) for key in sorted(keys)]
    wrong = {"update": "3", "history": 3, "best": "high", "gen_state": [1, 2], "best_update": 1.5, "scores": None}
    for key, sd in missing + [(k, dict(good, **{k: v})) for k, v in wrong.items()]:
        with pytest.raises(ValueError, match=key):
            rec.load_state_dict(sd, gen)
        assert _same(rec.state_dict(gen), before) and torch.equal(gen.get_state(), gen_before)


# ------------------------------------------------------------------------------------------------------------------------------------
# the requirements table of train/ppo_torch.py, row by row, from both sides
# ------------------------------------------------------------------------------------------------------------------------------------
# how a row is switched on, and how a need is met: (train() arguments, command line); a need that is not met is the default
ROW_ON = {"save_obs_filter": (dict(save_obs_filter="f.pt"), ["--save-obs-filter", "f.pt"]), "obs_filter": (dict(obs_filter=True), ["--obs-filter"]),
          "norm_reward": (dict(norm_reward=True), ["--norm-reward"]), "timeout_bootstrap": (dict(timeout_bootstrap=True), ["--timeout-bootstrap"]),
          "eval_every": (dict(eval_every=1), ["--eval-every", "1"]), "perm": (dict(perm="native"), ["--perm", "native"]),
          "resume": (dict(resume="/nonexistent/x.ckpt"), ["--resume", "/nonexistent/x.ckpt"]), "save_every": (dict(save_every=2), ["--save-every", "2"]),
          "adv_norm": (dict(adv_norm="minibatch"), ["--adv-norm", "minibatch"]), "update": (dict(update="native"), ["--update", "native"]),
          "ranks": (dict(), ["--gpus", "2"])}
NEED_MET = {"mode": (dict(mode="native"), ["--mode", "native"]), "update": (dict(update="native"), ["--update", "native"]),
            "obs_filter": (dict(obs_filter=True), ["--obs-filter"]), "save": (dict(save="x.ckpt"), ["--save", "x.ckpt"])}
# the arguments of train() that had a refusal of their own before there was a table, and the flags refused with more than one rank
REFUSING = {"update", "perm", "eval_every", "obs_filter", "save_obs_filter", "norm_reward", "timeout_bootstrap", "save_every", "resume", "adv_norm"}
ONE_RANK_ONLY = ["resume", "save_every", "obs_filter", "save_obs_filter", "norm_reward", "adv_norm"]


def _no_env(*a, **k):
    pytest.fail("an env was built before the refusal")


def _rows(mod):
    return [dict(zip(("name", "flag", "on", "needs", "one_rank_only", "why"), row)) for row in mod.REQUIREMENTS]


def test_the_table_covers_every_argument_with_a_refusal(single):
    import inspect
    rows = _rows(single)
    names = [r["name"] for r in rows]
    assert REFUSING <= set(names) and len(set(names)) == len(names) and set(names) == set(ROW_ON)
    params = inspect.signature(single.train).parameters
    assert all(n in params for n in names if n != "ranks")
    assert all(set(r["needs"]) <= set(single.NEEDS) and set(r["needs"]) <= set(NEED_MET) and r["why"] for r in rows)
    assert sorted(r["name"] for r in rows if r["one_rank_only"]) == sorted(ONE_RANK_ONLY)


def _cases():
    mod = load_script("train/ppo_torch.py")
    return [(r["name"], r["flag"], r["needs"], missing) for r in _rows(mod) for missing in r["needs"]]


@pytest.mark.parametrize("name,flag,needs,missing", _cases(), ids=["%s-without-%s" % (c[0], c[3]) for c in _cases()])
def test_a_row_whose_need_fails_is_refused_on_both_sides(name, flag, needs, missing, single, capsys, monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(single, "ShipVecEnv", _no_env)
    kw, argv = dict(ROW_ON[name][0]), list(ROW_ON[name][1])
    for need in needs:
        if need != missing:
            kw.update(NEED_MET[need][0])
            argv += NEED_MET[need][1]
    with pytest.raises(SystemExit) as ex:
        single.parse_args(argv)
    assert ex.value.code not in (0, None)
    err = capsys.readouterr().err
    assert flag in err and single.NEEDS[missing][0] in err, err
    if name == "ranks":
        monkeypatch.setattr(single, "job_ranks", lambda: (1, 2))
    with pytest.raises(ValueError, match=name) as ex:
        single.train(envs=8, updates=1, log=None, **kw)
    assert single.NEEDS[missing][1] in str(ex.value)


@pytest.mark.parametrize("name", ONE_RANK_ONLY)
def test_a_row_marked_multi_rank_is_refused_with_two_ranks(name, single, capsys, monkeypatch):
    row = [r for r in _rows(single) if r["name"] == name][0]
    kw, argv = dict(ROW_ON[name][0], mode="native", update="native"), ["--mode", "native", "--update", "native"] + ROW_ON[name][1]
    for need in row["needs"]:
        if need not in ("mode", "update"):
            kw.update(NEED_MET[need][0])
            argv += NEED_MET[need][1]
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert getattr(single.parse_args(argv), name) == kw[name]  # (one rank: fine)
    for extra, world in ((["--gpus", "2"], None), ([], "2")):
        if world:
            monkeypatch.setenv("WORLD_SIZE", world)
        with pytest.raises(SystemExit) as ex:
            single.parse_args(argv + extra)
        assert ex.value.code not in (0, None)
        err = capsys.readouterr().err
        assert row["flag"] in err and "more than one rank" in err, err
    monkeypatch.setattr(single, "ShipVecEnv", _no_env)
    monkeypatch.setattr(single, "job_ranks", lambda: (1, 2))
    with pytest.raises(ValueError, match=name) as ex:
        single.train(envs=8, updates=1, log=None, **kw)
    assert "more than one rank" in str(ex.value)


# ------------------------------------------------------------------------------------------------------------------------------------
# torch_update on the CPU
# ------------------------------------------------------------------------------------------------------------------------------------
def _rollout(horizon, envs, D=7, seed=0):
    g = torch.Generator()
    g.manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    b = {"obs": r(horizon, envs, D), "act": torch.randint(0, 3, (horizon, envs), generator=g), "logp": -r(horizon, envs) - 0.5,
         "val": r(horizon, envs) - 0.5, "rew": r(horizon, envs) - 0.5, "done": (r(horizon, envs) < 0.3).float()}
    return b, r(envs) - 0.5


def _net(mod, seed=1):
    torch.manual_seed(seed)
    net = mod.ActorCritic(7, 3, hidden=16)
    return net, torch.optim.Adam(net.parameters(), lr=3e-4)


@pytest.mark.parametrize("adv_norm", ["batch", "minibatch"])
def test_torch_update_with_one_sample_minibatches(adv_norm, single):
    """Horizon 2 x 3 envs in 6 minibatches: every minibatch is one sample, whose own std is taken as 0, not NaN."""
    b, last_val = _rollout(2, 3)
    net, opt = _net(single)
    start = [p.detach().clone() for p in net.parameters()]
    gen, twin = torch.Generator(), torch.Generator()
    gen.manual_seed(5)
    twin.manual_seed(5)
    single.torch_update(net, opt, b, last_val, 2, 6, gen, adv_norm=adv_norm)
    assert all(torch.isfinite(p).all() for p in net.parameters())
    assert any(not torch.equal(p, q) for p, q in zip(net.parameters(), start))
    for _ in range(2):  # exactly one randperm(6) per epoch, and nothing else
        torch.randperm(6, generator=twin)
    assert torch.equal(gen.get_state(), twin.get_state())


def test_torch_update_is_deterministic(single):
    b, last_val = _rollout(2, 4)
    out = []
    for _ in range(2):
        net, opt = _net(single)
        gen = torch.Generator()
        gen.manual_seed(5)
        single.torch_update(net, opt, b, last_val, 2, 2, gen, adv_norm="batch")
        out.append([p.detach().clone() for p in net.parameters()])
    assert all(torch.equal(p, q) for p, q in zip(*out)) and all(torch.isfinite(p).all() for p in out[0])


# ------------------------------------------------------------------------------------------------------------------------------------
# train/pbt_native.py: the layout and the schedule, on the host
# ------------------------------------------------------------------------------------------------------------------------------------
class _Env(object):
    """Records what is bound."""

    def __init__(self):
        self.bound = []

    def set_population_slices(self, sizes):
        self.bound.append(list(sizes))


def _run(env):
    return argparse.Namespace(env=env, n_total=64, quantum=16, horizon=8)


def test_layout_start_up_reslice_and_resume_go_through_one_function(pbt):
    from ship_sim_gym_amd.population import slices_for_batch_sizes
    lines = []
    env = _Env()
    run, st = _run(env), _fresh(pbt, "pbt")
    pbt.bind_layout(run, st, lines.append, 0, [10000, 40000])  # start-up
    assert st.slices == slices_for_batch_sizes([10000, 40000], 64, 16) == [16, 48]
    assert env.bound == [[16, 48]] and st.member_samples == [128, 384] and st.reslices == [(0, [16, 48])] and st.batch_sizes == [10000, 40000]
    assert len(lines) == 1 and "[16, 48]" in lines[0] and "quantum 16" in lines[0]
    pbt.bind_layout(run, st, lines.append, 4, [40000, 10000])  # after a perturbation
    assert st.slices == [48, 16] and env.bound[-1] == [48, 16] and st.member_samples == [384, 128]
    assert st.reslices == [(0, [16, 48]), (4, [48, 16])] and len(lines) == 2 and lines[1].startswith("update 4  re-slice")
    # a resumed run: the start-up layout is bound first, then the saved one, which is not logged again
    saved = st.state_dict(_gen())
    env2 = _Env()
    run2, st2 = _run(env2), _fresh(pbt, "pbt")
    pbt.bind_layout(run2, st2, lines.append, 0, [10000, 40000])
    st2.load_state_dict(saved, torch.Generator())
    pbt.bind_layout(run2, st2, lines.append)
    assert env2.bound == [[16, 48], [48, 16]] and st2.slices == [48, 16] and st2.member_samples == [384, 128]
    assert st2.reslices == st.reslices and st2.batch_sizes == [40000, 10000] and len(lines) == 3


def test_schedule_follows_the_members_own_samples(pbt):
    from ship_sim_gym_amd.ppo import chunk_split
    st = _fresh(pbt, "pbt")
    pbt.bind_layout(_run(_Env()), st, lambda *a: None, 0, [10000, 40000])
    assert st.member_samples == [128, 384]  # 16 / 48 envs at horizon 8
    raw = [(30, 2048), (0, 64)]
    pbt.set_schedule(st, 20, raw=raw)
    used = [pbt.clamp_schedule(i, s, n, 20) for (i, s), n in zip(raw, st.member_samples)]
    assert (st.iters, st.sizes) == ([u[0] for u in used], [u[1] for u in used]) == ([20, 1], [128, 128]) and st.counts == []
    pbt.set_schedule(st, 20, iters=[2, 3], counts=[4, 5])
    assert (st.iters, st.counts) == ([2, 3], [4, 5])
    assert st.sizes == [chunk_split(128, 4)[0], chunk_split(384, 5)[0]] and st.sizes[0] != st.sizes[1]
