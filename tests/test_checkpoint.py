"""Checkpoints, the host side: PBTScheduler's state, the file format and its atomic write, the trainers' flags and the configuration
check of a resumed run.  Nothing here needs a device."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(rel):
    from gpu_support import load_script
    return load_script(rel)


# ------------------------------------------------------------------------------------------------------------------------------------
# PBTScheduler
# ------------------------------------------------------------------------------------------------------------------------------------
def _hparams(P):
    return {"lambda": [0.9 + 0.01 * m for m in range(P)], "clip_param": [0.1 + 0.02 * m for m in range(P)],
            "lr": [[1e-3, 5e-4, 1e-4, 5e-5, 1e-5][m % 5] for m in range(P)], "num_sgd_iter": [10 + m for m in range(P)],
            "sgd_minibatch_size": [128 * (m + 1) for m in range(P)], "train_batch_size": [10000 + 1000 * m for m in range(P)]}


def _scores(P, k):
    return [((7 * m + 3 * k) % P) + 0.25 * k for m in range(P)]


def _plain_only(obj):
    import torch
    if isinstance(obj, dict):
        return all(isinstance(k, str) and _plain_only(v) for k, v in obj.items())
    if isinstance(obj, list):
        return all(_plain_only(v) for v in obj)
    return isinstance(obj, (bool, int, float, str)) or torch.is_tensor(obj)


def test_scheduler_round_trip_continues_the_originals_perturbations():
    from ship_sim_gym_amd.population import PBTScheduler, reference_mutations
    P = 8
    kw = dict(seed=11, perturbation_interval=2, quantile_fraction=0.25, resample_probability=0.33,
              mutations=reference_mutations(schedule=True, batch=True))
    a = PBTScheduler(P, **kw)
    hp = _hparams(P)
    for k in range(2):
        _, hp, _ = a.perturb(_scores(P, k), hp)
    sd = a.state_dict()
    assert _plain_only(sd) and sd["rng"]["gauss_next"] == []
    b = PBTScheduler(P, **dict(kw, seed=999))  # (another seed: the state must replace the generator's)
    assert b.load_state_dict(sd) is b
    hp_a, hp_b = hp, {k: list(v) for k, v in hp.items()}
    for k in range(2, 5):
        src_a, hp_a, ev_a = a.perturb(_scores(P, k), hp_a)
        src_b, hp_b, ev_b = b.perturb(_scores(P, k), hp_b)
        assert src_a == src_b and hp_a == hp_b and ev_a == ev_b
        assert ev_a and all(ev["mutations"] for ev in ev_a)  # (the comparison saw exploits and mutations)
    assert a.due(4) == b.due(4) is True and a.due(3) == b.due(3) is False


def test_scheduler_round_trip_through_a_file(tmp_path):
    import torch
    from ship_sim_gym_amd.population import PBTScheduler
    a = PBTScheduler(4, seed=3)
    a.rng.gauss(0.0, 1.0)  # (leaves a pending second normal in the generator: gauss_next is part of its state)
    path = str(tmp_path / "sched.pt")
    torch.save(a.state_dict(), path)
    b = PBTScheduler(4, seed=4).load_state_dict(torch.load(path, weights_only=True))
    assert a.rng.getstate() == b.rng.getstate()
    assert [a.rng.gauss(0.0, 1.0) for _ in range(3)] == [b.rng.gauss(0.0, 1.0) for _ in range(3)]


@pytest.mark.parametrize("change, field", [
    (dict(n_members=5), "n_members"), (dict(perturbation_interval=3), "perturbation_interval"),
    (dict(quantile_fraction=0.5), "quantile_fraction"), (dict(resample_probability=0.5), "resample_probability"),
    (dict(mutations={"lr": [1e-3, 1e-4]}), "mutations")])
def test_scheduler_refuses_a_state_of_other_arguments_and_stays_as_it_was(change, field):
    from ship_sim_gym_amd.population import PBTScheduler
    kw = dict(n_members=4, seed=1, perturbation_interval=2, quantile_fraction=0.25, resample_probability=0.33)
    sd = PBTScheduler(**dict(kw, **change)).state_dict()
    b = PBTScheduler(**kw)
    before = b.rng.getstate()
    with pytest.raises(ValueError, match=field):
        b.load_state_dict(sd)
    assert b.rng.getstate() == before
    bad = PBTScheduler(**kw).state_dict()
    bad["rng"]["state"] = bad["rng"]["state"][:10]
    with pytest.raises(ValueError, match="rng"):
        b.load_state_dict(bad)
    assert b.rng.getstate() == before


def test_scheduler_state_needs_no_torch():
    """The module still imports, and the scheduler still saves and loads, in an interpreter where torch cannot be imported."""
    code = ("import sys; sys.modules['torch'] = None\n"
            "from ship_sim_gym_amd.population import PBTScheduler\n"
            "a = PBTScheduler(4, seed=2); sd = a.state_dict(); b = PBTScheduler(4, seed=5).load_state_dict(sd)\n"
            "assert a.rng.random() == b.rng.random()\n"
            "assert 'torch' not in [m for m in sys.modules if sys.modules[m] is not None]\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ------------------------------------------------------------------------------------------------------------------------------------
# the file
# ------------------------------------------------------------------------------------------------------------------------------------
def _sections():
    import torch
    return {"policy": {"obs_dim": 20, "hidden": 16, "params": torch.arange(12, dtype=torch.float32), "activation": "tanh", "separate_value": True},
            "loop": {"update": 3, "history": [[0, -1.5, 0.25, 0.0], [1, float("-inf"), 0.5, 0.125]], "best": float("-inf"),
                     "gen_state": torch.arange(16, dtype=torch.uint8)},
            "config": {"horizon": 8, "perm": "native", "obs_filter": True, "env_kw": {"n_beams": 4}}}


def _same(a, b):
    import torch
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_save_then_load_with_weights_only(tmp_path):
    import torch
    from ship_sim_gym_amd import checkpoint
    path = str(tmp_path / "run.ckpt")
    sections = _sections()
    assert checkpoint.save(path, sections) == path
    assert not os.path.exists(path + ".tmp")
    raw = torch.load(path, map_location="cpu", weights_only=True)  # (no class in the file: the restricted unpickler reads it)
    assert raw["format"] == "ssg-checkpoint" and raw["version"] == 1
    got = checkpoint.load(path, require=("policy", "loop", "config"))
    assert checkpoint.is_checkpoint(got)
    assert _same({k: got[k] for k in sections}, sections)


def test_save_refuses_what_a_file_may_not_hold(tmp_path):
    from ship_sim_gym_amd import checkpoint
    path = str(tmp_path / "run.ckpt")
    with pytest.raises(TypeError, match=r"loop.*history.*tuple"):
        checkpoint.save(path, dict(_sections(), loop={"history": [(0, 1.0)]}))
    with pytest.raises(TypeError, match="NoneType"):
        checkpoint.save(path, dict(_sections(), loop={"best": None}))
    with pytest.raises(ValueError, match="optimizer"):
        checkpoint.save(path, dict(_sections(), optimizer={}))
    with pytest.raises(ValueError, match="policy.*population"):
        checkpoint.save(path, {"loop": {}})
    with pytest.raises(ValueError, match="policy.*population"):
        checkpoint.save(path, dict(_sections(), population={}))
    assert not os.path.exists(path) and not os.path.exists(path + ".tmp")


def test_load_refuses_by_name(tmp_path):
    import torch
    from ship_sim_gym_amd import checkpoint
    path = str(tmp_path / "run.ckpt")
    torch.save(dict(_sections(), format="something-else", version=1), path)
    with pytest.raises(ValueError, match="something-else"):
        checkpoint.load(path)
    torch.save(dict(_sections(), format="ssg-checkpoint", version=2), path)
    with pytest.raises(ValueError, match="version 2"):
        checkpoint.load(path)
    torch.save({"body.0.weight": torch.zeros(2, 2)}, path)  # (a module's state_dict)
    with pytest.raises(ValueError, match="format"):
        checkpoint.load(path)
    assert not checkpoint.is_checkpoint(checkpoint.read(path))
    checkpoint.save(path, _sections())
    with pytest.raises(ValueError, match="'trainer'"):
        checkpoint.load(path, require=("policy", "trainer"))
    with pytest.raises(ValueError, match="'env'"):
        checkpoint.load(path, require=("env",))


def test_a_failed_save_leaves_the_previous_file_whole(tmp_path, monkeypatch):
    import torch
    from ship_sim_gym_amd import checkpoint
    path = str(tmp_path / "run.ckpt")
    checkpoint.save(path, _sections())
    before = open(path, "rb").read()

    def dies(obj, f, *a, **k):
        with open(f, "wb") as fh:  # (killed half way through the write)
            fh.write(b"half a file")
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", dies)
    with pytest.raises(OSError, match="disk full"):
        checkpoint.save(path, dict(_sections(), loop={"update": 4}))
    assert open(path, "rb").read() == before
    assert not os.path.exists(path + ".tmp")
    monkeypatch.undo()
    assert checkpoint.load(path)["loop"]["update"] == 3


def test_config_sections():
    from ship_sim_gym_amd import checkpoint
    c = checkpoint.plain_config(dict(envs=320, lr=3e-4, perm="native", env_kw={"n_beams": 4}, lrs=None, epochs=(1, 2), obs_filter=True))
    assert c == {"envs": 320, "lr": 3e-4, "perm": "native", "env_kw": {"n_beams": 4}, "lrs": "None", "epochs": [1, 2], "obs_filter": True}
    checkpoint.check_plain(c)
    other = dict(c, envs=640, perm="torch", extra=1)
    assert checkpoint.config_differences(c, other) == ["envs", "extra", "perm"]
    assert checkpoint.config_differences(c, other, exempt=("envs", "extra")) == ["perm"]
    assert checkpoint.config_differences(c, dict(c)) == []


# ------------------------------------------------------------------------------------------------------------------------------------
# the trainers' flags
# ------------------------------------------------------------------------------------------------------------------------------------
def test_both_trainers_and_the_evaluation_parse_the_new_flags(capsys):
    single, pbt, ev = _script("train/ppo_torch.py"), _script("train/pbt_native.py"), _script("train/evaluate_native.py")
    a = single.parse_args(["--mode", "native", "--update", "native", "--save", "a.ckpt", "--save-every", "5", "--save-best", "b.ckpt",
                           "--resume", "a.ckpt", "--hidden", "16"])
    assert (a.save, a.save_every, a.save_best, a.resume, a.hidden) == ("a.ckpt", 5, "b.ckpt", "a.ckpt", 16)
    a = single.parse_args([])
    assert (a.save, a.save_every, a.save_best, a.resume, a.hidden) == (None, 0, None, None, 64)
    assert single.parse_args(["--mode", "graph", "--save", "a.ckpt"]).save == "a.ckpt"  # (saving the policy works in every mode)
    p = pbt.parse_args(["--save", "a.ckpt", "--save-every", "2", "--save-best", "b.ckpt", "--resume", "a.ckpt"])
    assert (p.save, p.save_every, p.save_best, p.resume) == ("a.ckpt", 2, "b.ckpt", "a.ckpt")
    p = pbt.parse_args([])
    assert (p.save, p.save_every, p.save_best, p.resume, p.hidden) == (None, 0, None, None, 64)
    e = ev.parse_args(["--checkpoint", "a.ckpt", "--member", "2"])
    assert (e.checkpoint, e.member) == ("a.ckpt", 2) and ev.parse_args([]).member is None
    for mod, argv, word in ((single, ["--mode", "graph", "--resume", "a.ckpt"], "--resume"),
                            (single, ["--mode", "native", "--update", "torch", "--resume", "a.ckpt"], "--resume"),
                            (single, ["--save-every", "2"], "--save-every"), (pbt, ["--save-every", "2"], "--save-every"),
                            (single, ["--save", "a", "--save-every", "-1"], "--save-every")):
        with pytest.raises(SystemExit):
            mod.parse_args(argv)
        assert word in capsys.readouterr().err


def test_train_refuses_resume_outside_the_device_update_before_it_reads_anything():
    single = _script("train/ppo_torch.py")
    for kw in (dict(mode="graph"), dict(mode="native", update="torch")):
        with pytest.raises(ValueError, match="resume"):
            single.train(resume="/nonexistent/file.ckpt", **kw)
    with pytest.raises(ValueError, match="save_every"):
        single.train(save_every=2)


def test_a_config_that_differs_is_refused_with_every_key_named(tmp_path):
    """Checked on the host, before any device work: the files are hand-built around each script's own run_config."""
    from ship_sim_gym_amd import checkpoint
    single, pbt = _script("train/ppo_torch.py"), _script("train/pbt_native.py")
    path = str(tmp_path / "single.ckpt")
    kw = dict(envs=320, horizon=8, mode="native", update="native", obs_filter=True)
    config = single.run_config(**kw)
    assert "horizon" in config and not set(config) & set(single.CONFIG_EXEMPT)
    full = {"policy": {}, "trainer": {}, "env": {}, "obs_filter": {}, "loop": {}, "config": config}
    checkpoint.save(path, full)
    with pytest.raises(ValueError, match=r"horizon \(the file has 8, this run 16\)") as ex:
        single.train(resume=path, **dict(kw, horizon=16, seed=5, updates=50, save="elsewhere.ckpt", eval_every=3, log=None))
    assert "seed (the file has 0, this run 5)" in str(ex.value)
    assert "updates (" not in str(ex.value) and "save (" not in str(ex.value) and "eval_every (" not in str(ex.value)
    checkpoint.save(path, {k: v for k, v in full.items() if k != "trainer"})  # (what --save writes without the device update)
    with pytest.raises(ValueError, match="no trainer section"):
        single.train(resume=path, **kw)
    checkpoint.save(path, {k: v for k, v in full.items() if k != "obs_filter"})
    with pytest.raises(ValueError, match="'obs_filter'"):
        single.train(resume=path, **kw)
    with pytest.raises(TypeError, match="no_such_argument"):
        single.run_config(no_such_argument=1)
    # the population trainer
    path = str(tmp_path / "pbt.ckpt")
    kw = dict(members=4, envs_per_member=64, horizon=8, perturb_every=2, mutate_schedule=True)
    checkpoint.save(path, {"population": {}, "trainer": {}, "env": {}, "scheduler": {}, "loop": {}, "config": pbt.run_config(**kw)})
    with pytest.raises(ValueError, match=r"horizon \(the file has 8, this run 4\)") as ex:
        pbt.train(resume=path, **dict(kw, horizon=4, perturb_every=3, updates=99))
    assert "perturb_every (the file has 2, this run 3)" in str(ex.value) and "updates (" not in str(ex.value)


def test_pbt_events_survive_the_file_form():
    pbt = _script("train/pbt_native.py")
    events = [{"member": 0, "source": 3, "mutations": [("lr", "perturb", 1e-3, 5e-4), ("num_sgd_iter", "resample", 10, 17)],
               "schedule": {"num_sgd_iter": 17, "sgd_minibatch_size": 128}}]
    from ship_sim_gym_amd import checkpoint
    plain = pbt.plain_events(events)
    checkpoint.check_plain(plain)
    assert pbt.events_from_plain(plain) == events and events[0]["mutations"][0] == ("lr", "perturb", 1e-3, 5e-4)
