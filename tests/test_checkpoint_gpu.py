"""Checkpoints on the device: a run that is saved, interrupted and resumed is bit for bit the run that was not.

Every comparison is torch.equal, or == on Python values: the claims follow from contracts the library already documents (the same
launches on the same inputs), so there is no tolerance anywhere.  All runs use hidden 16, 4 beams and history 2 (D = 20) and a step
limit of 11, so that resets, time-outs and the filters' per-env carries cross every save point: few episodes end early here, so the
envs time out together, and a limit that divides a save point's step count (8 steps per update) would put every save on an episode
boundary, where the carries are zero."""
import pytest

from gpu_support import DEV, env_config, load_script, torch_cuda  # noqa: F401
from ppo_reference import split_policy

pytestmark = pytest.mark.gpu

BEAMS, D, HIDDEN, MAX_STEPS = 4, 20, 16, 11  # (11: no save point, at 24 or 32 steps, falls on the common time-out)
QUIET = lambda *a, **k: None  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def short_episodes():
    """MAX_STEPS = 11 for every env of this module, the trainers' and the evaluation script's included (they read the config class)."""
    from ship_sim_gym_amd.config import EnvConfig
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(EnvConfig, "MAX_STEPS", MAX_STEPS)
        yield


def _env(n, history=2, **kw):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    kw.setdefault("n_beams", BEAMS)
    env = ShipVecEnv(n, n_maps=8, env_config=env_config(history), **kw)
    assert env.cfg.max_steps == MAX_STEPS
    return env


def _same(a, b):
    """Equality of plain data down to the bits: tensors by dtype and torch.equal, floats by ==, containers by structure."""
    import torch
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the env
# ------------------------------------------------------------------------------------------------------------------------------------
def _steps(env, acts, k0, k1):
    """Steps k0 .. k1-1 of the action rows: every step's (obs, reward, done, flags), the blob afterwards and the counters."""
    rows = []
    for k in range(k0, k1):
        env.step_tensor(acts[k])
        rows.append(tuple(t.clone() for t in (env.obs, env.reward, env.done, env.flags)))
    return rows, env.state.clone(), env.stats()


def test_env_snapshot_restores_in_place_and_into_a_fresh_env(torch_cuda, tmp_path):
    torch = torch_cuda
    from ship_sim_gym_amd import checkpoint
    env = _env(192)  # (three waves)
    env.reset_tensor()
    acts = env.random_actions(77, 0, 30)
    _steps(env, acts, 0, 10)
    snap = env.snapshot()
    checkpoint.check_plain(snap)
    assert snap["n_maps"] == 8 and snap["fingerprint"]["max_steps"] == MAX_STEPS and all(t.device.type == "cpu" for t in snap.values() if torch.is_tensor(t))
    path = str(tmp_path / "env.pt")
    torch.save(snap, path)
    snap = torch.load(path, weights_only=True)  # (through a file, read without trusting it)
    want_rows, want_blob, want_stats = _steps(env, acts, 10, 30)
    assert sum(int(r[2].sum()) for r in want_rows) > 192 and want_stats["episodes"] > 192  # (episodes ended on both sides of the save)
    assert not torch.equal(env.state.cpu(), snap["state"])
    ptrs = (env.state.data_ptr(), env.obs.data_ptr(), env.bank.data_ptr())
    assert env.restore(snap) is env
    assert ptrs == (env.state.data_ptr(), env.obs.data_ptr(), env.bank.data_ptr())  # (in place: handed-out tensors stay valid)
    assert torch.equal(env.state.cpu(), snap["state"]) and torch.equal(env._out_blob.cpu(), snap["out"])
    rows, blob, stats = _steps(env, acts, 10, 30)
    assert _same(rows, want_rows) and torch.equal(blob, want_blob) and stats == want_stats
    fresh = _env(192)  # (never reset: restore runs the handle's first full reset itself)
    fresh.restore(snap)
    rows, blob, stats = _steps(fresh, acts, 10, 30)
    assert _same(rows, want_rows) and torch.equal(blob, want_blob) and stats == want_stats
    for e in (env, fresh):  # a later full reset keeps the restored counters, as it keeps the original's
        e.reset_tensor()
    assert fresh.stats() == env.stats() and fresh.stats()["episodes"] >= want_stats["episodes"] and torch.equal(fresh.state, env.state)
    fresh.close()
    # another fingerprint: refused, nothing changes
    small = _env(128)
    small.reset_tensor()
    blob, out = small.state.clone(), small._out_blob.clone()
    with pytest.raises(ValueError, match=r"num_envs is 192 in the snapshot and 128 in this env"):
        small.restore(snap)
    with pytest.raises(ValueError, match="fingerprint"):
        small.restore({"state": snap["state"]})
    assert torch.equal(small.state, blob) and torch.equal(small._out_blob, out)
    small.close()
    other = _env(192, env_id_base=192)
    other.reset_tensor()
    blob = other.state.clone()
    with pytest.raises(ValueError, match="env_id_base"):
        other.restore(snap)
    assert torch.equal(other.state, blob)
    other.close()
    env.close()


@pytest.mark.parametrize("kind", ["n_ships", "fresh_device", "history"])
def test_env_snapshot_refuses_handles_with_host_state(torch_cuda, kind):
    torch = torch_cuda
    env = {"n_ships": lambda: _env(64, n_ships=4, n_beams=None), "fresh_device": lambda: _env(64, map_mode="fresh_device", ring=4),
           "history": lambda: _env(64, history=3)}[kind]()
    env.reset_tensor()
    blob, out = env.state.clone(), env._out_blob.clone()
    with pytest.raises(NotImplementedError, match=kind if kind != "history" else "history = 3"):
        env.snapshot()
    with pytest.raises(NotImplementedError):
        env.restore({"fingerprint": env.fingerprint()})
    torch.cuda.synchronize()
    assert torch.equal(env.state, blob) and torch.equal(env._out_blob, out)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. one trainer object
# ------------------------------------------------------------------------------------------------------------------------------------
def test_policy_and_trainer_rebuilt_from_their_state_continue_bit_for_bit(torch_cuda, tmp_path):
    torch = torch_cuda
    from ship_sim_gym_amd import checkpoint
    from ship_sim_gym_amd.policy import NativePolicy
    from ship_sim_gym_amd.ppo import NativePPO
    n, K = 320, 8  # (one GAE block of 256 envs plus a tail)
    env = _env(n)
    env.reset_tensor()
    net, pol = split_policy(torch, D, H=HIDDEN)
    kw = dict(vf_clip=0.2, max_grad_norm=0.5, kl_coef=1.0, kl_target=0.01, adv_norm="minibatch", perm_seed=7)
    ppo = NativePPO(pol, env, lr=1e-3, clip=0.15, **kw)
    for u in range(2):
        batch = env.rollout_policy(pol, K, seed=21, step0=K * u)
        ppo.gae(batch, 0.98, 0.9)
        ppo.update(batch, None, 2, 2)
    path = str(tmp_path / "pair.ckpt")
    checkpoint.save(path, {"policy": pol.state_dict(), "trainer": ppo.state_dict()})
    ckpt = checkpoint.load(path, require=("policy", "trainer"))
    assert ckpt["trainer"]["step"] == 8 and ckpt["trainer"]["updates"] == 2 and ckpt["trainer"]["hp"]["lr"] == 1e-3
    pol2 = NativePolicy.from_state_dict(ckpt["policy"], DEV)  # (no module)
    assert pol2.separate_value and pol2.hidden == HIDDEN and torch.equal(pol2.params, pol.params) and torch.equal(pol2.obs_scale, pol.obs_scale)
    ppo2 = NativePPO(pol2, env, adv_norm="minibatch").load_state_dict(ckpt["trainer"])  # (every other setting comes from the state)
    assert _same(ppo2.state_dict(), ppo.state_dict()) and ppo2.workspace.numel() == 0
    batch = env.rollout_policy(pol, K, seed=21, step0=2 * K)
    twin = {k: v.clone() for k, v in batch.items()}
    assert torch.equal(ppo.draw_perm(K * n, 2), ppo2.draw_perm(K * n, 2))
    for p, b in ((ppo, batch), (ppo2, twin)):
        p.gae(b, 0.98, 0.9)
        p.update(b, None, 2, 2)
    torch.cuda.synchronize()
    assert torch.equal(pol2.params, pol.params) and torch.equal(ppo2.adam_mv, ppo.adam_mv) and torch.equal(ppo2.kl_coef, ppo.kl_coef)
    assert (ppo2.step, ppo2.updates) == (ppo.step, ppo.updates) == (12, 3)
    assert bool(torch.isfinite(pol.params).all())
    assert torch.equal(ppo.draw_perm(K * n, 2), ppo2.draw_perm(K * n, 2))
    # a policy over a module: loading reaches the module too, so refresh() re-packs what was loaded
    net3, pol3 = split_policy(torch, D, H=HIDDEN, seed=5)
    pol3.load_state_dict(pol.state_dict())
    assert torch.equal(pol3.refresh(), pol.params) and torch.equal(net3.v.bias, pol.unpack()["bv"])
    # refusals: the field by name, and the object as it was
    _, big = split_policy(torch, D, H=32)
    before = pol.params.clone()
    with pytest.raises(ValueError, match=r"hidden is 32 in the state and 16 in this object"):
        pol.load_state_dict(big.state_dict())
    assert torch.equal(pol.params, before)
    plain = NativePPO(pol2, env)  # adv_norm="batch"
    with pytest.raises(ValueError, match=r"adv_norm is 'minibatch' in the state and 'batch' in this object"):
        plain.load_state_dict(ppo.state_dict())
    with pytest.raises(ValueError, match="adam_mv"):
        ppo.load_state_dict(NativePPO(big, env, adv_norm="minibatch").state_dict())
    with pytest.raises(ValueError, match="step is a str"):
        ppo.load_state_dict(dict(ppo.state_dict(), step="12"))
    assert (plain.step, plain.updates, ppo.step, ppo.updates) == (0, 0, 12, 3) and torch.equal(ppo.adam_mv, ppo2.adam_mv)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. ppo_torch.train, 5. evaluation, 6. --save-best
# ------------------------------------------------------------------------------------------------------------------------------------
SINGLE = dict(envs=320, horizon=8, mode="native", update="native", obs_filter=True, norm_reward=True, timeout_bootstrap=True, hidden=HIDDEN,
              separate_value=True, env_kw={"n_beams": BEAMS}, seed=3, return_details=True, log=QUIET)
_single_runs = {}


def _single(tmp_path_factory, perm):
    """Six uninterrupted updates (saving the best on the way and the last), and three updates saved then resumed to six."""
    if perm not in _single_runs:
        mod = load_script("train/ppo_torch.py")
        d = tmp_path_factory.mktemp("single_" + perm)
        paths = {k: str(d / (k + ".ckpt")) for k in ("full", "best", "half")}
        kw = dict(SINGLE, perm=perm)
        full = mod.train(updates=6, save=paths["full"], save_best=paths["best"], **kw)
        half = mod.train(updates=3, save=paths["half"], **kw)
        resumed = mod.train(updates=6, resume=paths["half"], **kw)
        _single_runs[perm] = {"mod": mod, "kw": kw, "paths": paths, "full": full, "half": half, "resumed": resumed}
    return _single_runs[perm]


@pytest.mark.parametrize("perm", ["native", "torch"])
def test_single_trainer_resumed_is_the_uninterrupted_run(torch_cuda, tmp_path_factory, perm):
    torch = torch_cuda
    from ship_sim_gym_amd import checkpoint
    run = _single(tmp_path_factory, perm)
    (h_full, d_full), (h_half, _), (h_res, d_res) = run["full"], run["half"], run["resumed"]
    assert len(h_full) == 6 and h_half == h_full[:3] and h_res == h_full  # (every history row)
    assert len(d_full["params"]) == len(d_res["params"]) and all(torch.equal(a, b) for a, b in zip(d_full["params"], d_res["params"]))
    assert _same(d_res["obs_filter"], d_full["obs_filter"]) and _same(d_res["ret_filter"], d_full["ret_filter"])
    assert torch.equal(d_res["env_state"], d_full["env_state"])
    assert d_res["episode_reward_mean"] == d_full["episode_reward_mean"] and (d_res["best"], d_res["best_update"]) == (d_full["best"], d_full["best_update"])
    # the run crossed what it was meant to cross: episodes and time-outs on both sides of the save, filters that kept merging
    half, full = checkpoint.load(run["paths"]["half"]), checkpoint.load(run["paths"]["full"])
    assert half["loop"]["update"] == 2 and full["loop"]["update"] == 5 and 0 < half["loop"]["episodes"] < full["loop"]["episodes"]
    assert float(half["ret_filter"]["carry"].abs().sum()) > 0 and half["trainer"]["updates"] == 3 and full["trainer"]["updates"] == 6
    assert 0 < float(half["obs_filter"]["state"][0, 3, 0]) < float(full["obs_filter"]["state"][0, 3, 0])
    assert half["trainer"]["has_perm_seed"] == (perm == "native")
    # a resumed run's own checkpoint is the uninterrupted run's, section by section (the loop's generator state included)
    again = str(tmp_path_factory.mktemp("again_" + perm) / "again.ckpt")
    run["mod"].train(updates=6, resume=run["paths"]["half"], save=again, **run["kw"])
    assert _same({k: v for k, v in checkpoint.load(again).items()}, {k: v for k, v in full.items()})
    # refusals that need the file
    with pytest.raises(ValueError, match=r"horizon \(the file has 8, this run 4\)"):
        run["mod"].train(updates=6, resume=run["paths"]["half"], **dict(run["kw"], horizon=4))


def test_a_policy_only_file_is_written_in_the_other_modes_and_cannot_be_resumed(torch_cuda, tmp_path):
    from ship_sim_gym_amd import checkpoint
    mod = load_script("train/ppo_torch.py")
    path = str(tmp_path / "eager.ckpt")
    kw = dict(envs=64, horizon=4, hidden=HIDDEN, env_kw={"n_beams": BEAMS}, log=QUIET)
    _, d = mod.train(updates=1, mode="native", update="torch", save=path, return_details=True, **kw)
    ckpt = checkpoint.load(path, require=("policy", "loop", "config"))
    assert "trainer" not in ckpt and "env" not in ckpt
    assert torch_cuda.equal(ckpt["policy"]["params"], torch_cuda.cat([p.reshape(-1) for p in d["params"]]).cpu())
    with pytest.raises(ValueError, match="no trainer section"):
        mod.train(updates=2, mode="native", update="native", resume=path, **kw)


def test_evaluation_reads_the_single_trainers_file(torch_cuda, tmp_path_factory):
    torch = torch_cuda
    from ship_gym.config import EnvConfig, GameConfig
    from ship_sim_gym_amd.evaluate import NativeEvaluator
    from ship_sim_gym_amd.obs_filter import ObsFilter
    from ship_sim_gym_amd.policy import NativePolicy
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    run = _single(tmp_path_factory, "native")
    ev = load_script("train/evaluate_native.py")
    got = ev.evaluate(envs=128, episodes=2, checkpoint=run["paths"]["full"], seed=4, log=QUIET)
    # the in-memory policy: the module the trainer returned, the filter it returned, an env built as the script builds it
    d = run["full"][1]
    net = run["mod"].ActorCritic(D, 3, hidden=HIDDEN, separate_value=True).to(DEV)
    with torch.no_grad():
        for p, q in zip(net.parameters(), d["params"]):
            p.copy_(q)
    env = ShipVecEnv(128, GameConfig, EnvConfig, device=DEV, n_beams=BEAMS)
    pol = NativePolicy.from_actor_critic(net, torch.full((D,), float(max(env.bounds)), dtype=torch.float64, device=DEV))
    env.set_obs_filter(ObsFilter(env, update=False).load_state_dict(d["obs_filter"]))
    want = NativeEvaluator(env).evaluate(pol, 2, greedy=True, seed=4)
    assert want["complete"] and got["complete"] and got["steps"] == want["steps"]
    assert got["per_member"].shape == (1, 8) and (got["per_member"] == want["per_member"].cpu().numpy()).all() and got["per_member"][0, 0] == 256
    env.close()
    with pytest.raises(ValueError, match="member"):
        ev.evaluate(envs=128, episodes=1, checkpoint=run["paths"]["full"], member=0, log=QUIET)
    # a plain module state_dict keeps working
    path = str(tmp_path_factory.mktemp("plain") / "net.pt")
    plain = run["mod"].ActorCritic(32, 3)
    torch.save(plain.state_dict(), path)
    assert ev.evaluate(envs=64, episodes=1, checkpoint=path, log=QUIET)["per_member"][0, 0] == 64


def test_save_best_holds_the_best_update(torch_cuda, tmp_path_factory):
    torch = torch_cuda
    from ship_sim_gym_amd import checkpoint
    run = _single(tmp_path_factory, "native")
    _, d = run["full"]
    best = checkpoint.load(run["paths"]["best"], require=("policy", "trainer", "env", "loop"))
    scores = d["episode_reward_mean"]
    ended = [s for s in scores if s != float("-inf")]
    assert len(scores) == 6 and ended  # (episodes ended: MAX_STEPS = 11 over 48 steps)
    assert best["loop"]["best"] == max(ended) == d["best"]
    u = best["loop"]["best_update"]
    assert u == scores.index(max(ended)) == d["best_update"] == best["loop"]["update"]
    # its parameters are the parameters after that update: run to that update again
    _, again = run["mod"].train(updates=u + 1, **run["kw"])
    assert torch.equal(best["policy"]["params"], torch.cat([p.reshape(-1) for p in again["params"]]).cpu())
    assert best["trainer"]["updates"] == u + 1
    # the criterion is part of the loop's state: the resumed run ended with the same best
    assert run["resumed"][1]["best"] == d["best"] and run["resumed"][1]["best_update"] == d["best_update"]


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. pbt_native.train, and 5. for a population
# ------------------------------------------------------------------------------------------------------------------------------------
PBT = dict(members=4, envs_per_member=64, horizon=8, perturb_every=2, mutate_schedule=True, mutate_batch=True, quantum=16, max_epochs=3,
           obs_filter=True, norm_reward=True, timeout_bootstrap=True, kl_coeff=1.0, hidden=HIDDEN, env_kw={"n_beams": BEAMS}, seed=2,
           return_details=True, log=QUIET)
PBT_KEYS = ("params", "exploits", "reslices", "member_steps", "kl_coef", "slices", "hparams", "train_batch_size", "obs_filter", "ret_filter",
            "env_state", "best", "best_update", "best_member", "episodes_ended")
_pbt_runs = {}


def _pbt(tmp_path_factory):
    if not _pbt_runs:
        mod = load_script("train/pbt_native.py")
        d = tmp_path_factory.mktemp("pbt")
        paths = {k: str(d / (k + ".ckpt")) for k in ("full", "best", "three", "four")}
        _pbt_runs.update(mod=mod, paths=paths, full=mod.train(updates=6, save=paths["full"], save_best=paths["best"], **PBT))
        for name, at in (("three", 3), ("four", 4)):  # between two perturbations, and just after one
            mod.train(updates=at, save=paths[name], **PBT)
            _pbt_runs[name] = mod.train(updates=6, resume=paths[name], **PBT)
    return _pbt_runs


@pytest.mark.parametrize("at", ["three", "four"])
def test_population_trainer_resumed_is_the_uninterrupted_run(torch_cuda, tmp_path_factory, at):
    from ship_sim_gym_amd import checkpoint
    run = _pbt(tmp_path_factory)
    (h_full, d_full), (h_res, d_res) = run["full"], run[at]
    assert len(d_full["exploits"]) == 3 and len(d_full["reslices"]) == 4 and len(set(map(tuple, (r[1] for r in d_full["reslices"])))) > 1
    assert any(ev["mutations"] for ev in d_full["exploits"]) and len(set(d_full["member_steps"])) > 1
    assert h_res == h_full and len(h_full) == 6  # (the score history)
    for k in PBT_KEYS:
        assert _same(d_res[k], d_full[k]), k
    saved = checkpoint.load(run["paths"][at])
    assert saved["loop"]["update"] == {"three": 3, "four": 4}[at] and saved["trainer"]["updates"] == saved["loop"]["update"]
    assert saved["loop"]["slices"] == d_full["reslices"][{"three": 1, "four": 2}[at]][1]  # (the layout of that moment, not the initial one)
    assert len(saved["loop"]["exploits"]) == {"three": 1, "four": 2}[at]


def test_evaluation_reads_the_population_file(torch_cuda, tmp_path_factory):
    torch = torch_cuda
    from ship_gym.config import EnvConfig, GameConfig
    from ship_sim_gym_amd import checkpoint
    from ship_sim_gym_amd.evaluate import NativeEvaluator
    from ship_sim_gym_amd.obs_filter import ObsFilter
    from ship_sim_gym_amd.population import NativePopulation
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    run = _pbt(tmp_path_factory)
    ev = load_script("train/evaluate_native.py")
    d = run["full"][1]
    scale = checkpoint.load(run["paths"]["full"])["population"]["obs_scale"].to(DEV)
    got = ev.evaluate(envs=128, episodes=2, checkpoint=run["paths"]["full"], seed=4, log=QUIET)
    env = ShipVecEnv(128, GameConfig, EnvConfig, device=DEV, n_beams=BEAMS)
    pop = NativePopulation.from_actor_critics(d["nets"], scale)
    assert torch.equal(pop.params, d["params"])
    env.set_obs_filter(ObsFilter(env, n_members=4, update=False).load_state_dict(d["obs_filter"]))
    want = NativeEvaluator(env).evaluate(pop, 2, greedy=True, seed=4)
    assert got["per_member"].shape == (4, 8) and (got["per_member"] == want["per_member"].cpu().numpy()).all()
    assert (got["per_member"][:, 0] == 64).all()
    # --member 2: that member alone on all the envs, with its own filter rows
    got2 = ev.evaluate(envs=128, episodes=2, checkpoint=run["paths"]["full"], seed=4, member=2, log=QUIET)
    one = dict(d["obs_filter"], state=d["obs_filter"]["state"][2:3].clone(), n_members=1)
    env.set_obs_filter(ObsFilter(env, update=False).load_state_dict(one))
    want2 = NativeEvaluator(env).evaluate(pop.member(2), 2, greedy=True, seed=4)
    assert got2["per_member"].shape == (1, 8) and (got2["per_member"] == want2["per_member"].cpu().numpy()).all()
    assert not (got2["per_member"][0] == got["per_member"][2]).all()  # (another env count: not the population run's row)
    env.close()
    with pytest.raises(ValueError, match="member 4 of a population of 4"):
        ev.evaluate(envs=128, episodes=1, checkpoint=run["paths"]["full"], member=4, log=QUIET)
    with pytest.raises(ValueError, match="do not split"):
        ev.evaluate(envs=126, episodes=1, checkpoint=run["paths"]["full"], log=QUIET)
    # the best file holds the whole population and names the member
    best, (h, _) = checkpoint.load(run["paths"]["best"]), run["full"]
    ended = [u for u in range(6) if d["episodes_ended"][u] > 0]
    top = max(max(h[u]) for u in ended)
    first = min(u for u in ended if max(h[u]) == top)
    assert best["loop"]["best"] == top == d["best"] and best["loop"]["best_update"] == first + 1 == d["best_update"]
    assert best["loop"]["best_member"] == h[first].index(top) and tuple(best["population"]["params"].shape) == tuple(d["params"].shape)
