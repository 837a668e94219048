"""The trainers' --episode-log on the device: the monitor file of train/ppo_torch.py is the numpy walk over the run's own rollout
buffers, a run that is saved and resumed leaves the uninterrupted run's file in every column but t and trains the same parameters as
a run without the flag, --best-window picks the update its rule says, and train/pbt_native.py's member column agrees with the layout.

All runs use hidden 16, 4 beams and a step limit of 11 (as tests/test_checkpoint_gpu.py does), so that every env ends an episode in
every update and the carries cross every rollout; the rollout buffers are captured where the trainers get them."""
import shutil

import numpy as np
import pytest

from gpu_support import load_script, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

BEAMS, HIDDEN, MAX_STEPS, ENVS, HORIZON = 4, 16, 11, 256, 8
QUIET = lambda *a, **k: None  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def short_episodes():
    from ship_sim_gym_amd.config import EnvConfig
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(EnvConfig, "MAX_STEPS", MAX_STEPS)
        yield


def _capture(mp, method):
    """Keep a copy of the reward / done / flags rows of every training rollout (envs of ENVS only: an evaluation env is not one)."""
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    seen, inner = [], getattr(ShipVecEnv, method)

    def outer(self, *a, **kw):
        b = inner(self, *a, **kw)
        seen.append(tuple(b[k].detach().cpu().numpy().copy() for k in ("rew", "done", "flags")))
        return b
    mp.setattr(ShipVecEnv, method, outer)
    return seen


def _walk(batches, n, members=None):
    """The log of the batches, and the episode count after each of them."""
    from ship_sim_gym_amd.episode_log import RECORD_DTYPE, episode_log_reference
    ring, head, cret, c, step0, ends = np.zeros(1 << 14, dtype=RECORD_DTYPE), np.zeros(2, dtype=np.int64), np.zeros(n), np.zeros((n, 2), dtype=np.int32), 0, []
    for rew, done, flags in batches:
        ring, head, cret, c = episode_log_reference(rew, done, flags, cret, c, head, ring, step0=step0, members=members)
        step0 += rew.shape[0]
        ends.append(int(head[0]))
    return ring[:int(head[0])], ends


def _but_t(path):
    with open(path) as f:
        lines = f.read().splitlines()
    return lines[:2], [",".join(c for i, c in enumerate(line.split(",")) if i != 2) for line in lines[2:]]


_runs = {}


def _single(tmp_path_factory):
    """Three updates with the log and a window of 100; the same saved after update 2 (two updates done) and resumed; the same without
    the flags."""
    if not _runs:
        mod = load_script("train/ppo_torch.py")
        d = tmp_path_factory.mktemp("episode_log_cli")
        p = {k: str(d / k) for k in ("log.csv", "full.csv", "half.csv", "best.ckpt", "half.ckpt")}
        kw = dict(envs=ENVS, horizon=HORIZON, mode="native", update="native", hidden=HIDDEN, env_kw={"n_beams": BEAMS}, seed=4, return_details=True, log=QUIET)
        flags = dict(episode_log=p["log.csv"], episode_log_capacity=4096, best_window=100)
        with pytest.MonkeyPatch.context() as mp:
            batches = _capture(mp, "rollout_policy")
            full = mod.train(updates=3, save_best=p["best.ckpt"], **kw, **flags)
            shutil.copy(p["log.csv"], p["full.csv"])
            batches = list(batches)
        half = mod.train(updates=2, save=p["half.ckpt"], **kw, **flags)
        shutil.copy(p["log.csv"], p["half.csv"])
        with open(p["log.csv"], "a") as f:  # the killed run had gone on past its checkpoint: rows the resumed run must cut
            f.write("0.5,3,0.1,24,0,0,0,1\n" * 5)
        resumed = mod.train(updates=3, resume=p["half.ckpt"], **kw, **flags)
        plain = mod.train(updates=3, **kw)
        _runs.update(mod=mod, paths=p, kw=kw, flags=flags, batches=batches, full=full, half=half, resumed=resumed, plain=plain)
    return _runs


def test_the_file_is_the_walk_over_the_runs_batches(torch_cuda, tmp_path_factory):
    from ship_sim_gym_amd.episode_log import read_monitor
    run = _single(tmp_path_factory)
    assert len(run["batches"]) == 3 and run["batches"][0][0].dtype == np.float64 and run["batches"][0][0].shape == (HORIZON, ENVS)
    want, ends = _walk(run["batches"], ENVS)
    hdr, cols = read_monitor(run["paths"]["full.csv"])
    assert set(hdr) == {"t_start", "env_id"} and want.shape[0] >= 2 * ENVS
    assert cols["r"].tolist() == want["ret"].tolist() and cols["l"].tolist() == want["length"].tolist()
    assert cols["timesteps"].tolist() == ((want["step"] + 1) * ENVS).tolist() and cols["env"].tolist() == want["env"].tolist()
    assert cols["goals"].tolist() == want["goals"].tolist() and cols["end"].tolist() == (want["end"] & 0xff).tolist() and not cols["member"].any()
    assert (cols["end"] & 0x8).any() and cols["l"].max() <= MAX_STEPS
    # one flush per update: the rows of an update share their t, and t does not decrease
    t = cols["t"]
    assert np.all(np.diff(t) >= 0) and [len(set(t[a:b])) for a, b in zip([0] + ends[:-1], ends)] == [1 if b > a else 0 for a, b in zip([0] + ends[:-1], ends)]


def test_saved_and_resumed_leaves_the_same_file_and_the_flag_changes_no_parameter(torch_cuda, tmp_path_factory):
    torch = torch_cuda
    from ship_sim_gym_amd import checkpoint
    run = _single(tmp_path_factory)
    p = run["paths"]
    head_full, rows_full = _but_t(p["full.csv"])
    head_half, rows_half = _but_t(p["half.csv"])
    head_res, rows_res = _but_t(p["log.csv"])
    _, ends = _walk(run["batches"], ENVS)
    assert len(rows_half) == ends[1] and rows_half == rows_full[:ends[1]] and len(rows_full) == ends[2] > ends[1]
    assert rows_res == rows_full and head_res == head_half and head_res[1] == head_full[1]  # (the resumed file keeps the half run's t_start)
    ck = checkpoint.load(p["half.ckpt"])
    assert ck["episode_log"]["rows_written"] == ck["episode_log"]["flushed"] == ends[1] and ck["episode_log"]["steps"] == 2 * HORIZON
    assert ck["config"]["episode_log"] == p["log.csv"] and ck["config"]["best_window"] == 100
    assert float(ck["episode_log"]["carry"][:, 0].sum()) > 0  # (episodes in flight across the save)
    (h_full, d_full), (h_res, d_res), (h_plain, d_plain) = run["full"], run["resumed"], run["plain"]
    assert h_full == h_res == h_plain
    for d in (d_res, d_plain):
        assert len(d["params"]) == len(d_full["params"]) and all(torch.equal(a, b) for a, b in zip(d["params"], d_full["params"]))
        assert torch.equal(d["env_state"], d_full["env_state"])
    assert d_res["episode_reward_mean"] == d_full["episode_reward_mean"] and (d_res["best"], d_res["best_update"]) == (d_full["best"], d_full["best_update"])
    # the section is required exactly when the flag is on
    with pytest.raises(ValueError, match="episode_log"):
        run["mod"].train(updates=3, resume=p["half.ckpt"], **run["kw"])
    bare = str(tmp_path_factory.mktemp("bare") / "bare.ckpt")
    run["mod"].train(updates=1, save=bare, **run["kw"])
    assert "episode_log" not in checkpoint.load(bare)
    with pytest.raises(ValueError, match="episode_log"):
        run["mod"].train(updates=2, resume=bare, **run["kw"], **run["flags"])


def test_best_window_picks_the_update_the_window_rule_says(torch_cuda, tmp_path_factory):
    from ship_sim_gym_amd import checkpoint
    run = _single(tmp_path_factory)
    want, ends = _walk(run["batches"], ENVS)
    scores, best, best_update = [], float("-inf"), -1
    for u, (a, b) in enumerate(zip([0] + ends[:-1], ends)):
        scores.append(float(np.mean(want["ret"][:b][-100:])) if b > a else float("-inf"))
        if scores[-1] > best:
            best, best_update = scores[-1], u
    d = run["full"][1]
    assert d["episode_reward_mean"] == scores and (d["best"], d["best_update"]) == (best, best_update)
    assert checkpoint.load(run["paths"]["best.ckpt"])["loop"]["update"] == best_update
    # the default criterion is the update's own mean, and it differs
    plain = run["plain"][1]["episode_reward_mean"]
    own = [float(np.sum(want["ret"][a:b])) / (b - a) if b > a else float("-inf") for a, b in zip([0] + ends[:-1], ends)]
    assert plain != scores and all(x == y or abs(x - y) < 1e-9 for x, y in zip(plain, own))


def test_the_population_trainer_writes_member_ids_that_agree_with_the_layout(torch_cuda, tmp_path):
    from ship_sim_gym_amd.episode_log import member_of_envs, read_monitor
    mod = load_script("train/pbt_native.py")
    path = str(tmp_path / "pbt.csv")
    kw = dict(members=4, envs_per_member=64, horizon=HORIZON, perturb_every=2, hidden=HIDDEN, env_kw={"n_beams": BEAMS}, seed=2, return_details=True,
              log=QUIET)
    with pytest.MonkeyPatch.context() as mp:
        batches = _capture(mp, "rollout_population")
        _, with_log = mod.train(updates=3, episode_log=path, **kw)
        batches = list(batches)
    members = member_of_envs(256, 4)
    want, ends = _walk(batches, 256, members)
    _, cols = read_monitor(path)
    assert len(batches) == 3 and want.shape[0] >= 2 * 256
    assert cols["member"].tolist() == (cols["env"] // 64).tolist() == members[want["env"]].tolist() and set(cols["member"].tolist()) == {0, 1, 2, 3}
    assert cols["r"].tolist() == want["ret"].tolist() and cols["l"].tolist() == want["length"].tolist()
    _, without = mod.train(updates=3, **kw)
    assert bool((with_log["params"] == without["params"]).all()) and with_log["episodes_ended"] == without["episodes_ended"] == list(np.diff([0] + ends))
