"""What the GPU test modules share besides the references: the torch_cuda fixture (imported by name into each module, which pytest then
collects as that module's own), the trainer-script loader, env configs and handles per obs_dim, the state columns, torch's sampling."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# obs_dim D = history * (6 + n_beams)
HIST_BEAMS = {7: (1, 1), 22: (1, 16), 27: (3, 3), 44: (4, 5), 88: (8, 5), 176: (8, 16)}
STATE_COLUMNS = ("F_X", "F_Y", "F_VX", "F_VY", "F_ANGLE", "F_W", "F_LIDAR", "F_RUDDER", "F_STEP_COUNT", "F_MAP_ID", "F_GOAL_MASK",
                 "F_CUM_REWARD")  # train/ppo_torch.py's env_columns()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def load_script(rel_path):
    """A fresh module object of a script of the repository, e.g. load_script("train/pbt_native.py")."""
    name = os.path.splitext(rel_path)[0].replace("/", "_") + "_under_test"
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *rel_path.split("/")))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def env_config(history, max_steps=None):
    from ship_sim_gym_amd.config import EnvConfig

    class E(EnvConfig):
        HISTORY_SIZE = history
    if max_steps is not None:
        E.MAX_STEPS = max_steps
    return E


def vec(n, D, base=0, n_maps=4):
    """A handle whose obs_dim is D."""
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    history, n_beams = HIST_BEAMS[D]
    env = ShipVecEnv(n, n_maps=n_maps, n_beams=n_beams, env_config=env_config(history), env_id_base=base)
    assert env.states_history == D
    return env


def state_columns(env):
    from ship_sim_gym_amd import _native as N
    return {name: env.field(getattr(N, name)).clone() for name in STATE_COLUMNS}


def same_columns(torch, a, b):
    ca, cb = state_columns(a), state_columns(b)
    return all(torch.equal(ca[k], cb[k]) for k in ca)


def torch_sample(torch, logits, u):
    """ppo_torch's Shard.step() sampling: log_softmax, cumsum(exp), count(u > cdf[:, :-1])."""
    logp_all = torch.log_softmax(logits, dim=-1)
    cdf = logp_all.exp().cumsum(dim=-1)
    act = (u.unsqueeze(-1) > cdf[:, :-1]).sum(dim=-1)
    return act, logp_all.gather(-1, act.unsqueeze(-1)).squeeze(-1), cdf


def check_near_rows(torch, near, u, cdf, act, logp, logp_all, tol=None, band=1e-5):
    """The rows a sampling test keeps out of its exact comparison because u lies within `band` of an entry of the reference's
    cdf [n, A]: the stored action is still one of the two the boundary separates (the reference's own choice for u - band and for
    u + band, which are those two unless a second boundary lies in the band too), and logp is the reference log-probability
    logp_all [n, A] of the action that WAS stored, within `tol` (None: the caller judges).  Returns |logp - reference| of the near rows."""
    if not bool(near.any()):
        return torch.zeros(0, dtype=logp_all.dtype, device=logp.device)
    u, cdf = u[near].double().unsqueeze(-1), cdf[near][:, :-1].double()       # (exact: both are f32 or f64 values)
    lo, hi = (u - band > cdf).sum(-1), (u + band > cdf).sum(-1)
    a = act[near].long()
    assert bool(((lo <= a) & (a <= hi)).all()) and bool((hi > lo).all()), (lo.tolist(), a.tolist(), hi.tolist())
    ref = logp_all[near].gather(-1, a.unsqueeze(-1)).squeeze(-1)
    err = (logp[near].to(ref.dtype) - ref).abs()
    assert tol is None or bool((err <= tol).all()), (err.tolist(), tol)
    return err
