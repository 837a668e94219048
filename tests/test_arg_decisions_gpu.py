"""Which tensor arguments the Python host layer takes and which it refuses, method by method: a table of (method, argument, defect)
rows over every public method whose tensor arguments go through the shared check (``_native.arg``; ReturnFilter's and EpisodeLog's rows
keep their strided-row predicate), on ONE 256-env handle with hidden width 32 and K = 4.

Defects, each applied to an argument the method takes as it stands: "dtype" (another dtype), "cpu" (the same values on the host),
"strided" (the same shape as a view of every second element of a wider tensor: not contiguous, rows not of unit stride), "short" (one
element too few, flat), "trail" (a trailing dimension one too long).  A refused row asserts the exception's type and that the message
names the class or method and the argument, in the words the messages have always used; an accepted row asserts that the call
returns.  Every refusal happens in Python before anything is launched.

What is decided, and has always been (DECIDED lists every row that is not a plain ValueError):
* the data-parallel trainer's ``set_moments`` / ``set_minibatch_rows`` / ``apply_rows`` convert their rows first (``.to(device,
  dtype).contiguous()``), so only a wrong shape is refused;
* ``ShipVecEnv.set_adv_table`` has never asked where the table lives: a host tensor of the right shape is bound;
* ``ReturnFilter.apply_rows`` and ``EpisodeLog.merge_blocks`` make their gathered rows contiguous themselves: any strides serve;
* ``NativePPO``'s sample count is obs.numel() // obs_dim, so an observation tensor of the wrong size shows as the NEXT entry's
  mismatch ("act"), and a flat ``rew`` in ``gae`` fails at ``rew.shape[1]`` (IndexError);
* the columns of ``stats`` (4 or 8) are the library's to judge: "trail" is not in their rows.
Accepted on purpose: ReturnFilter's [:, :N] views of wider buffers, NativePPO's batch entries in any shape of the right count, output
buffers with more rows than K."""
import re
import types

import pytest

from gpu_support import torch_cuda, vec  # noqa: F401
from ppo_reference import actor_critic_policy

pytestmark = pytest.mark.gpu

N_ENVS, D, H, K, P = 256, 22, 32, 4, 2
DEFECTS = ("dtype", "cpu", "strided", "short", "trail")


def other_dtype(torch, dt):
    return {torch.float64: torch.float32, torch.float32: torch.float64, torch.uint8: torch.int32, torch.int32: torch.int64,
            torch.int64: torch.int32}[dt]


def spoil(torch, t, defect):
    """The argument `t` (contiguous, on the device) with one defect."""
    if defect == "dtype":
        return t.to(other_dtype(torch, t.dtype))
    if defect == "cpu":
        return t.cpu()
    if defect == "strided":
        wide = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
        view = wide[..., ::2]
        view.copy_(t)
        assert tuple(view.shape) == tuple(t.shape) and not view.is_contiguous()
        return view
    if defect == "short":
        return t.reshape(-1)[:-1].clone()
    assert defect == "trail"
    return torch.zeros(tuple(t.shape[:-1]) + (t.shape[-1] + 1,), dtype=t.dtype, device=t.device)


def wider(torch, t, extra=64):
    """`t` ([K, N]) as the [:, :N] view of a buffer of row pitch N + extra."""
    wide = torch.zeros((t.shape[0], t.shape[1] + extra), dtype=t.dtype, device=t.device)
    view = wide[:, :t.shape[1]]
    view.copy_(t)
    return view


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    """The handle and everything the rows call, made once: a policy and a population of two, a rollout batch of each with gae() and
    one update() behind it, the trainers, the filters and the logs."""
    torch = torch_cuda
    from ship_sim_gym_amd.dp import DataParallelPPO
    from ship_sim_gym_amd.episode_log import EpisodeLog
    from ship_sim_gym_amd.obs_filter import ObsFilter
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    from ship_sim_gym_amd.ppo import NativePPO
    from ship_sim_gym_amd.ret_filter import ReturnFilter
    c = types.SimpleNamespace(torch=torch)
    c.env = env = vec(N_ENVS, D)
    c.pol = actor_critic_policy(torch, D, H=H, seed=1)[1]
    c.pop = NativePopulation([actor_critic_policy(torch, D, H=H, seed=10 + m)[1] for m in range(P)])
    env.reset_tensor()
    c.out = env.rollout_policy(c.pol, K, seed=3)  # (the buffers the rollout_policy rows write into; the batch below has its own)
    c.batch = dict(env.rollout_policy(c.pol, K, seed=7))
    c.ppo = NativePPO(c.pol, env, perm_seed=5)
    c.ppo.gae(c.batch)
    c.n = K * N_ENVS
    c.perm = c.ppo.draw_perm(c.n, 1)
    c.idx = c.perm[0, :c.n // 2].contiguous()
    c.stats = c.ppo.update(c.batch, c.perm, 1, 2, stats=True)
    c.pbatch = dict(env.rollout_population(c.pop, K, seed=4))
    c.pppo = PopulationPPO(c.pop, env, perm_seed=6)
    c.pppo.gae(c.pbatch)
    c.pperm = c.pppo.draw_perm(K, 1)
    c.pstats = c.pppo.update(c.pbatch, c.pperm, 1, 2, stats=True)
    c.dp = DataParallelPPO(c.pol, env)
    c.dp_mb = DataParallelPPO(c.pol, env, job_adv_norm="minibatch")
    c.flt, c.jflt = ObsFilter(env), ObsFilter(env, job=True)
    c.rf, c.jrf = ReturnFilter(env), ReturnFilter(env, job=True)
    c.log = EpisodeLog(env, capacity=1024)
    c.jlog = EpisodeLog(env, capacity=1024, job=True, rows=K, world=1, total_envs=N_ENVS)
    c.term = torch.zeros((K, N_ENVS, D), dtype=torch.float64, device=env.device)
    yield c
    torch.cuda.synchronize()
    env.close()


def _with(batch, key, t):
    b = dict(batch)
    b[key] = t
    return b


def _rows_batch(c, key, t):
    return _with({"rew": c.batch["rew"], "done": c.batch["done"], "flags": c.batch["flags"]}, key, t)


def _pending_block(c):
    """The job log with a shard_block waiting for its merge."""
    if c.jlog._pending is None:
        c.block = c.jlog.shard_block(_rows_batch(c, "rew", c.batch["rew"]))
    return c.block


def _no_pending_block(c):
    if c.jlog._pending is not None:
        c.jlog.merge_blocks(c.block[None])


def _shard_block_out(c, t):
    _no_pending_block(c)
    c.block = c.jlog.shard_block(_rows_batch(c, "rew", c.batch["rew"]), out=t)


def _set_adv_table(c, t):
    try:
        c.env.set_adv_table(t)
    finally:
        c.env.set_adv_table(None)


def _batch_rows(who, call, batch, keys):
    """Rows over entries of a batch dict: the good tensor is batch[key], the call gets the batch with that entry replaced."""
    return [(who, key, (lambda c, batch=batch, key=key: getattr(c, batch)[key]),
             (lambda c, t, call=call, batch=batch, key=key: call(c, _with(getattr(c, batch), key, t)))) for key in keys]


# (who: the class or method the message names, argument: the name it gives it, good(c): the argument as the method takes it, call(c, t))
SUBJECTS = (
    _batch_rows("NativePPO", lambda c, b: c.ppo.gae(b), "batch", ("rew", "done", "val", "last_val"))
    + [("NativePPO", "boot", lambda c: c.torch.zeros_like(c.batch["val"]), lambda c, t: c.ppo.gae(_with(c.batch, "boot", t)))]
    + _batch_rows("NativePPO", lambda c, b: c.ppo.grad(b, c.idx), "batch", ("obs", "act", "logp", "adv", "ret"))
    + _batch_rows("NativePPO", lambda c, b: c.ppo.update(b, c.perm, 1, 2), "batch", ("obs", "act", "logp", "adv", "ret"))
    + [("NativePPO", "out", lambda c: c.torch.zeros_like(c.perm), lambda c, t: c.ppo.draw_perm(c.n, 1, out=t)),
       ("NativePPO", "stats", lambda c: c.stats, lambda c, t: c.ppo.report(c.batch, stats=t))]
    + _batch_rows("PopulationPPO", lambda c, b: c.pppo.gae(b), "pbatch", ("rew", "done", "val", "last_val"))
    + _batch_rows("PopulationPPO", lambda c, b: c.pppo.update(b, c.pperm, 1, 2), "pbatch", ("obs", "act", "logp", "adv", "ret"))
    + [("PopulationPPO", "out", lambda c: c.torch.zeros_like(c.pperm), lambda c, t: c.pppo.draw_perm(K, 1, out=t)),
       ("PopulationPPO", "stats", lambda c: c.pstats, lambda c, t: c.pppo.report(c.pbatch, stats=t))]
    + _batch_rows("PopulationPPO", lambda c, b: c.pppo.episode_stats(b), "pbatch", ("rew", "done"))
    + [("DataParallelPPO.set_moments", "rows", lambda c: c.torch.tensor([[1.0, 1024.0, 1024.0, 0.0]], dtype=c.torch.float64, device=c.env.device),
        lambda c, t: c.dp.set_moments(t)),
       ("DataParallelPPO.set_minibatch_rows", "rows",
        lambda c: c.torch.tensor([[[1.0, 512.0, 512.0, 0.0]] * 2], dtype=c.torch.float64, device=c.env.device),
        lambda c, t: c.dp_mb.set_minibatch_rows(t)),
       ("DataParallelPPO.apply_rows", "rows", lambda c: c.torch.zeros((1, c.dp.n_params + 8), dtype=c.torch.float32, device=c.env.device),
        lambda c, t: c.dp.apply_rows(t, [c.n], True, False)),
       ("ObsFilter.update", "obs", lambda c: c.env.obs.clone(), lambda c, t: c.flt.update(t)),
       ("ObsFilter.merge_rows", "rows", lambda c: c.jflt.buffer[None].clone(), lambda c, t: c.jflt.merge_rows(t)),
       ("ReturnFilter", "rew", lambda c: c.batch["rew"], lambda c, t: c.rf.normalise(t, c.batch["done"])),
       ("ReturnFilter", "done", lambda c: c.batch["done"], lambda c, t: c.rf.normalise(c.batch["rew"], t)),
       ("ReturnFilter.shard_rows", "rew", lambda c: c.batch["rew"], lambda c, t: c.jrf.shard_rows({"rew": t, "done": c.batch["done"]})),
       ("ReturnFilter.shard_rows", "done", lambda c: c.batch["done"], lambda c, t: c.jrf.shard_rows({"rew": c.batch["rew"], "done": t})),
       ("ReturnFilter.apply_rows", "rew", lambda c: c.batch["rew"],
        lambda c, t: c.jrf.apply_rows({"rew": t}, c.torch.zeros((1, K, 4), dtype=c.torch.float64, device=c.env.device))),
       ("ReturnFilter.apply_rows", "rows", lambda c: c.torch.zeros((1, K, 4), dtype=c.torch.float64, device=c.env.device),
        lambda c, t: c.jrf.apply_rows({"rew": c.batch["rew"]}, t))]
    + [("EpisodeLog", key, (lambda c, key=key: c.batch[key]), (lambda c, t, key=key: c.log.append(_rows_batch(c, key, t))))
       for key in ("rew", "done", "flags")]
    + [("EpisodeLog.shard_block", "out", lambda c: c.torch.zeros(c.jlog.block_nbytes, dtype=c.torch.uint8, device=c.env.device), _shard_block_out),
       ("EpisodeLog.merge_blocks", "blocks", lambda c: _pending_block(c)[None].clone(), lambda c, t: (_pending_block(c), c.jlog.merge_blocks(t))),
       ("set_adv_table", "table", lambda c: c.torch.zeros((3, 4), dtype=c.torch.float32, device=c.env.device), _set_adv_table),
       ("timeout_values", "flags", lambda c: c.batch["flags"], lambda c, t: c.env.timeout_values(c.pol, t, c.term)),
       ("timeout_values", "term_obs", lambda c: c.term, lambda c, t: c.env.timeout_values(c.pol, c.batch["flags"], t)),
       ("timeout_values", "out", lambda c: c.torch.zeros_like(c.batch["val"]), lambda c, t: c.env.timeout_values(c.pol, c.batch["flags"], c.term, out=t))]
    + [("rollout_policy", key, (lambda c, key=key: c.out[key]), (lambda c, t, key=key: c.env.rollout_policy(c.pol, K, seed=3, out=_with(c.out, key, t))))
       for key in ("obs", "act", "done")]  # (last_val is [>= N]: one element more is a prefix that serves)
)

ACCEPT = "accept"
# the rows that are not a ValueError naming (who, argument): ACCEPT, or (exception type, the argument the message names instead)
DECIDED = {}
for _who in ("DataParallelPPO.set_moments", "DataParallelPPO.set_minibatch_rows", "DataParallelPPO.apply_rows"):
    for _defect in ("dtype", "cpu", "strided"):
        DECIDED[(_who, "rows", _defect)] = ACCEPT  # (converted first)
DECIDED[("set_adv_table", "table", "cpu")] = ACCEPT
DECIDED[("ReturnFilter.apply_rows", "rows", "strided")] = ACCEPT
DECIDED[("EpisodeLog.merge_blocks", "blocks", "strided")] = ACCEPT
DECIDED[("NativePPO", "obs", "short")] = DECIDED[("NativePPO", "obs", "trail")] = (ValueError, "act")
DECIDED[("NativePPO", "rew", "short")] = (IndexError, None)
DECIDED[("NativePPO", "rew", "trail")] = (ValueError, "done")  # (K and N are rew's: the next entry is the one that does not fit)
SKIPPED = {("NativePPO", "stats", "trail"), ("PopulationPPO", "stats", "trail")}  # (the columns are the library's to judge)

ROWS = [(i, defect) for i, s in enumerate(SUBJECTS) for defect in DEFECTS if (s[0], s[1], defect) not in SKIPPED]


@pytest.mark.parametrize("index,defect", ROWS, ids=["%s-%s-%s-%d" % (SUBJECTS[i][0], SUBJECTS[i][1], d, i) for i, d in ROWS])
def test_decision(ctx, index, defect):
    who, argument, good, call = SUBJECTS[index]
    t = spoil(ctx.torch, good(ctx), defect)
    decision = DECIDED.get((who, argument, defect), (ValueError, argument))
    if decision == ACCEPT:
        call(ctx, t)
        return
    exc, named = decision
    with pytest.raises(exc) as ex:
        call(ctx, t)
    assert type(ex.value) is exc, ex.value
    if named is not None:
        assert any(word in str(ex.value) for word in who.split(".")), str(ex.value)
        assert re.search(r"(?<![A-Za-z_])%s(?![A-Za-z_])" % re.escape(named), str(ex.value)), str(ex.value)  # (a word, not a substring)


def test_every_subject_takes_its_argument_as_it_stands(ctx):
    """The unspoiled argument of every row is accepted: the defects above are what is refused, not the rows' own set-up."""
    for who, argument, good, call in SUBJECTS:
        call(ctx, good(ctx))


def test_wider_pitch_views_serve_the_return_filter(ctx):
    torch, b = ctx.torch, ctx.batch
    rew, done = wider(torch, b["rew"]), wider(torch, b["done"])
    assert not rew.is_contiguous() and rew.stride(0) == N_ENVS + 64
    out, denom = ctx.rf.normalise(rew, done)
    assert tuple(out.shape) == (K, N_ENVS) and out.stride(0) == rew.stride(0) and tuple(denom.shape) == (K, 1)
    rows = ctx.jrf.shard_rows({"rew": rew, "done": done})
    assert tuple(rows.shape) == (K, 4)
    assert tuple(ctx.jrf.apply_rows({"rew": rew}, rows[None]).shape) == (K, N_ENVS)
    with pytest.raises(ValueError, match="row pitch"):
        ctx.rf.normalise(rew, b["done"])  # (each serves alone, but not two pitches in one call)


def test_reshaped_batch_entries_serve_native_ppo(ctx):
    """NativePPO reads its batch entries flat: any shape with the right element count."""
    b = dict(ctx.batch)
    b.update(obs=b["obs"].reshape(ctx.n, D), act=b["act"].reshape(-1), logp=b["logp"].reshape(N_ENVS, K), adv=b["adv"].reshape(2, -1),
             ret=b["ret"].reshape(-1, 1))
    g = ctx.ppo.grad(b, ctx.idx)
    assert tuple(g.shape) == (ctx.ppo.n_params,)
    st = ctx.ppo.update(b, ctx.perm, 1, 2, stats=True)
    assert tuple(st.shape) == (2, 4)


def test_output_buffers_with_more_rows_than_K_serve(ctx):
    torch, env = ctx.torch, ctx.env
    out = {k: (v if k == "last_val" else torch.zeros((K + 2,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)) for k, v in ctx.out.items()}
    got = env.rollout_policy(ctx.pol, K, seed=3, out=out)
    assert all(got[k].shape[0] == K and got[k].data_ptr() == out[k].data_ptr() for k in out if k != "last_val")
    vals = env.timeout_values(ctx.pol, ctx.batch["flags"], ctx.term, out=torch.zeros((K + 1, N_ENVS), dtype=torch.float32, device=env.device))
    assert tuple(vals.shape) == (K, N_ENVS)
    perm = ctx.ppo.draw_perm(ctx.n, 1, out=torch.zeros_like(ctx.perm))
    assert tuple(perm.shape) == (1, ctx.n)
