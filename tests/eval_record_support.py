"""What the evaluation recorder's test modules share (tests/test_eval_record_gpu.py, tests/test_eval_domain_gpu.py): the step-by-step
restatement of an evaluation run — the public one-step calls in a Python loop from a reset — its walks, a recorder whose buffers hold
sentinels, the run under test, and the comparison rules.  The defaults are test_eval_record_gpu's shapes.  Nothing here needs a device
at import."""
import numpy as np

E, CAP = 3, 32
IDS = [255, 0, 64, 65, 130]
ROWS = ("obs", "act", "logp", "value", "reward", "done", "flags", "next_obs")
SENT, SENT_U8, SENT_PIX = -7, 0xEE, 0x5A   # what the buffers hold before a run (0x5A is in no colour the rasteriser paints)


def _oracle(torch, env, pol, steps, ids, greedy, uniforms=None, sizes=(), debugs=(True, False)):
    """The step-wise restatement, from a reset: numpy arrays [steps, N, ...] keyed as record_walk's arguments, and the tracked envs'
    screens per (size, debug): uint8 [steps, R, W, H, 3], each taken when that step's observation was current."""
    from ship_sim_gym_amd.evaluate import next_observations
    env.reset_tensor()
    env.enable_terminal_obs(True)
    rows = {k: [] for k in ("obs", "act", "logp", "value", "rew", "done", "flags", "after", "term")}
    screens = {(s, d): [] for s in sizes for d in debugs}
    for k in range(steps):
        rows["obs"].append(env.obs.clone())
        for (s, d), frames in screens.items():
            frames.append(torch.stack([env.get_screen(e, s[0], s[1], debug=d) for e in ids]))
        a, lp, v, _ = env.policy_act(pol, greedy=greedy, uniforms=None if greedy else uniforms[k])
        rows["act"].append(a.clone()); rows["logp"].append(lp.clone()); rows["value"].append(v.clone())
        o, r, d, f = env.step_tensor(a)
        rows["rew"].append(r.clone()); rows["done"].append(d.clone()); rows["flags"].append(f.clone())
        rows["after"].append(o.clone()); rows["term"].append(env.term_obs.clone())
    env.enable_terminal_obs(False)
    s = {k: torch.stack(v).cpu().numpy() for k, v in rows.items()}
    s["next_obs"] = next_observations(s.pop("after"), s.pop("term"), s["done"])
    return s, {k: torch.stack(v).cpu().numpy() for k, v in screens.items()}


def _walk(s, ids, episodes, capacity, sl=slice(None), state=None):
    from ship_sim_gym_amd.evaluate import record_walk
    return record_walk(*(s[k][sl] for k in ("obs", "act", "logp", "value", "rew", "done", "flags", "next_obs")), ids, episodes, capacity,
                       state=state)


def _recorder(env, ids=IDS, capacity=CAP, **kw):
    from ship_sim_gym_amd.evaluate import EvalRecorder
    rec = EvalRecorder(env, ids, capacity, **kw)
    for k in ("obs", "next_obs", "act", "logp", "value", "reward"):
        getattr(rec, k).fill_(SENT)
    rec.done.fill_(SENT_U8); rec.flags.fill_(SENT_U8)
    if rec.frames is not None:
        rec.frames.fill_(SENT_PIX)
    return rec


def _run(env, pol, rec, calls, greedy, uniforms=None, episodes=E):
    """A reset, then one ssg_evaluate call per entry of `calls` (their step counts); returns the evaluator."""
    from ship_sim_gym_amd.evaluate import NativeEvaluator
    ev = NativeEvaluator(env)
    env.reset_tensor()
    if rec is not None:
        rec.reset()
    k0 = 0
    for n in calls:
        ev.run(pol, episodes, n, greedy=greedy, step0=k0, uniforms=None if greedy else uniforms[k0:k0 + n], recorder=rec)
        k0 += n
    return ev


def _assert_record(got, want):
    """Every buffer, cursor and overflow count equals the walk's; rows at and past the cursor still hold the sentinel."""
    assert np.array_equal(got["cursor"], want["cursor"]) and np.array_equal(got["overflow"], want["overflow"])
    for r, n in enumerate(want["cursor"]):
        for k in ROWS:
            assert np.array_equal(got[k][r, :n], want[k][r, :n]), (r, k)
            assert (got[k][r, n:] == (SENT_U8 if k in ("done", "flags") else SENT)).all(), (r, k)


def _assert_frames(got, want, screens, S):
    """Frame t / S of slot r is the screen taken when row t was filled (t % S == 0); every other frame keeps the sentinel."""
    frames, drawn = got["frames"], 0
    for r, n in enumerate(want["cursor"]):
        used = set()
        for t in range(0, int(n), S):
            assert np.array_equal(frames[r, t // S], screens[want["iteration"][r, t], r]), (r, t)
            used.add(t // S)
        for i in range(frames.shape[1]):
            if i not in used:
                assert (frames[r, i] == SENT_PIX).all(), (r, i)
        drawn += len(used)
    assert drawn > 0
