"""CPU-side checks of the population path (ssg_population, ssg_pop_*, ship_sim_gym_amd/population.py, train/pbt_native.py): the new
symbols in the header and the binding, the record against ctypes, the refusals before any device work, the workspace size, the host
table against the single-policy roundings, the PBT scheduler's semantics, and the trainer's argument parsing.  No GPU."""
import ctypes as C
import math
import os
import re
import struct
import sys

import pytest

from gpu_support import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POP_SYMBOLS = ("ssg_pop_act", "ssg_pop_rollout", "ssg_pop_pack_hparams", "ssg_pop_workspace_nbytes", "ssg_pop_gae", "ssg_pop_update",
               "ssg_pop_exploit", "ssg_pop_episode_stats")


def _header():
    return open(os.path.join(ROOT, "include", "shipsim.h")).read()


def test_population_symbols_are_declared_exported_and_abi_stays_9(native):
    text = _header()
    L = native.lib()
    for name in POP_SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert name in native.EXPORTS and hasattr(L, name), name
    assert native.ABI_VERSION == 9 and L.ssg_abi_version() == 9
    assert re.search(r"#define\s+SSG_ABI_VERSION\s+9\b", text)
    assert int(re.search(r"#define\s+SSG_POP_MAX_MEMBERS\s+(\d+)", text).group(1)) == native.POP_MAX_MEMBERS == 256
    # SSG_POP_TABLE_FLOATS as the header defines it: 8 floats per member, once for GAE / the loss and once per Adam step
    assert "#define SSG_POP_TABLE_FLOATS(n_members, n_steps) ((size_t)(n_members) * 8u * (size_t)(1 + (n_steps)))" in text
    assert native.pop_table_floats(120, 8) == 120 * 8 * 9


def test_population_record_matches_the_header(native):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct ssg_population \{(.*?)\} ssg_population;", text, flags=re.S).group(1)
    names = []
    for ctype, decl in re.findall(r"(uint32_t|int32_t|const double \*|float \*)\s*([\w\s,]+);", body):
        names += [(ctype.strip(), n.strip()) for n in decl.split(",")]
    assert [n for _, n in names] == [f for f, _ in native.Population._fields_]
    size_of = {"uint32_t": 4, "int32_t": 4, "const double *": C.sizeof(C.c_void_p), "float *": C.sizeof(C.c_void_p)}
    off = 0
    for ctype, name in names:
        sz = size_of[ctype]
        off = (off + sz - 1) // sz * sz
        assert getattr(native.Population, name).offset == off, name
        off += sz
    assert C.sizeof(native.Population) == (off + 7) // 8 * 8 == 48
    # the shape fields are ssg_policy's, in its order: a member is an ssg_policy over its row
    shape = [f for f, _ in native.Policy._fields_][1:6]
    assert [f for f, _ in native.Population._fields_][2:7] == shape


def _pop_record(native, P=4, D=32, H=64, L=2, A=3, params=0x10000, scale=0x20000):
    p = native.Population()
    p.struct_size = C.sizeof(native.Population)
    p.n_members, p.obs_dim, p.hidden, p.n_hidden_layers, p.n_actions, p.activation = P, D, H, L, A, native.POLICY_TANH
    p.dev_params, p.dev_obs_scale = params, scale
    return p


def _hparams(native, P, **kw):
    arr = (native.PpoHparams * P)()
    base = dict(gamma=0.99, lam=0.95, clip=0.2, vf_coef=0.5, ent_coef=0.01, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, adv_eps=1e-8)
    for m in range(P):
        arr[m].struct_size = C.sizeof(native.PpoHparams)
        for k, v in base.items():
            setattr(arr[m], k, kw[k][m] if k in kw else v)
    return arr


def _handle(native, n_envs, bound):
    L = native.lib()
    c = native.default_config()
    c.n_envs = n_envs
    h = C.c_void_p()
    native.check(L.ssg_create(C.byref(c), C.byref(h)))
    if bound:  # (host only: the address is recorded, never touched before a launch — and every call below is refused before one)
        native.check(L.ssg_bind_state(h, C.c_void_p(0x100000)), h)
    return h


def _calls(native, h, pop, K=4):
    """Every device entry point with plausible non-NULL pointers (never dereferenced on the host)."""
    L = native.lib()
    q = C.c_void_p(0x30000)
    src = (C.c_int32 * 256)(*range(256))
    P = pop.n_members if pop is not None else 4
    pr = C.byref(pop) if pop is not None else None
    return {
        "act": lambda: L.ssg_pop_act(h, pr, q, None, 0, 0, q, q, q, None, None),
        "rollout": lambda: L.ssg_pop_rollout(h, pr, K, None, 0, 0, q, q, q, q, None, q, q, None, None, 1 << 20, None),
        "gae": lambda: L.ssg_pop_gae(h, pr, q, K, q, q, q, q, q, q, q, 1 << 40, None),
        "update": lambda: L.ssg_pop_update(h, pr, q, 1 << 20, K, q, q, q, q, q, q, 2, 4, q, None, q, 1 << 40, None),
        "exploit": lambda: L.ssg_pop_exploit(h, pr, src, q, None),
        "episode_stats": lambda: L.ssg_pop_episode_stats(h, P, K, q, q, q, q, q, None),
    }


def test_population_entry_points_refuse_without_a_handle_or_a_blob(native):
    pop = _pop_record(native)
    for name, call in _calls(native, None, pop).items():
        assert call() == -1, name                                  # SSG_ERR_BAD_ARG without a handle
    h = _handle(native, 64, bound=False)
    try:
        for name, call in _calls(native, h, pop).items():
            assert call() == -3, name                              # SSG_ERR_NOT_BOUND without a bound blob
    finally:
        native.lib().ssg_destroy(h)


def test_population_refusal_matrix_before_any_device_work(native):
    """With a (host-recorded) blob, every bad record or argument is SSG_ERR_BAD_ARG — judged on the host, before the device is asked for
    anything, so this runs without one."""
    L = native.lib()
    h = _handle(native, 1000, bound=True)
    try:
        good = _pop_record(native, P=4)
        bad_records = {
            "P = 0": _pop_record(native, P=0), "P = 257": _pop_record(native, P=257), "n_envs % P": _pop_record(native, P=3),
            "hidden": _pop_record(native, H=40), "layers": _pop_record(native, L=3), "actions": _pop_record(native, A=5),
            "obs_dim": _pop_record(native, D=31), "params": _pop_record(native, params=0), "scale": _pop_record(native, scale=0),
        }
        short = _pop_record(native)
        short.struct_size -= 8
        bad_records["struct_size"] = short
        for what, rec in bad_records.items():
            for name, call in _calls(native, h, rec).items():
                if name == "episode_stats":
                    continue                                        # (takes the member count alone)
                assert call() == -1, (what, name)
        for name, call in _calls(native, h, None).items():
            if name != "episode_stats":
                assert call() == -1, ("NULL record", name)
        pr, q = C.byref(good), C.c_void_p(0x30000)
        # member counts of the statistics call
        for P in (0, 257, 3):
            assert L.ssg_pop_episode_stats(h, P, 4, q, q, q, q, q, None) == -1, P
        assert L.ssg_pop_episode_stats(h, 4, 0, q, q, q, q, q, None) == -1
        assert L.ssg_pop_episode_stats(h, 4, 4, q, None, q, q, q, None) == -1
        # NULL required pointers, K < 1, a stride below n_envs, a workspace too small / misaligned / NULL, too few table steps
        assert L.ssg_pop_act(h, pr, None, None, 0, 0, q, q, q, None, None) == -1
        assert L.ssg_pop_act(h, pr, q, None, 0, 0, q, None, q, None, None) == -1
        assert L.ssg_pop_rollout(h, pr, 0, None, 0, 0, q, q, q, q, None, q, q, None, None, 1000, None) == -1
        assert L.ssg_pop_rollout(h, pr, 4, None, 0, 0, q, q, q, q, None, q, q, None, None, 999, None) == -1
        assert L.ssg_pop_rollout(h, pr, 4, None, 0, 0, q, q, q, q, None, None, q, None, None, 1000, None) == -1
        assert L.ssg_pop_gae(h, pr, None, 4, q, q, q, q, q, q, q, 1 << 40, None) == -1
        assert L.ssg_pop_gae(h, pr, q, 0, q, q, q, q, q, q, q, 1 << 40, None) == -1
        assert L.ssg_pop_gae(h, pr, q, 4, q, q, q, q, q, q, q, 4096, None) == -1 and b"workspace" in L.ssg_last_error(h)
        assert L.ssg_pop_gae(h, pr, q, 4, q, q, q, q, q, q, None, 1 << 40, None) == -1
        assert L.ssg_pop_gae(h, pr, q, 4, q, q, q, q, q, q, C.c_void_p(0x30010), 1 << 40, None) == -1
        assert L.ssg_pop_update(h, pr, q, 8, 0, q, q, q, q, q, q, 2, 4, q, None, q, 1 << 40, None) == -1
        assert L.ssg_pop_update(h, pr, q, 8, 4, q, q, q, q, q, q, 0, 4, q, None, q, 1 << 40, None) == -1
        assert L.ssg_pop_update(h, pr, q, 8, 4, q, q, q, q, q, q, 2, 0, q, None, q, 1 << 40, None) == -1
        assert L.ssg_pop_update(h, pr, q, 8, 4, q, q, q, q, q, None, 2, 4, q, None, q, 1 << 40, None) == -1
        assert L.ssg_pop_update(h, pr, q, 8, 4, q, q, q, q, q, q, 2, 4, None, None, q, 1 << 40, None) == -1
        assert L.ssg_pop_update(h, pr, q, 7, 4, q, q, q, q, q, q, 2, 4, q, None, q, 1 << 40, None) == -1 and b"Adam steps" in L.ssg_last_error(h)
        assert L.ssg_pop_update(h, pr, q, 8, 4, q, q, q, q, q, q, 2, 4, q, None, q, 4096, None) == -1 and b"workspace" in L.ssg_last_error(h)
        # exploit: out of range, a chained source (1 <- 2 while 2 <- 3), NULL
        ok = (C.c_int32 * 4)(0, 3, 3, 3)
        for bad in ((0, 1, 2, 4), (0, -1, 2, 3), (0, 2, 3, 3), (1, 0, 2, 3)):
            assert L.ssg_pop_exploit(h, pr, (C.c_int32 * 4)(*bad), q, None) == -1, bad
        assert b"chained" in L.ssg_last_error(h)
        assert L.ssg_pop_exploit(h, pr, None, q, None) == -1 and L.ssg_pop_exploit(h, pr, ok, None, None) == -1
        # (no VALID call is made here: with a device present it would be launched on these made-up addresses)
    finally:
        L.ssg_destroy(h)


def test_pop_workspace_grows_with_members_and_rejects_bad_shapes(native):
    L = native.lib()
    nb = {}
    for P in (1, 2, 16, 120):
        out = C.c_size_t()
        pop = _pop_record(native, P=P)
        assert L.ssg_pop_workspace_nbytes(C.byref(pop), 32 * 512, 4096, C.byref(out)) == 0
        nb[P] = out.value
    plen = 64 * 32 + 64 + 64 * 64 + 64 + 3 * 64 + 3 + 64 + 1
    for P, v in nb.items():
        assert v >= 4096 + P * 64 * (plen + 4) * 4, P            # 64 gradient workgroups per member at 4096 samples
    assert nb[1] < nb[2] < nb[16] < nb[120]
    single, pol = C.c_size_t(), native.Policy()
    pol.struct_size = C.sizeof(native.Policy)
    pol.obs_dim, pol.hidden, pol.n_hidden_layers, pol.n_actions, pol.activation = 32, 64, 2, 3, native.POLICY_TANH
    assert L.ssg_ppo_workspace_nbytes(C.byref(pol), 32 * 512, 4096, C.byref(single)) == 0
    assert nb[16] - 4096 == 16 * (single.value - 256)            # P times the single policy's slots
    out = C.c_size_t()
    good = _pop_record(native)
    assert L.ssg_pop_workspace_nbytes(C.byref(good), 0, 1, C.byref(out)) == -1
    assert L.ssg_pop_workspace_nbytes(C.byref(good), 1, 0, C.byref(out)) == -1
    assert L.ssg_pop_workspace_nbytes(C.byref(good), 1, 1, None) == -1
    assert L.ssg_pop_workspace_nbytes(None, 1, 1, C.byref(out)) == -1
    for bad in (_pop_record(native, P=0), _pop_record(native, P=257), _pop_record(native, H=40), _pop_record(native, A=1)):
        assert L.ssg_pop_workspace_nbytes(C.byref(bad), 1, 1, C.byref(out)) == -1


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def test_pack_hparams_is_the_single_policy_rounding(native):
    """The table rows are the doubles loss_row / adam_args form for one policy's launches, rounded once to f32."""
    L = native.lib()
    P, steps, step0 = 3, 5, 7
    hp = _hparams(native, P, lam=[0.9, 0.95, 1.0], clip=[0.1, 0.2, 0.3], lr=[1e-3, 5e-4, 1e-5], beta1=[0.9, 0.3, 0.0],
                  ent_coef=[0.0, 0.01, 0.02])
    n = native.pop_table_floats(P, steps)
    buf = (C.c_float * n)()
    assert L.ssg_pop_pack_hparams(P, hp, step0, steps, buf, n) == 0
    for m in range(P):
        h = hp[m]
        want = [1.0 - h.clip, 1.0 + h.clip, h.clip, h.vf_coef, h.ent_coef, h.adv_eps, h.gamma, h.gamma * h.lam]
        assert list(buf[m * 8: m * 8 + 8]) == [_f32(x) for x in want], m
        for j in range(steps):
            t = step0 + 1 + j
            bc1, bc2 = 1.0 - h.beta1 ** t, 1.0 - h.beta2 ** t
            w1 = _f32(1.0 - h.beta1)
            want = [w1, _f32(1.0 - w1), _f32(h.beta2), _f32(1.0 - h.beta2), _f32(math.sqrt(bc2)), _f32(h.eps), _f32(-(h.lr / bc1)), 0.0]
            row = list(buf[(1 + j) * P * 8 + m * 8: (1 + j) * P * 8 + m * 8 + 8])
            assert row == want, (m, j, row, want)
    assert L.ssg_pop_pack_hparams(P, hp, 0, 0, buf, P * 8) == 0       # no Adam rows: GAE alone
    assert L.ssg_pop_pack_hparams(P, hp, step0, steps, buf, n - 1) == -1
    assert L.ssg_pop_pack_hparams(0, hp, 0, 0, buf, n) == -1 and L.ssg_pop_pack_hparams(257, hp, 0, 0, buf, n) == -1
    assert L.ssg_pop_pack_hparams(P, None, 0, 0, buf, n) == -1 and L.ssg_pop_pack_hparams(P, hp, 0, 0, None, n) == -1
    assert L.ssg_pop_pack_hparams(P, hp, -1, 0, buf, n) == -1 and L.ssg_pop_pack_hparams(P, hp, 0, -1, buf, n) == -1
    hp[1].clip = 0.0
    assert L.ssg_pop_pack_hparams(P, hp, 0, 0, buf, n) == -1


# ------------------------------------------------------------------------------------------------------------------------------------
# the scheduler
# ------------------------------------------------------------------------------------------------------------------------------------
LRS = [1e-3, 5e-4, 1e-4, 5e-5, 1e-5]


def _start(P):
    return {"lambda": [0.95] * P, "clip_param": [0.2] * P, "lr": [5e-4] * P, "ent_coef": [0.01 * (m + 1) for m in range(P)]}


def _score_table(P, rounds):
    import random
    rng = random.Random(1234)
    return [[rng.uniform(-5.0, 5.0) for _ in range(P)] for _ in range(rounds)]


def test_pbt_scheduler_quantiles_sources_and_mutations():
    from ship_sim_gym_amd.population import PBTScheduler
    P, rounds = 16, 200
    sched = PBTScheduler(P, seed=3, perturbation_interval=2)
    assert [sched.due(u) for u in range(0, 7)] == [False, False, True, False, True, False, True]
    hp = _start(P)
    resampled = {"lambda": [], "clip_param": [], "lr": []}
    kinds = set()
    for scores in _score_table(P, rounds):
        order = sorted(range(P), key=lambda m: (scores[m], m))
        bottom, top = order[:4], order[-4:]
        src, new, events = sched.perturb(scores, hp)
        dest = [m for m in range(P) if src[m] != m]
        assert sorted(dest) == sorted(bottom)                              # exactly the bottom quarter get a source
        assert all(src[m] in top for m in dest)                            # every source is in the top quarter
        assert all(src[src[m]] == src[m] for m in range(P))                # no source is a destination
        assert [e["member"] for e in events] == bottom and [e["source"] for e in events] == [src[m] for m in bottom]
        for m in range(P):
            if m not in dest:
                assert all(new[k][m] == hp[k][m] for k in hp), m          # everyone else keeps every value
        for e in events:
            m, s = e["member"], e["source"]
            assert new["ent_coef"][m] == hp["ent_coef"][s]                 # an unmutated key is the source's
            assert [k for k, _, _, _ in e["mutations"]] == ["lambda", "clip_param", "lr"]
            for key, kind, old, val in e["mutations"]:
                kinds.add((key, kind))
                assert old == hp[key][s] and new[key][m] == val
                if kind == "resample":
                    resampled[key].append(val)
                elif key == "lr":                                          # a neighbouring list entry (ray clamps at the ends)
                    i = LRS.index(old)
                    assert val in (LRS[max(0, i - 1)], LRS[min(len(LRS) - 1, i + 1)])
                else:
                    assert val in (old * 1.2, old * 0.8)                   # exactly 1.2x / 0.8x
        hp = new
    assert kinds == {(k, kind) for k in ("lambda", "clip_param", "lr") for kind in ("resample", "perturb")}
    assert len(resampled["lambda"]) > 100 and all(0.9 <= v <= 1.0 for v in resampled["lambda"])
    assert len(resampled["clip_param"]) > 100 and all(0.01 <= v <= 0.5 for v in resampled["clip_param"])
    assert set(resampled["lr"]) == set(LRS) and all(v in LRS for v in hp["lr"])
    # the share of resamples is the reference's 0.33 (3 keys x 4 members x 200 rounds = 2400 draws: 3 sigma is 0.029)
    total = rounds * 4 * 3
    assert abs(sum(len(v) for v in resampled.values()) / total - 0.33) < 0.03


def test_pbt_scheduler_is_reproducible_and_handles_small_populations():
    from ship_sim_gym_amd.population import PBTScheduler
    P = 12
    a, b, c = PBTScheduler(P, seed=5), PBTScheduler(P, seed=5), PBTScheduler(P, seed=6)
    ha, hb, hc = _start(P), _start(P), _start(P)
    differs = False
    for scores in _score_table(P, 50):
        ra, rb, rc = a.perturb(scores, ha), b.perturb(scores, hb), c.perturb(scores, hc)
        assert ra == rb                                                     # same seed: same sources, values and events
        differs = differs or ra[:2] != rc[:2]
        ha, hb, hc = ra[1], rb[1], rc[1]
    assert differs                                                          # (and the seed matters)
    # ceil(P / 4) members at each end, never more than half; one member: nothing to exploit
    for P, k in ((1, 0), (2, 1), (3, 1), (4, 1), (5, 2), (8, 2), (9, 3), (120, 30)):
        s = PBTScheduler(P, seed=0)
        bottom, top = s.quantiles(list(range(P)))
        assert len(bottom) == len(top) == k and not set(bottom) & set(top), P
        assert bottom == list(range(k)) and top == list(range(P - k, P))
    s = PBTScheduler(4, seed=0)
    assert s.quantiles([1.0, 1.0, 1.0, 1.0]) == ([0], [3])                  # ties: by index
    with pytest.raises(ValueError):
        s.perturb([1.0, 2.0], _start(4))
    with pytest.raises(ValueError):
        s.perturb([1.0] * 4, {"lambda": [0.95] * 4})
    with pytest.raises(ValueError):
        PBTScheduler(4, perturbation_interval=0)


def test_scheduler_module_imports_without_torch_or_ray():
    """population.py's import (the scheduler's home) pulls in neither torch nor ray: checked in a fresh interpreter."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); sys.modules['ray'] = None\n"
            "from ship_sim_gym_amd.population import PBTScheduler\n"
            "s = PBTScheduler(4, seed=0)\n"
            "print(s.perturb([0, 1, 2, 3], {'lambda': [0.95] * 4, 'clip_param': [0.2] * 4, 'lr': [5e-4] * 4})[0])\n"
            "assert 'torch' not in sys.modules, 'the scheduler imported torch'\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "[3, 1, 2, 3]"


def test_pbt_trainer_parses_its_arguments_and_imports_without_ray(monkeypatch):
    monkeypatch.setitem(sys.modules, "ray", None)                           # import ray -> ImportError
    mod = load_script("train/pbt_native.py")
    a = mod.parse_args([])
    assert (a.members, a.envs_per_member, a.horizon, a.perturb_every, a.seed, a.pbt, a.lrs) == (16, 512, 32, 5, 0, True, None)
    a = mod.parse_args(["--members", "4", "--envs-per-member", "512", "--updates", "3", "--horizon", "16", "--perturb-every", "1",
                        "--seed", "9"])
    assert (a.members, a.envs_per_member, a.updates, a.horizon, a.perturb_every, a.seed) == (4, 512, 3, 16, 1, 9)
    a = mod.parse_args(["--lrs", "1e-3,1e-4,1e-5", "--no-pbt"])            # the SB script's sweep: three members, no exploit
    assert a.members == 3 and a.lrs == [1e-3, 1e-4, 1e-5] and a.pbt is False
    for bad in (["--members", "0"], ["--perturb-every", "0"], ["--horizon", "0"], ["--lrs", "fast"]):
        with pytest.raises((SystemExit, ValueError)):
            mod.parse_args(bad)
    assert mod.INITIAL == {"lambda": 0.95, "clip_param": 0.2, "lr": 5e-4}   # the reference experiment's starting point
    assert "UPDATES" in mod.make_arg_parser().format_help()                 # the interval is counted in updates, and says so
    doc = open(os.path.join(ROOT, "train", "rllib_pbt.py")).read()
    assert "pbt_native.py" in doc.split('"""')[1]                           # the ray script points at the one that runs here
