"""CPU checks of the job-wide observation filter (include/shipsim.h "Job-wide observation filter"; ship_sim_gym_amd/obs_filter.py,
``ObsFilter(job=True)``): the four entry points as header, binding and library see them, every refusal by code and text (the library
judges on the host; no call here carries arguments that would pass), ``merge_rows_reference`` against long-double statistics of the
concatenated data, its exact cases, the state_dict round trip with and without ``job``, and the trainer's flag.  Nothing here launches a
kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpu_support import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
Q = 0x30000  # a plausible device address (256-byte aligned; never dereferenced on the host)
NEW = {"ssg_set_obs_filter_buffer": 2, "ssg_get_obs_filter_buffer": 2, "ssg_obs_filter_update_buffered": 5, "ssg_obs_filter_merge_rows": 6}


def test_header_binding_and_library_agree(native):
    text = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = native.lib()
    for name, n_args in NEW.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert name in native.EXPORTS and hasattr(L, name) and len(getattr(L, name).argtypes) == n_args, name
    assert "Job-wide observation filter (ABI 9 addition)" in text and native.ABI_VERSION == 9
    # the record and the plain update are what they were
    assert C.sizeof(native.ObsFilterRecord) == 56 and len(L.ssg_obs_filter_update.argtypes) == 4
    assert int(re.search(r"#define\s+SSG_DP_MAX_SHARDS\s+(\d+)", text).group(1)) == native.DP_MAX_SHARDS == 64


def _handle(native, n_envs=1000, beams=8, history=2, bound=False):
    c = native.default_config()
    c.n_envs, c.n_beams, c.history = n_envs, beams, history
    h = C.c_void_p()
    native.check(native.lib().ssg_create(C.byref(c), C.byref(h)))
    if bound:
        native.check(native.lib().ssg_bind_state(h, C.c_void_p(Q)), h)
    return h


def _record(native, n_envs=1000, D=28, P=1, **kw):
    r = native.ObsFilterRecord()
    r.struct_size = C.sizeof(native.ObsFilterRecord)
    r.flags, r.n_members, r.obs_dim, r.clip, r.eps = native.FILTER_UPDATE, P, D, 10.0, 1e-8
    r.dev_state, r.dev_workspace = 0x10000, 0x20000
    need = C.c_size_t()
    native.check(native.lib().ssg_obs_filter_workspace_nbytes(n_envs, D, max(1, min(P, 256)), C.byref(need)))
    r.workspace_nbytes = need.value
    for k, v in kw.items():
        setattr(r, k, v)
    return r


BLOCK = 4 * 28 * 8  # bytes of one member's state block at D = 28


def _bound_buffer(native, h):
    out = C.c_void_p(1)
    assert native.lib().ssg_get_obs_filter_buffer(h, C.byref(out)) == 0
    return out.value


def test_buffer_binding_and_its_refusals(native):
    L = native.lib()
    h = _handle(native)
    err = lambda: L.ssg_last_error(h)  # noqa: E731
    assert L.ssg_set_obs_filter_buffer(None, C.c_void_p(Q)) == -1 and b"NULL handle" in L.ssg_last_error(None)
    assert L.ssg_get_obs_filter_buffer(None, C.byref(C.c_void_p())) == -1 and L.ssg_get_obs_filter_buffer(h, None) == -1
    assert _bound_buffer(native, h) is None
    # no filter bound: neither a buffer nor NULL
    for buf in (C.c_void_p(Q), None):
        assert L.ssg_set_obs_filter_buffer(h, buf) == -1 and b"no observation filter is bound" in err()
    good = _record(native)
    assert L.ssg_set_obs_filter(h, C.byref(good)) == 0 and _bound_buffer(native, h) is None
    assert L.ssg_set_obs_filter_buffer(h, C.c_void_p(Q)) == 0 and _bound_buffer(native, h) == Q
    # refusals leave the binding: misaligned; any overlap with the record's dev_state block
    for bad, word in ((Q + 4, b"8-byte aligned"), (0x10000, b"overlaps"), (0x10000 + BLOCK - 8, b"overlaps"), (0x10000 - BLOCK + 8, b"overlaps")):
        assert L.ssg_set_obs_filter_buffer(h, C.c_void_p(bad)) == -1 and word in err() and b"ssg_set_obs_filter_buffer" in err(), hex(bad)
        assert _bound_buffer(native, h) == Q
    for fine in (0x10000 + BLOCK, 0x10000 - BLOCK):  # (the blocks touch, they do not overlap)
        assert L.ssg_set_obs_filter_buffer(h, C.c_void_p(fine)) == 0 and _bound_buffer(native, h) == fine
    assert L.ssg_set_obs_filter_buffer(h, C.c_void_p(Q)) == 0
    # a refused ssg_set_obs_filter leaves the record and the buffer; one that succeeds, bind or unbind, drops the buffer
    assert L.ssg_set_obs_filter(h, C.byref(_record(native, obs_dim=27))) == -1 and _bound_buffer(native, h) == Q
    assert L.ssg_set_obs_filter(h, C.byref(good)) == 0 and _bound_buffer(native, h) is None
    assert L.ssg_set_obs_filter_buffer(h, C.c_void_p(Q)) == 0 and L.ssg_set_obs_filter_buffer(h, None) == 0 and _bound_buffer(native, h) is None
    assert L.ssg_set_obs_filter_buffer(h, C.c_void_p(Q)) == 0 and L.ssg_set_obs_filter(h, None) == 0 and _bound_buffer(native, h) is None
    got = native.ObsFilterRecord()
    assert L.ssg_get_obs_filter(h, C.byref(got)) == 0 and got.struct_size == 0
    L.ssg_destroy(h)


def test_update_buffered_refusals(native):
    """No handle, no blob, then everything the host can judge: SSG_ERR_BAD_ARG with the entry point's name in the text."""
    L = native.lib()
    q, good = C.c_void_p(Q), _record(native)
    assert L.ssg_obs_filter_update_buffered(None, C.byref(good), q, q, None) == -1
    h = _handle(native)
    assert L.ssg_obs_filter_update_buffered(h, C.byref(good), q, q, None) == -3 and b"ssg_bind_state" in L.ssg_last_error(h)
    L.ssg_destroy(h)
    h = _handle(native, bound=True)
    err = lambda: L.ssg_last_error(h)  # noqa: E731
    assert L.ssg_obs_filter_update_buffered(h, None, q, q, None) == -1 and b"ssg_obs_filter_update_buffered: NULL ssg_obs_filter" in err()
    for kw in (dict(struct_size=8), dict(obs_dim=27), dict(n_members=0), dict(dev_state=None), dict(flags=2), dict(eps=float("nan")),
               dict(workspace_nbytes=good.workspace_nbytes - 1)):
        assert L.ssg_obs_filter_update_buffered(h, C.byref(_record(native, **kw)), q, q, None) == -1, kw
        assert b"ssg_obs_filter_update_buffered" in err(), kw
    for buf, word in ((None, b"NULL dev_buffer"), (Q + 4, b"8-byte aligned"), (0x10000, b"overlaps"), (0x10000 + BLOCK - 8, b"overlaps")):
        assert L.ssg_obs_filter_update_buffered(h, C.byref(good), C.c_void_p(buf) if buf else None, q, None) == -1 and word in err(), buf
    assert L.ssg_obs_filter_update_buffered(h, C.byref(good), q, None, None) == -1 and b"NULL dev_obs" in err()
    assert L.ssg_obs_filter_update_buffered(h, C.byref(_record(native, P=3)), q, q, None) == -1 and b"equal member slices" in err()
    # the plain update's texts are what they were
    assert L.ssg_obs_filter_update(h, None, q, None) == -1 and b"ssg_obs_filter_update: NULL ssg_obs_filter" in err()
    assert L.ssg_obs_filter_update(h, C.byref(good), None, None) == -1 and b"ssg_obs_filter_update: NULL dev_obs" in err()
    L.ssg_destroy(h)


def test_merge_rows_refusals(native):
    L = native.lib()
    q, r0, good = C.c_void_p(Q), C.c_void_p(0x50000), _record(native)
    assert L.ssg_obs_filter_merge_rows(None, C.byref(good), q, r0, 2, None) == -1
    h = _handle(native)
    assert L.ssg_obs_filter_merge_rows(h, C.byref(good), q, r0, 2, None) == -3 and b"ssg_bind_state" in L.ssg_last_error(h)
    L.ssg_destroy(h)
    h = _handle(native, bound=True)
    err = lambda: L.ssg_last_error(h)  # noqa: E731
    assert L.ssg_obs_filter_merge_rows(h, None, q, r0, 2, None) == -1 and b"ssg_obs_filter_merge_rows: NULL ssg_obs_filter" in err()
    for kw in (dict(struct_size=8), dict(obs_dim=27), dict(n_members=257), dict(dev_state=None), dict(dev_workspace=None), dict(clip=-1.0)):
        assert L.ssg_obs_filter_merge_rows(h, C.byref(_record(native, **kw)), q, r0, 2, None) == -1 and b"ssg_obs_filter_merge_rows" in err(), kw
    for base, rows in ((None, r0), (q, None)):
        assert L.ssg_obs_filter_merge_rows(h, C.byref(good), base, rows, 2, None) == -1 and b"NULL dev_base or dev_rows" in err()
    for base, rows in ((C.c_void_p(Q + 4), r0), (q, C.c_void_p(0x50004))):
        assert L.ssg_obs_filter_merge_rows(h, C.byref(good), base, rows, 2, None) == -1 and b"8-byte aligned" in err()
    for n_rows in (0, -1, native.DP_MAX_SHARDS + 1):
        assert L.ssg_obs_filter_merge_rows(h, C.byref(good), q, r0, n_rows, None) == -1 and b"1..SSG_DP_MAX_SHARDS" in err(), n_rows
    # dev_base must not alias the state; nor may any of the n_rows blocks of dev_rows
    for base in (0x10000, 0x10000 + BLOCK - 8, 0x10000 - BLOCK + 8):
        assert L.ssg_obs_filter_merge_rows(h, C.byref(good), C.c_void_p(base), r0, 2, None) == -1 and b"dev_base overlaps" in err(), hex(base)
    for rows, n_rows in ((0x10000, 1), (0x10000 - 3 * BLOCK + 8, 3), (0x10000 + BLOCK - 8, 64)):
        assert L.ssg_obs_filter_merge_rows(h, C.byref(good), q, C.c_void_p(rows), n_rows, None) == -1 and b"dev_rows overlaps" in err(), hex(rows)
    L.ssg_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------------------
# merge_rows_reference
# ------------------------------------------------------------------------------------------------------------------------------------
def _columns(rng, n):
    """tests/test_obs_filter.py's columns: positions, rudder, heading, lidar, the two constants, the history half's -1 / value mixture."""
    mix = np.where(rng.random_sample(n) < 0.5, -1.0, rng.uniform(0.0, 1000.0, n))
    return np.stack([rng.uniform(0.0, 1000.0, n), rng.uniform(-35.0, 35.0, n), rng.uniform(-3.2, 3.2, n), rng.uniform(0.0, 150.0, n),
                     np.full(n, -1.0), np.full(n, 150.0), mix], axis=1).reshape(n, 7)


CONST = (4, 5)
SHARDS = {1: [(700,), (0,)], 2: [(300, 1), (0, 513), (257, 0)], 3: [(1, 0, 2049), (64, 300, 7)],
          8: [(5, 0, 300, 0, 1, 769, 2, 0), (0, 0, 0, 0, 0, 0, 0, 40), (256, 255, 257, 1, 2, 3, 4, 5)]}


def _block(x):
    from ship_sim_gym_amd.obs_filter import merge_reference
    return merge_reference(np.zeros((4, 7)), x) if len(x) else np.zeros((4, 7))


@pytest.mark.parametrize("W", sorted(SHARDS))
@pytest.mark.parametrize("base_rows", [0, 1000])
def test_merge_rows_reference_against_long_double(W, base_rows):
    """The bound of tests/test_obs_filter.py::test_merge_reference_against_long_double, |mean - ref| <= 16 T u max|column| and
    |M2 - ref| <= 64 T u ref against the two-pass long-double statistics of all rows, with T = the non-empty blocks (the base and
    the shards): each block is one merge_reference of its rows into an empty state, and T blocks meet in T - 1 merges — no more
    operations than the T successive merges that test covers.  Unequal shards, empty shards, an empty base; constant columns exact."""
    from ship_sim_gym_amd.obs_filter import merge_rows_reference
    for case, sizes in enumerate(SHARDS[W]):
        rng = np.random.RandomState(100 * W + 10 * case + (base_rows > 0))
        data = [_columns(rng, n) for n in (base_rows,) + tuple(sizes)]
        got = merge_rows_reference(_block(data[0]), np.stack([_block(x) for x in data[1:]]))
        seen = np.concatenate(data)
        total, T = len(seen), sum(1 for x in data if len(x))
        assert got[3, 0] == total and not got[3, 1:].any()
        if total == 0:
            assert not got[:2].any() and (got[2] == 1.0).all()
            continue
        ld = seen.astype(np.longdouble)
        mu = ld.sum(axis=0) / np.longdouble(total)
        m2 = ((ld - mu) ** 2).sum(axis=0)
        for c in range(7):
            assert abs(np.longdouble(got[0, c]) - mu[c]) <= 16 * T * U * np.abs(seen[:, c]).max(), (sizes, c)
            assert abs(np.longdouble(got[1, c]) - m2[c]) <= 64 * T * U * m2[c], (sizes, c, got[1, c], m2[c])
        for c in CONST:  # a constant column keeps its mean bit for bit and M2 == 0.0
            assert got[0, c] == seen[0, c] and got[1, c] == 0.0, (sizes, c)
        want_den = np.sqrt(got[1] / (total - 1.0)) + 1e-8 if total >= 2 else np.ones(7)
        np.testing.assert_array_equal(got[2], want_den)


def test_merge_rows_reference_exact_cases():
    from ship_sim_gym_amd.obs_filter import merge_reference, merge_rows_reference
    rng = np.random.RandomState(7)
    empty = np.zeros((4, 7))
    # all-empty rows on an empty base: count 0, denom 1.0
    got = merge_rows_reference(empty, np.zeros((8, 4, 7)))
    assert got[3, 0] == 0.0 and not got[:2].any() and (got[2] == 1.0).all() and not got[3].any()
    # empty rows leave the base's statistics as they are; denom is formed again with the call's eps
    base = _block(_columns(rng, 300))
    got = merge_rows_reference(base, np.zeros((3, 4, 7)), eps=0.5)
    assert np.array_equal(got[[0, 1, 3]], base[[0, 1, 3]]) and np.array_equal(got[2], np.sqrt(base[1] / 299.0) + 0.5)
    # an empty base takes the first non-empty row as it is, and one row of one observation has denom 1.0
    one = _block(_columns(rng, 1))
    got = merge_rows_reference(empty, np.stack([empty, one, empty]))
    assert np.array_equal(got[[0, 1, 3]], one[[0, 1, 3]]) and (got[2] == 1.0).all() and got[3, 0] == 1.0
    # the association is the header's: ((base + r0) + r1), every product and sum on its own
    r0, r1 = _block(_columns(rng, 257)), _block(_columns(rng, 40))
    got = merge_rows_reference(base, np.stack([r0, r1]))
    n, mean, m2 = base[3, 0], base[0], base[1]
    for r in (r0, r1):
        nb = r[3, 0]
        n2 = n + nb
        w, delta = nb / n2, r[0] - mean
        mean, m2, n = mean + delta * w, (m2 + r[1]) + (delta * delta) * (n * w), n2
    assert got[3, 0] == n == 597.0 and np.array_equal(got[0], mean) and np.array_equal(got[1], m2)
    assert not np.array_equal(got[0], merge_rows_reference(base, np.stack([r1, r0]))[0])      # (the order shows)
    # one rank: base (+) buffer is the same statistics as the running state, not the same bits (no parity is claimed)
    a, b = _columns(rng, 300), _columns(rng, 300)
    running = merge_reference(merge_reference(base, a), b)
    job = merge_rows_reference(base, merge_reference(_block(a), b)[None])
    assert job[3, 0] == running[3, 0] and np.allclose(job[:3], running[:3], rtol=1e-12, atol=0.0)
    for bad in ((np.zeros((3, 7)), np.zeros((1, 4, 7))), (empty, np.zeros((4, 7))), (empty, np.zeros((0, 4, 7))), (empty, np.zeros((1, 4, 8)))):
        with pytest.raises(ValueError):
            merge_rows_reference(*bad)


# ------------------------------------------------------------------------------------------------------------------------------------
# the Python filter on the CPU
# ------------------------------------------------------------------------------------------------------------------------------------
class _Env(object):
    """What ObsFilter reads of an env, on the CPU."""
    num_envs, states_history = 300, 7

    def __init__(self):
        import torch
        self.device = torch.device("cpu")


def test_state_dict_round_trips_with_and_without_job():
    import torch
    from ship_sim_gym_amd.obs_filter import ObsFilter
    rng = np.random.RandomState(11)
    plain, job = ObsFilter(_Env(), n_members=2), ObsFilter(_Env(), n_members=2, job=True, clip=5.0, eps=1e-6)
    assert plain.job is False and plain.buffer is None and plain.base is None
    assert sorted(plain.state_dict()) == ["clip", "eps", "n_members", "obs_dim", "state"]      # a plain filter's dict is what it was
    assert job.job and job.buffer.shape == job.base.shape == job.state.shape == (2, 4, 7) and not job.buffer.any() and not job.base.any()
    assert len({t.data_ptr() for t in (job.state, job.buffer, job.base)}) == 3
    for t in (job.state, job.buffer, job.base):
        t.copy_(torch.from_numpy(rng.random_sample((2, 4, 7))))
    sd = job.state_dict()
    assert sorted(sd) == ["base", "buffer", "clip", "eps", "n_members", "obs_dim", "state"]
    assert all(sd[k].data_ptr() != getattr(job, k).data_ptr() for k in ("state", "base", "buffer"))
    g = ObsFilter(_Env(), n_members=2, job=True).load_state_dict(sd)
    assert all(torch.equal(getattr(g, k), getattr(job, k)) for k in ("state", "base", "buffer")) and (g.clip, g.eps) == (5.0, 1e-6)
    # a plain filter (evaluation) reads a job's dict: the state alone
    p = ObsFilter(_Env(), n_members=2, update=False).load_state_dict(sd)
    assert torch.equal(p.state, job.state) and p.buffer is None and (p.clip, p.eps) == (5.0, 1e-6)
    # a job filter reads a plain dict: its state is the base, the buffer is empty
    plain.state.copy_(job.state)
    g.load_state_dict(plain.state_dict())
    assert torch.equal(g.state, job.state) and torch.equal(g.base, job.state) and not g.buffer.any()
    for bad in ({k: v for k, v in sd.items() if k != "buffer"}, {k: v for k, v in sd.items() if k != "base"}, dict(sd, base=sd["base"][:1]),
                dict(sd, buffer=sd["buffer"][:, :, :6])):
        before = [t.clone() for t in (g.state, g.base, g.buffer)]
        with pytest.raises(ValueError):
            g.load_state_dict(bad)
        assert all(torch.equal(a, b) for a, b in zip(before, (g.state, g.base, g.buffer)))
    # frozen views share the state, have no buffer and never update
    fr = job.frozen()
    assert fr.state.data_ptr() == job.state.data_ptr() and fr.buffer is None and fr.job is False and fr.to_native().flags == 0
    with pytest.raises(ValueError, match="job=True"):
        plain.merge_rows(torch.zeros((1, 2, 4, 7), dtype=torch.float64))
    for rows in (torch.zeros((2, 4, 7), dtype=torch.float64), torch.zeros((0, 2, 4, 7), dtype=torch.float64),
                 torch.zeros((65, 2, 4, 7), dtype=torch.float64), torch.zeros((1, 2, 4, 7)), torch.zeros((1, 1, 4, 7), dtype=torch.float64),
                 torch.zeros((1, 2, 4, 14), dtype=torch.float64)[..., ::2]):
        with pytest.raises(ValueError, match="merge_rows"):
            job.merge_rows(rows)


# ------------------------------------------------------------------------------------------------------------------------------------
# the trainer's flag
# ------------------------------------------------------------------------------------------------------------------------------------
def _no_env(*a, **k):
    pytest.fail("an env was built before the refusal")


def test_trainer_flag_and_its_refusals(capsys, monkeypatch):
    single = load_script("train/ppo_torch.py")
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(single, "ShipVecEnv", _no_env)
    native_flags = ["--mode", "native", "--update", "native"]
    assert single.parse_args([]).job_obs_filter is False
    for extra in ([], ["--gpus", "2"], ["--gpus", "8"]):                   # one rank or more
        assert single.parse_args(native_flags + ["--job-obs-filter"] + extra).job_obs_filter is True
    # its row is not in REQUIREMENTS, and asks for the native rollout and the device update
    assert "job_obs_filter" not in [r[0] for r in single.REQUIREMENTS]
    (row,) = single.JOB_OBS_FILTER_REQUIREMENTS
    assert row[:2] == ("job_obs_filter", "--job-obs-filter") and row[3] == ("mode", "update") and row[4] is False
    for argv, words in ((["--job-obs-filter"], ("--job-obs-filter", "--mode native")),
                        (["--mode", "native", "--job-obs-filter"], ("--job-obs-filter", "--update native")),
                        (native_flags + ["--job-obs-filter", "--obs-filter"], ("--job-obs-filter", "together with --obs-filter")),
                        # both --obs-filter refusals still fire
                        (native_flags + ["--obs-filter", "--gpus", "2"], ("--obs-filter", "more than one rank")),
                        (native_flags + ["--obs-filter", "--save-obs-filter", "f.pt", "--gpus", "2"], ("--save-obs-filter", "more than one rank")),
                        (native_flags + ["--job-obs-filter", "--save-obs-filter", "f.pt"], ("--save-obs-filter", "--obs-filter")),
                        (native_flags + ["--job-obs-filter", "--norm-reward", "--gpus", "2"], ("--norm-reward", "more than one rank"))):
        with pytest.raises(SystemExit) as ex:
            single.parse_args(argv)
        err = capsys.readouterr().err
        assert ex.value.code not in (0, None) and all(w in err for w in words), (argv, err)
    for kw, words in ((dict(job_obs_filter=True), ("job_obs_filter", "mode='native'")),
                      (dict(job_obs_filter=True, mode="native"), ("job_obs_filter", "update='native'")),
                      (dict(job_obs_filter=True, obs_filter=True, mode="native", update="native"), ("job_obs_filter", "together with obs_filter"))):
        with pytest.raises(ValueError) as ex:
            single.train(envs=8, updates=1, log=None, **kw)
        assert all(w in str(ex.value) for w in words), (kw, str(ex.value))
    monkeypatch.setattr(single, "job_ranks", lambda: (1, 2))
    for kw, name in ((dict(obs_filter=True), "obs_filter"), (dict(obs_filter=True, save_obs_filter="f.pt"), "save_obs_filter")):
        with pytest.raises(ValueError, match=name) as ex:
            single.train(envs=8, updates=1, log=None, mode="native", update="native", **kw)
        assert "more than one rank" in str(ex.value)
    # the flag is part of a run's configuration, and a resumed run of it needs the filter's section
    assert single.run_config(job_obs_filter=True)["job_obs_filter"] is True and single.run_config()["job_obs_filter"] is False
    assert "job_obs_filter" not in single.CONFIG_EXEMPT
    assert "--job-obs-filter" in single.make_arg_parser().format_help()
