"""The rgb_array renderer (ssg_render / render_kernel, ShipVecEnv.get_screen / render / get_images, EnvHandle.render) pixel by pixel
against the exact rasteriser of tests/render_scenes.py.

One handle per (n_ships, n_beams, n_goals) holds its scenes, one per env, each on its own bank record; the scene's state is written
through field() (F_X, F_Y, F_ANGLE, F_GOAL_MASK, and F_TRAFFIC and F_GOAL_BODIES in config 4).  Per frame every CLEAR pixel equals its
expected colour and every BAND pixel is one of its candidates.  Further: no byte outside the frame's buffer is written and every byte
inside is, at every frame size; an env's frame does not depend on its neighbours or on the stream; a render leaves the state blob
bitwise alone and the stepping after it unchanged; frames rendered from the state that real steps leave behind; the Python surface.
"""
import collections
import ctypes as C

import numpy as np
import pytest

from gpu_support import same_columns, torch_cuda  # noqa: F401

import render_scenes as RS

pytestmark = pytest.mark.gpu

GUARD = 4096


class Handle:
    """a ShipVecEnv holding the given scenes, one per env, env e on bank record e"""

    def __init__(self, torch, N, scenes):
        from ship_sim_gym_amd import config as cfgmod
        from ship_sim_gym_amd.vec_env import ShipVecEnv
        ns, nb, ng = scenes[0].key()
        assert all(s.key() == (ns, nb, ng) for s in scenes)
        keep = cfgmod.N_GOALS
        cfgmod.N_GOALS = ng
        try:
            bank = np.stack([s.record() for s in scenes])
            self.vec = ShipVecEnv(len(scenes), bank=bank, n_beams=nb, n_ships=ns, auto_reset=False)
        finally:
            cfgmod.N_GOALS = keep
        assert self.vec.cfg.n_goals == ng
        self.scenes, vec, dev = scenes, self.vec, self.vec.device
        vec.reset_tensor(map_ids=torch.arange(len(scenes), dtype=torch.int32, device=dev))
        pose = torch.tensor([s.pose for s in scenes], dtype=torch.float64, device=dev)
        vec.field(N.F_X)[:] = pose[:, 0]
        vec.field(N.F_Y)[:] = pose[:, 1]
        vec.field(N.F_ANGLE)[:] = pose[:, 2]
        vec.field(N.F_GOAL_MASK)[:] = torch.tensor([s.mask for s in scenes], dtype=torch.uint8, device=dev)
        if ns > 1:
            T, G = vec.field(N.F_TRAFFIC), vec.field(N.F_GOAL_BODIES)
            t = T.cpu().numpy().copy()
            g = G.cpu().numpy().copy()
            for e, s in enumerate(scenes):
                for k in range(3):
                    t[9 * k: 9 * k + 9, e] = 0.0
                    t[9 * k: 9 * k + 3, e] = s.traffic[k]
                for j in range(ng):
                    g[8 * j: 8 * j + 8, e] = 0.0
                    g[8 * j: 8 * j + 2, e] = s.bodies[j]
            T.copy_(torch.from_numpy(t).to(dev))
            G.copy_(torch.from_numpy(g).to(dev))
            vec.wake_dynamics()

    def frame(self, e):
        s = self.scenes[e]
        return self.vec.get_screen(e, width=s.width, height=s.height, debug=s.debug).cpu().numpy()


@pytest.fixture(scope="module")
def built(oracle):
    scenes = RS.build_scenes(oracle)
    return scenes, [RS.render(oracle, s) for s in scenes]


@pytest.fixture(scope="module")
def handles(torch_cuda, native, built):
    scenes, frames = built
    by = collections.defaultdict(list)
    for i, s in enumerate(scenes):
        by[s.key()].append(i)
    out = {key: (Handle(torch_cuda, native, [scenes[i] for i in idx]), idx) for key, idx in by.items()}
    yield out
    for h, _ in out.values():
        h.vec.close()


def _report(bad_clear, bad_band):
    return "%d wrong CLEAR pixels %r; %d BAND pixels outside their candidates %r" % (len(bad_clear), bad_clear[:6], len(bad_band), bad_band[:6])


def test_every_scene_pixel_by_pixel(built, handles):
    scenes, frames = built
    assert sorted(handles) == [(1, 1, 5), (1, 8, 1), (1, 8, 5), (1, 8, 6), (1, 16, 5), (4, 8, 5)]
    count = {f: [0, 0, 0, 0] for f in RS.FAMILIES}  # CLEAR targets, BAND targets, CLEAR pixels, BAND pixels
    failures = []
    for key, (h, idx) in sorted(handles.items()):
        for e, i in enumerate(idx):
            s, f = scenes[i], frames[i]
            bad_clear, bad_band = RS.check_frame(f, h.frame(e))
            if bad_clear or bad_band:
                failures.append("%s (handle %r env %d of %d): %s" % (s.tag, key, e, len(idx), _report(bad_clear, bad_band)))
            c = count[s.family]
            for t in s.targets:
                c[1 if t in f.band else 0] += 1
            c[2] += s.width * s.height - len(f.band)
            c[3] += len(f.band)
    print("CLEAR/BAND target pixels (all pixels) per family: " +
          " ".join("%s %d/%d (%d/%d)" % (fam, c[0], c[1], c[2], c[3]) for fam, c in count.items()))
    assert not failures, "%d frames differ:\n%s" % (len(failures), "\n".join(failures[:12]))
    for fam, c in count.items():
        assert c[0] >= 10 and c[1] >= 10, (fam, c)


def test_no_byte_outside_the_frame_and_every_byte_inside(torch_cuda, native, built, handles):
    """the frame rendered into the middle of a buffer of 0x5A (no palette value): both guards stay, every inner byte is written, at
    every frame size (the last block of a row holds 1, 127 or 128 live pixels; 8192 is the largest width ssg_render accepts)"""
    torch = torch_cuda
    scenes, frames = built
    h, idx = handles[(1, 8, 5)]
    assert all(0x5A not in c for c in RS.PALETTE)
    seen = set()
    for e, i in enumerate(idx):
        s = scenes[i]
        if s.family != "frames" or (s.width, s.height) in seen:
            continue
        seen.add((s.width, s.height))
        n = s.width * s.height * 3
        buf = torch.full((GUARD + n + GUARD,), 0x5A, dtype=torch.uint8, device=h.vec.device)
        with torch.cuda.device(h.vec.device):
            native.check(native.lib().ssg_render(h.vec._h, e, s.width, s.height, C.c_void_p(buf.data_ptr() + GUARD), 1, h.vec._stream()),
                         h.vec._h, "ssg_render")
        got = buf.cpu().numpy()
        where = "%dx%d" % (s.width, s.height)
        assert (got[:GUARD] == 0x5A).all() and (got[GUARD + n:] == 0x5A).all(), "guard bytes written at " + where
        inner = got[GUARD: GUARD + n]
        assert (inner != 0x5A).all(), "%d bytes not written at %s" % (int((inner == 0x5A).sum()), where)
        bad_clear, bad_band = RS.check_frame(frames[i], inner.reshape(s.width, s.height, 3))
        assert not bad_clear and not bad_band, where + ": " + _report(bad_clear, bad_band)
    assert seen == set(RS.FRAME_SIZES)


def test_env_selection_and_streams(torch_cuda, native, built, handles):
    """env e's frame is the same bytes whatever its neighbours hold and on whichever stream; the first and the last env of a handle
    are both right"""
    torch = torch_cuda
    scenes, frames = built
    for key in ((1, 8, 5), (4, 8, 5)):
        h, idx = handles[key]
        n = len(idx)
        for e in (0, n - 1):
            bad_clear, bad_band = RS.check_frame(frames[idx[e]], h.frame(e))
            assert not bad_clear and not bad_band, (key, e, _report(bad_clear, bad_band))
        # the same scenes between other neighbours, on other records, in a handle of three envs
        picks = [n // 3, n - 1, 0, n // 2]
        for a, e, b in ((picks[0], picks[1], picks[2]), (picks[3], picks[2], picks[1])):
            small = Handle(torch, native, [scenes[idx[a]], scenes[idx[e]], scenes[idx[b]]])
            try:
                assert np.array_equal(small.frame(1), h.frame(e)), (key, a, e, b)
            finally:
                small.vec.close()
        # a second stream
        e = n // 2
        s = scenes[idx[e]]
        first = h.frame(e)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=h.vec.device)
        with torch.cuda.stream(side):
            img = h.vec.get_screen(e, width=s.width, height=s.height, debug=s.debug)
            side.synchronize()
            second = img.cpu().numpy()
        assert np.array_equal(first, second), key


@pytest.mark.parametrize("n_ships", [1, 4])
def test_render_reads_the_state_and_writes_none_of_it(torch_cuda, native, n_ships):
    """the state blob is bitwise unchanged by renders (config 4 keeps its queues and memo tables there), and a handle that renders
    between its steps steps exactly like its twin that does not"""
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    torch = torch_cuda
    a, b = (ShipVecEnv(128, n_maps=8, n_ships=n_ships) for _ in range(2))
    try:
        oa, ob = a.reset_tensor(), b.reset_tensor()
        assert torch.equal(oa, ob)
        acts = a.random_actions(7, 0, 12)
        for k in range(12):
            if k >= 4:
                before = a.state.clone()
                for e, (w, h, dbg) in ((0, (33, 17, True)), (127, (64, 64, True)), (k, (129, 2, False))):
                    a.get_screen(e, width=w, height=h, debug=dbg)
                torch.cuda.synchronize()
                assert torch.equal(a.state, before), "a render changed the state blob before step %d" % k
            ra = [t.clone() for t in a.step_tensor(acts[k])]
            rb = b.step_tensor(acts[k])
            for name, x, y in zip(("obs", "reward", "done", "flags"), ra, rb):
                assert torch.equal(x, y), (name, k)
            assert same_columns(torch, a, b), k
            if n_ships > 1:
                for fid in (native.F_TRAFFIC, native.F_GOAL_BODIES, native.F_DYN_FLAGS):
                    assert torch.equal(a.field(fid), b.field(fid)), (fid, k)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("n_ships", [1, 4])
def test_frames_of_the_state_that_real_steps_leave(torch_cuda, native, oracle, n_ships):
    """30 random steps of a default handle, then three envs rendered and compared with the rasteriser fed from the state read back
    through field(): the first of them has reached a goal, which the rasteriser then leaves out as its mask bit says"""
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    torch, N = torch_cuda, native
    vec = ShipVecEnv(64, n_maps=8, n_ships=n_ships)
    try:
        vec.reset_tensor()
        for act in vec.random_actions(1, 0, 30):
            vec.step_tensor(act)
        col = lambda fid: vec.field(fid).cpu().numpy()
        x, y, ang, mask, maps = (col(f) for f in (N.F_X, N.F_Y, N.F_ANGLE, N.F_GOAL_MASK, N.F_MAP_ID))
        T = col(N.F_TRAFFIC) if n_ships > 1 else None
        G = col(N.F_GOAL_BODIES) if n_ships > 1 else None
        ng = vec.cfg.n_goals
        full = (1 << ng) - 1
        reached = [e for e in range(64) if (int(mask[e]) & full) != full]
        assert reached, "no env has reached a goal after 30 steps of action seed 1"
        done, have_reached = [], False
        for e in reached + [0, 63] + list(range(1, 63)):
            if e in done:
                continue
            m = int(maps[e])
            sc = RS.live_scene(vec.bank_polys[m], vec.bank_goals[m], (x[e], y[e], ang[e]), int(mask[e]), n_ships,
                               None if T is None else [T[9 * k: 9 * k + 3, e] for k in range(3)],
                               None if G is None else [G[8 * j: 8 * j + 2, e] for j in range(ng)], vec.cfg.n_beams, 150, 120,
                               "env %d after 30 steps" % e)
            if not all(c for _, _, _, c in RS.beam_marks(oracle, sc)):
                continue  # (a beam at a decision boundary of the lidar: another env)
            f = RS.render(oracle, sc)
            got = vec.get_screen(e, width=150, height=120).cpu().numpy()
            bad_clear, bad_band = RS.check_frame(f, got)
            assert not bad_clear and not bad_band, (e, _report(bad_clear, bad_band))
            have_reached |= e in reached
            done.append(e)
            if len(done) >= 3:
                break
        assert have_reached and len(done) == 3, done
    finally:
        vec.close()


def test_python_surface(torch_cuda, native):
    """get_screen defaults to the bounds; render('rgb_array', env=i) is its [y][x] transpose; render('human') is None; get_images()[i]
    and env(i).render('rgb_array') are env i's frame"""
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    vec = ShipVecEnv(3, n_maps=3)
    try:
        vec.reset_tensor()
        screens = [vec.get_screen(i).cpu().numpy() for i in range(3)]
        assert all(s.shape == (int(vec.bounds[0]), int(vec.bounds[1]), 3) and s.dtype == np.uint8 for s in screens)
        assert not np.array_equal(screens[0], screens[1]) and not np.array_equal(screens[1], screens[2])  # three records
        assert np.array_equal(vec.get_screen().cpu().numpy(), screens[0])
        for i in range(3):
            r = vec.render('rgb_array', env=i)
            assert isinstance(r, np.ndarray) and np.array_equal(r, screens[i].transpose(1, 0, 2))
            assert np.array_equal(vec.env(i).render('rgb_array'), r)
        assert vec.render('human') is None and vec.render() is None and vec.env(1).render('human') is None
        images = vec.get_images()
        assert len(images) == 3 and all(np.array_equal(images[i], screens[i].transpose(1, 0, 2)) for i in range(3))
        plain = vec.get_screen(2, debug=False).cpu().numpy()
        assert {tuple(c) for c in np.unique(plain.reshape(-1, 3), axis=0)} == {RS.BG, RS.YELLOW}
    finally:
        vec.close()
