"""The renderer's reference (tests/render_scenes.py) on its own, no GPU: frames small enough to verify by hand, the y flip and the
[x][y] order, the painter's order, the exact path against the f64 path, and the conditions that keep test_render_gpu.py from passing
vacuously (enough CLEAR and BAND target pixels in every family, BAND pixels rare, every colour of the palette in use)."""
import collections
import math
import time

import numpy as np
import pytest

import lidar_scenes as LS
import render_scenes as RS
from render_scenes import BANK, BG, BLACK, GREEN, RED, WHITE, YELLOW

OUT = [-500.0, -500.0]
LEFT = [(0.0, 0.0), (150.0, 0.0), (150.0, 600.0), (0.0, 600.0)]       # x < 150
RIGHT = [(450.0, 0.0), (600.0, 0.0), (600.0, 600.0), (450.0, 600.0)]  # x > 450


@pytest.fixture(scope="module")
def built(oracle):
    t0 = time.time()
    scenes = RS.build_scenes(oracle)
    frames = [RS.render(oracle, s) for s in scenes]
    print("render_scenes: %d scenes, %d pixels, built and rendered in %.1f s" % (len(scenes), sum(s.width * s.height for s in scenes),
                                                                                 time.time() - t0))
    return scenes, frames


def _scene(width, height, **kw):
    a = dict(left=LS.pad12(LEFT), right=LS.pad12(RIGHT), goals=[OUT] * 5, pose=(-500.0, -500.0, 0.0), n_beams=1, width=width, height=height)
    a.update(kw)
    return RS.Scene("hand", "hand", a.pop("left"), a.pop("right"), a.pop("goals"), a.pop("pose"), **a)


def _expect(width, height, cells):
    img = np.empty((width, height, 3), dtype=np.uint8)
    img[:] = BG
    for (sx, sy), col in cells.items():
        img[sx, sy] = col
    return img


def test_4x4_frame_by_hand(oracle):
    """Pixel centres x = 75, 225, 375, 525 and, downwards, y = 525, 375, 225, 75.  Banks x < 150 and x > 450: columns 0 and 3.  The
    player at (225, 375): its hull (20 x 45 from there) holds that one centre, and the marker covers it.  Goal 0 at (375, 225): pixel
    (2, 2); goal 1 on (375, 525) has its bit cleared.  The one beam leaves (235, 397.5) at 45 degrees and ends at (305.7, 468.2), 89
    units from the nearest centre."""
    sc = _scene(4, 4, pose=(225.0, 375.0, 0.0), goals=[[375.0, 225.0], [375.0, 525.0], OUT, OUT, OUT], mask=0x3D)
    f = RS.render(oracle, sc)
    cells = {(0, y): BANK for y in range(4)}
    cells.update({(3, y): BANK for y in range(4)})
    cells.update({(1, 1): YELLOW, (2, 2): GREEN})
    assert not f.band
    np.testing.assert_array_equal(f.img, _expect(4, 4, cells))
    sc.debug = False
    np.testing.assert_array_equal(RS.render(oracle, sc).img, _expect(4, 4, {(1, 1): YELLOW}))


def test_8x6_frame_by_hand(oracle):
    """Pixel centres x = 37.5 + 75 i and, downwards, y = 550, 450, 350, 250, 150, 50.  Banks: columns 0, 1 and 6, 7.  Config 4.  The
    player at (262.5, 250): pixel (3, 3), yellow.  Its beam leaves (272.5, 272.5) at 45 degrees, misses and ends at (343.21, 343.21),
    8.9 units from the centre (337.5, 350): pixel (4, 2), green.  Goal 0's record position is (187.5, 350) but its body is at
    (187.5, 150): pixel (2, 4) is green, pixel (2, 2) is not.  Goal 1 on (337.5, 50) has its bit cleared.  Traffic ship 2 (10 x 45, the
    bow a triangle above 30) at (408, 410): at the height 40 of the centre (412.5, 450) it is 3.3 wide around its axis 413: pixel
    (5, 1), black.  The other traffic ships are parked outside the frame."""
    sc = _scene(8, 6, pose=(262.5, 250.0, 0.0), goals=[[187.5, 350.0], [337.5, 50.0], OUT, OUT, OUT], mask=0x1D, n_ships=4,
                bodies=[[187.5, 150.0], [337.5, 50.0], OUT, OUT, OUT], traffic=[(-500.0, -500.0, 0.0), (-400.0, -500.0, 0.0), (408.0, 410.0, 0.0)])
    f = RS.render(oracle, sc)
    cells = {(x, y): BANK for x in (0, 1, 6, 7) for y in range(6)}
    cells.update({(3, 3): YELLOW, (4, 2): GREEN, (2, 4): GREEN, (5, 1): BLACK})
    assert not f.band
    np.testing.assert_array_equal(f.img, _expect(8, 6, cells))
    ex, ey, hit, clear = RS.beam_marks(oracle, sc)[0]
    assert clear and not hit and abs(ex - (272.5 + 100 / math.sqrt(2))) < 1e-9 and abs(ey - ex) < 1e-9


def test_y_flip_and_x_first_layout(oracle):
    """a goal in the world's upper left shows in the first column at the top: index [small x][small y] of a [width][height][3] array"""
    sc = _scene(6, 4, goals=[[50.0, 525.0], OUT, OUT, OUT, OUT], left=LS.pad12([(-90.0, -90.0), (-80.0, -90.0), (-80.0, -80.0)]),
                right=LS.pad12([(700.0, -90.0), (710.0, -90.0), (710.0, -80.0)]))
    f = RS.render(oracle, sc)
    assert f.img.shape == (6, 4, 3) and f.img.dtype == np.uint8
    np.testing.assert_array_equal(f.img, _expect(6, 4, {(0, 0): GREEN}))
    assert RS.pixel_world(6, 4, 0, 0) == (50.0, 525.0) and RS.pixel_world(6, 4, 5, 3) == (550.0, 75.0)
    assert RS.nearest_pixel(6, 4, 50.0, 525.0) == (0, 0) and RS.nearest_pixel(6, 4, 599.0, 1.0) == (5, 3)


def test_painters_order(oracle, built):
    """One pixel, (1, 1) of a 4x4 frame at (225, 375), under more and more layers: bank, goal, player hull, traffic hull, beam disc,
    marker.  Then the overlap scenes: a traffic ship's edge splits its target between black and what the ship covers."""
    wide = LS.pad12([(0.0, 0.0), (300.0, 0.0), (300.0, 600.0), (0.0, 600.0)])
    goals = [[227.0, 374.0], OUT, OUT, OUT, OUT]
    steps = ((dict(mask=0), BANK), (dict(), GREEN), (dict(pose=(215.0, 340.0, 0.0)), WHITE),
             (dict(pose=(215.0, 340.0, 0.0), traffic=[(220.0, 370.0, 0.0), (-500.0, -500.0, 0.0), (-400.0, -500.0, 0.0)]), BLACK),
             # the beam leaves (155, 307.5), inside the left bank: a hit, drawn at its far end (225.7, 378.2), 3.3 from the pixel
             (dict(pose=(145.0, 285.0, 0.0), traffic=[(220.0, 370.0, 0.0), (-500.0, -500.0, 0.0), (-400.0, -500.0, 0.0)]), RED),
             (dict(pose=(222.0, 370.0, 0.0), traffic=[(220.0, 370.0, 0.0), (-500.0, -500.0, 0.0), (-400.0, -500.0, 0.0)]), YELLOW))
    for kw, want in steps:
        a = dict(left=wide, goals=goals, n_ships=4, traffic=[(-500.0, -500.0, 0.0), (-450.0, -500.0, 0.0), (-400.0, -500.0, 0.0)])
        a.update(kw)
        sc = _scene(4, 4, **a)
        f = RS.render(oracle, sc)
        assert (1, 1) not in f.band and tuple(f.img[1, 1]) == want, (kw, tuple(f.img[1, 1]), want)
    scenes, frames = built
    under = {"overlap: traffic 0": WHITE, "overlap: traffic 1": GREEN, "overlap: traffic 2": BANK}
    seen = collections.defaultdict(set)
    for s, f in zip(scenes, frames):
        if s.group in under and abs(s.off) == 1e-6:
            assert s.targets[0] not in f.band
            seen[s.group].add(tuple(int(v) for v in f.img[s.targets[0]]))
    assert {g: seen[g] for g in under} == {g: {BLACK, c} for g, c in under.items()}


def test_targets_sit_on_their_boundaries(built):
    """a boundary placed 1e-6 to either side of a target pixel's centre gives the pixel two different colours, both decided; placed
    within 1e-12 it leaves the pixel BAND between exactly those two"""
    scenes, frames = built
    groups = collections.defaultdict(dict)
    for s, f in zip(scenes, frames):
        if s.off is not None:
            groups[(s.family, s.group)][s.off] = (s, f)
    flat = 0
    for key, by in groups.items():
        if not {1e-6, -1e-6, 0.0} <= set(by):
            continue
        (sa, fa), (sb, fb) = by[1e-6], by[-1e-6]
        t = sa.targets[0]
        ca, cb = tuple(int(v) for v in fa.img[t]), tuple(int(v) for v in fb.img[t])
        assert t not in fa.band and t not in fb.band, key
        if ca == cb:  # (a goal whose mask bit is cleared draws nothing on either side)
            flat += 1
            assert "mask 0x1b" in key[1], key
            continue
        s0, f0 = by[0.0]
        assert f0.band.get(s0.targets[0]) == {ca, cb}, (key, f0.band.get(s0.targets[0]), ca, cb)
    assert flat == 1


def test_beam_discs_overlap_each_other_the_ship_and_the_marker(oracle, built):
    """the beam family holds pixels where a beam disc lies over another beam's disc, over the player's hull and under the marker, a
    disc whose centre is outside the frame, hits on either hull, misses and an origin inside a bank"""
    scenes, frames = built
    got = collections.Counter()
    for s, f in zip(scenes, frames):
        if s.family != "beam" or s.off != 1e-6:
            continue
        X, Y = f.X[:, None], f.Y[None, :]
        inside = [RS._g64(p, X, Y) <= 0 for p in f.prims]
        discs = [i for i, p in enumerate(f.prims) if p[0] == "disc" and p[3] == RS.BEAM_DELTA]
        ship = next(i for i, p in enumerate(f.prims) if p[2] == WHITE)
        assert len(discs) == s.n_beams
        got["disc over disc"] += int(any((inside[a] & inside[b]).any() for a in discs for b in discs if a < b))
        got["disc over ship"] += int(any((inside[a] & inside[ship]).any() for a in discs))
        got["disc under marker"] += int(any((inside[a] & inside[-1]).any() for a in discs))
        got["centre outside"] += int(any(f.prims[a][1][1] > RS.H for a in discs))
        got["red"] += int(any(f.prims[a][2] == RED for a in discs))
        got["green"] += int(any(f.prims[a][2] == GREEN for a in discs))
    print("beam scenes with:", dict(got))
    for k in ("disc over disc", "disc over ship", "disc under marker", "centre outside", "red", "green"):
        assert got[k] >= 2, (k, dict(got))
    assert {s.n_beams for s in scenes if s.family == "beam"} == {1, 8, 16}


def test_exact_path_agrees_with_f64_path(oracle, built):
    """every CLEAR pixel of the hand frames, and the targets and a sample of the CLEAR pixels of every third scene, through
    exact_colours: one colour, the f64 path's"""
    scenes, frames = built
    rng = np.random.RandomState(5)
    hand = _scene(8, 6, pose=(262.5, 250.0, 0.3), goals=[[187.5, 350.0], [337.5, 50.0], OUT, OUT, OUT], n_beams=8)
    work = [(hand, RS.render(oracle, hand), [(x, y) for x in range(8) for y in range(6)])]
    for s, f in list(zip(scenes, frames))[::3]:
        px = [(int(rng.randint(s.width)), int(rng.randint(s.height))) for _ in range(4)] + list(s.targets)
        work.append((s, f, px))
    n = 0
    for s, f, px in work:
        for sx, sy in px:
            if (sx, sy) in f.band:
                continue
            cols = RS.exact_colours(f.prims, f.X[sx], f.Y[sy])
            assert cols == {tuple(int(v) for v in f.img[sx, sy])}, (s.tag, sx, sy, cols)
            n += 1
    assert n > 600


def test_the_gpu_test_cannot_pass_vacuously(built):
    scenes, frames = built
    assert {s.family for s in scenes} == set(RS.FAMILIES)
    count = RS.count_targets(scenes, frames)
    print("CLEAR/BAND target pixels per family: " + " ".join("%s %d/%d" % (f, count[f][0], count[f][1]) for f in RS.FAMILIES))
    for fam in RS.FAMILIES:
        assert count[fam][0] >= 10 and count[fam][1] >= 10, (fam, count[fam])
    total = sum(s.width * s.height for s in scenes)
    band = sum(len(f.band) for f in frames)
    print("BAND pixels: %d of %d" % (band, total))
    assert band * 1000 <= total
    for s, f in zip(scenes, frames):
        assert len(f.band) * 100 <= s.width * s.height, (s.tag, len(f.band))
        assert all(len(c) >= 2 and c <= set(RS.PALETTE) for c in f.band.values())
    used = set()
    for f in frames:
        used |= {tuple(int(v) for v in c) for c in np.unique(f.img.reshape(-1, 3), axis=0)}
    assert used == set(RS.PALETTE)
    # every frame size of the issue, the large one once; every handle shape
    sizes = collections.Counter((s.width, s.height) for s in scenes if s.family == "frames")
    assert set(sizes) == set(RS.FRAME_SIZES) and sizes[(600, 600)] == 1
    assert {s.key() for s in scenes} == {(1, 8, 5), (1, 1, 5), (1, 16, 5), (1, 8, 1), (1, 8, 6), (4, 8, 5)}
    assert {s.mask & 0x80 for s in scenes} == {0, 0x80} and any(s.mask & 0x3F != 0x3F for s in scenes)
    assert any(not s.debug and s.n_ships == 4 for s in scenes)
