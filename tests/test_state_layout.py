"""The state blob's layout and the step kernel's launch geometry, pinned over every branch that decides them.

tests/golden/state_layout.json holds, per configuration, what the library answered before the layout came to be built as one record
(recorded from that library; `python tests/test_state_layout.py OUT.json` records the same tables from the library in use):

* "layouts": ssg_state_nbytes, and for every field id from -1 to one past SSG_F_DYN_ARB_IMPULSE the return code and the four outputs of
  ssg_state_field (each output starts as -7: a refused call shows that it wrote nothing).  The configurations reach every branch:
  n_envs at and around the 256-env padding, the smallest and largest beam counts, history on both sides of 2 (the staging rows),
  1 and 4 ships (the config-4 sections), and map_ring (the refill's work queue) with history <= 2.
* "geometries": ssg_debug_launch_geometry (envs per workgroup, bank staged in LDS or not, LDS bytes) after ssg_set_map_bank with a
  made-up 16-byte-aligned address, on env counts around the workgroup-size thresholds, bank sizes around what the LDS holds, 1 and 4
  ships, with and without SSG_FLAG_BANK_IN_GLOBAL.  SSG_BLOCK is left unset.

Host only: made-up addresses, nothing reaches a device."""
import ctypes as C
import itertools
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "state_layout.json")
Q = 0x30000
UNSET = -7
FIELDS = range(-1, 23)  # SSG_F_DYN_ARB_IMPULSE = 21


def layout_configs():
    """(n_envs, n_beams, history, n_ships, map_ring)"""
    out = [(n, 8, h, 1, 0) for n in (1, 256, 257, 4096) for h in (1, 2, 3, 8)]
    out += [(257, b, h, s, 0) for b in (1, 16) for s in (1, 4) for h in (2, 3)]
    out += [(n, 8, h, 4, 0) for n in (1, 256, 4096) for h in (1, 8)]
    out += [(1, 8, 1, 1, 2), (257, 16, 2, 1, 128), (256, 1, 2, 1, 2), (4096, 8, 1, 1, 128),
            (1, 1, 2, 4, 128), (257, 8, 1, 4, 2), (256, 16, 2, 4, 128), (4096, 8, 2, 4, 2)]
    return out


def geometry_configs():
    """(n_envs, n_beams, n_maps, n_ships, SSG_FLAG_BANK_IN_GLOBAL)"""
    return list(itertools.product((64, 16384, 16385, 32768, 32769, 65536), (8, 10, 16), (1, 64, 100, 120, 4096), (1, 4), (0, 1)))


def _create(native, **fields):
    c, h = native.default_config(), C.c_void_p()
    for k, v in fields.items():
        setattr(c, k, v)
    native.check(native.lib().ssg_create(C.byref(c), C.byref(h)))
    return h


def layout_of(native, cfg):
    n, b, hist, ships, ring = cfg
    L = native.lib()
    h = _create(native, n_envs=n, n_beams=b, history=hist, n_ships=ships, map_ring=ring)
    try:
        nbytes = C.c_size_t()
        native.check(L.ssg_state_nbytes(h, C.byref(nbytes)), h)
        fields = []
        for f in FIELDS:
            off, es, nc, stride = C.c_size_t(UNSET), C.c_int(UNSET), C.c_int(UNSET), C.c_size_t(UNSET)
            rc = L.ssg_state_field(h, f, C.byref(off), C.byref(es), C.byref(nc), C.byref(stride))
            fields.append([rc, C.c_int64(off.value).value, es.value, nc.value, C.c_int64(stride.value).value])
        return {"nbytes": nbytes.value, "fields": fields}
    finally:
        L.ssg_destroy(h)


def geometry_of(native, cfg):
    n, b, n_maps, ships, in_global = cfg
    L = native.lib()
    h = _create(native, n_envs=n, n_beams=b, n_ships=ships, flags=native.FLAG_AUTO_RESET | (native.FLAG_BANK_IN_GLOBAL if in_global else 0))
    try:
        native.check(L.ssg_set_map_bank(h, C.c_void_p(Q + 16), n_maps), h)
        epw, lds, nb = C.c_int(UNSET), C.c_int(UNSET), C.c_size_t(UNSET)
        native.check(L.ssg_debug_launch_geometry(h, C.byref(epw), C.byref(lds), C.byref(nb)), h)
        return [epw.value, lds.value, nb.value]
    finally:
        L.ssg_destroy(h)


def record(native):
    return {"layouts": [{"config": list(c), **layout_of(native, c)} for c in layout_configs()],
            "geometries": [{"config": list(c), "geometry": geometry_of(native, c)} for c in geometry_configs()]}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def no_block_override(monkeypatch):
    monkeypatch.delenv("SSG_BLOCK", raising=False)


@pytest.mark.parametrize("i", range(len(layout_configs())), ids=["n%d-b%d-h%d-s%d-r%d" % c for c in layout_configs()])
def test_layout_is_the_recorded_one(native, golden, i):
    want = golden["layouts"][i]
    assert want["config"] == list(layout_configs()[i])
    got = layout_of(native, layout_configs()[i])
    assert got["nbytes"] == want["nbytes"]
    for f, g, w in zip(FIELDS, got["fields"], want["fields"]):
        assert g == w, "field %d" % f


def test_launch_geometry_is_the_recorded_one(native, golden):
    cfgs = geometry_configs()
    assert [g["config"] for g in golden["geometries"]] == [list(c) for c in cfgs]
    for c, g in zip(cfgs, golden["geometries"]):
        assert geometry_of(native, c) == g["geometry"], c


def test_the_configurations_reach_every_branch(golden):
    cfgs = layout_configs()
    assert len(cfgs) == len(set(cfgs)) and 36 <= len(cfgs) <= 44
    for i, values in enumerate(((1, 256, 257, 4096), (1, 8, 16), (1, 2, 3, 8), (1, 4), (0, 2, 128))):
        assert {c[i] for c in cfgs} == set(values)
    assert all(c[2] <= 2 for c in cfgs if c[4])
    geo = [tuple(g["geometry"][:2]) for g in golden["geometries"]]
    assert {e for e, _ in geo} == {64, 128, 256} and {s for _, s in geo} == {0, 1}  # every workgroup size, staged and gathered


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from ship_sim_gym_amd import _native
    os.environ.pop("SSG_BLOCK", None)
    with open(sys.argv[1], "w") as out:
        json.dump(record(_native), out, separators=(",", ":"))
