"""vec_env.native_config: the ssg_config, the effective auto_reset and the fused-RLlib decision of a ShipVecEnv as a function of its
constructor's arguments, for every combination of map_mode, auto_reset, rllib and history in {2, 3} (ring = 4)."""
import pytest

A, G = 0x1, 0x4  # SSG_FLAG_AUTO_RESET, SSG_FLAG_BANK_IN_GLOBAL
# (map_mode, auto_reset, rllib, history): (flags, map_ring, auto_reset, rllib_fused)
TABLE = {
    ("bank", True, False, 2): (A, 0, True, False),
    ("bank", True, False, 3): (A, 0, True, False),
    ("bank", True, True, 2): (A, 0, True, True),
    ("bank", True, True, 3): (0, 0, False, False),
    ("bank", False, False, 2): (0, 0, False, False),
    ("bank", False, False, 3): (0, 0, False, False),
    ("bank", False, True, 2): (0, 0, False, True),
    ("bank", False, True, 3): (0, 0, False, False),
    ("fresh", True, False, 2): (G, 0, True, False),
    ("fresh", True, False, 3): (G, 0, True, False),
    ("fresh", True, True, 2): (G, 0, False, False),
    ("fresh", True, True, 3): (G, 0, False, False),
    ("fresh", False, False, 2): (G, 0, False, False),
    ("fresh", False, False, 3): (G, 0, False, False),
    ("fresh", False, True, 2): (G, 0, False, False),
    ("fresh", False, True, 3): (G, 0, False, False),
    ("fresh_device", True, False, 2): (A, 4, True, False),
    ("fresh_device", True, False, 3): (A, 4, True, False),
    ("fresh_device", True, True, 2): (A, 4, True, True),
    ("fresh_device", True, True, 3): (0, 4, False, False),
    ("fresh_device", False, False, 2): (0, 4, False, False),
    ("fresh_device", False, False, 3): (0, 4, False, False),
    ("fresh_device", False, True, 2): (0, 4, False, True),
    ("fresh_device", False, True, 3): (0, 4, False, False),
}


@pytest.mark.parametrize("case", sorted(TABLE), ids=lambda c: "-".join(str(v) for v in c))
def test_native_config(native, case):
    from ship_sim_gym_amd import config, vec_env
    map_mode, auto_reset, rllib, history = case

    class E(config.EnvConfig):
        HISTORY_SIZE = history

    c, auto, fused = vec_env.native_config(64, config.GameConfig, E, 0, map_mode=map_mode, auto_reset=auto_reset, rllib=rllib, ring=4)
    assert (c.flags, c.map_ring, auto, fused) == TABLE[case]
    assert (c.n_envs, c.history, c.device_id, c.n_ships) == (64, history, 0, 1)


def test_native_config_other_flags_and_map_mode(native):
    from ship_sim_gym_amd import config, vec_env
    c, _, _ = vec_env.native_config(8, config.GameConfig, config.EnvConfig, 1, fix_collision_reward=True, bank_in_global=True,
                                    exact_lidar=True, dyn_memo=False, n_ships=4, n_beams=8, env_id_base=16)
    assert c.flags == 0x1 | 0x2 | 0x4 | 0x8 | 0x10
    assert (c.device_id, c.n_ships, c.n_beams, c.env_id_base, c.map_ring) == (1, 4, 8, 16, 0)
    with pytest.raises(ValueError, match="map_mode"):
        vec_env.native_config(8, config.GameConfig, config.EnvConfig, 0, map_mode="disk")
