"""Which (n_beams, history) rows the step kernel's three GPU tests run against the oracle: one table, plain tuples.

step_kernel is compiled once per beam count 1 .. 16, and the beam count selects code there (how an observation row is written,
whether the split and speculative rows exist, how the beams are dealt to the lidar waves, every tile's LDS layout), so a beam
count that no row holds is an instantiation that ships untested.  tests/test_step_rows.py asserts that the union of these tables
holds every beam count at history 1 and at history 2: thin a table and it says what was dropped.
"""

# tests/test_step_masked_regions_gpu.py: (n_beams, history).  Every beam count at history 1 and 2; history 3 (the two-frame
# staging rows and history_shift_kernel) at one beam count of each compiled group and at 12.
LANE_ROWS = (
    (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (8, 1), (9, 1), (10, 1), (11, 1), (12, 1), (13, 1), (14, 1), (15, 1), (16, 1),
    (1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (6, 2), (7, 2), (8, 2), (9, 2), (10, 2), (11, 2), (12, 2), (13, 2), (14, 2), (15, 2), (16, 2),
    (1, 3), (4, 3), (7, 3), (12, 3), (16, 3))

# tests/test_lidar_edges_gpu.py, test_lidar_at_its_decision_boundaries: (n_beams, history, exact_lidar), thinned: both histories on
# both paths, and the EXACT path (SSG_FLAG_EXACT_LIDAR is built for 8 and 10 beams) beside the default one at its beam counts.
LIDAR_ROWS = ((1, 2, False), (7, 1, False), (8, 1, True), (8, 2, False), (10, 1, False), (10, 2, True), (16, 1, False), (16, 2, False))

# tests/test_lidar_edges_gpu.py, test_lidar_at_the_other_beam_counts: (n_beams, history), the beam counts LIDAR_ROWS leaves out, the
# history alternating
LIDAR_MORE_ROWS = ((2, 1), (3, 2), (4, 1), (5, 2), (6, 1), (9, 2), (11, 1), (12, 2), (13, 1), (14, 2), (15, 1))

# tests/test_event_edges_gpu.py: (n_beams, history, fix_collision_reward, n_goals, n_ships), thinned: one beam count from each
# compiled beam group and both BASELINE counts, history 1 .. 3, both reward rules, n_goals 1, 5 and 6; the rows with four ships are
# config 4 (the DYN instantiation): below 8 beams, at 10, at 12 (the highest count with 256-env workgroups) and at 16 (64-env
# workgroups only: no 256 above 12 beams, and config 4's 128 folds to 64)
EVENT_ROWS = ((1, 2, False, 5, 1), (8, 1, True, 6, 1), (8, 3, False, 5, 1), (10, 2, True, 1, 1), (10, 3, False, 6, 1), (16, 1, False, 5, 1),
              (16, 2, True, 5, 1), (10, 2, False, 5, 4), (6, 1, True, 5, 4), (12, 2, False, 5, 4), (16, 1, False, 5, 4))


def beams_and_histories():
    """{(n_beams, history)} over the three tests"""
    return {r[:2] for table in (LANE_ROWS, LIDAR_ROWS, LIDAR_MORE_ROWS, EVENT_ROWS) for r in table}
