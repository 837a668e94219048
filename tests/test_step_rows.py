"""tests/step_rows.py holds every compiled beam count: what the step kernel's three GPU tests run against the oracle."""
import step_rows as R

BEAMS = set(range(1, 17))  # ssg_create's n_beams, one step_kernel instantiation each


def test_every_beam_count_is_stepped_at_history_1_and_2():
    have = R.beams_and_histories()
    missing = sorted((nb, h) for nb in BEAMS for h in (1, 2) if (nb, h) not in have)
    assert not missing, "no GPU test steps these (n_beams, history) against the oracle: %r" % (missing,)


def test_each_table_holds_what_it_is_for():
    # the lane patterns: every beam count at both histories by itself (the one test that designs which lanes part ways), and
    # history 3 in every compiled group of four beam counts
    assert {(nb, h) for nb in BEAMS for h in (1, 2)} <= set(R.LANE_ROWS)
    assert {(nb - 1) // 4 for nb, h in R.LANE_ROWS if h == 3} == {0, 1, 2, 3}
    # the lidar scenes: every beam count, both histories, the two tables disjoint
    lidar = [r[0] for r in R.LIDAR_ROWS] + [r[0] for r in R.LIDAR_MORE_ROWS]
    assert set(lidar) == BEAMS and not {r[0] for r in R.LIDAR_ROWS} & {r[0] for r in R.LIDAR_MORE_ROWS}
    assert len({r[0] for r in R.LIDAR_MORE_ROWS}) == len(R.LIDAR_MORE_ROWS) and {r[1] for r in R.LIDAR_MORE_ROWS} == {1, 2}
    # config 4: below 8 beams, at 12 and at 16
    dyn = {r[0] for r in R.EVENT_ROWS if r[4] == 4}
    assert {12, 16} <= dyn and min(dyn) < 8
    # no row twice, every row inside the compiled range
    for table in (R.LANE_ROWS, R.LIDAR_ROWS, R.LIDAR_MORE_ROWS, R.EVENT_ROWS):
        assert len(set(table)) == len(table) and all(r[0] in BEAMS and r[1] in (1, 2, 3) for r in table)
