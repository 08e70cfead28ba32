"""The long-list fixtures of tests/match_long_cases.py without a GPU: that the pair lists reach what they are for (a block list
longer than the grid, runs of more than one pair per scanning thread, empty and 1-row sides inside the list, every branch of the
ratio rule); the two host twins against the numpy restatements at EVERY descriptor length 1 .. 64; and `live_prefix`, the model of
the three bounds in the argument list of rwh_match_ratio_graph (include/rwh.h), on tables whose answer is written out here."""
import numpy as np
import pytest

import match_cases as mc
import match_long_cases as lc
import match_ratio_cases as rc


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ransac_with_homography_amd import _lib
    return _lib.load()


def test_pool_is_sized_from_the_block_shape():
    sizes = lc.pool_sizes()
    assert sizes == [0, 1, 2, 3, 63, 64, 65, 70, 130, 257, 300, 2 * 256 + 69]
    images = lc.pool(32)
    assert [im.shape for im in images] == [(n, 32) for n in sizes] and all(im.dtype == np.uint8 for im in images)
    assert all(np.array_equal(a, b) for a, b in zip(images, lc.pool(32)))            # seeded


def test_long_lists_pass_the_grid_and_the_scan_width():
    (_, _, _, grid2), (_, _, _, grid1) = lc.block_shape()
    sizes = lc.pool_sizes()
    counts = {P: (lc.blocks_ratio(sizes, lc.long_list(P)), lc.blocks_cross(sizes, lc.long_list(P))) for P in lc.LONG_P}
    print("blocks (ratio, cross-check) per P: %s" % counts)
    # below the cap up to 513: a block takes one item; at 2016 some blocks take a second; at 4500 every block takes a third
    assert all(counts[P][0] < grid2 and counts[P][1] < grid1 for P in (256, 257, 513))
    assert grid2 < counts[2016][0] < 2 * grid2 and grid1 < counts[2016][1] < 2 * grid1
    assert counts[4500][0] >= 3 * grid2 and counts[4500][1] >= 3 * grid1
    # the setup kernels scan runs of ceil(P / 256) pairs with 256 threads: one pair each at 256, two from 257 on (where the last
    # threads' runs are empty), and P + 1 table entries pass 256 everywhere
    assert lc.ceil_div(256, 256) == 1 and all(lc.ceil_div(P, 256) >= 2 for P in lc.LONG_P if P >= 257)
    assert all(lc.ceil_div(P, lc.ceil_div(P, 256)) < 256 for P in (257, 513, 2016, 4500)) and lc.ceil_div(4500, 256) == 18
    for P in lc.LONG_P:
        pairs = lc.long_list(P)
        assert len(pairs) == P and pairs == lc.long_list(P) and len(set(pairs)) < P                     # seeded, with repeats
        assert any(s == d for s, d in pairs)
        inner = pairs[:-1]
        assert any(sizes[s] == 0 for s, _ in inner) and any(sizes[d] == 0 for _, d in inner) and any(sizes[d] == 1 for _, d in inner)
        assert any(sizes[s] == 1 for s, _ in inner)
        # runs of equal entries in the tables the binary searches walk: a pair without blocks, one without rows
        assert any(sizes[s] == 0 or sizes[d] < 2 for s, d in inner)
    assert len(set(lc.long_list(4500))) == 144                                       # every pair of the pool


def test_every_branch_of_the_ratio_rule_is_taken_in_the_pool():
    images, ratio, cross = lc.restated(32)
    assert len(ratio) == len(cross) == 144
    cand = ties = dropped = 0
    for s, d in sorted(ratio):
        c, t, r = rc.candidates(images[s], images[d])
        cand, ties, dropped = cand + c, ties + t, dropped + r
    print("pool at 32 bytes: %d candidates, %d ties, %d dropped by rule 3" % (cand, ties, dropped))
    assert cand > 0 and ties > 0 and dropped > 0
    assert sum(int((w[0] >= 0).sum()) for w in ratio.values()) > 144 and sum(int((w[0] >= 0).sum()) for w in cross.values()) > 144
    # the restatements are shared: a second request gives the same objects
    assert lc.restated(32)[1] is ratio


@pytest.mark.parametrize("nbytes", range(1, 65))
def test_host_twins_equal_restatements_at_every_length(lib, nbytes):
    for na, nb in ((63, 65), (130, 257)):
        A, B = mc.random_pair(na, nb, nbytes, seed=7000 + 100 * nbytes + na)
        got = rc.host_match(lib, A, B)
        assert got[0] == 0 and all(np.array_equal(g, w) and g.dtype == np.int32 for g, w in zip(got[1:], rc.per_query(A, B))), (na, nb)
        got = mc.host_match(lib, A, B)
        assert got[0] == 0 and all(np.array_equal(g, w) and g.dtype == np.int32 for g, w in zip(got[1:], mc.per_query(A, B))), (na, nb)


def test_live_prefix_on_hand_written_tables():
    """"A pair whose rows would pass total_query or total_train has no matches", "a pair whose partial results would not fit into the
    workspace given has no matches", and none behind such a pair either (include/rwh.h)."""
    (_, _, S, _), _ = lc.block_shape()
    assert S == 256
    # all live: partials 70 * 1 + 70 * 3 + 65 * 1 = 345
    na, nb = [70, 70, 65], [65, 600, 70]
    assert lc.live_prefix(na, nb, 205, 735, 345) == [True, True, True]
    assert lc.live_prefix(na, nb, 205, 735, 344) == [True, True, False]
    # the second pair of three starved: 70 + 210 partials against the 205 the smallest workspace holds; the third would fit by itself
    # (70 + 65 <= 205) and is not live either
    assert lc.live_prefix(na, nb, 205, 735, 205) == [True, False, False]
    # total_query understated: 70 + 65 <= 145 < 70 + 65 + 70
    na, nb = [70, 65, 70], [65, 70, 65]
    assert lc.live_prefix(na, nb, 145, 200, 10 ** 6) == [True, True, False]
    assert lc.live_prefix(na, nb, 69, 200, 10 ** 6) == [False, False, False]
    # total_train understated by one row
    assert lc.live_prefix(na, nb, 205, 65 + 70 + 64, 10 ** 6) == [True, True, False]
    assert lc.live_prefix(na, nb, 205, 200, 205) == [True, True, True]
    # a pair without rows behind a dead one stays dead; in front of it, it is live
    assert lc.live_prefix([0, 70, 0], [0, 65, 0], 69, 65, 70) == [True, False, False]


def test_block_counts_on_hand_written_pairs():
    sizes = [0, 1, 2, 256, 257, 513]
    assert lc.blocks_ratio(sizes, [(3, 3)]) == 1 and lc.blocks_ratio(sizes, [(4, 3), (3, 4)]) == 4 and lc.blocks_ratio(sizes, [(5, 5)]) == 9
    assert lc.blocks_ratio(sizes, [(5, 1), (5, 0), (0, 5)]) == 0 and lc.blocks_ratio(sizes, [(1, 2)]) == 1
    assert lc.blocks_cross(sizes, [(5, 1)]) == 3 and lc.blocks_cross(sizes, [(1, 5)]) == 3 and lc.blocks_cross(sizes, [(5, 0), (0, 5)]) == 0


def test_extreme_problems_are_what_their_docstring_says():
    probs = lc.extreme_problems()
    cross = [[tuple(int(v) for v in m) for m in zip(*mc.oracle(A, B))] for A, B in probs]
    ratio = [[tuple(int(v) for v in m) for m in zip(*rc.oracle(A, B))] for A, B in probs]
    assert cross == [[(0, 0, 512)], [(37, 0, 1)], [(0, 0, 0), (37, 5, 1)], [(0, 0, 0), (37, 5, 0)]]
    assert ratio == [[], [], [(37, 5, 1, 511)], [(37, 5, 0, 512)]]
    assert int(mc.distances(*probs[0]).min()) == 512 == 8 * 64
