"""The extractor's edge cases without a GPU (orb_cases.edge_cases: the arc mosaics, the bin wheel, the 65536-pixel wide and tall
images, the narrow images, the strips): the host twin against the numpy restatement, exact equality, and the properties each
builder was made for -- checked on the restatement AND on the host twin, so that test_orb_edges_gpu.py, which holds the device to
both, cannot pass on a case that holds nothing."""
import numpy as np
import pytest

import orb_cases as oc


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ransac_with_homography_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def results(lib):
    """name -> (image, restatement, host twin's result), computed once; n_features above every case's keypoint count."""
    out = {}
    for name, img, kw in oc.edge_cases():
        st, got = oc.host_extract(lib, img, **kw)
        assert st == 0, name
        out[name] = (img, oc.restate(img, **kw), got)
    return out


def _where(r):
    """(x, y) -> (score, bin, position in the order) of a result."""
    return {(int(x), int(y)): (int(s), int(b), i) for i, ((x, y), s, b) in enumerate(zip(r["kps"], r["score"], r["bin"]))}


def test_host_twin_equals_restatement(results):
    for name, (img, want, got) in results.items():
        assert oc.same(got, want), name
        assert want["found"] == len(want["score"]), name                     # nothing was cut: the lists below are complete


@pytest.mark.parametrize("threshold", [20, 254])
def test_arc_mosaic(results, threshold):
    """16 arc starts x 2 polarities: 9 pixels at threshold + 1 is a keypoint of exactly that score, 9 at threshold and 8 at the
    largest difference are none."""
    img, must, must_not = oc.arc_mosaic(threshold)
    assert img.shape == (264, 396) and len(must) == 32 and len(must_not) == 64 and len(set(must_not) | {m[:2] for m in must}) == 96
    assert np.array_equal(img, results["arcs at threshold %d" % threshold][0])
    if threshold == 254:
        assert {s for _, _, s in must} == {255} and set(np.unique(img).tolist()) == {0, 1, 254, 255}
        assert (img[:132] == 0).sum() > (img[:132] != 0).sum() and (img[132:] == 255).sum() > (img[132:] != 255).sum()
    else:
        assert {s for _, _, s in must} == {21} and np.bincount(img.reshape(-1)).argmax() == 128
    for r in results["arcs at threshold %d" % threshold][1:]:
        got = _where(r)
        assert all(got.get((x, y), (None,))[0] == s for x, y, s in must)
        assert not any(c in got for c in must_not)
    # the cells are what they claim: a 9-arc at threshold + 1 scores exactly that, one at the threshold the threshold, an 8-arc 0
    S = oc.scores(img)
    assert all(S[y, x] == threshold + 1 for x, y, _ in must)
    assert sorted(int(S[y, x]) for x, y in must_not) == [0] * 32 + [threshold] * 32


def test_bin_wheel(results):
    img, centres = oc.bin_wheel()
    assert img.shape == (165, 198) and len(centres) == 30
    for r in results["bin wheel"][1:]:
        assert r["kps"][:30].astype(int).tolist() == [list(c) for c in centres]
        assert r["bin"][:30].tolist() == list(range(30)) and (r["score"][:30] == 255).all() and (r["score"][30:] < 255).all()


def test_wide_and_tall(results):
    """Keypoints in the first and the last legal column (row) of a side of 65536, and the weaker dot of every seam pair absent."""
    for name, (img, strong, weak) in (("wide", oc.wide_image()), ("tall", oc.tall_image())):
        assert img.shape == ((33, 65536) if name == "wide" else (65536, 33))
        far = (65519, 16) if name == "wide" else (16, 65519)
        assert (16, 16) in strong and far in strong and len(weak) == 3
        for r in results[name][1:]:
            got = _where(r)
            assert set(got) == set(strong) and not set(weak) & set(got)
            assert all(img[y, x] == 200 for x, y in weak) and min(s for s, _, _ in got.values()) > 200
    # the two are one image: the same scores at the transposed places
    w, t = results["wide"][1], results["tall"][1]
    assert {(x, y): s for (x, y), (s, _, _) in _where(w).items()} == {(y, x): s for (x, y), (s, _, _) in _where(t).items()}


def test_narrow_and_strips(results):
    shapes = [results["narrow %d" % s][0].shape for s in range(12)]
    assert set(shapes) == {(33, 65), (33, 65, 3), (33, 65, 4)}
    found = [results["narrow %d" % s][1]["found"] for s in range(12)]
    assert min(found[:3]) >= 3 and sum(f > 0 for f in found[3:]) >= 8
    for s in range(12):
        r = results["narrow %d" % s][1]
        assert (r["kps"][:, 1] == 16).all() and ((r["kps"][:, 0] >= 16) & (r["kps"][:, 0] <= 48)).all()
    # a planted dot under a stronger one is suppressed by a pixel that can be no keypoint itself
    g = oc.gray(oc.narrow(3))
    under = [x for x in range(16, 49) if g[16, x] >= 60 and g[15, x] >= 60]
    assert under and not {(x, 16) for x in under} & set(_where(results["narrow 3"][1]))
    for name in results:
        if name.startswith("strip"):
            assert results[name][0].shape[0] == 1 and results[name][1]["found"] == 0 and results[name][2]["found"] == 0


def test_numbered_images_differ():
    """The long batch of test_orb_edges_gpu.py: every image holds a keypoint, and neighbours in the batch differ."""
    keys = [oc.key_set(oc.numbered(i)) for i in range(600)]
    assert all(1 <= len(k) <= 3 for k in keys) and {len(k) for k in keys} == {1, 2, 3}
    assert all(keys[i] != keys[i + 1] for i in range(599)) and keys[255] != keys[256] and keys[0] != keys[256]
    shapes = {oc.numbered(i).shape for i in range(600)}
    assert {h for h, _ in shapes} == set(range(33, 41)) and {w for _, w in shapes} == set(range(33, 49))
