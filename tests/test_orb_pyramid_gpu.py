"""The scale pyramid of the extractor on the MI355X (rules 6 - 8 of include/rwh.h): rwh_orb_pyramid_batched against the host twin
rwh_host_orb_pyramid, byte for byte, with canaries around the planes; features.extract_batch(n_levels=...) against
rwh_host_orb_extract_pyramid -- keypoints, descriptors, levels, sizes, scores, bins, exact equality -- with and without the capacity
retry; n_levels = 1 against the call without the argument; batches of 70 images (210 and 280 table rows, most without keypoints);
malformed table rows; stitching(features={"n_levels": 8}) on a pair that differs in zoom by 1.5."""
import numpy as np
import pytest

import orb_cases as oc
import orb_pyramid_cases as pc

pytestmark = pytest.mark.gpu
CANARY = 0xCD


@pytest.fixture(scope="module")
def gpu():
    return oc.gpu_torch()


@pytest.fixture(scope="module")
def lib(gpu):
    from ransac_with_homography_amd import _lib
    return _lib.load()


def _pyramid(torch, images, scales, gap, table=None, behind=64):
    """Runs the device call on a buffer [head | gap | planes | behind], everything but the head filled with CANARY and the `behind`
    bytes lying past images_bytes -> (buffer as numpy, head, table, planes_offset, images_bytes, spans)."""
    from ransac_with_homography_amd import kernels
    head, rows, off, end, spans = pc.layout(images, scales, gap)
    buf = np.full(end + behind, CANARY, dtype=np.uint8)
    buf[:head.size] = head
    dev = torch.from_numpy(buf).cuda()
    rows = rows if table is None else table(rows)
    kernels.orb_pyramid_batched(dev[:end], off, torch.from_numpy(rows).cuda(), scales)
    return dev.cpu().numpy(), head, rows, off, end, spans


@pytest.mark.parametrize("which", ["four levels", "caller's table"])
def test_planes_equal_host_twin_and_nothing_else_is_written(gpu, lib, which):
    import ransac as rs
    scales = rs.orb_scales(4) if which == "four levels" else pc.CALLER_SCALES
    images = pc.gpu_images()
    got, head, _, off, end, spans = _pyramid(gpu, images, scales, gap=37)
    written = np.zeros(got.size, dtype=bool)
    widths = set()
    for img, sp in zip(images, spans):
        st, want = pc.host_planes(lib, img, scales)
        assert st == 0
        for (at, hl, wl), w in zip(sp, want):
            assert w.shape == (hl, wl) and np.array_equal(got[at:at + hl * wl].reshape(hl, wl), w), (img.shape, hl, wl)
            written[at:at + hl * wl] = True
            widths.add(wl)
    assert np.array_equal(got[:off], head)                                   # the images
    assert (got[off:][~written[off:]] == CANARY).all() and (~written[off:]).sum() == 37 + 64     # before and behind the planes
    assert any(w % 4 for w in widths) and any(w > 64 and w % 64 for w in widths)
    if which == "four levels":                                               # 33 x 300 falls below 33 rows on level 1
        assert spans[2][0][1] < 33 and spans[0][0][1:] == (125, 169)


@pytest.mark.parametrize("threshold", [0, 20])
def test_extract_batch_equals_host_twin(gpu, lib, monkeypatch, threshold):
    """threshold 0 on noise finds thousands of keypoints per level; with the usual room cut to 64 the overflow retry runs with levels."""
    import ransac as rs
    from ransac_with_homography_amd import features as impl
    if threshold == 0:
        monkeypatch.setattr(impl, "_ORB_DEFAULT_CAPACITY", 64)
    images = pc.gpu_images()
    scales = rs.orb_scales(4)
    quotas = rs.orb_level_quotas(500, scales)
    got = oc.extract(images, per_level=True, n_levels=4, threshold=threshold)
    total = 0
    for img, g in zip(images, got):
        st, want = pc.host_extract_pyramid(lib, img, scales, quotas, threshold=threshold)
        assert st == 0 and pc.same(g, want), img.shape
        total += len(want["score"])
    assert total > 300 and len(set(got[0]["level"].tolist())) == 4 and got[2]["found"][1:] == [0, 0, 0]
    if threshold == 0:
        assert max(got[0]["found"]) > 64
    # the caller's table and quotas, one of them zero
    mine = oc.extract(images[:2], per_level=True, scales=pc.CALLER_SCALES, quotas=[40, 0, 7], threshold=threshold)
    for img, g in zip(images, mine):
        st, want = pc.host_extract_pyramid(lib, img, pc.CALLER_SCALES, [40, 0, 7], threshold=threshold)
        assert st == 0 and pc.same(g, want), img.shape


@pytest.fixture(scope="module")
def one_level(gpu):
    """The batch of the one-level tests and its extraction with the defaults: (images, features, info)."""
    import ransac as rs
    images = pc.gpu_images() + [oc.foto("A")[200:400, 300:600]]
    info = {}
    return images, rs.extract_batch(images, info=info), info


def test_one_level_is_the_call_without_the_argument(gpu, one_level):
    import ransac as rs
    (images, a, ia), ib = one_level, {}
    b = rs.extract_batch(images, n_levels=1, info=ib)
    c = rs.extract_batch(images, scales=[256], quotas=[500])
    for (ka, da), (kb, db), (kc, dc) in zip(a, b, c):
        assert ka.dtype == kb.dtype and gpu.equal(ka, kb) and gpu.equal(da, db) and gpu.equal(ka, kc) and gpu.equal(da, dc)
    assert ia["found"] == ib["found"] and ia["counts"] == ib["counts"] and sum(ia["counts"]) > 500
    assert all(gpu.equal(x, y) for k in ("score", "bin", "level", "size") for x, y in zip(ia[k], ib[k]))
    assert all(int(l.sum()) == 0 and (z == 31).all() for l, z in zip(ib["level"], ib["size"]))


def _same_call(torch, a, ia, b, ib):
    """Every returned tensor and every `info` entry of two extract_batch calls: dtype, shape and bits."""
    same = lambda x, y: x.dtype == y.dtype and x.is_cuda and y.is_cuda and torch.equal(x, y)
    assert len(a) == len(b) and all(same(ka, kb) and same(da, db) for (ka, da), (kb, db) in zip(a, b))
    assert sorted(ia) == sorted(ib) == ["bin", "counts", "found", "found_levels", "level", "score", "size"]
    assert all(len(ia[k]) == len(ib[k]) == len(a) and all(same(x, y) for x, y in zip(ia[k], ib[k])) for k in ("score", "bin", "level", "size"))
    assert all(ia[k] == ib[k] and len(ia[k]) == len(a) for k in ("counts", "found", "found_levels"))


def test_one_level_quota_is_n_features(gpu, one_level):
    """quotas=[40] on the only level is n_features=40, for an image that finds more and for one that finds fewer."""
    import ransac as rs
    images, _, first = one_level
    assert max(first["found"]) > 40 > min(first["found"]) > 0
    ia, ib = {}, {}
    a = rs.extract_batch(images, quotas=[40], info=ia)
    b = rs.extract_batch(images, n_features=40, info=ib)
    _same_call(gpu, a, ia, b, ib)
    assert ia["counts"] == [min(f, 40) for f in first["found"]] and ia["found"] == first["found"]


def test_one_level_overflow_retry(gpu, one_level, monkeypatch):
    """The usual room cut to 64 with one level: images that find more meet the overflow status, the detect call is repeated with
    room for all, and the result is the call's with the usual room."""
    import ransac as rs
    from ransac_with_homography_amd import features as impl
    images, want, iw = one_level
    assert max(iw["found"]) > 64
    monkeypatch.setattr(impl, "_ORB_DEFAULT_CAPACITY", 64)
    info = {}
    got = rs.extract_batch(images, info=info)
    _same_call(gpu, got, info, want, iw)


@pytest.mark.parametrize("levels", [3, 4])
def test_seventy_images(gpu, lib, levels):
    """70 images of 40 x 40 and 33 x 64, mixed: 210 table rows with 3 levels, 280 (more than one row per lane of the setup block) with
    4; most rows hold no keypoint, some levels are narrower than 33."""
    import ransac as rs
    images = [oc.random_image(40, 40, 300 + i, channels=(1, 3)[i % 2]) if i % 3 else oc.random_image(33, 64, 300 + i, channels=1) for i in range(70)]
    scales = rs.orb_scales(levels)
    quotas = rs.orb_level_quotas(60, scales)
    got = oc.extract(images, per_level=True, n_levels=levels, n_features=60)
    on_level = np.zeros(levels, dtype=int)
    for i, (img, g) in enumerate(zip(images, got)):
        st, want = pc.host_extract_pyramid(lib, img, scales, quotas)
        assert st == 0 and pc.same(g, want), i
        on_level += np.bincount(want["level"], minlength=levels)
    assert on_level[0] > 70 and on_level[1] > 0 and on_level[2:].sum() == 0


def test_malformed_rows_leave_their_planes_alone(gpu, lib):
    """Image 1's row has a negative offset, image 2's ends past the buffer, and the last level of image 0 claims a plane that ends past
    the buffer: none of their planes is written, nothing else changes, and the detector finds no keypoint in any of them."""
    import ransac as rs
    from ransac_with_homography_amd import kernels
    torch = gpu
    scales = rs.orb_scales(3)
    images = pc.gpu_images()

    def spoil(rows):
        rows = rows.copy()
        rows[3, 0] = -1
        end = rows[8, 0] + rows[8, 2] * rows[8, 3]                         # images_bytes: the end of the last plane
        rows[6, 0] = end - 10                                              # an image that ends past the buffer
        rows[2, 0] = end - rows[2, 2] * rows[2, 3] + 5                     # a plane that ends five bytes past it
        return rows
    got, head, rows, off, end, spans = _pyramid(torch, images, scales, gap=0, table=spoil)
    st, want = pc.host_planes(lib, images[0], scales)
    at, hl, wl = spans[0][0]
    assert st == 0 and np.array_equal(got[at:at + hl * wl].reshape(hl, wl), want[0])
    assert np.array_equal(got[:off], head) and (got[at + hl * wl:] == CANARY).all()
    dev = torch.from_numpy(got[:end]).cuda()
    gray_bytes = int(rows[-1, 1] + rows[-1, 2] * rows[-1, 3])
    _, _, counts = kernels.orb_detect_batched(dev, torch.from_numpy(rows).cuda(), gray_bytes, 20, 4096)
    counts = counts.cpu().numpy()
    assert counts[0] > 0 and counts[1] > 0 and (counts[2:] == 0).all()


def test_argument_errors(gpu):
    import ransac as rs
    img = pc.gpu_images()[1]
    for kw in (dict(n_levels=0), dict(n_levels=17), dict(n_levels=9, scale=1.2), dict(n_levels=3, scale=1.0), dict(scales=[256, 256]),
               dict(scales=[255, 300]), dict(scales=[256, 1025]), dict(n_levels=3, scales=[256, 300]), dict(n_levels=2, quotas=[5]),
               dict(n_levels=2, quotas=[5, -1]), dict(n_levels=2, quotas=[2 ** 30, 7])):
        with pytest.raises(ValueError):
            rs.extract_batch([img], **kw)
    with pytest.raises(ValueError):
        rs.stitching(img, img, features="pyramid")


def test_stitching_a_pair_that_differs_in_zoom(gpu, monkeypatch):
    """B is A shrunk by 1.5 (bilinear, not the rule's resampling): with 8 levels the H of stitching() is the similarity
    x_B = (x_A + 0.5) / 1.5 - 0.5 -- the four corners of A land within RANSAC's own threshold, th = 5 px, of where it sends them."""
    import ransac as rs
    from ransac_with_homography_amd import ransac as impl
    A = pc.textured()
    B = pc.shrink_bilinear(A)
    A3, B3 = (np.ascontiguousarray(np.stack([v] * 3, axis=2)) for v in (A, B))
    seen = {}
    real = impl.stitchPanorama

    def capture(*args, **kw):
        seen["H"] = np.array(kw["H"], dtype=np.float64)
        return real(*args, **kw)
    monkeypatch.setattr(impl, "stitchPanorama", capture)
    np.random.seed(2)
    canvas = rs.stitching(A3.copy(), B3.copy(), features={"n_levels": 8}, ransacMet="fwd", th=5, d=70, k=1000)
    assert isinstance(canvas, np.ndarray) and canvas.dtype == np.uint8 and canvas.ndim == 3 and canvas.size > 0
    H = seen["H"] / seen["H"][2, 2]
    h, w = A.shape
    corners = np.array([[0, 0, 1], [w - 1, 0, 1], [0, h - 1, 1], [w - 1, h - 1, 1]], dtype=np.float64).T
    p = H @ corners
    p = p[:2] / p[2]
    want = (corners[:2] + 0.5) / 1.5 - 0.5
    err = np.hypot(*(p - want))
    print("corner errors of H, px:", err)
    assert (err <= 5.0).all(), err
