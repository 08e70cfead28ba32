"""The gain rule on the GPU: rwh_sequence_overlap_stats and rwh_stitch_sequence_ex against their host twins (which
tests/test_sequence_gains_cpu.py holds to the numpy restatement) on sample grids that cross every launch edge, the Python layers
above them, and the pipeline entry ransac.stitch_sequence(gains="auto").  Every comparison is exact."""
import numpy as np
import pytest

import gain_cases as gc
import sequence_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return sc.library(gpu=True)


hstats, host_ex, upload, device_ex = gc.hstats, sc.host_ex, sc.upload, sc.device


class DeviceTables(object):
    """The two output tables on the device, pre-filled with 0xA5 bytes between canaries; call() runs
    rwh_sequence_overlap_stats into them and returns (count, sum) as numpy arrays, the canaries checked."""

    def __init__(self, n):
        import torch
        host, _, _, self.check = gc.guarded_tables(n)
        self.n, self.size = n, n * n * 8
        self.buf = torch.from_numpy(host.copy()).cuda()

    def table(self, k):
        at = k * (self.size + 128) + 64
        return self.buf[at:at + self.size]

    def call(self, lib, images, Gs, anchor, stride, on=None):
        import torch
        from ransac_with_homography_amd import _lib
        t = sc.tables(images, Gs, anchor)
        fh, fw = t["size"]
        dev = upload(images) if on is None else on
        ptrs = np.array([d.data_ptr() for d in dev], dtype=np.uint64)
        need = lib.rwh_sequence_overlap_stats_workspace_bytes(self.n, fh, fw, stride)
        assert need > 0
        ws = torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda")
        st = lib.rwh_sequence_overlap_stats(ptrs.ctypes.data, t["hw"].ctypes.data, t["inv"].ctypes.data, t["rects"].ctypes.data, self.n, anchor,
                                            fh, fw, t["origin"][0], t["origin"][1], stride, self.table(0).data_ptr(), self.table(1).data_ptr(),
                                            ws.data_ptr(), need, _lib.stream_ptr())
        assert st == 0
        flat = self.buf.cpu().numpy()
        self.check(flat)
        size = self.size
        return [flat[k * (size + 128) + 64:k * (size + 128) + 64 + size].view(np.uint64).reshape(self.n, self.n).copy() for k in range(2)]


def device_stats(lib, images, Gs, anchor=0, stride=1):
    return DeviceTables(len(images)).call(lib, images, Gs, anchor, stride)


EDGES = sc.edge_canvases()


# ---- statistics ----
@pytest.mark.parametrize("case", EDGES, ids=["fw%d-fh%d" % (c[0], c[1]) for c in EDGES])
def test_device_stats_are_the_host_twin_across_launch_edges(lib, case):
    """The statistics take no row range: edge_canvases()'s fh = 1 cases are their two-row canvases here, whose sample grid has
    one row from stride 2 on."""
    fw, fh, images, Gs, _, _ = case
    fh = max(fh, 2)
    dev = upload(images)
    for stride in (1, 2, 3, 7):
        want = hstats(lib, images, Gs, 0, stride)
        got = DeviceTables(len(images)).call(lib, images, Gs, 0, stride, on=dev)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), stride
        wa = images[0].shape[1]                                                  # the anchor lies at the canvas origin, fh rows high
        assert got[0][0, 0] == -(-wa // stride) * -(-fh // stride)


def test_forty_candidates_in_one_tile(lib):
    images, Gs = gc.forty_in_one_tile()
    for stride in (1, 3):
        want = hstats(lib, images, Gs, 0, stride)
        got = device_stats(lib, images, Gs, 0, stride)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_all_4096_pairs_in_one_tile(lib):
    images, Gs = gc.sixty_four_half_steps()
    t = sc.tables(images, Gs, 0)
    assert t["size"][1] <= 256 and t["size"][0] <= 8
    want = hstats(lib, images, Gs, 0, 1)
    assert (want[0] > 0).all()                                                  # every pair meets
    got = device_stats(lib, images, Gs, 0, 1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_sixty_four_strip_twice_and_on_a_second_stream(lib):
    import torch
    images, Gs = sc.translated_strip(64)
    tabs = DeviceTables(64)
    dev = upload(images)
    want = hstats(lib, images, Gs, 0, 1)
    first = tabs.call(lib, images, Gs, 0, 1, on=dev)
    assert np.array_equal(first[0], want[0]) and np.array_equal(first[1], want[1])
    again = tabs.call(lib, images, Gs, 0, 1, on=dev)                             # the same tables: they are zeroed by the call
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    want3 = hstats(lib, images, Gs, 0, 3)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        other = tabs.call(lib, images, Gs, 0, 3, on=dev)
    assert np.array_equal(other[0], want3[0]) and np.array_equal(other[1], want3[1])


def test_kernels_sequence_overlap_stats(lib):
    import torch
    from ransac_with_homography_amd import kernels
    _, images, Gs, anchor, _ = sc.general_cases()[4]
    t = sc.tables(images, Gs, anchor)
    count, total = kernels.sequence_overlap_stats(upload(images), t["inv"], t["rects"], anchor, t["origin"], t["size"], 2)
    assert count.dtype == total.dtype == torch.int64 and count.is_cuda and tuple(count.shape) == tuple(total.shape) == (5, 5)
    want = hstats(lib, images, Gs, anchor, 2)
    assert np.array_equal(count.cpu().numpy().view(np.uint64), want[0]) and np.array_equal(total.cpu().numpy().view(np.uint64), want[1])
    for stride in (0, 256):
        with pytest.raises(ValueError):
            kernels.sequence_overlap_stats(upload(images), t["inv"], t["rects"], anchor, t["origin"], t["size"], stride)


# ---- the compositor with gains ----
@pytest.mark.parametrize("case", EDGES, ids=["fw%d-fh%d" % (c[0], c[1]) for c in EDGES])
def test_device_ex_is_the_host_twin_across_launch_edges(lib, case):
    fw, fh, images, Gs, order, rows = case
    gains = gc.mixed_gains(len(images))
    dev = upload(images)
    for blend in (sc.PASTE, sc.FEATHER):
        want = host_ex(lib, images, Gs, 0, blend, order, rows=rows, gains=gains)
        got = device_ex(images, Gs, 0, blend, order, gains=gains, on=dev, rows=rows)
        assert got.shape == (max(fh, 2), fw, 3) and np.array_equal(got, want)      # rows that were not launched keep the fill in both
        st, plain = sc.host_twin(lib, images, Gs, 0, blend, order, rows=rows)
        assert st == 0 and not np.array_equal(got, plain)


def test_device_ex_on_the_sixty_four_strip_and_with_unit_gains(lib):
    images, Gs = sc.translated_strip(64)
    gains = gc.mixed_gains(64)
    dev = upload(images)
    for blend in (sc.PASTE, sc.FEATHER):
        want = host_ex(lib, images, Gs, 0, blend, gains=gains)
        assert np.array_equal(device_ex(images, Gs, 0, blend, gains=gains, on=dev), want)
        plain = device_ex(images, Gs, 0, blend, on=dev)
        assert np.array_equal(device_ex(images, Gs, 0, blend, gains=np.ones(64), on=dev), plain)
        assert not np.array_equal(plain, want)


# ---- the Python layers ----
def test_sequence_gains_and_auto(lib):
    import torch
    import homography as hg
    rng = np.random.default_rng(77)
    images = [sc.random_image(30, 41, 4), sc.random_image(27, 38, 5), sc.random_image(33, 29, 6)]
    Hs = [sc.homography(rng, 22.5, 3.2), sc.homography(rng, 19.1, -5.7)]
    before = [im.copy() for im in images]
    for anchor, blending, blend in ((0, False, sc.PASTE), (1, "feather", sc.FEATHER)):
        Gs = sc.chain(Hs, anchor)
        info = {}
        got = hg.sequence_gains(images, Hs=Hs, anchor=anchor, info=info)
        count, total = hstats(lib, images, Gs, anchor, 4)
        st, want = gc.host_gains(lib, count, total)
        assert st == 0 and got.dtype == np.float64 and np.array_equal(got, want)
        assert np.array_equal(info["count"], count) and np.array_equal(info["sum"], total)
        for stride, sn, sg in ((1, 10.0, 0.1), (3, 5.0, 0.2)):
            want = gc.host_gains(lib, *hstats(lib, images, Gs, anchor, stride), sn, sg)[1]
            assert np.array_equal(hg.sequence_gains(images, Gs=Gs, anchor=anchor, stride=stride, sigma_n=sn, sigma_g=sg), want)
        auto = hg.stitchSequence(images, Hs=Hs, anchor=anchor, blending=blending, gains="auto")
        given = hg.stitchSequence(images, Hs=Hs, anchor=anchor, blending=blending, gains=got)
        twin = host_ex(lib, images, Gs, anchor, blend, gains=got)
        assert isinstance(auto, np.ndarray) and np.array_equal(auto, given) and np.array_equal(auto, twin)
        tens = [torch.from_numpy(im).cuda() for im in images]
        out = hg.stitchSequence(tens, Hs=Hs, anchor=anchor, blending=blending, gains="auto")
        assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), twin)
        assert np.array_equal(hg.sequence_gains(tens, Hs=Hs, anchor=anchor), got)
        assert all(np.array_equal(t.cpu().numpy(), b) for t, b in zip(tens, before))
        assert np.array_equal(hg.stitchSequence(images, Hs=Hs, anchor=anchor, blending=blending, gains=None),
                              hg.stitchSequence(images, Hs=Hs, anchor=anchor, blending=blending))
    assert all(np.array_equal(a, b) for a, b in zip(images, before))


def test_auto_gains_level_the_exposure_fixture(lib):
    """Three crops of one scene exposed at 0.7 / 1.0 / 1.3: in the columns where two crops overlap, the pasted canvas with image 0
    on top and the one with image 2 on top differ by less with gains="auto" than without -- both numbers measured here."""
    import homography as hg
    images, Gs = gc.exposure_fixture()
    overlap = np.zeros(440, dtype=bool)
    overlap[90:260] = True
    overlap[180:350] = True
    diff = {}
    for gains in (None, "auto"):
        up = hg.stitchSequence(images, Gs=Gs, order=[0, 1, 2], gains=gains).astype(np.int64)
        down = hg.stitchSequence(images, Gs=Gs, order=[2, 1, 0], gains=gains).astype(np.int64)
        assert up.shape == (200, 440, 3)
        diff[gains] = float(np.abs(up - down)[:, overlap].mean())
    print("mean |order 0,1,2 - order 2,1,0| in the overlap columns: %.3f without gains, %.3f with gains='auto'" % (diff[None], diff["auto"]))
    assert diff["auto"] < diff[None]


def test_pipeline_passes_gains_through(lib):
    import homography as hg
    import ransac as rs
    scene = sc.scene()
    crops = [np.ascontiguousarray(scene[:, x:x + 260]) for x in (0, 90, 180)]      # test_sequence_gpu's crops: known to register
    before = [c.copy() for c in crops]
    info = {}
    can = rs.stitch_sequence(crops, th=5, gains="auto", info=info)
    assert isinstance(can, np.ndarray) and info["gains"].shape == (3,) and info["gains"].dtype == np.float64
    assert np.array_equal(can, hg.stitchSequence(crops, Hs=info["Hs"], gains=info["gains"]))
    assert np.array_equal(info["gains"], hg.sequence_gains(crops, Hs=info["Hs"]))
    given = np.array([0.9, 1.0, 1.2])
    info2 = {}
    can2 = rs.stitch_sequence(crops, th=5, gains=given, info=info2)
    assert np.array_equal(info2["gains"], given) and np.array_equal(can2, hg.stitchSequence(crops, Hs=info2["Hs"], gains=given))
    info3 = {}
    can3 = rs.stitch_sequence(crops, th=5, info=info3)
    assert info3["gains"] is None and np.array_equal(can3, hg.stitchSequence(crops, Hs=info3["Hs"]))
    assert all(np.array_equal(a, b) for a, b in zip(crops, before))
