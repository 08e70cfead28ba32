"""The extractor's branches that test_orb_gpu.py's small images never enter, on the MI355X, every comparison exact equality against
the numpy restatement and the host twin (tests/orb_cases.py; the cases' own properties are in test_orb_edges_cpu.py):
a block of orb_detect_kernel walking to a second, third, ... tile (below and at the cap of the grid); orb_setup_kernel with several
images per lane (more than 256 images); table rows that describe no image; coordinates that need all 16 bits of a key's fields;
the compass early-out of the score on every arc start and polarity at threshold + 1; all 30 orientation bins with the wrap at
lane 29; the skip paths of orb_describe_kernel."""
import numpy as np
import pytest

import orb_cases as oc

pytestmark = pytest.mark.gpu
KEY_NONE = 0x7F7F7F7F7F7F7F7F
FILL = 0xEE


@pytest.fixture(scope="module")
def gpu():
    return oc.gpu_torch()


def _host(img, **kw):
    from ransac_with_homography_amd import _lib
    st, got = oc.host_extract(_lib.load(), img, **kw)
    assert st == 0
    return got


def _sizing(images):
    """(tiles, blocks) of one detect call on `images`.  This MIRRORS rwh_orb_detect_batched (csrc/rwh_orb.hip) at the time of
    writing -- tiles of 64 x 16 pixels, a grid of min(2 * (gray_bytes / 1024) + n_images, 16384) blocks -- so that the walk tests
    can say when a change of the launch's sizing has left them without a walk."""
    tiles = sum(-(-im.shape[1] // 64) * -(-im.shape[0] // 16) for im in images)
    gray_bytes = sum(im.shape[0] * im.shape[1] for im in images)
    return tiles, min(2 * (gray_bytes // 1024) + len(images), 16384)


def _pack(torch, images):
    """(pixels uint8 [bytes], table int64 [n, 5], gray_bytes) on the GPU, the planes back to back as extract_batch lays them out."""
    table, src_off, gray_off = [], 0, 0
    for im in images:
        h, w, c = im.shape[0], im.shape[1], 1 if im.ndim == 2 else im.shape[2]
        table.append((src_off, gray_off, h, w, c))
        src_off, gray_off = src_off + h * w * c, gray_off + h * w
    src = torch.from_numpy(np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images])).cuda()
    return src, torch.tensor(table, dtype=torch.int64, device="cuda"), gray_off


def _gray_planes_equal(torch, images, found):
    """One detect call at the kernels level: the whole gray buffer is rule 1 of every image, concatenated, and the counts agree."""
    from ransac_with_homography_amd import kernels
    src, table, gray_bytes = _pack(torch, images)
    gray, _, counts = kernels.orb_detect_batched(src, table, gray_bytes, 20, 64)
    assert gray.shape[0] == gray_bytes and counts.cpu().tolist() == found
    return np.array_equal(gray.cpu().numpy(), np.concatenate([oc.gray(im).reshape(-1) for im in images]))


def test_strided_walk_small(gpu):
    """1 480 tiles on 334 blocks: every block walks four or five tiles, and the images with keypoints come last in the list."""
    strips = [oc.strip(4097, (1, 3, 4)[i % 3], 200 + i) for i in range(20)]
    narrows = [oc.narrow(s) for s in range(30)]
    images = strips + narrows
    tiles, blocks = _sizing(images)
    assert (tiles, blocks) == (1480, 334) and tiles >= 4 * blocks
    first = oc.extract(images)
    assert [r["found"] for r in first[:20]] == [0] * 20
    for s, (img, got) in enumerate(zip(narrows, first[20:])):
        assert oc.same(got, oc.restate(img)) and oc.same(got, _host(img)), s
    assert sum(r["found"] for r in first[20:]) > 40
    assert _gray_planes_equal(gpu, images, [r["found"] for r in first])
    again = oc.extract(images)
    assert all(oc.same(a, b) for a, b in zip(again, first))


def test_strided_walk_capped_grid(gpu):
    """About 140 000 tiles on the capped grid of 16 384 blocks, eight or nine tiles per block, as every large frame has it; behind
    130 strips the wide and the tall image with keypoints at 65519 and five narrow images."""
    strips = [oc.strip(65536, 1, 300 + i) for i in range(130)]
    (wide, strong_w, weak_w), (tall, strong_t, weak_t) = oc.wide_image(), oc.tall_image()
    rest = [wide.copy(), tall] + [oc.narrow(s) for s in (0, 1, 2, 7, 11)]    # the shared image is read-only; torch wants a writable one
    images = strips + rest
    tiles, blocks = _sizing(images)
    assert blocks == 16384 and tiles >= 4 * blocks
    first = oc.extract(images)
    assert [r["found"] for r in first[:130]] == [0] * 130
    for i, (img, got) in enumerate(zip(rest, first[130:])):
        assert oc.same(got, oc.restate(img)) and oc.same(got, _host(img)), i
    for got, strong, weak in ((first[130], strong_w, weak_w), (first[131], strong_t, weak_t)):
        kept = set(map(tuple, got["kps"].astype(int).tolist()))
        assert kept == set(strong) and not kept & set(weak) and max(max(k) for k in kept) == 65519
    assert _gray_planes_equal(gpu, images, [r["found"] for r in first])


@pytest.mark.parametrize("n", [257, 600])
def test_more_than_256_images(gpu, n):
    """orb_setup_kernel gives each of its 256 lanes ceil(n / 256) = 2 or 3 images; every image of the batch is numbered."""
    images = [oc.numbered(i) for i in range(n)]
    got = oc.extract(images)
    for i, (img, r) in enumerate(zip(images, got)):
        x, y, s = oc.keypoints(oc.scores(img), 20)
        assert r["found"] == len(x) >= 1 and np.array_equal(r["kps"], np.stack([x, y], axis=1).astype(np.float32)), i
        assert np.array_equal(r["score"], s.astype(np.int32)), i
    for i in sorted({0, 1, 64, 127, n // 2, 254, 255, 256, n - 2, n - 1}):
        alone, = oc.extract([images[i]])
        assert oc.same(alone, got[i]) and oc.same(alone, oc.restate(images[i])), i


def _detect_alone(torch, img, capacity):
    from ransac_with_homography_amd import kernels
    src, table, gray_bytes = _pack(torch, [img])
    _, keys, counts = kernels.orb_detect_batched(src, table, gray_bytes, 20, capacity)
    return keys.cpu().numpy()[0], int(counts.cpu()[0])


def test_void_rows(gpu):
    """A hand-made table: six narrow images between rows that describe no image, one for each reason include/rwh.h names; row 0
    and the last row are void, rows 2 and 3 are consecutive void rows.  A void row has no keypoints and writes nothing; its
    neighbours are found as they are alone.  The buffers are laid out with gaps, a spare region the void rows point at, and guard
    bytes behind; the last image ends exactly at images_bytes and gray_bytes, and two void rows are that row moved on by one byte."""
    torch = gpu
    from ransac_with_homography_amd import kernels
    valid = [oc.narrow(s) for s in (0, 1, 2, 3, 5, 7)]
    assert {im.shape[2:] for im in valid} == {(), (3,), (4,)}
    H, W, CAP, NF = 33, 65, 32, 16
    rng = np.random.RandomState(12)
    src_np, src_at, gray_at, gray_bytes = [], [], [], 0
    for i, im in enumerate(valid):
        if i == len(valid) - 1:                                               # the spare region sits before the last image
            spare_src, spare_gray = sum(len(a) for a in src_np), gray_bytes
            src_np.append(rng.randint(0, 256, H * W * 4).astype(np.uint8))
            gray_bytes += H * W
        src_at.append(sum(len(a) for a in src_np))
        gray_at.append(gray_bytes)
        src_np += [im.reshape(-1)] + ([rng.randint(0, 256, 5).astype(np.uint8)] if i < len(valid) - 1 else [])
        gray_bytes += H * W + (7 if i < len(valid) - 1 else 0)
    src_np = np.concatenate(src_np)
    images_bytes = len(src_np)
    c_last = valid[-1].shape[2]
    assert src_at[-1] + H * W * c_last == images_bytes and gray_at[-1] + H * W == gray_bytes
    V = lambda i: (src_at[i], gray_at[i], H, W, 1 if valid[i].ndim == 2 else valid[i].shape[2])
    rows = [(spare_src, spare_gray, 0, W, 1), V(0), (spare_src, spare_gray, H, 0, 1), (spare_src, spare_gray, 65537, 1, 1), V(1),
            (spare_src, spare_gray, H, W, 2), V(2), (-1, spare_gray, H, W, 1), V(3), (spare_src, -1, H, W, 1), V(4),
            (src_at[-1] + 1, spare_gray, H, W, c_last), V(5), (spare_src, gray_at[-1] + 1, H, W, 1)]
    where = {1: 0, 4: 1, 6: 2, 8: 3, 10: 4, 12: 5}                            # table row -> valid image
    n = len(rows)
    src_buf = torch.zeros(images_bytes + 64, dtype=torch.uint8, device="cuda")
    src_buf[:images_bytes] = torch.from_numpy(src_np).cuda()
    table = torch.tensor(rows, dtype=torch.int64, device="cuda")
    gray_buf = torch.full((gray_bytes + 64,), FILL, dtype=torch.uint8, device="cuda")
    guard = torch.full((n * CAP + 64,), -12345, dtype=torch.int64, device="cuda")
    gray, keys, counts = kernels.orb_detect_batched(src_buf[:images_bytes], table, gray_bytes, 20, CAP, out_keys=guard[:n * CAP].view(n, CAP),
                                                    out_gray=gray_buf)
    assert gray.data_ptr() == gray_buf.data_ptr() and keys.data_ptr() == guard.data_ptr()
    g, k, cnt = gray_buf.cpu().numpy(), guard.cpu().numpy(), counts.cpu().numpy()
    want_gray = np.full(gray_bytes + 64, FILL, dtype=np.uint8)
    for i, im in enumerate(valid):
        want_gray[gray_at[i]:gray_at[i] + H * W] = oc.gray(im).reshape(-1)
    assert np.array_equal(g, want_gray)                                      # gaps, spare plane and guard bytes keep the prefill
    assert (k[n * CAP:] == -12345).all()
    k = k[:n * CAP].reshape(n, CAP)
    for r in range(n):
        if r not in where:
            assert cnt[r] == 0 and (k[r] == KEY_NONE).all(), r
            continue
        img = valid[where[r]]
        alone_keys, alone_count = _detect_alone(torch, img, CAP)
        truth = oc.key_set(img)
        assert cnt[r] == alone_count == len(truth) <= CAP and (k[r, cnt[r]:] == KEY_NONE).all(), r
        assert set(k[r, :cnt[r]].tolist()) == set(alone_keys[:alone_count].tolist()) == truth, r
    assert sum(int(cnt[r]) for r in where) > 10
    bin_table, rot = oc.tables()
    out = kernels.orb_describe_batched(gray_buf, gray_bytes, table, torch.sort(keys, dim=1).values.contiguous(), counts, NF,
                                       torch.from_numpy(bin_table).cuda(), torch.from_numpy(rot).cuda())
    kps, desc, score, bins = (t.cpu().numpy() for t in out)
    for r in range(n):
        c = int(cnt[r]) if r in where else 0
        assert not kps[r, c:].any() and not desc[r, c:].any() and not score[r, c:].any() and not bins[r, c:].any(), r
        if r in where:
            want = oc.restate(valid[where[r]], n_features=NF)
            assert c == len(want["score"]) <= NF
            assert oc.same(dict(kps=kps[r, :c], desc=desc[r, :c], score=score[r, :c], bin=bins[r, :c], found=c), want), r


def test_arcs_and_bins_on_the_device(gpu):
    """Both mosaics and the bin wheel in one batch, at threshold 20 and again at 254: each image equals the restatement and the host
    twin at that threshold, and on the device's own result every 9-arc at threshold + 1 is a keypoint of that score, every 9-arc at
    the threshold and every 8-arc is none, and the wheel's 30 centres have the bins 0 .. 29."""
    (m20, must20, not20), (m254, must254, not254), (wheel, centres) = oc.arc_mosaic(20), oc.arc_mosaic(254), oc.bin_wheel()
    images = [m20, m254, wheel]
    for threshold, k, must, must_not in ((20, 0, must20, not20), (254, 1, must254, not254)):
        got = oc.extract(images, threshold=threshold)
        for i, (img, r) in enumerate(zip(images, got)):
            assert oc.same(r, oc.restate(img, threshold=threshold)) and oc.same(r, _host(img, threshold=threshold)), (threshold, i)
        at = {(int(x), int(y)): int(s) for (x, y), s in zip(got[k]["kps"], got[k]["score"])}
        assert len(must) == 32 and all(at.get((x, y)) == s == threshold + 1 for x, y, s in must)
        assert len(must_not) == 64 and not any(c in at for c in must_not)
        assert got[k]["found"] == len(got[k]["score"])                       # nothing cut: `at` is every keypoint
        w = got[2]
        assert w["kps"][:30].astype(int).tolist() == [list(c) for c in centres] and w["bin"][:30].tolist() == list(range(30))
        assert (w["score"][:30] == 255).all() and w["found"] == (55 if threshold == 20 else 30)


def test_describe_skip_paths(gpu):
    """The keys of a small real batch, damaged: the slots include/rwh.h says are skipped stay zero in all four outputs, every other
    slot is what the undamaged keys give.  A: 40 x 48 RGB, B: 50 x 70 gray, C: three dots."""
    torch = gpu
    from ransac_with_homography_amd import kernels
    A, B = oc.random_image(40, 48, 1), oc.random_image(50, 70, 9, channels=1)
    C = oc.dots(40, 48, [(16, 16, 200), (31, 23, 255), (24, 20, 90)])
    images, CAP, NF = [A, B, C], 128, 32
    src, table, gray_bytes = _pack(torch, images)
    gray, keys, counts = kernels.orb_detect_batched(src, table, gray_bytes, 20, CAP)
    keys = torch.sort(keys, dim=1).values.contiguous()
    cnt = counts.cpu().tolist()
    assert 8 < cnt[0] < NF < cnt[1] < CAP and cnt[2] == 3                    # B is cut at n_features
    bin_table, rot = oc.tables()
    bins_t, rot_t = torch.from_numpy(bin_table).cuda(), torch.from_numpy(rot).cuda()

    def describe(keys, counts, nf=NF):
        return [t.cpu().numpy() for t in kernels.orb_describe_batched(gray, gray_bytes, table, keys, counts, nf, bins_t, rot_t)]
    clean = describe(keys, counts)
    for i, img in enumerate(images):
        want, kept = oc.restate(img, n_features=NF), min(cnt[i], NF)
        assert oc.same(dict(kps=clean[0][i, :kept], desc=clean[1][i, :kept], score=clean[2][i, :kept], bin=clean[3][i, :kept], found=cnt[i]), want), i
        assert not any(t[i, kept:].any() for t in clean)
    # 1. damaged keys inside A's count, and C's count raised above key_stride (its slots 3 .. 31 are then read: KEY_NONE, skipped)
    k = keys.cpu().numpy().copy()
    k[0, 1] = KEY_NONE
    k[0, 2] |= 1 << 40
    k[0, 3] = (k[0, 3] & ~0xFFFF) | 15                                       # one column left of the border
    k[0, 4] = (k[0, 4] & ~0xFFFFFFFF) | 30 << 16 | 50                        # (50, 30): a legal centre of B (50 x 70), not of A (40 x 48)
    c = counts.clone()
    c[2] = CAP + 5
    bad = describe(torch.from_numpy(k).cuda(), c)
    for t_bad, t_clean in zip(bad, clean):
        want = t_clean.copy()
        want[0, 1:5] = 0
        assert np.array_equal(t_bad, want)
    # 2. key_stride < n_features: only the first key_stride slots of a row exist
    STRIDE = 8
    short = describe(keys[:, :STRIDE].contiguous(), counts)
    for t_short, t_clean in zip(short, clean):
        want = t_clean.copy()
        want[:, STRIDE:] = 0
        assert np.array_equal(t_short, want)
    assert all(clean[j][:2, STRIDE:].any() for j in range(3))               # there was something to leave out
