"""The stream contract of include/rwh.h on the GPU: every record of tests/stream_contract_cases.py eager on a side stream, captured
into a graph on that stream, and replayed twice on new device inputs after its host arguments were overwritten.  A launch or memset
on another stream, a synchronisation or an allocation fails the capture; work done at capture time shows in the outputs, which must
still hold their fill; a host table read at replay, or state left by the first replay and read by the second, shows as a wrong
result.  Every comparison is exact."""
import numpy as np
import pytest

import sequence_cases as sc
import stream_contract_cases as scc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return sc.library(gpu=True)


def _check(live, inputs, want, step, tail=True):
    got = [out.fetch() for out in live.outputs]                      # asserts the canaries
    if live.compare is not None:
        live.compare(got, want)
    else:
        for k, (out, g, w) in enumerate(zip(live.outputs, got, want)):
            assert g.shape == w.shape and np.array_equal(g, w), "%s: %s (output %d) differs in %d of %d bytes" % (
                step, out.what, k, int((g != w).sum()), w.size)
    if live.verify is not None:
        live.verify(inputs, got)
    if tail and live.workspace is not None:
        live.workspace.check_tail()


def _want(live, seed):
    """New device inputs, and what the outputs have to be for them: the record's reference, or, where the suite has no bit-exact
    one, the same call made eagerly on the default stream into the shadow's own outputs and workspace."""
    import torch
    inputs = live.refresh(seed)
    if live.shadow is None:
        return inputs, live.expected(inputs)
    for out in live.shadow.outputs:
        out.reset()
    torch.cuda.synchronize()
    assert live.shadow.call(torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    want = [out.fetch() for out in live.shadow.outputs]
    if live.shadow.workspace is not None:
        live.shadow.workspace.check_tail()
    return inputs, want


def _differ(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(scc.RECORDS))
def test_record(lib, name):
    import torch
    live = scc.RECORDS[name].make(lib)
    live.alloc()                                                      # every allocation, before the capture
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    inputs, want = _want(live, 0)
    wants = [want]
    torch.cuda.synchronize()
    # 1. eager on a side stream (the warm-up a capture needs as well)
    assert live.call(s.cuda_stream) == 0
    s.synchronize()
    _check(live, inputs, want, "eager on a side stream")
    # 2. capture, one call on one stream
    for out in live.outputs:
        out.reset()
    if live.workspace is not None:
        live.workspace.reset()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        status = live.call(torch.cuda.current_stream().cuda_stream)
    assert status == 0
    torch.cuda.synchronize()
    # 3. nothing ran and nothing leaked
    for out in live.outputs:
        assert np.array_equal(out.fetch(), out.untouched()), "the capture wrote the %s: work ran outside the captured stream" % out.what
    assert live.workspace is None or live.workspace.untouched(), "the capture wrote the workspace: work ran outside the captured stream"
    # 4. host memory was read before the call returned
    live.spoil_host_args()
    # 5. two replays on new device inputs, the second on what the first left behind
    for seed in (1, 2):
        inputs, want = _want(live, seed)
        wants.append(want)
        if live.constant:                                             # nothing to refresh: the fill comes back, so that a flag the
            for out in live.outputs:                                  # call does not clear itself cannot come out right
                out.reset()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _check(live, inputs, want, "replay %d" % seed, tail=seed == 2)
    # (a record without any device input has nothing to refresh: its outputs were put back to their fill before the capture instead)
    assert live.constant or (_differ(wants[0], wants[1]) and _differ(wants[0], wants[2]) and _differ(wants[1], wants[2])), "a stale output could pass"
    print("%s: %s" % (name, live.reached))


def test_launchers_run_on_torchs_current_stream(lib):
    """_lib.stream_ptr() follows torch's current stream, and two launchers that take `out=` and device inputs alone are captured on a
    side stream and replay to their eager result: stitch_sequence_on without gains, and refit_batched."""
    import torch
    import refit_cases as rf
    from ransac_with_homography_amd import _lib, kernels
    s = torch.cuda.Stream()
    assert _lib.stream_ptr().value == (torch.cuda.current_stream().cuda_stream or None)
    with torch.cuda.stream(s):
        assert _lib.stream_ptr().value == s.cuda_stream
    assert _lib.stream_ptr().value == (torch.cuda.current_stream().cuda_stream or None)
    _, images, Gs, anchor, order = sc.general_cases()[4]
    t = sc.tables(images, Gs, anchor, order)
    on = sc.upload(images)
    geom = sc.geometry(t)
    eager = kernels.stitch_sequence_on(on, geom, t["order"], sc.FEATHER).clone()
    can = torch.full_like(eager, scc.FILL)
    u, v = rf.synthetic(300)
    words = rf.pack(rf.random_bits(300, 5))
    pa, pb = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
    off = torch.tensor([0, 300], dtype=torch.int32, device="cuda")
    masks = torch.from_numpy(words.view(np.int64).reshape(1, -1)).cuda()
    H, status = (x.clone() for x in kernels.refit_batched(pa, pb, off, masks))
    assert int(status[0]) == 0
    torch.cuda.synchronize()
    with torch.cuda.stream(s):                                        # the warm-up a capture needs
        kernels.stitch_sequence_on(on, geom, t["order"], sc.FEATHER, out=can)
        kernels.refit_batched(pa, pb, off, masks)
    s.synchronize()
    can.fill_(scc.FILL)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        kernels.stitch_sequence_on(on, geom, t["order"], sc.FEATHER, out=can)
        H2, status2 = kernels.refit_batched(pa, pb, off, masks)
    torch.cuda.synchronize()
    assert (can == scc.FILL).all()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(can, eager) and torch.equal(H2.view(torch.int64), H.view(torch.int64)) and torch.equal(status2, status)
