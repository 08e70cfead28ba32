"""The stream contract of include/rwh.h's preamble, one record per device entry point (and per driver that enqueues differently):
host memory is read before the call returns, work is enqueued on the caller's stream without synchronising, nothing is allocated and
no state is kept.  tests/test_stream_contract_gpu.py walks every record through a side stream, a capture and two replays;
tests/test_stream_contract_cpu.py holds the table to the header.

A record is made on the host alone (`RECORDS[name].make(lib)` -> a `Live`), so its references can be checked without a GPU; `alloc()`
then puts its inputs, outputs and workspace on the device.  The references are the existing ones: the host twins of the library and
the restatements of the case modules, byte for byte wherever the suite itself holds the entry point to them byte for byte.

Where it does not, a record has a `shadow`: the same call made eagerly on the default stream into outputs and a workspace of its
own, whose bytes the side-stream call and the replays must equal -- the test is about streams, not arithmetic -- and a `verify`
with what the suite's reference does say.  These are:
  the fast warp plans (u8 bilinear, the batch walk, nearest)  other tests hold their accuracy against the oracle (1e-4 relative);
  rwh_dlt4_batched       K1's H is the float32 rounding of an elimination, the oracle's of LAPACK's SVD: tests/test_k1_gpu.py counts the
                         rows that agree bit for bit and bounds the rest; verify: the repeated-index flags, which are exact;
  rwh_ransac_search      K1 in front: the hypotheses are K1's.  'fwd': verify holds counts, masks and keys to the oracle on K1's own
                         H, exactly; 'reproj' scores through the kernel's own float64 inverse, which the header says rounds apart from
                         numpy.linalg.inv for a nearly singular sample (random samples hold some), so only the keys are held to the counts;
  rwh_ransac_batched     the same K1 in front; the header's claim is equality with rwh_ransac_search, device against device;
                         verify: the device sampler against tests/philox_ref.py, exactly;
  rwh_score_interval     its numpy emulation (tests/interval_emulation.py) rounds an fma differently: the suite allows +-1 there;
                         verify: 0 <= lo <= hi <= m;
  rwh_refit_batched      tests/test_refit_gpu.py prints, and does not assert, bit identity with rwh_host_refit (sqrt and divide may
                         round differently on the two targets); verify: that test's own hold, statuses and the yardstick's margin."""
import ctypes

import numpy as np

import block_gain_cases as bg
import gain_cases as gc
import projection_cases as pc
import ring_cases as rc
import sequence_cases as sc

FILL, SPOIL, TAIL = 0xA5, 0x5A, 4096


# ---- what a record is made of ----
class DevIn(object):
    """A device input and its host mirror: `host` is what the reference reads, `dev` the tensor the entry point reads.  vary(seed):
    new contents of the same shape and dtype for `refresh`; None: the input keeps its contents (geometry on the device)."""
    def __init__(self, host, vary=None):
        self.host, self.vary, self.dev = np.ascontiguousarray(host), vary, None

    def alloc(self):
        import torch
        self.dev = torch.from_numpy(self.host.copy()).cuda()

    def set(self, host):
        import torch
        host = np.ascontiguousarray(host, dtype=self.host.dtype)
        assert host.shape == self.host.shape
        self.host = host
        if self.dev is not None:
            self.dev.copy_(torch.from_numpy(host.copy()))          # the same tensor: the address a captured call holds stays

    @property
    def ptr(self):
        return self.dev.data_ptr()


class Out(object):
    """A device output of `nbytes`, filled with 0xA5 between two 64-byte canaries (as sc.guarded_device_canvas).  initial: the bytes
    an accumulator starts from (the packed keys of rwh_score_count, which the caller clears): an output that is an input too, put
    back by every `refresh`; None: 0xA5, and only `reset` puts it back."""
    def __init__(self, nbytes, what="output", initial=None):
        self.nbytes, self.what, self.buf = int(nbytes), what, None
        self.initial = None if initial is None else np.ascontiguousarray(initial).view(np.uint8).reshape(-1).copy()
        assert self.initial is None or self.initial.size == self.nbytes

    def alloc(self):
        import torch
        self.buf = torch.full((self.nbytes + 128,), FILL, dtype=torch.uint8, device="cuda")
        self.reset()

    def reset(self):
        import torch
        self.buf.fill_(FILL)
        if self.initial is not None:
            self.buf[64:-64].copy_(torch.from_numpy(self.initial))

    def untouched(self):
        """The payload as `reset` leaves it."""
        return np.full(self.nbytes, FILL, dtype=np.uint8) if self.initial is None else self.initial

    def clone(self):
        return Out(self.nbytes, self.what, self.initial)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 64

    def fetch(self):
        flat = self.buf.cpu().numpy()
        assert (flat[:64] == FILL).all() and (flat[-64:] == FILL).all(), "a byte outside the %s was written" % self.what
        return flat[64:-64].copy()


class Workspace(object):
    """A workspace of the size function's bytes, filled with 0xA5, and a 4096-byte tail behind it that must stay so."""
    def __init__(self, nbytes):
        assert nbytes > 0, nbytes
        self.nbytes, self.buf = int(nbytes), None

    def alloc(self):
        import torch
        self.buf = torch.full((self.nbytes + TAIL,), FILL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 8 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def reset(self):
        self.buf.fill_(FILL)

    def untouched(self):
        return bool((self.buf.cpu().numpy() == FILL).all())

    def check_tail(self):
        assert (self.buf[self.nbytes:].cpu().numpy() == FILL).all(), "a byte beyond the workspace's stated size was written"


class Live(object):
    """One record, made: call(stream_ptr) -> status; host_args: the numpy arrays the call passes as host memory; refresh(seed) ->
    inputs (seed 0: the case's own contents); outputs: [Out]; workspace: Workspace or None; expected(inputs) -> one uint8 array per
    output, compared byte for byte; reached: which kernel or driver the record is there for (profiles/stream_contract.txt)."""
    def __init__(self, inputs, outputs, workspace, host_args, call, expected, reached, shadow=None, compare=None, verify=None):
        self.inputs, self.outputs, self.workspace, self.host_args = inputs, outputs, workspace, host_args
        self._call, self._expected, self.reached = call, expected, reached
        # shadow: for an entry point without a bit-exact reference in the suite, the same call with outputs and a workspace of its
        # own, run eagerly on the default stream: its result is what the record's outputs are compared with; compare(got, want):
        # in place of the byte comparison; verify(inputs, got): what the suite's reference does say about the outputs
        self.shadow, self.compare, self.verify = shadow, compare, verify
        self.on_device = False
        self.constant = False        # True: the entry point has no device input, so `refresh` cannot change what it computes

    def alloc(self, inputs=True):
        for x in (self.inputs if inputs else []) + self.outputs + ([] if self.workspace is None else [self.workspace]):
            x.alloc()
        self.on_device = True
        if self.shadow is not None:
            self.shadow.alloc(inputs=False)

    def refresh(self, seed):
        for i, x in enumerate(self.inputs):
            if x.vary is not None:
                x.set(x.vary(seed) if seed else x.first)
        if self.on_device:
            for out in self.outputs:
                if out.initial is not None and not getattr(out, "keep", False):
                    out.reset()
        return [x.host.copy() for x in self.inputs]

    def call(self, stream_ptr):
        return self._call(ctypes.c_void_p(stream_ptr))

    def expected(self, inputs):
        return [np.ascontiguousarray(e).view(np.uint8).reshape(-1) for e in self._expected(inputs)]

    def spoil_host_args(self):
        for a in self.host_args:
            a.view(np.uint8).reshape(-1)[:] = SPOIL


def _live(inputs, *a, **k):
    for x in inputs:
        x.first = x.host.copy()
    return Live(inputs, *a, **k)


class Record(object):
    def __init__(self, name, entry, make):
        self.name, self.entry, self.make = name, entry, make


RECORDS = {}

# entry points that take a stream and have no record, each with its reason
EXEMPT = {
    "rwh_sequence_seams": "synchronises the stream between its relaxation passes (the seam rule): it cannot be captured",
    "rwh_sequence_seams_proj": "synchronises the stream between its relaxation passes (the seam rule): it cannot be captured",
    "rwh_ransac_run": "synchronises `stream`: the settle step reads counts and flags on the host",
}
# lab kernels: not part of the data path, excused from the header check of the exemptions
EXEMPT_LAB = {
    "rwh_lab_clock_probe": "a lab kernel that keeps one wavefront spinning on purpose for up to two seconds",
}


def record(name, entry):
    def deco(make):
        assert name not in RECORDS, name
        RECORDS[name] = Record(name, entry, make)
        return make
    return deco


def image_vary(shape, key):
    return lambda seed: np.random.default_rng(100000 * seed + key).integers(0, 256, shape, dtype=np.uint8)


# ---- the sequence family: one maker for every entry point of the layout `images hw mats rects n ... workspace bytes stream ...` ----
def _conv(items, side):
    """An argument list for one side: "dev" the device call, "host" the host twin on pristine tables."""
    out = []
    for it in items:
        if isinstance(it, DevIn):
            out.append(it.ptr if side == "dev" else it.host.ctypes.data)
        elif isinstance(it, Out):
            out.append(it.ptr if side == "dev" else it.twin.ctypes.data)
        elif isinstance(it, _Table):
            out.append(it.live.ctypes.data if side == "dev" else it.pristine.ctypes.data)
        else:
            out.append(it)
    return tuple(out)


class _Table(object):
    """A host table of the call: `live` is passed to the device call (and spoiled after the capture), `pristine` to the twin."""
    def __init__(self, array):
        self.pristine = np.ascontiguousarray(array)
        self.live = self.pristine.copy()

    def clone(self):
        return _Table(self.pristine)


def sequence_live(lib, entry, t, images, own, canvas, tail, post, ws_bytes, reached):
    """entry: the device entry point; its twin is rwh_host_<rest> with the same list less `workspace bytes stream`.  t: sc.tables,
    pc.tables or rc.tables; own / canvas / tail / post: the pieces of bg.layout, `post` what follows the stream; items are scalars,
    numpy arrays (host tables), DevIn (device inputs) and Out (device outputs)."""
    n = t["n"]
    curved = "m" in t
    imgs = [DevIn(im, image_vary(im.shape, 7 * i + 1)) for i, im in enumerate(images)]
    rays = [DevIn(t["col"]), DevIn(t["row"])] if curved else []
    pieces = [[_Table(it) if isinstance(it, np.ndarray) else it for it in p] for p in (own, canvas, tail, post)]
    flat = [it for p in pieces for it in p]
    extra = [it for it in flat if isinstance(it, DevIn)]
    outs = [it for it in flat if isinstance(it, Out)]
    tabs = {k: _Table(t[k]) for k in ("hw", "m" if curved else "inv", "rects")}
    ptrs = _Table(np.zeros(n, dtype=np.uint64))
    ws = Workspace(ws_bytes)
    twin = getattr(lib, "rwh_host_" + entry[len("rwh_"):])
    device = getattr(lib, entry)

    def call(stream):
        ptrs.live[:] = [x.ptr for x in imgs]
        td = dict(t, **{k: v.live for k, v in tabs.items()})
        if curved:
            td.update(col=bg._Addr(rays[0].ptr), row=bg._Addr(rays[1].ptr))
        o, c, tl, p = (_conv(x, "dev") for x in pieces)
        st = device(*bg.layout(td, ptrs.live, o, c, tl + (ws.ptr, ws.nbytes, stream) + p))
        return st

    def expected(inputs):
        hosts = [np.ascontiguousarray(a) for a in inputs[:n]]
        kept = [x.host for x in extra]
        for x, a in zip(extra, inputs[n + len(rays):]):
            x.host = np.ascontiguousarray(a)
        hp = np.array([a.ctypes.data for a in hosts], dtype=np.uint64)
        th = dict(t, **{k: v.pristine for k, v in tabs.items()})
        for o in outs:
            o.twin = np.full(o.nbytes + 128, FILL, dtype=np.uint8)[64:-64]
        o_, c, tl, p = (_conv(x, "host") for x in pieces)
        st = twin(*bg.layout(th, hp, o_, c, tl + p))
        for x, a in zip(extra, kept):
            x.host = a
        assert st == 0, (entry, st)
        for o in outs:
            assert (o.twin.base[:64] == FILL).all() and (o.twin.base[-64:] == FILL).all()
        return [o.twin.copy() for o in outs]

    host_args = [ptrs.live] + [v.live for v in tabs.values()] + [it.live for it in flat if isinstance(it, _Table)]
    return _live(imgs + rays + extra, outs, ws, host_args, call, expected, reached)


def _plane5():
    _, images, Gs, anchor, order = sc.general_cases()[4]
    return images, sc.tables(images, Gs, anchor, order)


def _proj5():
    _, images, Gs, anchor, order, f = pc.general_cases()[4]
    return images, pc.tables(images, Gs, anchor, "cylindrical", f, order)


def _ring12():
    return rc.circle_tables(256, "cylindrical")


def _strip64():
    images, Gs = sc.translated_strip(64)
    return images, sc.tables(images, Gs, 0)


def _maps_case(form):
    if form == "":
        images, Gs = bg.partial_cells()
        return images, sc.tables(images, Gs, 0)
    images, Gs, kind, f = bg.cylinder_case()
    return images, pc.tables(images, Gs, 0, kind, f)


SEQ_CASES = {"": _plane5, "_proj": _proj5, "_ring": _ring12}
B = 16


def _maps_in(t, seed0):
    n, size = t["n"], t["size"]
    return DevIn(bg.wavy_maps(n, size, B, seed0), lambda seed: bg.wavy_maps(n, size, B, seed0 + 10 * seed))


def _labels_in(t, seed0):
    n, size = t["n"], t["size"]
    return DevIn(bg.stripes(size, n, seed0), lambda seed: bg.stripes(size, n, seed0 + 10 * seed))


def _compositor(name, form, blend, gains, rows=None, case=None):
    """rwh_stitch_sequence (gains "off": the plain entry, plane only) / _ex / _proj / _ring (gains None or "n") / _maps / _maps_proj."""
    maps = gains == "maps"
    entry = "rwh_stitch_sequence" + ("_maps" + form if maps else ("" if gains == "off" else form or "_ex"))

    @record(name, entry)
    def make(lib):
        images, t = (case or ((lambda: _maps_case(form)) if maps else SEQ_CASES[form]))()
        fh, fw = t["size"]
        r0, r1 = (0, fh) if rows is None else (rows[0], fh - rows[1])
        if maps:
            post = (_maps_in(t, 3), bg.shift_of(B))
        elif gains == "off":
            post = ()
        else:
            post = (None if gains is None else np.ascontiguousarray(gc.mixed_gains(t["n"]), dtype=np.float64),)
        return sequence_live(lib, entry, t, images, (t["order"], blend), (Out(fh * fw * 3, "canvas"), fh, fw), (r0, r1), post,
                             lib.rwh_stitch_sequence_workspace_bytes(t["n"]),
                             "seq_%s, %s, %d images%s" % ("feather" if blend else "paste", {None: "no gains", "off": "no gains", "n": "N gains",
                                                                                         "maps": "gain maps"}[gains], t["n"],
                                                          "" if rows is None else ", rows %d .. %d" % (r0, r1)))


_compositor("stitch_sequence paste", "", sc.PASTE, "off")
_compositor("stitch_sequence feather rows", "", sc.FEATHER, "off", rows=(3, 4))
_compositor("stitch_sequence strip of 64", "", sc.PASTE, "off", case=_strip64)
for _form in ("", "_proj", "_ring"):
    _n = "stitch_sequence" + (_form or "_ex")
    _compositor(_n + " paste no gains", _form, sc.PASTE, None)
    _compositor(_n + " feather gains", _form, sc.FEATHER, "n")
    _compositor(_n + " paste gains", _form, sc.PASTE, "n")
_compositor("stitch_sequence_ex feather strip of 64 gains", "", sc.FEATHER, "n", case=_strip64)
_compositor("stitch_sequence_proj feather rows", "_proj", sc.FEATHER, None, rows=(2, 3))
_compositor("stitch_sequence_ring paste rows", "_ring", sc.PASTE, "n", rows=(1, 2))
for _form in ("", "_proj"):
    _compositor("stitch_sequence_maps%s paste" % _form, _form, sc.PASTE, "maps")
    _compositor("stitch_sequence_maps%s feather" % _form, _form, sc.FEATHER, "maps")


def _multiband(name, form, bands, gains=None, labels=False, case=None):
    """rwh_stitch_multiband / _proj / _ring, _labels / _labels_proj, _maps / _maps_proj (labels: a plane, or NULL)."""
    maps = gains == "maps"
    entry = "rwh_stitch_multiband" + ("_maps" if maps else "_labels" if labels else "") + form

    @record(name, entry)
    def make(lib):
        images, t = (case or ((lambda: _maps_case(form)) if maps else SEQ_CASES[form]))()
        fh, fw = t["size"]
        lab = (_labels_in(t, 5),) if labels else ()
        if maps:
            own = (bands, _maps_in(t, 4), bg.shift_of(B)) + (lab or (None,))
        else:
            own = (bands, None if gains is None else np.ascontiguousarray(gc.mixed_gains(t["n"]), dtype=np.float64)) + lab
        if form == "_ring":
            need = lib.rwh_stitch_multiband_ring_workspace_bytes(t["rects"].ctypes.data, t["n"], fh, fw, bands)
        else:
            ox, oy = bg.origin_of(t)
            need = lib.rwh_stitch_multiband_workspace_bytes(t["rects"].ctypes.data, t["n"], fh, fw, ox, oy, bands)
        return sequence_live(lib, entry, t, images, own, (Out(fh * fw * 3, "canvas"), fh, fw), (), (), need,
                             "multiband, %d bands, %s%s, %d images" % (bands, {None: "no gains", "n": "N gains", "maps": "gain maps"}[gains],
                                                                      ", labels" if labels else "", t["n"]))


for _form in ("", "_proj", "_ring"):
    _multiband("stitch_multiband%s bands 1" % _form, _form, 1)
    _multiband("stitch_multiband%s bands 3 gains" % _form, _form, 3, "n")
_multiband("stitch_multiband bands 2 strip of 64", "", 2, case=_strip64)
for _form in ("", "_proj"):
    _multiband("stitch_multiband_labels%s bands 1" % _form, _form, 1, labels=True)
    _multiband("stitch_multiband_labels%s bands 3 gains" % _form, _form, 3, "n", labels=True)
    _multiband("stitch_multiband_maps%s bands 1" % _form, _form, 1, "maps")
    _multiband("stitch_multiband_maps%s bands 3 labels" % _form, _form, 3, "maps", labels=True)


def _label_paste(name, form, gains):
    maps = gains == "maps"
    entry = "rwh_stitch_sequence_labels" + ("_maps" if maps else "") + form

    @record(name, entry)
    def make(lib):
        images, t = (_maps_case(form) if maps else SEQ_CASES[form]())
        fh, fw = t["size"]
        if maps:
            own = (_maps_in(t, 6), bg.shift_of(B), _labels_in(t, 7))
        else:
            own = (None if gains is None else np.ascontiguousarray(gc.mixed_gains(t["n"]), dtype=np.float64), _labels_in(t, 7))
        return sequence_live(lib, entry, t, images, own, (Out(fh * fw * 3, "canvas"), fh, fw), (), (),
                             lib.rwh_stitch_sequence_workspace_bytes(t["n"]),
                             "label paste, %s, %d images" % ({None: "no gains", "n": "N gains", "maps": "gain maps"}[gains], t["n"]))


for _form in ("", "_proj"):
    _label_paste("stitch_sequence_labels%s" % _form, _form, None)
    _label_paste("stitch_sequence_labels%s gains" % _form, _form, "n")
    _label_paste("stitch_sequence_labels_maps%s" % _form, _form, "maps")


def _overlap(name, form, stride, case=None):
    entry = "rwh_sequence_overlap_stats" + form

    @record(name, entry)
    def make(lib):
        images, t = (case or SEQ_CASES[form])()
        fh, fw = t["size"]
        n = t["n"]
        return sequence_live(lib, entry, t, images, (), (fh, fw), (stride, Out(n * n * 8, "count table"), Out(n * n * 8, "sum table")), (),
                             lib.rwh_sequence_overlap_stats_workspace_bytes(n, fh, fw, stride),
                             "overlap statistics, stride %d, %d images: slabs zeroed on the stream" % (stride, n))


for _form in ("", "_proj", "_ring"):
    _overlap("sequence_overlap_stats%s" % _form, _form, 1)
_overlap("sequence_overlap_stats strip of 64 stride 3", "", 3, case=_strip64)


def _cells(name, form, maker, stride=1):
    entry = "rwh_sequence_cell_stats" + form

    @record(name, entry)
    def make(lib):
        if form == "":
            images, Gs = maker()
            t = sc.tables(images, Gs, 0)
        else:
            images, Gs, kind, f = maker()
            t = pc.tables(images, Gs, 0, kind, f)
        fh, fw = t["size"]
        K = bg.slots(lib, t, B)
        gh, gw = bg.grid(t["size"], B)
        assert K >= 1 and lib.rwh_sequence_cell_stats_table_bytes(fh, fw, bg.shift_of(B), K) == gh * gw * 2 * K * K * 4
        return sequence_live(lib, entry, t, images, (), (fh, fw), (bg.shift_of(B), stride, K, Out(gh * gw * 2 * K * K * 4, "cell table")), (),
                             lib.rwh_sequence_cell_stats_workspace_bytes(t["n"]),
                             "cell statistics, %d x %d cells of %d slots, %d images" % (gh, gw, K, t["n"]))


def _curved(maker):
    def make():
        images, Gs = maker()
        return images, Gs, "cylindrical", 40.0
    return make


_cells("sequence_cell_stats empty_cell", "", bg.empty_cell)
_cells("sequence_cell_stats sixty_four_on_one_cell", "", bg.sixty_four_on_one_cell)
_cells("sequence_cell_stats_proj cylinder", "_proj", bg.cylinder_case)
_cells("sequence_cell_stats_proj empty_cell", "_proj", _curved(bg.empty_cell))


# ---- every other entry point: the argument list as the header has it ----
STREAM = "the stream goes here"
_F64P = ctypes.POINTER(ctypes.c_double)


class F64Table(_Table):
    """A float64 host table whose parameter is bound as POINTER(c_double)."""
    def clone(self):
        return F64Table(self.pristine)


def flat_live(fn, args, reference, reached, eager=False, eager_args=None, compare=None, verify=None, linked=()):
    """fn: the bound entry point; args: its list -- scalars, DevIn, Out, Workspace, numpy arrays (host tables) and STREAM.
    reference(*host inputs, in the order of the DevIn among args) -> one array per Out, in their order.  eager: the entry point has
    no bit-exact reference in the suite -- the record gets a shadow (eager_args: its argument list where it differs; inputs are
    shared, by identity); `reference` may then be None."""
    args = [F64Table(a) if isinstance(a, np.ndarray) and a.dtype == np.float64 else _Table(a) if isinstance(a, np.ndarray) else a for a in args]

    def parts(items):
        inputs = [a for a in items if isinstance(a, DevIn)]
        outs = [a for a in items if isinstance(a, Out)]
        ws = [a for a in items if isinstance(a, Workspace)]
        tabs = [a for a in items if isinstance(a, _Table)]
        return inputs, outs, (ws[0] if ws else None), tabs

    def caller(items):
        def call(stream):
            out = []
            for a in items:
                if a is STREAM:
                    out.append(stream)
                elif isinstance(a, F64Table):
                    out.append(a.live.ctypes.data_as(_F64P))
                elif isinstance(a, _Table):
                    out.append(a.live.ctypes.data)
                elif isinstance(a, (DevIn, Out, Workspace)):
                    out.append(a.ptr)
                else:
                    out.append(a)
            return fn(*out)
        return call

    inputs, outs, ws, tabs = parts(args)
    inputs = inputs + list(linked)
    shadow = None
    if eager:
        twin = [a if isinstance(a, DevIn) or a is STREAM or not hasattr(a, "clone") else a.clone() for a in (eager_args or args)]
        twin = [F64Table(a) if isinstance(a, np.ndarray) and a.dtype == np.float64 else _Table(a) if isinstance(a, np.ndarray) else a for a in twin]
        twin = [Workspace(a.nbytes) if isinstance(a, Workspace) else a for a in twin]
        _, souts, sws, _ = parts(twin)
        assert [o.nbytes for o in souts] == [o.nbytes for o in outs]
        shadow = Live([], souts, sws, [], caller(twin), None, reached)
    expected = None if reference is None else (lambda snap: reference(*snap))
    return _live(inputs, outs, ws, [t.live for t in tabs], caller(args), expected, reached, shadow=shadow, compare=compare, verify=verify)


def _rng(*key):
    return np.random.default_rng(list(key))


def _matches(m=185):
    import refit_cases as rf
    a, b = rf.matchespoints()
    return np.ascontiguousarray(a[:m]), np.ascontiguousarray(b[:m])


def _jitter(pts, key):
    """New contents for a point table: the same points moved by up to a third of a pixel."""
    return lambda seed: (pts + _rng(seed, key).uniform(-0.3, 0.3, pts.shape)).astype(np.float32)


def _idx_vary(k, m, key):
    return lambda seed: _rng(seed, key).integers(0, m, (k, 4)).astype(np.int32)


def _words(m):
    return (m + 63) // 64


def _pack_bits(bits, words):
    """bool [K, M] -> uint64 [K, words], bit i of word i // 64 = pair i."""
    K, M = bits.shape
    padded = np.zeros((K, 64 * words), dtype=np.uint8)
    padded[:, :M] = bits
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64)


def packed_keys(counts, need, base=0):
    """The two words of rwh_score_count's accumulator, from zero, for these counts."""
    counts = np.asarray(counts, dtype=np.int64)
    k = np.arange(len(counts), dtype=np.int64) + base
    w0 = int(((counts << 32) | (0xFFFFFFFF - k)).max()) if len(counts) else 0
    hit = np.flatnonzero(counts >= need)
    w1 = 0xFFFFFFFF - int(k[hit[0]]) if hit.size else 0
    return np.array([w0, w1], dtype=np.uint64)


def _mild_hypotheses(k, key):
    """k float32 hypotheses about the homography of refit_cases.synthetic: translations moved by up to 6 px, so counts differ."""
    def vary(seed):
        rng = _rng(seed, key)
        H = np.tile(np.array([[1.03, 0.02, 40.0], [-0.015, 0.98, 25.0], [2e-5, -1e-5, 1.0]]), (k, 1, 1))
        H[:, :2, 2] += rng.uniform(-6, 6, (k, 2))
        H[:, :2, :2] *= 1 + rng.uniform(-2e-3, 2e-3, (k, 2, 2))
        return np.ascontiguousarray(H.reshape(k, 9), dtype=np.float32)
    return vary


def _scorer(name, entry, m, k, loss, inv=False):
    """rwh_score_count / rwh_score_count_inv against the oracle's errors: counts, masks and the two packed keys."""
    @record(name, entry)
    def make(lib):
        import refit_cases as rf
        import scorer_cases as sk
        from ransac_with_homography_amd import kernels
        u, v = rf.synthetic(m)
        th, need = 5.0, kernels.need_count(m, 60, 4)
        hv = _mild_hypotheses(k, m)
        H, pa, pb = DevIn(hv(0), hv), DevIn(u), DevIn(v)
        ins = [H]
        if inv:
            hi = lambda seed: np.ascontiguousarray(kernels.host_inverses(hv(seed)), dtype=np.float32)
            ins.append(DevIn(hi(0), hi))
        outs = [Out(4 * k, "counts"), Out(8 * k * _words(m), "masks"), Out(16, "packed keys", np.zeros(2, dtype=np.uint64))]

        def reference(h, *rest):
            bits, counts = sk.decisions(sk.oracle_errors(h, u.T, v.T, loss), th)
            return [counts.astype(np.int32), _pack_bits(bits, _words(m)), packed_keys(counts, need)]
        args = ins + [pa, pb, m, k, th, {"fwd": 0, "backward": 1, "reproj": 2}[loss], need, 0] + outs + [None, STREAM]
        return flat_live(getattr(lib, entry), args, reference,
                         "scorer, M = %d (%s), K = %d, %s%s" % (m, "the chunked form with its memset of the counts" if m > 4096 else
                                                                "M in registers" if m <= 256 else "chunks of 256", k, loss,
                                                                ", numpy's inverses" if inv else ""))


_scorer("score_count fwd M 185", "rwh_score_count", 185, 300, "fwd")
_scorer("score_count reproj M 185", "rwh_score_count", 185, 300, "reproj")
_scorer("score_count fwd M 4200", "rwh_score_count", 4200, 200, "fwd")
_scorer("score_count_inv reproj M 185", "rwh_score_count_inv", 185, 300, "reproj", inv=True)
_scorer("score_count_inv reproj M 4200", "rwh_score_count_inv", 4200, 200, "reproj", inv=True)


@record("dlt4_batched", "rwh_dlt4_batched")
def _dlt4(lib):
    import k1_cases as kc
    a, b = _matches()
    k = 500
    iv = _idx_vary(k, 185, 1)
    idx = DevIn(iv(0), iv)

    def verify(inputs, got):
        flags = got[1]
        assert np.array_equal((flags & kc.REPEATED) != 0, kc.repeated_rule(inputs[2], 185))
    return flat_live(lib.rwh_dlt4_batched, [DevIn(a), DevIn(b), 185, idx, k, Out(36 * k, "hypotheses"), Out(k, "flags"), STREAM], None,
                     "K1, K = %d" % k, eager=True, verify=verify)


def _search(name, m, k, loss):
    @record(name, "rwh_ransac_search")
    def make(lib):
        import refit_cases as rf
        import scorer_cases as sk
        from ransac_with_homography_amd import kernels
        u, v = _matches() if m == 185 else rf.synthetic(m)
        iv = _idx_vary(k, m, m)
        need = kernels.need_count(m, 60, 4)
        outs = [Out(36 * k, "hypotheses"), Out(k, "flags"), Out(4 * k, "counts"), Out(8 * k * _words(m), "masks"), Out(16, "packed keys")]

        def verify(inputs, got):
            """What the oracle says of K2 on K1's own hypotheses ('fwd': the kernel's arithmetic is the oracle's), and the keys."""
            H, counts = got[0].view(np.float32).reshape(k, 9), got[2].view(np.int32)
            assert np.array_equal(got[4].view(np.uint64), packed_keys(counts, need))
            if loss == "fwd":
                fin = np.isfinite(H).all(axis=1)
                bits, want = sk.decisions(sk.oracle_errors(H[fin], u.T, v.T, loss), 5.0)
                assert np.array_equal(counts[fin], want)
                assert np.array_equal(got[3].view(np.uint64).reshape(k, -1)[fin], _pack_bits(bits, _words(m)))
        args = [DevIn(u), DevIn(v), m, DevIn(iv(0), iv), k, 5.0, {"fwd": 0, "reproj": 2}[loss], need, 0] + outs + [1, STREAM]
        return flat_live(lib.rwh_ransac_search, args, None, "K1 + K2 with the key reset, M = %d%s, K = %d, %s"
                         % (m, " (the chunked scorer and its memset)" if m > 4096 else "", k, loss), eager=True, verify=verify)


_search("ransac_search fwd M 185", 185, 2000, "fwd")
_search("ransac_search reproj M 185", 185, 500, "reproj")
_search("ransac_search fwd M 4200", 4200, 300, "fwd")
_search("ransac_search reproj M 4200", 4200, 300, "reproj")


def _batched(name, sizes, k, sampling, early_stop=False):
    @record(name, "rwh_ransac_batched")
    def make(lib):
        import philox_ref
        from ransac_with_homography_amd import kernels
        a, b = _matches()
        P, m_max, seed = len(sizes), max(sizes), 77
        A, Bv = np.concatenate([a[:m] for m in sizes]), np.concatenate([b[:m] for m in sizes])
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        needs = np.array([kernels.need_count(m, 40 if early_stop else 70, 4) for m in sizes], dtype=np.int32)
        words = _words(m_max)
        pa, pb = DevIn(A), DevIn(Bv, _jitter(Bv, 3))
        if sampling:
            idx = Out(16 * P * k, "samples")
        else:
            iv = lambda seed: np.stack([_rng(seed, p).integers(0, m, (k, 4)) for p, m in enumerate(sizes)]).astype(np.int32)
            idx = DevIn(iv(0), iv)
        outs = [Out(36 * P * k, "hypotheses"), Out(P * k, "flags"), Out(4 * P * k, "counts"), Out(8 * P * k * words, "masks"),
                Out(16 * P, "packed keys")]
        flags = (1 if sampling else 0) | (2 if early_stop else 0)
        head = [pa, pb, DevIn(offs), P, m_max, k]
        tail = [seed, 0, 5.0, 0, DevIn(needs)]

        def arglist(idx_, outs_, fl):
            return head + [idx_] + tail + outs_ + [fl, STREAM]

        def keys_of(counts):
            return np.stack([packed_keys(counts.view(np.int32).reshape(P, k)[p], needs[p]) for p in range(P)])

        def verify(inputs, got):
            """The device sampler against its restatement, and -- the eager call shares the library with the record, so this is what
            holds the key reset -- the packed keys against the counts they summarise, from zero."""
            o = 1 if sampling else 0
            if sampling:
                for p, m in enumerate(sizes):
                    assert np.array_equal(got[0].view(np.int32).reshape(P, k, 4)[p], philox_ref.sample4(seed, p, k, m)), p
            if not early_stop:
                assert np.array_equal(got[o + 4].view(np.uint64).reshape(P, 2), keys_of(got[o + 2]))

        def compare(got, want):
            """Early stop against the run that scores everything (test_batched_early_stop_and_device_handoff's rule): samples,
            hypotheses and flags are the same; a hypothesis that was scored has the full run's count and mask, a skipped one -1 and
            zero words; the exit key is the same, and so is the decoded winner."""
            o = 1 if sampling else 0
            for j in range(o + 2):
                assert np.array_equal(got[j], want[j]), j
            cg, cw = got[o + 2].view(np.int32), want[o + 2].view(np.int32)
            mg, mw = got[o + 3].view(np.uint64).reshape(P * k, words), want[o + 3].view(np.uint64).reshape(P * k, words)
            scored = cg >= 0
            assert (cg[~scored] == -1).all() and np.array_equal(cg[scored], cw[scored]) and np.array_equal(mg[scored], mw[scored])
            assert not mg[~scored].any()
            bg_, bw = got[o + 4].view(np.uint64).reshape(P, 2), want[o + 4].view(np.uint64).reshape(P, 2)
            assert np.array_equal(bw, keys_of(want[o + 2]))          # the full run's keys are its counts', from zero
            assert np.array_equal(bg_[:, 1], bw[:, 1])
            for p in range(P):
                assert kernels.decode_best(bg_[p], k) == kernels.decode_best(bw[p], k), p
        souts = [o.clone() for o in outs]
        sidx = idx.clone() if sampling else idx
        return flat_live(lib.rwh_ransac_batched, arglist(idx, outs, flags), None,
                         "batched search, P = %d, K = %d, %s%s" % (P, k, "device sampling" if sampling else "the caller's tables",
                                                                  ", early stop (keys cleared by the DLT launch)" if early_stop else ""),
                         eager=True, eager_args=arglist(sidx, souts, flags & 1), compare=compare if early_stop else None, verify=verify)


_batched("ransac_batched caller's tables", [185, 120, 90, 60], 512, False)
_batched("ransac_batched device sampling", [185, 120, 90, 60], 512, True)
_batched("ransac_batched device sampling early stop", [185, 120, 90, 60], 2000, True, early_stop=True)
_batched("ransac_batched P 3 K 10", [185, 40, 7], 10, False)


@record("score_interval", "rwh_score_interval")
def _interval(lib):
    import refit_cases as rf
    m, k = 185, 300
    u, v = rf.synthetic(m)
    hv = _mild_hypotheses(k, 9)
    rows = np.arange(0, k, 2, dtype=np.int32)
    fl = lambda seed: (_rng(seed, 5).integers(0, 2, k) * 4).astype(np.uint8)
    n = len(rows)

    def verify(inputs, got):
        lo, hi = got[0].view(np.int32), got[1].view(np.int32)
        assert (0 <= lo).all() and (lo <= hi).all() and (hi <= m).all()
    args = [DevIn(hv(0), hv), DevIn(rows), n, DevIn(fl(0), fl), DevIn(u), DevIn(v), m, 5.0, 1920.0, 16 * 2.0 ** -24, 64 * 2.0 ** -24,
            Out(4 * n, "lower counts"), Out(4 * n, "upper counts"), STREAM]
    return flat_live(lib.rwh_score_interval, args, None, "K2i, %d listed rows of %d, M = %d" % (n, k, m), eager=True, verify=verify)


def _project(name, inverse):
    @record(name, "rwh_project_points")
    def make(lib):
        from oracle import rwh_oracle as orc
        a, _ = _matches()
        hv = _mild_hypotheses(1, 21)

        def reference(h, pts):
            val = h.reshape(3, 3)
            with np.errstate(all="ignore"):
                return [(orc.project_back if inverse else orc.project_fwd)(val, np.ascontiguousarray(pts.T))]
        return flat_live(lib.rwh_project_points, [DevIn(hv(0), hv), DevIn(a, _jitter(a, 22)), 185, inverse, Out(12 * 185, "projections"), STREAM],
                         reference, "projection of 185 points, %s" % ("through the inverse" if inverse else "forward"))


_project("project_points fwd", 0)
_project("project_points inverse", 1)


def _project_ex(name, dtype, code):
    @record(name, "rwh_project_points_ex")
    def make(lib):
        from oracle import rwh_oracle as orc
        a, _ = _matches()
        hv0 = _mild_hypotheses(1, 23)
        hv = lambda seed: hv0(seed).astype(dtype)
        pv = lambda seed: np.ascontiguousarray(np.vstack([a.T + _rng(seed, 24).uniform(-0.3, 0.3, (2, 185)), _rng(seed, 25).uniform(0.5, 2.0, (1, 185))]),
                                               dtype=dtype)

        def reference(h, p3):
            with np.errstate(all="ignore"):
                out = orc.project_fwd(h.reshape(3, 3), p3)
            assert out.dtype == dtype
            return [out]
        return flat_live(lib.rwh_project_points_ex, [DevIn(hv(0), hv), DevIn(pv(0), pv), 185, code, Out(3 * 185 * np.dtype(dtype).itemsize,
                                                                                                   "projections"), STREAM],
                         reference, "general projection, %s" % np.dtype(dtype).name)


_project_ex("project_points_ex f32", np.float32, 1)
_project_ex("project_points_ex f64", np.float64, 2)


@record("refit_batched", "rwh_refit_batched")
def _refit(lib):
    import refit_cases as rf
    sizes = [63, 64, 130]
    probs = [rf.synthetic(m) for m in sizes]
    A, Bv = np.concatenate([p[0] for p in probs]), np.concatenate([p[1] for p in probs])
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    words, P = 3, len(sizes)
    bits = lambda seed: [rf.random_bits(m, 50 + seed) for m in sizes]
    mv = lambda seed: np.stack([rf.pack(x, words) for x in bits(seed)])

    def verify(inputs, got):
        """The suite's own hold on the kernel against its twin (test_host_twin_agrees_with_the_kernel): the statuses, and an H inside
        the yardstick's margin of the twin's; bit identity is not asserted there either."""
        H, st = got[0].view(np.float64).reshape(P, 3, 3), got[1].view(np.int32)
        masks = inputs[3]
        for p, (u, v) in enumerate(probs):
            Hh, sh = rf.host_refit(lib, u, v, masks[p])
            assert sh == st[p] == rf.OK
            b = np.unpackbits(masks[p].view(np.uint8), bitorder="little")[:sizes[p]].astype(bool)
            assert rf.deviation(Hh, H[p], u) <= rf.yardstick(u, v, b)[1], p
    args = [DevIn(A), DevIn(Bv), DevIn(offs), P, DevIn(mv(0), mv), words, Out(72 * P, "homographies"), Out(4 * P, "statuses"), STREAM]
    return flat_live(lib.rwh_refit_batched, args, None, "refit, %d problems" % P, eager=True, verify=verify)


def _edge_blocks(name, entry, cases, block, record_width, key):
    @record(name, entry)
    def make(lib):
        import bundle_cases as bc
        c = cases.size_list_case()
        E = len(c["sizes"])
        rec = np.ascontiguousarray(c[key], dtype=np.float64).reshape(E, record_width)
        mv = lambda seed: bc.mask_sets(c["sizes"], seed=3 + seed)["random"]
        words = mv(0).shape[1]

        def reference(pa, pb, offsets, masks):
            st, blocks, count, status = bc.rule_host_blocks(lib, entry.replace("rwh_", "rwh_host_"), block, record_width, pa, pb, offsets, masks, rec)
            assert st == 0
            return [blocks, count, status]
        args = [DevIn(c["pa"]), DevIn(c["pb"], _jitter(c["pb"], 31)), DevIn(c["offsets"]), E, DevIn(mv(0), mv), words, DevIn(rec),
                Out(8 * E * block, "blocks"), Out(4 * E, "counts"), Out(4 * E, "statuses"), STREAM]
        return flat_live(getattr(lib, entry), args, lambda pa, pb, offsets, masks, _: reference(pa, pb, offsets, masks),
                         "edge blocks, %d edges, one launch" % E)


def _registration():
    import bundle_cases as bc
    import camera_cases as cc
    _edge_blocks("bundle_blocks", "rwh_bundle_blocks", bc, bc.BLOCK, 9, "T")
    _edge_blocks("camera_blocks", "rwh_camera_blocks", cc, cc.BLOCK, cc.RECORD, "rec")


_registration()


@record("match_hamming_batched", "rwh_match_hamming_batched")
def _match(lib):
    import match_cases as mc
    shapes = [(70, 90), (1, 5), (300, 257)]
    nbytes = 32
    pairs = lambda seed: [mc.random_pair(na, nb, nbytes, seed=40 + 10 * seed + p) for p, (na, nb) in enumerate(shapes)]
    av = lambda seed: np.concatenate([p[0] for p in pairs(seed)])
    bv = lambda seed: np.concatenate([p[1] for p in pairs(seed)])
    oa = np.concatenate([[0], np.cumsum([s[0] for s in shapes])]).astype(np.int32)
    ob = np.concatenate([[0], np.cumsum([s[1] for s in shapes])]).astype(np.int32)
    ta, tb, P = int(oa[-1]), int(ob[-1]), len(shapes)

    def reference(A, Bv, *_):
        train, dist = [], []
        for p in range(P):
            st, t, d = mc.host_match(lib, A[oa[p]:oa[p + 1]], Bv[ob[p]:ob[p + 1]])
            assert st == 0
            train.append(t), dist.append(d)
        return [np.concatenate(train), np.concatenate(dist)]
    args = [DevIn(av(0), av), DevIn(bv(0), bv), nbytes, DevIn(oa), DevIn(ob), P, ta, tb, Out(4 * ta, "train rows"), Out(4 * ta, "distances"),
            Workspace(lib.rwh_match_workspace_bytes(P, ta, tb)), lib.rwh_match_workspace_bytes(P, ta, tb), STREAM]
    return flat_live(lib.rwh_match_hamming_batched, args, reference, "cross-check matcher, %d pairs, four launches" % P)


@record("match_ratio_graph", "rwh_match_ratio_graph")
def _match_ratio(lib):
    import match_cases as mc
    import match_ratio_cases as mr
    from ransac_with_homography_amd import kernels
    rows, nbytes = [70, 0, 1, 300, 257], 32
    pairs = np.array([(0, 3), (3, 4), (4, 3), (1, 3), (3, 1), (2, 4), (3, 3), (0, 3)], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)

    def dv(seed):
        A, Bv = mc.random_pair(300, 257, nbytes, seed=60 + seed)
        rng = np.random.RandomState(seed)
        small = [np.stack([mr.flipped(r, rng, 2) for r in A[:70]]), np.zeros((0, nbytes), dtype=np.uint8), Bv[:1].copy()]
        return np.ascontiguousarray(np.concatenate(small + [A, Bv]))
    na, nb = kernels.match_ratio_rows(off, pairs, int(off[-1]))
    tq, tt, mt = int(na.sum()), int(nb.sum()), int(nb.max())
    need = lib.rwh_match_ratio_workspace_bytes(len(pairs), tq, tt, mt)

    def reference(desc, *_):
        outs = [[], [], []]
        for s, d in pairs:
            st, t, d1, d2 = mr.host_match(lib, desc[off[s]:off[s + 1]], desc[off[d]:off[d + 1]])
            assert st == 0
            for o, x in zip(outs, (t, d1, d2)):
                o.append(x)
        return [np.concatenate(o).astype(np.int32) for o in outs]
    args = [DevIn(dv(0), dv), nbytes, DevIn(off), len(rows), int(off[-1]), DevIn(pairs), len(pairs), tq, tt, 7, 10,
            Out(4 * tq, "train rows"), Out(4 * tq, "distances"), Out(4 * tq, "second distances"), Workspace(need), need, STREAM]
    return flat_live(lib.rwh_match_ratio_graph, args, reference, "ratio matcher over a pair graph, %d pairs, four launches" % len(pairs))


# ---- the extractor ----
KEY_NONE = 0x7F7F7F7F7F7F7F7F
ORB_SHAPES = ((55, 150, 1), (70, 100, 3))


def _dotted(shape, seed):
    """Noise of 0 .. 10 under 14 planted dots of 200 .. 250 at legal centres at least five pixels apart: every dot is a keypoint."""
    h, w, c = shape
    rng = np.random.RandomState(1000 + seed)
    img = rng.randint(0, 11, (h, w) if c == 1 else (h, w, c)).astype(np.uint8)
    spots = []
    for _ in range(10000):
        if len(spots) == 14:
            break
        x, y = int(rng.randint(16, w - 16)), int(rng.randint(16, h - 16))
        if all(abs(x - u) > 5 or abs(y - v) > 5 for u, v in spots):
            spots.append((x, y))
            img[y, x] = rng.randint(200, 251)
    assert len(spots) == 14
    return img


def _orb_images(seed):
    return [_dotted(sh, 10 * seed + i) for i, sh in enumerate(ORB_SHAPES)]


def _orb_table():
    rows, src, gray = [], 0, 0
    for h, w, c in ORB_SHAPES:
        rows.append((src, gray, h, w, c))
        src, gray = src + h * w * c, gray + h * w
    return np.array(rows, dtype=np.int64), src, gray


def _orb_keys(img, threshold=20):
    import orb_cases as oc
    x, y, s = oc.keypoints(oc.scores(oc.gray(img)), threshold)
    return ((255 - s.astype(np.int64)) << 32) | (y.astype(np.int64) << 16) | x.astype(np.int64)


@record("orb_detect_batched", "rwh_orb_detect_batched")
def _orb_detect(lib):
    import orb_cases as oc
    table, images_bytes, gray_bytes = _orb_table()
    n, capacity = len(ORB_SHAPES), 64
    flat = lambda seed: np.concatenate([im.reshape(-1) for im in _orb_images(seed)])
    need = lib.rwh_orb_workspace_bytes(n)

    def reference(pixels, _):
        grays, keys, counts, at = [], np.full((n, capacity), KEY_NONE, dtype=np.int64), [], 0
        for i, (h, w, c) in enumerate(ORB_SHAPES):
            img = pixels[at:at + h * w * c].reshape((h, w) if c == 1 else (h, w, c))
            at += h * w * c
            grays.append(oc.gray(img).reshape(-1))
            k = _orb_keys(img)
            assert 0 < len(k) <= capacity
            keys[i, :len(k)] = k
            counts.append(len(k))
        return [np.concatenate(grays), keys, np.array(counts, dtype=np.int32)]

    def compare(got, want):
        """A row's keys arrive in no particular order (include/rwh.h): the rows are compared sorted."""
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
        assert np.array_equal(np.sort(got[1].view(np.int64).reshape(n, capacity), axis=1), want[1].view(np.int64).reshape(n, capacity))
    args = [DevIn(flat(0), flat), images_bytes, DevIn(table), n, 20, Out(gray_bytes, "gray planes"), gray_bytes, Out(8 * n * capacity, "keys"),
            capacity, Out(4 * n, "counts"), Workspace(need), need, STREAM]
    return flat_live(lib.rwh_orb_detect_batched, args, reference, "detector, %d images: keys and counts cleared on the stream" % n, compare=compare)


@record("orb_describe_batched", "rwh_orb_describe_batched")
def _orb_describe(lib):
    import orb_cases as oc
    table, _, gray_bytes = _orb_table()
    n, stride, nf, nbytes = len(ORB_SHAPES), 64, 10, 32
    bin_table, rotated = oc.tables(nbytes)
    grays = lambda seed: [oc.gray(im) for im in _orb_images(seed)]
    gv = lambda seed: np.concatenate([g.reshape(-1) for g in grays(seed)])

    def kv(seed):
        keys = np.full((n, stride), KEY_NONE, dtype=np.int64)
        for i, im in enumerate(_orb_images(seed)):
            k = _orb_keys(im)
            keys[i, :len(k)] = k                                     # ascending: rule 3's order
        return keys
    cv = lambda seed: np.array([(kv(seed)[i] != KEY_NONE).sum() for i in range(n)], dtype=np.int32)

    def reference(gray, _, keys, counts, *rest):
        kps = np.full(n * nf * 8, FILL, dtype=np.uint8).view(np.float32).reshape(n, nf, 2)
        desc = np.full((n, nf, nbytes), FILL, dtype=np.uint8)
        score = np.full(n * nf * 4, FILL, dtype=np.uint8).view(np.int32).reshape(n, nf)
        bins = score.copy()
        at = 0
        for i, (h, w, c) in enumerate(ORB_SHAPES):
            g = gray[at:at + h * w].reshape(h, w)
            at += h * w
            m = min(int(counts[i]), nf, stride)
            assert m == nf                                           # more keys than features: the cut is taken
            k = keys[i, :m]
            x, y, s = k & 0xFFFF, (k >> 16) & 0xFFFF, 255 - (k >> 32)
            b, _, _ = oc.orientation_bins(g, x, y, bin_table)
            kps[i, :m], desc[i, :m], score[i, :m], bins[i, :m] = np.stack([x, y], axis=1), oc.descriptors(g, x, y, b, rotated), s, b
        return [kps, desc, score, bins]
    args = [DevIn(gv(0), gv), gray_bytes, DevIn(table), n, DevIn(kv(0), kv), stride, DevIn(cv(0), cv), nf, DevIn(bin_table),
            DevIn(np.ascontiguousarray(rotated)), nbytes, Out(8 * n * nf, "keypoints"), Out(n * nf * nbytes, "descriptors"), Out(4 * n * nf, "scores"),
            Out(4 * n * nf, "bins"), STREAM]
    return flat_live(lib.rwh_orb_describe_batched, args, reference, "describer, %d images, %d keypoints each" % (n, nf))


class Linked(DevIn):
    """The input region at the head of an in-place buffer (rwh_orb_pyramid_batched's d_images): no tensor of its own."""
    def __init__(self, host, vary, out):
        DevIn.__init__(self, host, vary)
        self.out = out
        self.set(self.host)

    def alloc(self):
        pass

    def set(self, host):
        import torch
        self.host = np.ascontiguousarray(host, dtype=np.uint8)
        self.out.initial[:self.host.size] = self.host
        if self.out.buf is not None:
            self.out.buf[64:64 + self.host.size].copy_(torch.from_numpy(self.host.copy()))


@record("orb_pyramid_batched", "rwh_orb_pyramid_batched")
def _orb_pyramid(lib):
    import orb_pyramid_cases as op
    scales = op.CALLER_SCALES
    head, table, planes_offset, images_bytes, spans = op.layout(_orb_images(0), scales, gap=24)
    buf = Out(images_bytes, "images and level planes", np.full(images_bytes, FILL, dtype=np.uint8))
    buf.keep = True                                                  # the planes of one replay stay where the next one writes
    flat = lambda seed: np.concatenate([im.reshape(-1) for im in _orb_images(seed)])
    pixels = Linked(flat(0), flat, buf)
    rows = len(table)
    need = lib.rwh_orb_workspace_bytes(rows)

    def reference(_, px):
        want, at = np.full(images_bytes, FILL, dtype=np.uint8), 0
        want[:planes_offset] = px
        for i, (h, w, c) in enumerate(ORB_SHAPES):
            img = px[at:at + h * w * c].reshape((h, w) if c == 1 else (h, w, c))
            at += h * w * c
            st, planes = op.host_planes(lib, img, scales)
            assert st == 0
            for (o, hl, wl), pl in zip(spans[i], planes):
                want[o:o + hl * wl] = pl.reshape(-1)
        return [want]
    args = [buf, images_bytes, planes_offset, DevIn(table), len(ORB_SHAPES), scales.copy(), len(scales), Workspace(need), need, STREAM]
    return flat_live(lib.rwh_orb_pyramid_batched, args, reference, "pyramid, %d images x %d levels, the scales in kernel arguments"
                     % (len(ORB_SHAPES), len(scales)), linked=[pixels])


# ---- the warps ----
WARP_H = sc.homography(np.random.default_rng(5), 3.3, -2.6, 0.01, 2e-5)
U8, F32, F64, U16 = 0, 1, 2, 4
ZERO_ORIGIN, EXACT = 1, 2


def _warp_grid(h, w):
    from oracle import rwh_oracle as orc
    mx, my, mw, mh = orc.output_bounds(h, w, WARP_H)
    sx = 1.0 if mw > 1 else 0.0                                      # numpy.linspace: (stop - start) / (num - 1) of an integer grid
    return (float(mx), sx, float(mx + mw - 1), float(my), 1.0 if mh > 1 else 0.0, float(my + mh - 1)), (mh, mw)


def _warp_plan(lib, h, w, c, src_code, batch, inv, grid, size, interp, dst_code, flags):
    buf = ctypes.create_string_buffer(128)
    st = lib.rwh_warp_plan(h, w, c, src_code, batch, inv.ctypes.data_as(_F64P), 1, *grid, size[0], size[1], h, w, interp, dst_code, 0, size[0],
                           flags, buf, 128)
    assert st == 0, st
    return buf.value.decode()


def _fast_warp(name, batch, interp, plan):
    """A fast plan of rwh_warp_backward: no bit-exact reference, so the eager call is the yardstick (the module's docstring)."""
    @record(name, "rwh_warp_backward")
    def make(lib):
        h, w, c = 48, 200, 3
        grid, (mh, mw) = _warp_grid(h, w)
        inv = np.ascontiguousarray(np.linalg.inv(WARP_H).reshape(9))
        assert _warp_plan(lib, h, w, c, U8, batch, inv, grid, (mh, mw), interp, U8, ZERO_ORIGIN) == plan
        src = DevIn(image_vary((batch, h, w, c), 900 + batch)(0), image_vary((batch, h, w, c), 900 + batch))
        args = [src, h, w, c, U8, h * w * c, batch, inv, 1, *grid, mh, mw, h, w, interp, Out(batch * mh * mw * c, "warped images"), U8,
                mh * mw * c, 0, mh, ZERO_ORIGIN, STREAM]
        return flat_live(lib.rwh_warp_backward, args, None, "%s, %d frame%s of %d x %d" % (plan, batch, "s" if batch > 1 else "", h, w), eager=True)


_fast_warp("warp_backward u8 bilinear fast", 1, 1, "rwh::warp_rgb8_fast8<unsigned char, 6>")
_fast_warp("warp_backward u8 bilinear batch walk", 24, 1, "rwh::warp_rgb8_fast8<unsigned char, 6>")      # (the plan names the family)
_fast_warp("warp_backward u8 nearest", 1, 0, "rwh::warp_rgb8_nn<6>")


def _in_place(host, vary, what):
    """An image the call writes (texel (0,0) is blanked, as the reference does to its caller's array): an output that `refresh`
    restores, and the input it is restored from -> (the Out to pass, the Linked input)."""
    flat = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
    out = Out(flat.size, what, flat.copy())
    return out, Linked(flat, lambda seed: np.ascontiguousarray(vary(seed)).view(np.uint8).reshape(-1), out)


def _exact_warp(name, dtype, src_code, dst_dtype, dst_code, plan):
    """RWH_WARP_EXACT through the oracle's wrap_perspective, bit for bit; the source's texel (0,0) is blanked in place."""
    @record(name, "rwh_warp_backward")
    def make(lib):
        from oracle import rwh_oracle as orc
        h, w, c = 40, 61, 3
        grid, (mh, mw) = _warp_grid(h, w)
        inv = np.ascontiguousarray(np.linalg.inv(WARP_H).reshape(9))
        assert _warp_plan(lib, h, w, c, src_code, 1, inv, grid, (mh, mw), 1, dst_code, ZERO_ORIGIN | EXACT) == plan
        top = int(np.iinfo(dtype).max) + 1
        vary = lambda seed: _rng(seed, 41, src_code).integers(0, top, (h, w, c)).astype(dtype)
        src, pixels = _in_place(vary(0), vary, "source image")

        def reference(px):
            img = px.view(dtype).reshape(h, w, c).copy()
            out, _, _ = orc.wrap_perspective(img, WARP_H, "bilinear")
            assert out.shape == (mh, mw, c) and out.dtype == np.float64
            return [img, out.astype(dst_dtype)]                      # (the oracle blanked img's texel (0,0), as the call does)
        isz = np.dtype(dtype).itemsize
        args = [src, h, w, c, src_code, h * w * c * isz, 1, inv, 1, *grid, mh, mw, h, w, 1, Out(mh * mw * c * np.dtype(dst_dtype).itemsize,
                                                                                            "warped image"), dst_code,
                mh * mw * c * np.dtype(dst_dtype).itemsize, 0, mh, ZERO_ORIGIN | EXACT, STREAM]
        return flat_live(lib.rwh_warp_backward, args, reference, "%s, exact" % plan, linked=[pixels])


_exact_warp("warp_backward exact u16 bilinear", np.uint16, U16, np.float64, F64, "rwh::warp_any<unsigned short, double, 1>")
_exact_warp("warp_backward exact u8 bilinear", np.uint8, U8, np.uint8, U8, "rwh::warp_exact<unsigned char, 3, unsigned char, 1>")


@record("sample_points bilinear", "rwh_sample_points")
def _sample_points(lib):
    from oracle import rwh_oracle as orc
    h, w, c, n = 40, 61, 3, 500
    vary = image_vary((h, w, c), 51)
    img, pixels = _in_place(vary(0), vary, "image")

    def cv(key, top):
        """Coordinates inside the image (short of the last texel, where the reference indexes past it) and a tenth outside."""
        def f(seed):
            rng = _rng(seed, key)
            v = rng.uniform(0.0, top - 1.001, n)
            v[::10] = rng.uniform(-3.0, -0.5, len(v[::10]))
            return v
        return f
    xs, ys = DevIn(cv(52, w)(0), cv(52, w)), DevIn(cv(53, h)(0), cv(53, h))

    def reference(x, y, px):
        im = px.reshape(h, w, c).copy()
        out = orc.bilinear(np.stack([x, y, np.ones(n)]), im, h, w, n, 1)
        return [im, out.reshape(n, c)]
    args = [img, h, w, c, U8, xs, ys, n, h, w, 1, Out(8 * n * c, "samples"), F64, ZERO_ORIGIN, STREAM]
    return flat_live(lib.rwh_sample_points, args, lambda x, y, px: reference(x, y, px), "the exact bilinear interpolator on %d points" % n,
                     linked=[pixels])


@record("warp_index_check", "rwh_warp_index_check")
def _index_check(lib):
    """The identity on the image's own grid: bilinear reads texel x + 1 on the last column and row, so both bits are set.  The call
    has no device input at all; its flag, cleared on the stream and then OR-ed into, is the output."""
    h, w = 40, 61
    inv = np.ascontiguousarray(np.eye(3).reshape(9))
    args = [h, w, inv, 0.0, 1.0, float(w - 1), 0.0, 1.0, float(h - 1), h, w, h, w, 1, Out(4, "flag"), STREAM]
    live = flat_live(lib.rwh_warp_index_check, args, lambda: [np.array([3], dtype=np.int32)], "the index check: flag cleared on the stream")
    live.constant = True
    return live


# ---- the panorama compositors: texel (0,0) of d_img_t is blanked in place ----
def _pair(dtype=np.uint8):
    seed, Q, T, H = sc.oracle_pairs(1)[0]
    qv = lambda s: Q if s == 0 else image_vary(Q.shape, 61)(s)
    tv = lambda s: T if s == 0 else image_vary(T.shape, 62)(s)
    if dtype != np.uint8:                                            # the bytes and a fraction: float texels that are no integers
        qf, tf = qv, tv
        qv = lambda s: (qf(s) * 0.996).astype(dtype)
        tv = lambda s: (tf(s) * 0.996).astype(dtype)
    return qv, tv, H


def _panorama(name, entry, blend, rows=None, dtype=np.uint8, code=U8):
    @record(name, entry)
    def make(lib):
        from oracle import rwh_oracle as orc
        qv, tv, H = _pair(dtype)
        (hq, wq, _), (ht, wt, _) = qv(0).shape, tv(0).shape
        mx, my, mw, mh = orc.output_bounds(ht, wt, H)
        (tsx, tsy, _, _), (qsx, qsy, _, _), (fw, fh) = orc.stitch_geometry(mw, mh, wq, hq, mx, my)
        inv = np.ascontiguousarray(np.linalg.inv(np.asarray(H, dtype=np.float64)).reshape(9))
        img_t, pixels = _in_place(tv(0), tv, "imgT")
        img_q = DevIn(qv(0), qv)
        r0, r1 = (0, fh) if rows is None else (rows[0], fh - rows[1])
        canvas = Out(fh * fw * 3, "canvas")

        def reference(q, px):
            t = px.view(dtype).reshape(ht, wt, 3).copy()
            with np.errstate(all="ignore"):
                can = orc.stitch_panorama(q, t.copy(), H, "Rate" if blend else False, 0.2)
            assert can.shape == (fh, fw, 3) and can.dtype == np.uint8
            want = np.full((fh, fw, 3), FILL, dtype=np.uint8)
            want[r0:r1] = can[r0:r1]
            t[0, 0] = 0                                              # the write to the caller's array, whatever the blend
            return [t, want]
        geo = [inv, mx, my, mw, mh, tsx, tsy, qsx, qsy, fh, fw]
        if entry == "rwh_stitch_panorama_ex":
            args = [img_t, ht, wt, 3, code, img_q, hq, wq, 3, code] + geo + [3, blend, 0.2, canvas, r0, r1, ZERO_ORIGIN, STREAM]
        else:
            args = [img_t, ht, wt, img_q, hq, wq] + geo + [blend, 0.2, canvas] + ([r0, r1] if entry.endswith("_rows") else []) + [ZERO_ORIGIN, STREAM]
        return flat_live(getattr(lib, entry), args, reference, "the exact compositor, %s, %s, canvas %d x %d%s"
                         % (np.dtype(dtype).name, "rate blend" if blend else "paste", fh, fw, "" if rows is None else ", rows %d .. %d" % (r0, r1)),
                         linked=[pixels])


_panorama("stitch_panorama paste", "rwh_stitch_panorama", 0)
_panorama("stitch_panorama rate", "rwh_stitch_panorama", 1)
_panorama("stitch_panorama_rows paste", "rwh_stitch_panorama_rows", 0, rows=(2, 3))
_panorama("stitch_panorama_ex f32 paste", "rwh_stitch_panorama_ex", 0, dtype=np.float32, code=F32)
