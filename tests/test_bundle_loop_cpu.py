"""What sits around the bundle rule's arithmetic, without a GPU: the Levenberg-Marquardt loop of `sequence_adjust(on="host")` --
its minimum against an independent optimiser (bundle_cases.reference_optimum), its reject branch, its lambda ceiling, its prefix,
a BEHIND candidate, a determinant flip, a singular step, wide mask rows, a non-finite b --, every side of the validity test and the two ends of a
launch on the host twin against the numpy restatement.  The steps tried are counted by wrapping kernels.host_bundle_step and
kernels.host_bundle_blocks; the library is not changed for it."""
import math
import sys
import time

import numpy as np
import pytest

import bundle_cases as bc
import sequence_cases as sc

REL = 1e-9              # the optimum's tolerance: two orders over the 8.7e-12 seen against another optimiser, seven under the 5 %
                        # between the chain's start and the minimum
TRIED_LIMIT = 200       # a loop that does not raise lambda on a reject never ends: the wrapper fails the test instead


@pytest.fixture(scope="module")
def lib():
    return sc.library()


@pytest.fixture(scope="module")
def grid():
    return bc.grid_scene()


@pytest.fixture(scope="module")
def start(lib, grid):
    return bc.snake_start(lib, grid)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def traced_adjust(Gs, grid, on_step=None, on_blocks=None, singular_at=None, events=None, **kw):
    """sequence_adjust(on="host") with both kernels entries wrapped -> (Gs, info, events).  events: ("blocks", blocks, status) for
    every evaluation, ("step", lambda, the blocks it was given, delta) for every step tried (a list given as `events` receives them,
    for a run that raises).  on_step(k, delta) / on_blocks(k, status) may replace what call k (from 0) returns; singular_at makes
    step k report RWH_BUNDLE_SINGULAR."""
    import homography as hg
    from ransac_with_homography_amd import kernels
    events, info = [] if events is None else events, {}
    real_step, real_blocks = kernels.host_bundle_step, kernels.host_bundle_blocks

    def step(n, anchor, edges, blocks, lam):
        k = sum(ev[0] == "step" for ev in events)
        assert k < TRIED_LIMIT, "the loop does not end"
        delta, st = real_step(n, anchor, edges, blocks, lam)
        if on_step is not None:
            delta = on_step(k, delta)
        if singular_at == k:
            delta, st = np.zeros_like(delta), bc.SINGULAR
        events.append(("step", float(lam), np.array(blocks, dtype=np.float64, copy=True), delta.copy()))
        return delta, st

    def blocks(*a):
        k = sum(ev[0] == "blocks" for ev in events)
        out, count, status = real_blocks(*a)
        if on_blocks is not None:
            status = on_blocks(k, status)
        events.append(("blocks", out.copy(), status.copy()))
        return out, count, status

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(kernels, "host_bundle_step", step)
        mp.setattr(kernels, "host_bundle_blocks", blocks)
        out = hg.sequence_adjust(Gs, grid["pairs"], grid["matches"], on="host", info=info, **kw)
    return out, info, events


def audit(events, info):
    """Walks the events by the loop's stated contract and asserts it call by call: every step gets the blocks of the last
    ACCEPTED evaluation (after a reject the same bits as the step before) and the lambda that the accepts and rejects so far
    give; a step is accepted iff its candidate was evaluated, no edge reports BEHIND and the cost is strictly lower.
    -> (tried, accepts, rejects)."""
    assert events[0][0] == "blocks" and not events[0][2].any()
    current, cost, lam = events[0][1], float(events[0][1][:, -1].sum()), 1e-3
    history, accepts, rejects, i = [cost], 0, 0, 1
    while i < len(events):
        kind, got_lam, got_blocks, _ = events[i]
        assert kind == "step"
        assert got_lam == lam, "step %d ran at lambda %r, the accepts and rejects before it give %r" % (accepts + rejects, got_lam, lam)
        assert same_bits(got_blocks, current), "step %d did not get the blocks of the last accepted evaluation" % (accepts + rejects)
        evaluated = i + 1 < len(events) and events[i + 1][0] == "blocks"
        accepted = False
        if evaluated:
            cand, status = events[i + 1][1], events[i + 1][2]
            ccost = float(cand[:, -1].sum())
            accepted = not status.any() and ccost < cost
        i += 2 if evaluated else 1
        if accepted:
            current, cost, lam = cand, ccost, lam / 10.0
            history.append(cost)
            accepts += 1
        else:
            lam *= 10.0
            rejects += 1
    assert info["iters"] == accepts and info["lambda"] == lam
    assert info["cost"] == history and len(history) == accepts + 1
    assert all(b < a for a, b in zip(history, history[1:]))
    return accepts + rejects, accepts, rejects


def relative(a, b):
    return abs(a - b) / b


# ---- 1. the loop finds the minimum ----
@pytest.fixture(scope="module")
def reference(grid, start):
    t = time.perf_counter()
    Gs, cost = bc.reference_optimum(start, grid["pairs"], grid["matches"], 0)
    print("reference optimum %.10f in %.2f s" % (cost, time.perf_counter() - t))
    return cost


def starts(start):
    one, many = bc.FAR_ONE_REJECT, bc.FAR_MANY_REJECTS
    return {"chain": (start, 0), "one reject": (bc.far_start(start, one["seed"], one["persp"]), 0),
            "many rejects": (bc.far_start(start, many["seed"], many["persp"]), 0), "anchor 5": (bc.reframed(start, 5), 5)}


@pytest.fixture(scope="module")
def runs(grid, start):
    """name -> the traced run from that start, made once, inside the first test that asks for it."""
    done, begins = {}, starts(start)

    def run(name):
        if name not in done:
            Gs, info, events = traced_adjust(begins[name][0], grid, anchor=begins[name][1])
            done[name] = dict(Gs=Gs, info=info, events=events, anchor=begins[name][1],
                              cost=bc.reference_cost(Gs, grid["pairs"], grid["matches"]))
        return done[name]
    return run


def test_reference_optimum_does_not_depend_on_its_start_or_frame(grid, start, reference):
    """The yardstick itself: from the single-reject far start and in image 5's frame it ends at the same cost.  1e-12: a forward
    difference with a relative step of 1e-7 leaves the gradient wrong by about 1e-7 of itself, which moves the cost at the point
    it converges to by the square of that, 1e-14 of it, and two orders are left over; 5e-15 and 2e-15 where this was written.
    Nothing of the library runs here."""
    far = bc.reference_optimum(bc.far_start(start, bc.FAR_ONE_REJECT["seed"], bc.FAR_ONE_REJECT["persp"]), grid["pairs"], grid["matches"], 0)[1]
    other = bc.reference_optimum(bc.reframed(start, 5), grid["pairs"], grid["matches"], 5)[1]
    print("reference optimum: far start %.3e, anchor 5 %.3e relative to the chain start's" % (relative(far, reference), relative(other, reference)))
    assert relative(far, reference) <= 1e-12 and relative(other, reference) <= 1e-12
    assert reference < bc.reference_cost(start, grid["pairs"], grid["matches"]) * 0.96       # the chain's start is 5 % above it


@pytest.mark.parametrize("name", ["chain", "one reject", "many rejects", "anchor 5"])
def test_loop_ends_at_the_reference_optimum(grid, runs, reference, name):
    """`reference_cost` at the returned Gs against `reference_cost` at the reference optimiser's result, 1e-9 relative in both
    directions: above would be a loop that stops short (or a Jacobian column with the wrong sign, which still lowers the cost
    on this scene), below would be rows that went missing.  Where this was written: 2398.2901415223 on both sides, the gaps
    -7.6e-16 (chain), 1.9e-16, -9.5e-16, -1.9e-16."""
    run = runs(name)
    gap = (run["cost"] - reference) / reference
    print("%s: cost %.10f, reference %.10f, gap %.3e, %d accepted" % (name, run["cost"], reference, gap, run["info"]["iters"]))
    assert abs(gap) <= REL
    assert np.array_equal(run["Gs"][run["anchor"]], np.eye(3))


def test_the_four_runs_agree(runs):
    costs = [runs(name)["cost"] for name in ("chain", "one reject", "many rejects", "anchor 5")]
    assert max(costs) - min(costs) <= REL * min(costs)


@pytest.mark.parametrize("name", ["chain", "one reject", "many rejects", "anchor 5"])
def test_reported_cost_is_the_cost_of_the_returned_maps(grid, runs, name):
    """info["cost"][-1] (the kernel rule's sum, T divided by its largest entry) against `reference_cost` at the SAME Gs: the plain
    summation bound (2 rows + 64) u relative, 1.1e-12 for 4881 rows of two terms; 5.7e-16 at most where this was written.  A loop that
    returned a rejected candidate, or the Gs of another step than the cost it reports, fails here."""
    run = runs(name)
    rows = sum(grid["sizes"])
    diff = relative(run["info"]["cost"][-1], run["cost"])
    print("%s: reported %.12f, from the geometry %.12f, relative %.3e" % (name, run["info"]["cost"][-1], run["cost"], diff))
    assert diff <= (2 * rows + 64) * bc.U


# ---- 2. reject, then accept ----
@pytest.mark.parametrize("name, want", [("chain", None), ("one reject", bc.FAR_ONE_REJECT), ("many rejects", bc.FAR_MANY_REJECTS),
                                        ("anchor 5", None)])
def test_every_step_follows_the_loops_contract(runs, name, want):
    """`audit` on the four runs.  The far starts reject: one step of 8 (seed 3), 21 of 27 (seed 35; 6 accepted, and lambda ends
    above the ceiling) where this was written; the counts are printed, the conditions are structural."""
    run = runs(name)
    tried, accepts, rejects = audit(run["events"], run["info"])
    info = run["info"]
    print("%s: %d tried, %d accepted, lambda %.3g" % (name, tried, accepts, info["lambda"]))
    assert len(info["cost"]) == info["iters"] + 1 and accepts >= 1
    assert round(math.log10(info["lambda"])) == -3 + rejects - accepts
    if want is None:
        assert tried == info["iters"]
    else:
        assert tried > info["iters"] and rejects >= 1
        assert (rejects == 1) == (want["tried"] - want["accepted"] == 1)        # the single reject, the long run of rejects
        assert rejects >= min(want["tried"] - want["accepted"], 8)
        # after every rejected step the next one ran at 10 x lambda (audit compares the float exactly; here the sequence is shown)
        lams = [ev[1] for ev in run["events"] if ev[0] == "step"]
        assert any(b > a for a, b in zip(lams, lams[1:])) and any(b < a for a, b in zip(lams, lams[1:]))


def test_ceiling_from_the_adjusted_result(grid, runs):
    """From the optimum no step lowers the cost: 16 steps tried at lambda 1e-3 .. 1e12, none accepted, the input returned."""
    Gs0 = runs("chain")["Gs"]
    Gs, info, events = traced_adjust(Gs0, grid)
    tried, accepts, rejects = audit(events, info)
    lams = [ev[1] for ev in events if ev[0] == "step"]
    print("ceiling: %d tried, lambda %.3g -> %.3g, ends at %.3g" % (tried, lams[0], lams[-1], info["lambda"]))
    assert (tried, accepts) == (16, 0) and info["iters"] == 0 and len(info["cost"]) == 1
    assert info["lambda"] > 1e12 and round(math.log10(info["lambda"])) == 13
    assert [round(math.log10(v)) for v in lams] == list(range(-3, 13))
    assert same_bits(Gs, Gs0)


def test_max_iters_gives_a_prefix(grid, start, runs):
    full = runs("chain")["info"]
    Gs, info, events = traced_adjust(start, grid, max_iters=2)
    audit(events, info)
    assert info["iters"] == 2 and info["cost"] == full["cost"][:3]
    assert info["lambda"] == 1e-3 / 10.0 / 10.0 and round(math.log10(info["lambda"])) == -5
    none, info0, events0 = traced_adjust(start, grid, max_iters=0)
    assert info0["cost"] == full["cost"][:1] and len(events0) == 1 and same_bits(none, np.asarray(start))


# ---- 3. the two rejections no random start reaches ----
def test_a_candidate_with_a_behind_edge_is_rejected_not_raised(grid, start, runs):
    """A stand-in: the second evaluation (the first candidate's) reports RWH_BUNDLE_BEHIND on edge 3.  No ValueError; the step
    counts as rejected; the next runs at 10 x lambda from the start's blocks (audit), and the run ends at the same optimum."""
    def spoil(k, status):
        if k == 1:
            status = status.copy()
            status[3] = bc.BEHIND
        return status
    Gs, info, events = traced_adjust(start, grid, on_blocks=spoil)
    tried, accepts, rejects = audit(events, info)
    assert [ev[0] for ev in events[:4]] == ["blocks", "step", "blocks", "step"] and events[2][2][3] == bc.BEHIND
    assert events[3][1] == 1e-3 * 10.0 and same_bits(events[3][2], events[0][1])
    assert rejects >= 1 and info["cost"][0] == runs("chain")["info"]["cost"][0]
    cost = bc.reference_cost(Gs, grid["pairs"], grid["matches"])
    assert relative(cost, runs("chain")["cost"]) <= REL


def test_a_determinant_flip_is_rejected_without_an_evaluation(grid, start, runs):
    """A stand-in: the first step returns delta[1][0] = -2, so I + D(delta_1) has -1 at [0][0] and det G_1 changes its sign.  The
    candidate is not evaluated at all: the next event is the next step, at 10 x lambda, from the same blocks."""
    def flip(k, delta):
        if k == 0:
            delta = delta.copy()
            delta[1][0] = -2.0
        return delta
    Gs, info, events = traced_adjust(start, grid, on_step=flip)
    tried, accepts, rejects = audit(events, info)
    assert [ev[0] for ev in events[:4]] == ["blocks", "step", "step", "blocks"]
    assert events[1][3][1][0] == -2.0 and events[2][1] == 1e-3 * 10.0
    assert rejects >= 1
    assert all(np.sign(np.linalg.det(G)) == np.sign(np.linalg.det(G0)) for G, G0 in zip(Gs, start))
    assert relative(bc.reference_cost(Gs, grid["pairs"], grid["matches"]), runs("chain")["cost"]) <= REL


@pytest.mark.parametrize("at", [0, 1])
def test_a_singular_step_raises_at_any_step(grid, start, at):
    """A stand-in: step `at` reports RWH_BUNDLE_SINGULAR -- the first step tried, and the first one after an accepted step (from
    the chain's start step 0 is accepted: its candidate's cost is lower and no edge is BEHIND, asserted).  ValueError both times,
    where the camera rule counts the later one as a rejected step; no further step is tried and nothing more is evaluated."""
    events = []
    with pytest.raises(ValueError, match="sequence_adjust: the step's system is singular"):
        traced_adjust(start, grid, singular_at=at, events=events)
    assert [ev[0] for ev in events] == ["blocks", "step"] * (at + 1)
    assert not events[-1][3].any()
    if at == 1:
        assert not events[2][2].any() and events[2][1][:, -1].sum() < events[0][1][:, -1].sum()
        assert events[3][1] == 1e-3 / 10.0 and same_bits(events[3][2], events[2][1])


# ---- 4. masks ----
def test_mask_rows_wider_than_needed_change_nothing(grid, start):
    """The "random" masks over GRID, and the same rows with two words of ones behind them (bits past an edge's last row): the
    same bits out.  Cost 1259.72 -> 1195.56 in 5 steps where this was written; the reported cost is the geometry's over the
    masked rows (summation bound), and the masked minimum is the reference optimiser's (1e-9)."""
    import homography as hg
    masks = bc.mask_sets(grid["sizes"])["random"]
    wide = np.concatenate([masks, np.full((len(masks), 2), -1, dtype=np.int64)], axis=1)
    a_info, b_info = {}, {}
    a = hg.sequence_adjust(start, grid["pairs"], grid["matches"], masks=masks, on="host", info=a_info)
    b = hg.sequence_adjust(start, grid["pairs"], grid["matches"], masks=wide, on="host", info=b_info)
    print("random masks: cost %.2f -> %.2f in %d steps" % (a_info["cost"][0], a_info["cost"][-1], a_info["iters"]))
    assert same_bits(a, b) and a_info == b_info and a_info["iters"] >= 1
    rows = sum(bc.mask_bit(masks[e].view(np.uint64), i) for e, m in enumerate(grid["sizes"]) for i in range(m))
    assert 0 < rows < sum(grid["sizes"])
    cost = bc.reference_cost(a, grid["pairs"], grid["matches"], masks)
    assert relative(a_info["cost"][-1], cost) <= (2 * rows + 64) * bc.U
    assert relative(a_info["cost"][0], bc.reference_cost(start, grid["pairs"], grid["matches"], masks)) <= (2 * rows + 64) * bc.U
    best = bc.reference_optimum(start, grid["pairs"], grid["matches"], 0, masks)[1]
    assert abs(cost - best) <= REL * best


# ---- 5. a b that is not finite ----
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_b_names_its_pair(grid, start, bad):
    matches = [(a, b.copy()) for a, b in grid["matches"]]
    matches[6][1][17, 1] = bad
    import homography as hg
    s, d = grid["pairs"][6]
    with pytest.raises(ValueError, match=r"sequence_adjust: pair 6 \(images %d and %d\) has a cost that is not finite" % (s, d)):
        hg.sequence_adjust(start, grid["pairs"], matches, on="host")
    masks = bc.mask_sets(grid["sizes"])["ones"]
    masks[6, 0] &= ~np.int64(1 << 17)                                       # the same row as no inlier: nothing to report
    info = {}
    hg.sequence_adjust(start, grid["pairs"], matches, masks=masks, on="host", max_iters=1, info=info)
    assert info["iters"] == 1 and np.isfinite(info["cost"]).all()


# ---- 6. fma of the restatement ----
def test_fma_takes_every_float():
    """Finite operands: one rounding of the exact value (against math.fma where Python has it, and on cases worked by hand);
    non-finite operands and overflow as IEEE 754 has them."""
    inf, nan = float("inf"), float("nan")
    assert bc.fma(2.0 ** 53 + 2, 1.0, 1.0) == 2.0 ** 53 + 4                # 2^53 + 3 lies halfway: ties to even
    assert bc.fma(1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52, -1.0) == -2.0 ** -104    # exact, where product-then-sum gives 0
    assert bc.fma(0.1, 10.0, -1.0) == 2.0 ** -54
    assert math.isnan(bc.fma(nan, 1.0, 1.0)) and math.isnan(bc.fma(1.0, 1.0, nan)) and math.isnan(bc.fma(0.0, inf, 1.0))
    assert math.isnan(bc.fma(inf, 1.0, -inf))
    assert bc.fma(inf, 2.0, 1.0) == inf and bc.fma(-3.0, inf, 1e300) == -inf and bc.fma(1.0, 1.0, -inf) == -inf
    assert bc.fma(1e308, 10.0, 1.0) == inf and bc.fma(-1e308, 10.0, 1.0) == -inf
    assert bc.fma(1e308, 10.0, -1e308) == inf
    assert bc.fma(2.0 ** 1023, 2.0, 2.0 ** 1023) == inf                     # 3 * 2^1023 exactly: beyond the largest float64
    assert bc.fma(2.0 ** 1023, 2.0, -sys.float_info.max) == 2.0 ** 971      # the product alone overflows, the sum does not
    zeros = [(0.0, 5.0, 0.0, False), (-0.0, 5.0, -0.0, True), (0.0, -5.0, -0.0, True), (-0.0, 5.0, 0.0, False), (0.0, 5.0, -0.0, False),
             (3.0, 2.0, -6.0, False), (-0.0, -5.0, -0.0, False)]
    for a, b, c, negative in zeros:
        got = bc.fma(a, b, c)
        assert got == 0.0 and math.copysign(1.0, got) == (-1.0 if negative else 1.0), (a, b, c)
    assert bc.fma(2.0 ** -1074, 0.5, 0.0) == 0.0 and bc.fma(2.0 ** -1074, 0.75, 0.0) == 2.0 ** -1074      # underflow rounds to even
    if hasattr(math, "fma"):
        rng = np.random.default_rng(8)
        for a, b, c in rng.normal(0, 1, (200, 3)) * 10.0 ** rng.integers(-5, 6, (200, 3)):
            assert bc.fma(a, b, c) == math.fma(a, b, c)


# ---- 7. every side of the validity test ----
VALIDITY = ["x nan", "x +inf", "y -inf", "x 3e38", "p2 +0", "p2 -0", "p2 negative", "p2 denormal"]


@pytest.fixture(scope="module")
def validity():
    c, masks, cleared, cases = bc.validity_cases()
    assert [name for name, _, _ in cases] == VALIDITY
    return c, masks, cleared, {name: (pa, T) for name, pa, T in cases}


def hblocks(lib, *a):
    st, blocks, count, status = bc.host_blocks(lib, *a)
    assert st == 0
    return blocks, count, status


@pytest.mark.parametrize("name", VALIDITY)
def test_one_invalid_row_is_reported_and_isolated(lib, validity, name):
    """Row 130 of edge 1, invalid in one of eight ways: BEHIND on that edge alone, 199 rows counted, finite blocks with the bits of
    the run that has the row's mask bit cleared, the other edges untouched, and the twin is the restatement."""
    c, masks, cleared, cases = validity
    pa, T = cases[name]
    blocks, count, status = hblocks(lib, pa, c["pb"], c["offsets"], masks, T)
    assert status.tolist() == [bc.OK, bc.BEHIND, bc.OK] and count.tolist() == [70, 199, 9]
    assert np.isfinite(blocks).all()
    blocks2, count2, status2 = hblocks(lib, pa, c["pb"], c["offsets"], cleared, T)
    assert status2.tolist() == [bc.OK, bc.OK, bc.OK] and count2.tolist() == [70, 199, 9]
    assert same_bits(blocks, blocks2)
    plain, _, _ = hblocks(lib, c["pa"], c["pb"], c["offsets"], masks, c["T"])
    assert same_bits(blocks[[0, 2]], plain[[0, 2]])
    want, want_count, want_status = bc.restate(pa, c["pb"], c["offsets"], masks, T)
    assert same_bits(blocks, want) and np.array_equal(count, want_count) and np.array_equal(status, want_status)


def test_validity_cases_give_the_p2_they_name(validity):
    """The fixture's own claim, in exact rationals: what p2 is at row 130 in the four transfer cases."""
    from fractions import Fraction
    c, _, _, cases = validity
    at = int(c["offsets"][1]) + bc.VALIDITY_ROW
    want = {"p2 +0": Fraction(0), "p2 -0": Fraction(0), "p2 negative": Fraction(-1, 2), "p2 denormal": Fraction(1, 2 ** 1070)}
    for name, p2 in want.items():
        pa, T = cases[name]
        x, y = Fraction(float(pa[at, 0])), Fraction(float(pa[at, 1]))
        assert Fraction(T[1][2, 0]) * x + Fraction(T[1][2, 1]) * y + Fraction(T[1][2, 2]) == p2, name
    pa, T = cases["p2 -0"]
    assert np.signbit(pa[at]).all() and np.signbit(T[1][2, 2]) and np.signbit(bc.row_p2(T[1], pa[at]))
    assert not np.signbit(bc.row_p2(cases["p2 +0"][1][1], cases["p2 +0"][0][at]))
    assert 0.0 < bc.row_p2(cases["p2 denormal"][1][1], cases["p2 denormal"][0][at]) < 2.0 ** -1022


# ---- 8. the two ends of a launch ----
def test_twin_is_the_restatement_on_the_largest_launchs_first_edges(lib):
    """The 2016-edge case of the GPU test: the twin over all of it in one call, the restatement over its first 90 edges (ten of
    every size 0, 1, 2, 3, 4, 5, 7, 64, 65), and edges 0 and 2015 alone (n_edges = 1, offsets from 0) against their rows."""
    c, masks = bc.launch_case()
    assert len(c["sizes"]) == 2016 and int(c["offsets"][-1]) == 33824 and len(set(c["pairs"])) == 2016
    blocks, count, status = hblocks(lib, c["pa"], c["pb"], c["offsets"], masks, c["T"])
    assert not status.any() and np.isfinite(blocks).all()
    o = int(c["offsets"][90])
    want, want_count, _ = bc.restate(c["pa"][:o], c["pb"][:o], c["offsets"][:91], masks[:90], c["T"][:90])
    assert same_bits(blocks[:90], want) and np.array_equal(count[:90], want_count)
    for e in (0, 2015):
        one, one_count, one_status = hblocks(lib, *bc.single_edge(c, masks, e))
        assert same_bits(one, blocks[e:e + 1]) and one_count[0] == count[e] and one_status[0] == status[e]
    assert count[0] == 0 and not blocks[0].any() and 0 < count[2015] <= c["sizes"][2015]
