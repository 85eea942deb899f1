"""The CPU oracle's spatial resource step against an independent specification
(tests/res_spec.py: the reference's SetPointers table and FlowAll loop in
plain Python), in bits, over the whole matrix the device is then held to in
test_res_step_gpu.py -- degenerate tori, few rows, window edges, boxes that
wrap, exceed the world, are inverted or empty, CELL lists with duplicates and
ids outside the world, signed zeros, denormals and amounts up to 2^950.

The oracle reaches a neighbour by Mod(x + dx) arithmetic, the specification
through the pointer table: at the degenerate shapes they are two opinions.

This file also asserts the conditions on the INPUTS that keep both suites
from passing vacuously, from the specification's counts (see each test).
"""
import functools
import math

import pytest

import res_spec as rs
import res_util as ru

# the pure-Python walk costs ~1 us a flow: the two largest shapes run every
# environment but only the ordinary grids plus environment A's extreme ones
# (A holds every parameter set but R2); every other shape runs everything
LARGE = {(125, 12), (187, 6)}


def _cases(shape):
    return [(w, k) for w in ru.ENVS for k in ru.KINDS if shape not in LARGE or k == "ordinary" or w == "A"]


@functools.lru_cache(maxsize=None)
def spec_case(which, gkind, X, Y):
    """the specification's run of one case: per update (level bits, grid bits)
    like res_util.run_case, the Counts per resource, the amounts after update 1"""
    env = ru.make_env(which, X, Y)
    levels, grids = ru.make_grids(which, gkind, X, Y, env)
    counts = [rs.Counts() for _ in env.resources]
    out, first = [], None
    for u in range(ru.UPDATES):
        for r, q in enumerate(env.resources):
            if q.geometry:
                cells = [c for c in env.cells if c.resource == r]
                grids[r] = rs.step(q, cells, X, Y, grids[r], counts[r])
        if u == 0:
            first = [list(g) for g in grids]
        out.append(([rs.level(g) if q.geometry else None for g, q in zip(grids, env.resources)],
                    [ru.bits(g) for g in grids]))
    return env, out, counts, first


@pytest.mark.parametrize("shape", ru.SHAPES, ids=ru.shape_id)
def test_oracle_equals_spec(golden, shape):
    """Oracle == specification, levels and per-cell amounts in bits, after
    every one of 5 updates of an empty world (a global pool's level is the
    oracle's own business: the specification is of the spatial step)."""
    X, Y = shape
    for which, gkind in _cases(shape):
        env, want, _, _ = spec_case(which, gkind, X, Y)
        got = ru.run_case("oracle", golden, which, gkind, X, Y)
        for u, ((lw, gw), (lg, gg)) in enumerate(zip(want, got)):
            for r, q in enumerate(env.resources):
                if not q.geometry:
                    continue
                if gw[r] != gg[r]:
                    c = next(i for i in range(X * Y) if gw[r][i] != gg[r][i])
                    pytest.fail(f"env {which} {gkind} update {u} resource {q.name} cell {c}: "
                                f"spec {gw[r][c]:016x} oracle {gg[r][c]:016x}")
                assert ru.bits([lw[r]]) == [lg[r]], (which, gkind, u, q.name)


@pytest.mark.parametrize("shape", ru.SHAPES, ids=ru.shape_id)
def test_inputs_reach_the_paths(shape):
    """Conditions on the test inputs (not tolerances), from the specification's
    counts; with another seed if one ever fails, never with a weaker condition.

    * extreme grids, every environment (all four have flows), shapes of at
      least 9 cells: a quotient operand in each of the classes zero, inside
      [2^-900, 2^900] and outside it, every amount finite after all 5 updates;
      in the environments with gravity the zero class must also be reached
      where the device really divides (Counts.zero_live);
    * ordinary grids, shapes of at least 9 cells, every environment: a flow
      between equal amounts (a +-0 diffusion term) and a negative amount in
      the seeded grid (what makes the max(.., 0) of Sink and CellOutflow
      matter in the first step); and in at least one environment of the shape
      a negative amount is still there after the first update, so the clamps
      matter in the later steps too.  (Not in every environment: D's only
      resource at X = 1 feeds every cell 10 / 9 a step, more than the seeded
      negatives of (-1, 0) can outlast.)
    * environment A, X >= 3: R0's inflow box covers cells a different number
      of times, at least twice and at least three times.  (The box is X + 4
      columns by Y + 2 rows, so a cell is covered cx * cy times with cx in
      {1, 2} (X >= 4; {2, 3} at X = 3) and cy in {1, 2} (Y >= 3; 2 at Y = 2, 3
      at Y = 1): the counts reached are 2 and 4 -- 3 and 6 at Y = 1, up to 6
      at X = 3 -- never exactly 2 AND exactly 3 in one world.)"""
    X, Y = shape
    still_negative = False
    for which, gkind in _cases(shape):
        env, _, counts, first = spec_case(which, gkind, X, Y)
        tot = {f: sum(getattr(c, f) for c in counts) for f in ("zero", "zero_live", "inside", "outside", "equal_ends")}
        if X * Y >= 9 and gkind == "extreme":
            assert tot["zero"] > 0 and tot["inside"] > 0 and tot["outside"] > 0, (which, tot)
            if which in ru.GRAVITY_ENVS:
                assert tot["zero_live"] > 0, (which, tot)
            assert all(c.finite for c in counts), which
        if X * Y >= 9 and gkind == "ordinary":
            assert tot["equal_ends"] > 0, which
            seeded = ru.make_grids(which, gkind, X, Y, env)[1]
            assert any(a < 0.0 for g, q in zip(seeded, env.resources) if q.geometry for a in g), which
            still_negative |= any(a < 0.0 for g, q in zip(first, env.resources) if q.geometry for a in g)
        if which == "A" and X >= 3:
            multi = sorted({c for c in counts[1].cover if c >= 2})
            assert len(multi) >= 2 and multi[-1] >= 3, multi
    assert still_negative or X * Y < 9


def _res(**kw):
    from avida_amd import files
    base = dict(geometry=2, inflow=0.0, outflow=0.0, xdiffuse=0.0, ydiffuse=0.0, xgravity=0.0, ygravity=0.0)
    base.update(kw)
    return files.Resource("T", **base)


def test_spec_conserves_on_a_torus():
    """No source (inflow 0: the NONE box feeds one cell nothing) and no sink:
    flows only move matter, so the total changes by rounding alone -- each of
    the n cells' sums of 8 terms and the n-term total round a few times, well
    inside n * ulp(total) per step for amounts of like size."""
    import numpy as np
    X, Y = 7, 5
    g = (1.0 + np.random.default_rng(ru.SEED).random(X * Y)).tolist()
    p = _res(xdiffuse=1.0, ydiffuse=0.5, xgravity=0.2, ygravity=-0.3)
    t0 = rs.level(g)
    for _ in range(ru.UPDATES):
        g = rs.step(p, [], X, Y, g)
        assert abs(rs.level(g) - t0) <= X * Y * math.ulp(t0)
        assert g != [g[0]] * (X * Y)


def test_spec_grid_gravity_loses_nothing_over_the_edges():
    """A GRID with gravity only: matter piles up against the +x / -y walls but
    none leaves (no pointer crosses an edge); the far wall's cells gain."""
    X, Y = 5, 4
    g = [1.0] * (X * Y)
    p = _res(geometry=1, xgravity=0.5, ygravity=-0.5)
    for _ in range(ru.UPDATES):
        g = rs.step(p, [], X, Y, g)
        assert abs(rs.level(g) - X * Y) <= X * Y * math.ulp(float(X * Y))
    assert g[X - 1] > 1.0 and g[(Y - 1) * X] < 1.0     # top right gained, bottom left drained
    assert all(a >= 0.0 for a in g)


def test_spec_hand_computed_2x2():
    """One step of a 2x2 GRID, diffusion 1 / 1, no gravity, amounts 16 0 / 0 0,
    by hand.  Pointers of cell 0: E -> 1, SE -> 3, S -> 2; cell 1: SW -> 2, S ->
    3; cell 2: E -> 3.  Flows out of cell 0: E = 1 * 16 / 16 = 1 (x term only),
    S = 1, SE = (1 + 1) / 2 / sqrt(2) = 1 / sqrt(2); all other flows run
    between zeros.  So cell 0 keeps 16 - 1 - 1/sqrt(2) - 1."""
    p = _res(geometry=1, xdiffuse=1.0, ydiffuse=1.0)
    d = 1.0 / math.sqrt(2.0)
    assert rs.step(p, [], 2, 2, [16.0, 0.0, 0.0, 0.0]) == [((0.0 - 1.0) - d - 1.0) + 16.0, 1.0, 1.0, d]
    # and the pointer table itself: a 2x2 torus reaches cell 1 both E and W
    t = rs.set_pointers(rs.TORUS, 2, 2)
    assert [t[0][k][0] for k in range(8)] == [3, 2, 3, 1, 3, 2, 3, 1]
    assert [rs.set_pointers(rs.GRID, 2, 2)[0][k][0] for k in range(8)] == [-99, -99, -99, 1, 3, 2, -99, -99]


@pytest.mark.parametrize("shape,T", ru.STRIPS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"T{v}")
def test_oracle_strips_equal_untiled(golden, shape, T):
    """Empty worlds cut into T strips of 2 rows (the fewest set_tile takes):
    every strip's rows == the untiled oracle's, the global pool too, in bits
    after every update -- environments A and C, both grid kinds."""
    X, Y = shape
    for which in ("A", "C"):
        for gkind in ru.KINDS:
            want = ru.run_case("oracle", golden, which, gkind, X, Y)
            got = ru.run_strips("oracle", golden, which, gkind, X, Y, T)
            assert ru.strips_difference(ru.make_env(which, X, Y), want, got) is None, (which, gkind)


@pytest.mark.parametrize("shape,T", ru.REFUSED_STRIPS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"T{v}")
def test_oracle_refuses_narrow_strips(golden, shape, T):
    """2-row strips of worlds narrower than 128 columns are no whole merit
    blocks: set_tile refuses them (the product must too:
    test_res_step_gpu.py)."""
    err = ru.strips_refused("oracle", golden, *shape, T)
    assert err is not None and ("256" in err or "rows" in err), err


def _fma(a, b, c):
    """RN(a * b + c), exactly: Fraction arithmetic, one rounding"""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def test_tiny_amounts_inputs(golden):
    """The one extra case of test_res_step_gpu.py (environment A, all amounts
    at 2^-1074 .. 2^-1010, res_util.tiny_grid): oracle == specification, and
    the inputs hold quotients that div_const WITHOUT its range guard would get
    wrong -- y = RN(x r), e = RN(x - c y), RN(y + e r), whose residual e
    underflows down there -- so the guard's full division is what the device
    is held to.  (In the matrix's extreme grids such an operand nearly always
    sits beside amounts 2^1900 times larger, which absorb its last bit.)"""
    X, Y = ru.TINY_SHAPE
    env, want, counts, _ = spec_case("A", "tiny", X, Y)
    got = ru.run_case("oracle", golden, "A", "tiny", X, Y)
    for (_, gw), (_, gg) in zip(want, got):
        assert gw[1:] == gg[1:]
    wrong = 0
    for c in counts:
        for x, d in c.tiny[:4000]:
            r = 1.0 / d
            y = x * r
            wrong += _fma(_fma(-d, y, x), r, y) != x / d
    assert wrong >= 10, wrong
