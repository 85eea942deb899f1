"""Helpers of the directed spatial-resource tests (test_res_spec.py on the CPU,
test_res_step_gpu.py on the device): bit views, the parameter sets and
environments, the seeded grids, empty worlds -- and, run as a program, one
child process that steps environment A on the GPU under whatever
AVGPU_RES_ROWS its parent set and prints every update's bits as hex."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    for _p in (os.path.dirname(HERE), HERE):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from avida_amd import capi, files   # noqa: E402

NONE = files.RES_NONE
UPDATES = 5                  # the double buffer swaps an odd and an even number of times
KINDS = ("ordinary", "extreme")
ALL_KINDS = KINDS + ("tiny",)   # tiny: one extra case (test_tiny_amounts_...), not part of the matrix
ENVS = ("A", "B", "C", "D")
GRAVITY_ENVS = ("A", "C")    # environments with a resource whose gravity is not zero

# (X, Y): degenerate tori; few rows with E = W and N = S neighbours; the
# 62-column window +-1 with Y mod 8 = 3, 1, 4, 3; 2, 3 and 4 windows, the last
# writing 62, 1 and 1 columns, with Y mod 8 = 2, 4, 6
SHAPES = [(1, 1), (1, 9), (9, 1),
          (2, 2), (2, 3), (3, 2), (3, 3), (4, 4),
          (61, 3), (62, 9), (63, 4), (64, 11),
          (124, 2), (125, 12), (187, 6)]


# the grid seed of a shape: the first (from 1 up) whose grids meet every
# condition test_res_spec.py::test_inputs_reach_the_paths states for the shape
SEED = 1
SEEDS = {(1, 9): 2, (9, 1): 6, (3, 3): 22}


def seed_of(X, Y):
    return SEEDS.get((X, Y), SEED)


def shape_id(shape):
    return f"{shape[0]}x{shape[1]}-seed{seed_of(*shape)}"


def bits(seq):
    """doubles viewed as uint64 (a list of ints): -0.0 differs from 0.0 and
    every NaN from every other"""
    return np.ascontiguousarray(seq, dtype=np.float64).view(np.uint64).tolist()


def set_resources(backend, levels, grids):
    """avgpu_set_resources: one level per resource (used for the global
    pools), one grid of ncells doubles per resource (ignored for those)"""
    n = backend.ncells
    lv = (C.c_double * max(1, len(levels)))(*levels)
    sp = (C.c_double * max(1, len(grids) * n))(*[v for g in grids for v in g])
    backend._call("set_resources", backend.h, lv, sp)


# ---- parameter sets (files.Resource objects, through capi.resources_arrays) ----
def res_G():
    return files.Resource("G", geometry=0, initial=50.0, inflow=10.0, outflow=0.1)


def res_R0(X, Y, name="R0"):
    """torus, diffusion and gravity; the inflow box wraps and exceeds the world,
    the outflow box is partial"""
    return files.Resource(name, geometry=2, inflow=10.0, outflow=0.1,
                          inflow_x1=X - 2, inflow_x2=2 * X + 1, inflow_y1=-1, inflow_y2=Y,
                          outflow_x1=0, outflow_x2=X // 2, outflow_y1=0, outflow_y2=Y - 1,
                          xdiffuse=1.0, ydiffuse=0.5, xgravity=0.2, ygravity=-0.3)


def res_R1(X, Y, name="R1"):
    """grid, diffusion and gravity; both boxes exactly the world"""
    return files.Resource(name, geometry=1, inflow=10.0, outflow=0.1,
                          inflow_x1=0, inflow_x2=X - 1, inflow_y1=0, inflow_y2=Y - 1,
                          outflow_x1=0, outflow_x2=X - 1, outflow_y1=0, outflow_y2=Y - 1,
                          xdiffuse=0.3, ydiffuse=1.0, xgravity=-0.4, ygravity=0.25)


def res_R2(X, Y, geometry, name):
    """diffusion only; an inflow box of the world's height whose width is not
    the world's (X - 1; 2 for X = 1, covering the one column twice)"""
    return files.Resource(name, geometry=geometry, inflow=10.0, outflow=0.05,
                          inflow_x1=0, inflow_x2=X - 2 if X > 1 else 1, inflow_y1=0, inflow_y2=Y - 1,
                          outflow_x1=0, outflow_x2=X - 1, outflow_y1=0, outflow_y2=Y - 1,
                          xdiffuse=1.0, ydiffuse=0.25, xgravity=0.0, ygravity=0.0)


def res_R3(X, Y):
    """grid, gravity only; every box coordinate NONE: no sink, and the inflow
    feeds the one cell (Mod(-99, X), Mod(-99, Y))"""
    return files.Resource("R3", geometry=1, inflow=10.0, outflow=0.1,
                          xdiffuse=0.0, ydiffuse=0.0, xgravity=0.5, ygravity=-0.5)


def res_R4(X, Y):
    """torus, no flows, partial boxes"""
    return files.Resource("R4", geometry=2, inflow=10.0, outflow=0.1,
                          inflow_x1=0, inflow_x2=X // 2, inflow_y1=Y // 2, inflow_y2=Y - 1,
                          outflow_x1=X // 2, outflow_x2=X - 1, outflow_y1=0, outflow_y2=Y // 2,
                          xdiffuse=0.0, ydiffuse=0.0, xgravity=0.0, ygravity=0.0)


def res_R5(X, Y, by, name):
    """grid, no flows, an inverted inflow box (x2 = x1 - by): by = 2 a
    negative share nothing adds, by = 1 (R5z) zero cells and an infinite one"""
    return files.Resource(name, geometry=1, inflow=10.0, outflow=0.1,
                          inflow_x1=1, inflow_x2=1 - by, inflow_y1=0, inflow_y2=Y - 1,
                          outflow_x1=0, outflow_x2=X - 1, outflow_y1=0, outflow_y2=Y - 1,
                          xdiffuse=0.0, ydiffuse=0.0, xgravity=0.0, ygravity=0.0)


def cell_list(r, X, Y):
    """CELL entries of resource index r, in the order that matters: cell 0, the
    last cell twice with different rates, a middle cell with outflow 0 and
    again with outflow 1 and no inflow, then three ids outside the world"""
    n, mid = X * Y, (X * Y) // 2
    rows = [(0, 1.0, 0.1), (n - 1, 0.5, 0.2), (n - 1, 2.0, 0.05), (mid, 1.0, 0.0), (mid, 0.0, 1.0),
            (-1, 3.0, 0.5), (n, 3.0, 0.5), (n + 5, 3.0, 0.5)]
    return [files.CellResource(r, c, initial=0.0, inflow=i, outflow=o) for c, i, o in rows]


def make_env(which, X, Y):
    """environments A..D (no reactions: nothing consumes)"""
    env = files.Environment()
    if which == "A":     # one fused launch, six resources, gravity somewhere; G first: index != slot
        env.resources = [res_G(), res_R0(X, Y), res_R1(X, Y), res_R3(X, Y), res_R4(X, Y),
                         res_R5(X, Y, 2, "R5"), res_R5(X, Y, 1, "R5z")]
    elif which == "B":   # one fused launch without gravity
        env.resources = [res_R2(X, Y, 2, "R2t"), res_R2(X, Y, 1, "R2g"), res_R4(X, Y)]
    elif which == "C":   # two resources through the rates kernels, one fused
        env.resources = [res_R0(X, Y, "R0c"), res_G(), res_R1(X, Y, "R1c"), res_R2(X, Y, 2, "R2t")]
        env.cells = cell_list(0, X, Y) + cell_list(2, X, Y)
    elif which == "D":   # the rates path without gravity
        env.resources = [res_R2(X, Y, 2, "R2t")]
        env.cells = cell_list(0, X, Y)
    else:
        raise ValueError(which)
    return env


# ---- seeded grids ----
def _rng(X, Y, which, kind, r):
    return np.random.default_rng([seed_of(X, Y), X, Y, ENVS.index(which), ALL_KINDS.index(kind), r])


def ordinary_grid(rng, X, Y):
    """per cell one of: uniform [0, 3), 0.0, -0.0, a negative value in (-1, 0),
    1.0; plus one 3x3 patch of equal values clipped to the world"""
    n = X * Y
    pick = rng.integers(0, 5, n)
    u = rng.random(n) * 3.0
    neg = -(rng.random(n) * 0.999 + 0.0005)
    g = np.where(pick == 0, u, np.where(pick == 1, 0.0, np.where(pick == 2, -0.0, np.where(pick == 3, neg, 1.0))))
    x0, y0, v = int(rng.integers(0, X)), int(rng.integers(0, Y)), float(rng.random() * 3.0)
    g = g.reshape(Y, X)
    g[y0:y0 + 3, x0:x0 + 3] = v
    return g.reshape(n).tolist()


def extreme_grid(rng, X, Y):
    """sign * 2^e * m, e uniform over the integers of [-1070, 950] (denormals
    included), m in [1, 2); every eighth cell exactly 0.0 or -0.0"""
    n = X * Y
    e = rng.integers(-1070, 951, n)
    m = 1.0 + rng.random(n)
    s = np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0)
    g = s * np.ldexp(m, e)
    z = np.where(rng.integers(0, 2, n) == 0, 0.0, -0.0)
    eighth = np.arange(n) % 8 == 0
    return np.where(eighth, z, g).tolist()


def tiny_grid(rng, X, Y):
    """sign * 2^e * m with e in [-1074, -1010]: every amount so small that the
    residual of a reciprocal-multiply quotient underflows, and no large
    neighbour to absorb a wrong last bit; every eighth cell +-0"""
    n = X * Y
    g = np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0) * np.ldexp(1.0 + rng.random(n), rng.integers(-1074, -1009, n))
    z = np.where(rng.integers(0, 2, n) == 0, 0.0, -0.0)
    return np.where(np.arange(n) % 8 == 0, z, g).tolist()


TINY_SHAPE = (64, 11)


def make_grids(which, kind, X, Y, env):
    """(levels, grids) for set_resources: a grid per resource (a global pool's
    is ignored), 50.0 as every pool's level"""
    build = {"ordinary": ordinary_grid, "extreme": extreme_grid, "tiny": tiny_grid}[kind]
    grids = [build(_rng(X, Y, which, kind, r), X, Y) if q.geometry else [0.0] * (X * Y)
             for r, q in enumerate(env.resources)]
    return [50.0] * len(env.resources), grids


# ---- worlds ----
def instset(golden):
    return files.read_instset(os.path.join(golden, "resources_9r", "instset-heads.cfg"))


def empty_world(kind, golden, X, Y, env, ncells=0):
    """a world without organisms: nothing but the resource kernels decides its
    resource amounts"""
    import oracle_lib as ol
    cfg = capi.cfg_from_avida(files.read_avida_cfg(None, {"WORLD_X": X, "WORLD_Y": Y}), seed=seed_of(X, Y))
    return ol.Backend(kind, cfg, instset(golden), env, ncells=ncells or X * Y)


def snapshot(b):
    """(bits of the levels, bits of every grid) of a world"""
    lv, gr = b.resources(spatial=True)
    return bits(lv), [bits(g) for g in gr]


def run_case(kind, golden, which, gkind, X, Y, updates=UPDATES):
    """the snapshots after each update of one (environment, grid kind, shape)"""
    env = make_env(which, X, Y)
    b = empty_world(kind, golden, X, Y, env)
    try:
        set_resources(b, *make_grids(which, gkind, X, Y, env))
        out = []
        for _ in range(updates):
            b.run_update()
            out.append(snapshot(b))
        return out
    finally:
        b.close()


def first_difference(want, got):
    """None, or (update, resource or 'levels', cell, want bits, got bits) of the
    first place two run_case results differ"""
    for u, ((lw, gw), (lg, gg)) in enumerate(zip(want, got)):
        for r, (a, b) in enumerate(zip(gw, gg)):
            if a != b:
                c = next(i for i in range(len(a)) if a[i] != b[i])
                return (u, r, c, "%016x" % a[c], "%016x" % b[c])
        if lw != lg:
            r = next(i for i in range(len(lw)) if lw[i] != lg[i])
            return (u, "levels", r, "%016x" % lw[r], "%016x" % lg[r])
    return None


# ---- strips ----
# (shape, strips) with 2 rows a strip.  set_tile takes whole 256-cell merit
# blocks only, so 2-row strips need WORLD_X to be a multiple of 128; narrower
# ones are refused by the oracle and the product alike (REFUSED_STRIPS)
STRIPS = [((128, 8), 4), ((128, 6), 3)]
REFUSED_STRIPS = [((5, 8), 4), ((63, 6), 3), ((1, 4), 2)]


def run_strips(kind, golden, which, gkind, X, Y, T, device="cpu", after_update=None):
    """run_case over T row strips (tile_util.make_tile, tiles.StripWorld over
    a LoopbackTransport): per update (bits of strip 0's levels, bits of every
    resource's grid, the strips' rows joined).  A spatial resource's level is
    a strip's own sum, so only the global pools' compare with the untiled
    world's."""
    from avida_amd import tiles
    import tile_util as tu
    env = make_env(which, X, Y)
    levels, grids = make_grids(which, gkind, X, Y, env)
    per = X * Y // T
    pairs = [tu.make_tile(kind, golden, X, Y, T, k, device=device, env=env, empty=True) for k in range(T)]
    try:
        for k, (b, _) in enumerate(pairs):
            set_resources(b, levels, [g[k * per:(k + 1) * per] for g in grids])
        world = tiles.StripWorld([t for _, t in pairs], tiles.LoopbackTransport())
        out = []
        for _ in range(UPDATES):
            world.update()
            if after_update:
                after_update()
            snaps = [snapshot(b) for b, _ in pairs]
            out.append((snaps[0][0], [sum((s[1][r] for s in snaps), []) for r in range(len(env.resources))]))
        return out
    finally:
        for b, _ in pairs:
            b.close()


def strips_difference(env, want, got):
    """first_difference of an untiled run_case result and a run_strips one"""
    for u, ((lw, gw), (lg, gg)) in enumerate(zip(want, got)):
        for r, q in enumerate(env.resources):
            if q.geometry and gw[r] != gg[r]:
                c = next(i for i in range(len(gw[r])) if gw[r][i] != gg[r][i])
                return (u, r, c, "%016x" % gw[r][c], "%016x" % gg[r][c])
            if not q.geometry and lw[r] != lg[r]:
                return (u, "levels", r, "%016x" % lw[r], "%016x" % lg[r])
    return None


def strips_refused(kind, golden, X, Y, T):
    """the error set_tile gives for strip 0 of T of an X x Y world, or None"""
    from avida_amd import tiles
    env = make_env("A", X, Y)
    b = empty_world(kind, golden, X, Y, env, ncells=(Y // T) * X)
    try:
        tiles.Tile(b.lib, b.p, b.h, 0, T, "cpu")
    except RuntimeError as e:
        return str(e)
    finally:
        b.close()
    return None


BAND_SHAPES = [(64, 11), (3, 3)]


def _child_main():
    """environment A, both grid kinds, on BAND_SHAPES on the GPU; one line a
    case: `X Y kind` and the hex bits of every update's levels and grids"""
    golden = os.path.join(HERE, "golden")
    for X, Y in BAND_SHAPES:
        for gkind in KINDS:
            res = run_case("gpu", golden, "A", gkind, X, Y)
            words = [f"{w:x}" for lv, gr in res for w in lv + [v for g in gr for v in g]]
            print(X, Y, gkind, " ".join(words), flush=True)


if __name__ == "__main__":
    _child_main()
