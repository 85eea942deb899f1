"""Time the device distance calls on the bench world against the host route
they replace (measurement only).

The world is bench.py's (its build_world: 1024 x 1024 cells seeded from
detail-50000.pop, 150 burn-in updates).  On one device in one session:

* avgpu_cell_distances: every cell's Hamming and Levenshtein distance to the
  dominant genotype's genome (its first cell's tape prefix) -- device ms (HIP
  events, avgpu_last_distance_ms) and wall ms of the call, after one warm-up
  call that allocates the scratch; the Hamming-only call beside it;
* avgpu_site_histogram: the same two figures, and the consensus genome's
  length and edit distance to the dominant;
* the host route: avgpu_get_states of a 65 536-cell slice (a 2-KiB tape per
  cell crosses to the host) plus the fallback of avida_amd.distance over those
  states (the specification, one distance per distinct genome), wall ms; the
  whole world's figure is that times cells / 65 536, EXTRAPOLATED and labelled
  so.  The slice's distances and histogram are compared with the device's
  before anything is printed.

    python tools/distance_timing.py [--out profiles/distance_timing.txt] [--side 1024]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLICE = 65536


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--burn-in", type=int, default=None)
    ap.add_argument("--seed", type=int, default=101)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import numpy as np
    import bench
    from avida_amd import capi, distance, files
    lib = capi.load_product()
    golden = os.path.join(ROOT, "tests", "golden")
    h, cfg, n, _ = bench.build_world(lib, capi, files, golden, a.side, a.seed, 0, 0, 1)
    burn = bench.BURN_IN if a.burn_in is None else a.burn_in
    for _ in range(burn):
        capi.check(lib, lib.avgpu_run_update(h, None))
    capi.check(lib, lib.avgpu_sync(h))

    class World:                                  # what avida_amd.distance asks of a world
        p = "avgpu_"
        ncells = n

        @staticmethod
        def states(first, count, cap=capi.MAX_GENOME):
            st = (capi.AvgpuCpuState * count)()
            ops = np.zeros(count * cap, dtype=np.uint8)
            fl = np.zeros(count * cap, dtype=np.uint8)
            capi.check(lib, lib.avgpu_get_states(h, first, count, st, ops.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                 fl.ctypes.data_as(C.POINTER(C.c_uint8)), cap))
            return st, ops.tobytes(), None
    World.lib, World.h = lib, h

    s = capi.classify_genotypes(lib, h, burn, 3)
    dom_cell, dom_units = int(s["dominant"]["first_cell"]), int(s["dominant"]["num_units"])
    st, ops, _ = World.states(dom_cell, 1)
    dom = ops[:st[0].birth_length]
    lines = [f"# bench world {a.side} x {a.side}, {burn} burn-in updates: {int(s['num_organisms'])} organisms, "
             f"{int(s['num_genotypes'])} genotypes; dominant: {dom_units} organisms, {len(dom)} sites",
             "# case cells device_ms call_wall_ms"]

    def timed(name, call):
        call()                                    # the scratch exists from here on
        t0 = time.perf_counter()
        out = call()
        wall = (time.perf_counter() - t0) * 1e3
        ms, _, cells = distance.last_timing(World)
        lines.append(f"{name} {cells} {ms:.3f} {wall:.3f}")
        print(lines[-1], flush=True)
        return out

    ham, edit = timed("cell_distances-hamming+edit", lambda: distance.cell_distances(World, dom))
    timed("cell_distances-hamming", lambda: distance.cell_distances(World, dom, edit=False))
    hist, living = timed("site_histogram", lambda: distance.site_histogram(World))
    iset = files.read_instset(os.path.join(golden, "instset-classic.cfg"))
    con = distance.consensus(hist, len(iset.names))
    alive = ham >= 0
    lines.append(f"# living {living}: mean hamming {ham[alive].mean():.3f}, mean edit {edit[alive].mean():.3f}, "
                 f"max edit {int(edit.max())}, cells at distance 0: {int((edit == 0).sum())}; consensus genome "
                 f"{con.length} sites, edit distance to the dominant {distance.spec_edit_fast(con.genome, dom)}, "
                 f"total entropy {con.total_entropy:.4f}")
    # the host route on a slice
    first = (n // 2) // SLICE * SLICE if n >= 2 * SLICE else 0
    count = min(SLICE, n)

    class Slice(World):
        last = None

        @staticmethod
        def states(f, c, cap=capi.MAX_GENOME):
            Slice.last = World.states(f, c, cap)
            return Slice.last
    t0 = time.perf_counter()
    Slice.states(first, count)
    t1 = time.perf_counter()
    keep = Slice.last
    Slice.states = staticmethod(lambda f, c, cap=capi.MAX_GENOME: keep)      # (the copy is timed once)
    sh, se = distance.cell_distances(Slice, dom, first, count, device=False)
    t2 = time.perf_counter()
    shist, sliving = distance.site_histogram(Slice, first, count, n_ops=len(iset.names), device=False)
    t3 = time.perf_counter()
    assert sh.tobytes() == ham[first:first + count].tobytes() and se.tobytes() == edit[first:first + count].tobytes()
    dhist, dliving = distance.site_histogram(World, first, count)
    assert dliving == sliving and dhist.tobytes() == shist.tobytes()
    scale = n / count
    get_ms, dist_ms, hist_ms = (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3
    lines += [f"# host route on cells {first} .. {first + count - 1} ({count} cells), wall ms, and x {scale:g} "
              f"EXTRAPOLATED to the {n} cells",
              "# step slice_wall_ms extrapolated_world_ms",
              f"get_states {get_ms:.1f} {get_ms * scale:.0f}",
              f"fallback-distances {dist_ms:.1f} {dist_ms * scale:.0f}",
              f"fallback-histogram {hist_ms:.1f} {hist_ms * scale:.0f}"]
    lib.avgpu_destroy(h)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
