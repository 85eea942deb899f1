"""Per-update cost of the systematics step on the bench world.

The world is bench.py's (its build_world: 1024 x 1024 cells seeded from
detail-50000.pop, 150 burn-in updates).  Over 20 further updates, after each
update, the script times what the driver does for the genotype data files:

* a build with the device table (avgpu_get_genotypes): capi.get_genotypes
  (wall), the device time of its kernels (HIP events on the world's stream,
  avgpu_last_genotypes_ms), the bytes copied to the host, and
  GenotypeArbiter.update_table (wall);
* a build without it (--root <checkout of an earlier commit>): get_census
  (wall, 48 B per cell) and GenotypeArbiter.update (wall).

The update itself is timed the same way (queued run_update + sync, wall).

    python tools/systematics_timing.py [--root DIR] [--updates 20] [--side 1024]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout to measure (its bench.py, avida_amd and built library)")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--burn-in", type=int, default=None)
    ap.add_argument("--seed", type=int, default=101)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    torch.cuda.init()
    import bench
    from avida_amd import capi, files, systematics
    assert os.path.abspath(bench.ROOT) == root, bench.ROOT
    lib = capi.load_product()
    golden = os.path.join(root, "tests", "golden")
    h, cfg, n, _ = bench.build_world(lib, capi, files, golden, a.side, a.seed, 0, 0, 1)
    burn = bench.BURN_IN if a.burn_in is None else a.burn_in
    for _ in range(burn):
        capi.check(lib, lib.avgpu_run_update(h, None))
    capi.check(lib, lib.avgpu_sync(h))
    table_path = hasattr(capi, "get_genotypes")
    arb = systematics.GenotypeArbiter()
    rows = []
    for u in range(a.updates + 1):            # row 0 (every genotype is new; scratch allocated) is reported apart
        t0 = time.perf_counter()
        capi.check(lib, lib.avgpu_run_update(h, None))
        capi.check(lib, lib.avgpu_sync(h))
        t1 = time.perf_counter()
        r = {"update": burn + u, "update_ms": 1e3 * (t1 - t0)}
        if table_path:
            table, totals = capi.get_genotypes(lib, h)
            t2 = time.perf_counter()
            arb.update_table(table, totals, burn + u)
            t3 = time.perf_counter()
            ms, nbytes = C.c_double(), C.c_int64()
            capi.check(lib, lib.avgpu_last_genotypes_ms(h, C.byref(ms), C.byref(nbytes)))
            r.update(genotypes=len(table), organisms=int(totals.num_organisms), device_ms=ms.value,
                     bytes_to_host=nbytes.value, get_genotypes_ms=1e3 * (t2 - t1), update_table_ms=1e3 * (t3 - t2))
        else:
            census = capi.get_census(lib, "avgpu_", h, 0, n)
            t2 = time.perf_counter()
            arb.update(census, burn + u)
            t3 = time.perf_counter()
            r.update(genotypes=arb.num_genotypes(), organisms=int((census["genotype_key"] != 0).sum()),
                     bytes_to_host=census.nbytes, get_census_ms=1e3 * (t2 - t1), arbiter_update_ms=1e3 * (t3 - t2))
        r["systematics_ms"] = 1e3 * (t3 - t1)
        r["dominant"] = [arb.dominant().id, arb.dominant().num_units, arb.num_threshold()]
        rows.append(r)
        print(json.dumps(r), flush=True)
    steady = rows[1:]
    mean = lambda k: sum(x[k] for x in steady) / len(steady)     # noqa: E731
    out = {"path": "device table" if table_path else "census + host grouping", "cells": n,
           "updates": len(steady), "first_classification_ms": rows[0]["systematics_ms"],
           "mean": {k: mean(k) for k in steady[0] if k not in ("update", "dominant")}}
    if table_path:
        # the last table against the census of the same world: integers exact, the
        # double sums to num_gestated * 2^-52 (two summation orders of terms >= 0)
        import numpy as np
        ref, rtot = systematics.table_from_census(capi.get_census(lib, "avgpu_", h, 0, n))
        exact = all(np.array_equal(table[f], ref[f]) for f in table.dtype.names if not f.startswith("sum_") or
                    table.dtype[f].kind == "i")
        exact = exact and all(getattr(totals, f) == getattr(rtot, f) for f, _ in capi.GENOTYPE_TOTALS._fields_)
        worst = 0.0
        for f in ("sum_merit", "sum_fitness", "sum_repro_rate"):
            bound = ref["num_gestated"] * 2.0 ** -52 * ref[f]
            dev = np.abs(table[f] - ref[f])
            exact = exact and bool((dev <= bound).all())
            worst = max(worst, float((dev / np.maximum(ref[f], 1e-300)).max()))
        out["check"] = {"table_equals_census_table": exact, "max_relative_sum_deviation": worst}
    print(json.dumps(out), flush=True)
    lib.avgpu_destroy(h)


if __name__ == "__main__":
    main()
