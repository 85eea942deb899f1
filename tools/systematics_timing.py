"""Per-update cost of the systematics step on the bench world.

The world is bench.py's (its build_world: 1024 x 1024 cells seeded from
detail-50000.pop, 150 burn-in updates).  Over 20 further updates, after each
update, the script times what the driver does for the genotype data files:

* a build with the device table (avgpu_get_genotypes): capi.get_genotypes
  (wall), the device time of its kernels (HIP events on the world's stream,
  avgpu_last_genotypes_ms), the bytes copied to the host, and
  GenotypeArbiter.update_table (wall);
* a build with the device arbiter (avgpu_classify_genotypes) too: in the same
  session, on the same world, right after the route above at every update,
  DeviceGenotypeArbiter.classify (wall), the device time of its kernels
  (avgpu_last_arbiter_ms) and the bytes that crossed to the host; the two
  arbiters are compared at the end;
* a build without it (--root <checkout of an earlier commit>): get_census
  (wall, 48 B per cell) and GenotypeArbiter.update (wall).

With --table FILE the per-update means of the routes are also written as a
text table (device ms, bytes to the host, wall ms of the systematics step).

The update itself is timed the same way (queued run_update + sync, wall).

With --lineage the script measures the lineage store instead:
the store is turned on before the first classification, every update is
classified on the device, and per update it reports the device ms of the
arbiter (avgpu_last_arbiter_ms: the classification without the store) and of
the store's part (avgpu_last_lineage_ms), the rows appended and the store's
size; after the last update one prune, with its device ms and what it keeps.

    python tools/systematics_timing.py [--root DIR] [--updates 20] [--side 1024] [--lineage]
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
    ap.add_argument("--table", default=None, help="write the routes' means as a text table to this file")
    ap.add_argument("--lineage", action="store_true", help="measure the lineage store (DESIGN.md 10.6)")
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
    if a.lineage:
        lineage_timing(a, lib, capi, h, n, burn)
        lib.avgpu_destroy(h)
        return
    table_path = hasattr(capi, "get_genotypes")
    arb = systematics.GenotypeArbiter()
    device_path = table_path and hasattr(lib, "avgpu_classify_genotypes")
    if device_path:
        class World:                              # what DeviceGenotypeArbiter asks of a world
            classify_genotypes = staticmethod(lambda update, thr: capi.classify_genotypes(lib, h, update, thr))
            arbiter_state = staticmethod(lambda: capi.get_arbiter(lib, h))
        darb = systematics.DeviceGenotypeArbiter(arb.threshold)
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
        if device_path:
            t4 = time.perf_counter()
            darb.classify(World, burn + u)
            t5 = time.perf_counter()
            ms, nbytes = C.c_double(), C.c_int64()
            capi.check(lib, lib.avgpu_last_arbiter_ms(h, C.byref(ms), C.byref(nbytes)))
            r.update(classify_device_ms=ms.value, classify_bytes_to_host=nbytes.value,
                     classify_systematics_ms=1e3 * (t5 - t4))
            g = darb.dominant()
            assert r["dominant"] == [g.id, g.num_units, darb.num_threshold()], (r["dominant"], g.id)
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
    if device_path:
        import numpy as np
        same = all(np.array_equal(getattr(darb, f), getattr(arb, f))
                   for f in ("keys", "ids", "lengths", "born", "units", "total", "thr", "name_no"))
        same = same and (darb.next_id, darb.tot_genotypes, darb.tot_threshold, darb.sz_count, darb.best_key) == \
            (arb.next_id, arb.tot_genotypes, arb.tot_threshold, arb.sz_count, arb.best_key)
        m = out["mean"]
        out.setdefault("check", {})["device_arbiter_equals_host_arbiter"] = bool(same)
        out["ratio_systematics_ms"] = m["systematics_ms"] / m["classify_systematics_ms"]
    print(json.dumps(out), flush=True)
    if a.table:
        m = out["mean"]
        lines = ["# tools/systematics_timing.py --side %d: per-update means over the %d updates after %d burn-in updates,"
                 % (a.side, len(steady), burn),
                 "# %d cells, %.0f organisms, %.0f genotypes; update itself %.3f ms (wall)"
                 % (n, m["organisms"], m["genotypes"], m["update_ms"]),
                 "%-44s %12s %16s %16s" % ("route", "device ms", "bytes to host", "systematics ms")]
        if table_path:
            lines.append("%-44s %12.3f %16.0f %16.3f" % ("get_genotypes + GenotypeArbiter.update_table",
                                                        m["device_ms"], m["bytes_to_host"], m["systematics_ms"]))
        else:
            lines.append("%-44s %12s %16.0f %16.3f" % ("get_census + GenotypeArbiter.update", "-",
                                                      m["bytes_to_host"], m["systematics_ms"]))
        if device_path:
            lines.append("%-44s %12.3f %16.0f %16.3f" % ("classify_genotypes (device arbiter)",
                                                        m["classify_device_ms"], m["classify_bytes_to_host"],
                                                        m["classify_systematics_ms"]))
            lines.append("# ratio of the systematics step, host route / device route: %.1f"
                         % out["ratio_systematics_ms"])
            lines.append("# the two arbiters agree at the end: %s" % out["check"]["device_arbiter_equals_host_arbiter"])
            import statistics
            mh = statistics.median(x["systematics_ms"] for x in steady)
            md = statistics.median(x["classify_systematics_ms"] for x in steady)
            lines.append("# medians over the same %d updates: host route %.3f ms, device route %.3f ms (ratio %.1f)"
                         % (len(steady), mh, md, mh / md))
            slow = [x for x in steady if x["classify_systematics_ms"] > 3.0 * md]
            if slow:
                lines.append("# device route, wall time above 3 x its median (in the mean above): "
                             + ", ".join("update %d %.1f ms (device %.3f ms)"
                                         % (x["update"], x["classify_systematics_ms"], x["classify_device_ms"])
                                         for x in slow))
            lines.append("# first classification (update %d: every genotype new, buffers allocated): host route %.1f ms, "
                         "device route %.3f ms wall, %.3f ms device"
                         % (rows[0]["update"], rows[0]["systematics_ms"], rows[0]["classify_systematics_ms"],
                            rows[0]["classify_device_ms"]))
            lines.append("#")
            lines.append("# per update: update, device ms and wall ms of classify_genotypes, wall ms of the host route, "
                         "wall ms of the update")
            lines += ["%d %.3f %.3f %.2f %.3f" % (x["update"], x["classify_device_ms"], x["classify_systematics_ms"],
                                                  x["systematics_ms"], x["update_ms"]) for x in rows]
        with open(a.table, "w") as f:
            f.write("\n".join(lines) + "\n")
    lib.avgpu_destroy(h)


def lineage_timing(a, lib, capi, h, n, burn):
    capi.enable_lineage(lib, h, True)
    rows = []
    for u in range(a.updates + 1):            # row 0: every genotype is new, the buffers are allocated
        t0 = time.perf_counter()
        capi.check(lib, lib.avgpu_run_update(h, None))
        capi.check(lib, lib.avgpu_sync(h))
        t1 = time.perf_counter()
        s = capi.classify_genotypes(lib, h, burn + u, 3)
        t2 = time.perf_counter()
        ams, nb, lms, pms = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        capi.check(lib, lib.avgpu_last_arbiter_ms(h, C.byref(ams), C.byref(nb)))
        capi.check(lib, lib.avgpu_last_lineage_ms(h, C.byref(lms), C.byref(pms)))
        ls = capi.get_lineage(lib, h, summary_only=True)[2]
        r = {"update": burn + u, "update_ms": 1e3 * (t1 - t0), "classify_wall_ms": 1e3 * (t2 - t1),
             "arbiter_device_ms": ams.value, "lineage_device_ms": lms.value, "genotypes": int(s["num_genotypes"]),
             "rows_appended": int(s["num_new"]), "store_rows": int(ls["rows"]), "arena_bytes": int(ls["arena_bytes"]),
             "num_unsequenced": int(ls["num_unsequenced"]), "num_orphans": int(ls["num_orphans"]),
             "max_depth": int(ls["max_depth"])}
        rows.append(r)
        print(json.dumps(r), flush=True)
    before = rows[-1]
    t0 = time.perf_counter()
    ps = capi.prune_lineage(lib, h)
    t1 = time.perf_counter()
    lms, pms = C.c_double(), C.c_double()
    capi.check(lib, lib.avgpu_last_lineage_ms(h, C.byref(lms), C.byref(pms)))
    steady = rows[1:]
    mean = lambda k: sum(x[k] for x in steady) / len(steady)     # noqa: E731
    out = {"cells": n, "updates": len(steady), "mean": {k: mean(k) for k in steady[0] if k != "update"},
           "prune": {"update": before["update"], "device_ms": pms.value, "wall_ms": 1e3 * (t1 - t0),
                     "rows_before": before["store_rows"], "rows_kept": int(ps["rows"]),
                     "active_rows": int(ps["active_rows"]), "dropped": int(ps["dropped_last_prune"]),
                     "arena_bytes_before": before["arena_bytes"], "arena_bytes_kept": int(ps["arena_bytes"])}}
    print(json.dumps(out), flush=True)
    if a.table:
        m, p = out["mean"], out["prune"]
        lines = ["# tools/systematics_timing.py --lineage --side %d: %d updates after %d burn-in updates, %d cells"
                 % (a.side, len(steady), burn, n),
                 "# per-update means: %.0f genotypes, %.0f rows appended; device ms: arbiter %.3f, lineage part %.3f "
                 "(classification with the store %.3f); wall ms of the classification %.3f; the update itself %.3f"
                 % (m["genotypes"], m["rows_appended"], m["arbiter_device_ms"], m["lineage_device_ms"],
                    m["arbiter_device_ms"] + m["lineage_device_ms"], m["classify_wall_ms"], m["update_ms"]),
                 "# first classification (update %d, %d rows appended): arbiter %.3f ms, lineage part %.3f ms device"
                 % (rows[0]["update"], rows[0]["rows_appended"], rows[0]["arbiter_device_ms"],
                    rows[0]["lineage_device_ms"]),
                 "# prune after update %d: %.3f ms device (%.3f ms wall); rows %d -> %d (%d active, %d dropped); "
                 "arena bytes %d -> %d" % (p["update"], p["device_ms"], p["wall_ms"], p["rows_before"], p["rows_kept"],
                                           p["active_rows"], p["dropped"], p["arena_bytes_before"],
                                           p["arena_bytes_kept"]),
                 "# store at the last update: %d unsequenced, %d orphans, largest depth %d"
                 % (before["num_unsequenced"], before["num_orphans"], before["max_depth"]),
                 "#", "# per update: update, genotypes, rows appended, store rows, arena bytes, arbiter device ms, "
                 "lineage device ms, classification wall ms"]
        lines += ["%d %d %d %d %d %.3f %.3f %.3f" % (x["update"], x["genotypes"], x["rows_appended"], x["store_rows"],
                                                    x["arena_bytes"], x["arbiter_device_ms"], x["lineage_device_ms"],
                                                    x["classify_wall_ms"]) for x in rows]
        with open(a.table, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
