"""Time the device landscape calls against the route they replace (measurement only).

Substitution landscapes (avgpu_landscapes; default): the two-step golden
landscape (735 000 mutants of one 49-site genome) and the one-step landscapes
of the 90 lineage genomes in one call (tests/golden/landscape/).  With
--indel (avgpu_landscapes_indel, avgpu_landscape_pairs): the golden genome's
insertion landscape, the insertion landscapes of the 90 lineage genomes in
one call, and the golden genome's all-pairs epistasis test.  On one device in
one session, per case:

* device ms of the call (avgpu_last_landscape_ms) and its wall ms, after one
  warm-up call that allocates the scratch test world;
* wall ms of the same mutants through avgpu_test_genomes in batches of 65536
  with the viability recursion on the host (avida_amd.landscape.spec,
  spec_indel, spec_pairs over the product's test_genomes): the only route
  before the device call existed.

Both routes' integer results are compared before anything is printed.

    python tools/landscape_timing.py [--out profiles/landscape_timing.txt]
    python tools/landscape_timing.py --indel [--out profiles/landscape_indel_timing.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from avida_amd import capi, files, landscape  # noqa: E402
import oracle_lib as ol  # noqa: E402

SEQ = "sirzaqcppqqbadpncqblcoqvcecpqcgptcbpfcoqutttycsva"
INTS = ("total_count", "dead_count", "neg_count", "neut_count", "pos_count", "peak_rank", "gestations", "site_count")
EPI_INTS = landscape.Epistasis.INT_FIELDS + ("gestations",)


def same(name, got, old, fields):
    for f in fields:
        assert getattr(got, f) == getattr(old, f), (name, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-two-step", action="store_true")
    ap.add_argument("--indel", action="store_true", help="the insertion and all-pairs cases")
    a = ap.parse_args()
    golden = os.path.join(ROOT, "tests", "golden")
    iset = files.read_instset(os.path.join(golden, "instset-classic.cfg"))
    env = files.read_environment(os.path.join(golden, "environment-logic9.cfg"))
    cfg = capi.cfg_from_avida(files.read_avida_cfg(None))
    gpu = ol.Backend("gpu", cfg, iset, env, ncells=256)
    ni = len(iset.names)
    rows = landscape.data_tokens(os.path.join(golden, "landscape", "detail.dat"))
    lineage = [iset.parse_sequence(r[20]) for r in rows]
    one = [iset.parse_sequence(SEQ)]
    tg = gpu.test_genomes
    # (name, the device call, the test_genomes route, the comparison of the two)
    if a.indel:
        def indel(genomes):
            return (lambda: landscape.full_indel(gpu, genomes, landscape.INSERT),
                    lambda: [landscape.spec_indel(tg, g, ni, landscape.INSERT) for g in genomes],
                    lambda name, x, y: same(name, x, y, INTS))

        def pairs_same(name, x, y):
            same(name, x[0], y[0], INTS[:-1])
            same(name, x[1], y[1], EPI_INTS)

        cases = [("golden-insertion",) + indel(one), ("lineage-90xinsertion",) + indel(lineage),
                 ("golden-allpairs", lambda: landscape.full_pairs(gpu, one, chart=False),
                  lambda: [landscape.spec_pairs(tg, one[0], ni)], pairs_same)]
    else:
        def sub(genomes, distance):
            return (lambda: landscape.full(gpu, genomes, distance, chart=False),
                    lambda: [landscape.spec(tg, g, ni, distance) for g in genomes],
                    lambda name, x, y: same(name, x, y, INTS))

        cases = [("lineage-90x1step",) + sub(lineage, 1)]
        if not a.skip_two_step:
            cases.append(("golden-2step",) + sub(one, 2))
    lines = ["# case mutants test_cpu_runs device_ms call_wall_ms test_genomes_route_wall_ms route/call"]
    landscape.full(gpu, [lineage[0]], 1)          # the scratch test world exists from here on
    for name, call, route_of, compare in cases:
        t0 = time.perf_counter()
        got = call()
        wall = (time.perf_counter() - t0) * 1e3
        ms, mutants, runs = landscape.last_timing(gpu)
        t0 = time.perf_counter()
        old = route_of()
        route = (time.perf_counter() - t0) * 1e3
        for x, y in zip(got, old):
            compare(name, x, y)
        lines.append(f"{name} {mutants} {runs} {ms:.2f} {wall:.2f} {route:.2f} {route / wall:.1f}")
        print(lines[-1], flush=True)
    gpu.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
