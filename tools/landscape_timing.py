"""Time avgpu_landscapes against the route it replaces (measurement only).

For the two-step golden landscape (735 000 mutants of one 49-site genome) and
for the one-step landscapes of the 90 lineage genomes in one call
(tests/golden/landscape/), on one device in one session:

* device ms of the call (avgpu_last_landscape_ms) and its wall ms, after one
  warm-up call that allocates the scratch test world;
* wall ms of the same mutants through avgpu_test_genomes in batches of 65536
  with the viability recursion on the host (avida_amd.landscape.spec over the
  product's test_genomes): the only route before avgpu_landscapes existed.

Both routes' integer results are compared before anything is printed.

    python tools/landscape_timing.py [--out profiles/landscape_timing.txt]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-two-step", action="store_true")
    a = ap.parse_args()
    golden = os.path.join(ROOT, "tests", "golden")
    iset = files.read_instset(os.path.join(golden, "instset-classic.cfg"))
    env = files.read_environment(os.path.join(golden, "environment-logic9.cfg"))
    cfg = capi.cfg_from_avida(files.read_avida_cfg(None))
    gpu = ol.Backend("gpu", cfg, iset, env, ncells=256)
    ni = len(iset.names)
    rows = landscape.data_tokens(os.path.join(golden, "landscape", "detail.dat"))
    lineage = [iset.parse_sequence(r[20]) for r in rows]
    cases = [("lineage-90x1step", lineage, 1)]
    if not a.skip_two_step:
        cases.append(("golden-2step", [iset.parse_sequence(SEQ)], 2))
    lines = ["# case mutants test_cpu_runs device_ms call_wall_ms test_genomes_route_wall_ms route/call"]
    landscape.full(gpu, [lineage[0]], 1)          # the scratch test world exists from here on
    for name, genomes, distance in cases:
        t0 = time.perf_counter()
        got = landscape.full(gpu, genomes, distance, chart=False)
        wall = (time.perf_counter() - t0) * 1e3
        ms, mutants, runs = landscape.last_timing(gpu)
        t0 = time.perf_counter()
        old = [landscape.spec(gpu.test_genomes, g, ni, distance) for g in genomes]
        route = (time.perf_counter() - t0) * 1e3
        for x, y in zip(got, old):
            for f in INTS:
                assert getattr(x, f) == getattr(y, f), (name, f)
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
