"""Write tests/golden/landscape/land-2step-exact.json: the two-step landscape of
the golden genome by the specification (avida_amd.landscape.spec) over the CPU
oracle -- the integer fields, gestations, site_count, peak_rank and the sums as
hex floats (about 20 s).  tests/test_landscape_spec.py checks the file against
the same computation and against the reference's land-2step.dat.

    python tools/landscape_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from avida_amd import capi, files, landscape  # noqa: E402
import oracle_lib as ol  # noqa: E402
import test_landscape_spec as t  # noqa: E402


def main():
    golden = os.path.join(ROOT, "tests", "golden")
    iset = files.read_instset(os.path.join(golden, "instset-classic.cfg"))
    env = files.read_environment(os.path.join(golden, "environment-logic9.cfg"))
    cfg = capi.cfg_from_avida(files.read_avida_cfg(None))
    b = ol.Backend("oracle", cfg, iset, env, ncells=1)
    ls = landscape.spec(b.test_genomes, iset.parse_sequence(t.SEQ), len(iset.names), 2)
    assert ls.cases == t.CASES_2STEP, ls.cases
    with open(os.path.join(golden, "landscape", "land-2step-exact.json"), "w") as f:
        json.dump(t.exact_of(ls), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
