"""The ancestry invariants of a structured population save (SavePopulation
with save_historic, main/cPopulation.cc:6490): one checker, applied to the
reference's own tests/golden/detail-100.spop, which satisfies it, and to a
lineage-on save of the host arbiter; the lineage-off save is
byte for byte what it was."""
import os

import numpy as np

from avida_amd import population, systematics
import lineage_util as lu


def check_spop_ancestry(path):
    """the parents column is closed within the file, depth = the parent's
    depth + 1 (0 without a parent), a deactivated genotype has no organisms
    and a historic row (num_units 0) no cells; returns (rows, historic rows)"""
    rows = {}
    for line in open(path):
        if not line.strip() or line.startswith("#"):
            continue
        f = line.split()
        rows[int(f[0])] = dict(parents=[] if f[3] == "(none)" else [int(p) for p in f[3].split(",")],
                               num_units=int(f[4]), deactivated=int(f[12]), depth=int(f[13]), fields=len(f))
    historic = 0
    for gid, r in rows.items():
        for p in r["parents"]:
            assert p in rows, (gid, p)
            assert p < gid
        if r["parents"]:
            assert r["depth"] == max(rows[p]["depth"] for p in r["parents"]) + 1, gid
        else:
            assert r["depth"] == 0, gid
        if r["num_units"] == 0:
            historic += 1
            assert r["fields"] == 17 and r["deactivated"] >= 0, gid      # no cells, offsets, lineage labels
        else:
            assert r["fields"] == 20 and r["deactivated"] == -1, gid
    return len(rows), historic


def test_reference_save_satisfies_the_checker(golden):
    n, historic = check_spop_ancestry(os.path.join(golden, "detail-100.spop"))
    assert n == 35 and historic == 3


class _Derived:
    """an oracle world that reports the parent keys the RNG-key derivation gives"""

    def __init__(self, b):
        self.b, self.census, self.states = b, b.census, b.states
        self.exp = np.zeros(b.ncells, dtype=np.uint64)

    def parent_keys(self):
        return self.exp


def test_lineage_on_save_satisfies_the_checker_and_off_is_unchanged(golden, tmp_path):
    b, step, _ = lu.make_world("oracle", golden, "torus16_bm0")
    w = _Derived(b)
    on, off = systematics.GenotypeArbiter(3, lineage=True), systematics.GenotypeArbiter(3)
    handlers = b.instset.handlers
    before = lu.Snapshot(b)
    for u in range(41):
        if u:
            step()
            after = lu.Snapshot(b)
            w.exp = lu.expected_parent_keys(w.exp, before, after)[0]
            before = after
        systematics.classify_with_lineage(on, w, u, handlers)
        off.update(b.census(), u)
    on.prune()
    p_on, p_off, p_none = (str(tmp_path / n) for n in ("on.spop", "off.spop", "none.spop"))
    n_on = population.save_population(b, b.instset, on, p_on, 40, lineage=on.lineage)
    n_off = population.save_population(b, b.instset, off, p_off, 40)
    population.save_population(b, b.instset, on, p_none, 40)          # a lineage arbiter, saved without the argument
    rows, historic = check_spop_ancestry(p_on)
    assert rows == n_on == n_off + historic and historic > 0
    assert historic == int((on.lineage.rows["update_deactivated"] >= 0).sum())
    depths = [int(l.split()[13]) for l in open(p_on) if l.strip() and not l.startswith("#")]
    assert max(depths) >= 2

    def body(p):
        return [l for l in open(p) if not l.startswith("# ") or "Structured" in l]
    assert body(p_off) == body(p_none)
    # the lineage-off rows are the lineage-on file's living rows with the ancestry columns blanked
    living = [l.split() for l in open(p_on) if l.strip() and not l.startswith("#") and len(l.split()) == 20]
    plain = [l.split() for l in open(p_off) if l.strip() and not l.startswith("#")]
    assert [r[:3] + r[4:10] + r[11:13] + r[14:] for r in living] == [r[:3] + r[4:10] + r[11:13] + r[14:] for r in plain]
    assert all(r[3] == "(none)" and r[10] == "0" and r[13] == "0" for r in plain)
    b.close()
