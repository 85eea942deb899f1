"""Ancestry end to end: the host lineage rules fed from a
running world -- the device's genotype table, the parent keys it records with
every birth, and the new genotypes' tape prefixes."""
import os

import numpy as np
import pytest

from avida_amd import capi, driver, systematics
import lineage_util as lu
import oracle_lib as ol


class _World:
    """the calls classify_with_lineage makes, over the tests' product Backend"""

    def __init__(self, b):
        self.b, self.census, self.states = b, b.census, b.states

    def genotypes(self):
        return capi.get_genotypes(self.b.lib, self.b.h)

    def parent_keys(self):
        return lu.parent_keys(self.b)


def test_driver_refuses_lineage_on_a_world_without_parent_keys(golden, tmp_path):
    cfgdir = os.path.join(golden, "spatial_res_100u", "config")
    with pytest.raises(ValueError, match="parent keys"):
        driver.Driver(cfgdir, str(tmp_path), make_world=lambda c, i, e: ol.Backend("oracle", c, i, e), lineage=True)
    arb = systematics.GenotypeArbiter(3, lineage=True)
    b = ol.Backend("oracle", *_cfg(golden))
    with pytest.raises(ValueError, match="parent keys"):
        systematics.classify_with_lineage(arb, b, 0, b.instset.handlers)
    b.close()


def _cfg(golden):
    import parity_util as pu
    iset, env, cfg = pu.load_env(golden, overrides={"WORLD_X": 8, "WORLD_Y": 8}, seed=3)
    return cfg, iset, env


@pytest.mark.gpu
def test_lineage_of_a_real_run(golden):
    """the 16 x 16 world, 60 updates, one batch step per update, a
    classification after every update: every new genotype's parent is the
    genotype the derivation (lineage_util: RNG keys alone) names for its first
    cell; no orphan arises (a newborn stops before its first viable divide, so
    every parent was classified an update earlier); every captured sequence
    hashes to its key; the dominant's lineage ends at an injected genotype
    with the depth falling by one per step and neighbouring genomes differing"""
    b, step, _ = lu.make_world("gpu", golden, "torus16_bm0")
    w = _World(b)
    arb = systematics.GenotypeArbiter(3, lineage=True)
    handlers = b.instset.handlers
    systematics.classify_with_lineage(arb, w, 0, handlers)
    store = arb.lineage
    assert len(store.rows) == 1 and int(store.rows["parent_id"][0]) == 0 and int(store.rows["depth"][0]) == 0
    before = lu.Snapshot(b)
    exp = np.zeros(b.ncells, dtype=np.uint64)
    for u in range(1, 61):
        step()
        after = lu.Snapshot(b)
        exp, new, unres, amb, _ = lu.expected_parent_keys(exp, before, after)
        assert unres == 0 and amb == 0
        n0 = len(store.rows)
        table, _ = w.genotypes()
        systematics.classify_with_lineage(arb, w, u, handlers)
        first = {int(k): int(c) for k, c in zip(table["genotype_key"], table["first_cell"])}
        for r in store.rows[n0:]:
            want = int(exp[first[int(r["genotype_key"])]])
            assert want != 0 and int(r["parent_id"]) > 0, (u, int(r["id"]))
            parent = store.rows[store.index(int(r["parent_id"]))]
            assert int(parent["genotype_key"]) == want
            assert int(r["depth"]) == int(parent["depth"]) + 1 and int(r["update_born"]) == u
        if u % 20 == 0:
            kept = {int(i) for i in store.rows["id"][store.kept_by_prune()]}
            arb.prune()
            assert {int(i) for i in store.rows["id"]} == kept
        before = after
    s = store.summary()
    assert s["num_orphans"] == 0 and s["rows"] > 50 and s["max_depth"] >= 2, s
    captured = 0
    for r in store.rows:
        seq = store.sequence(int(r["id"]))
        if seq is not None:
            captured += 1
            assert len(seq) == int(r["genome_length"]) and systematics.genome_key(seq) == int(r["genotype_key"])
    assert captured == int((store.rows["seq_off"] >= 0).sum()) and captured > s["rows"] // 2
    dom = arb.dominant()
    path = arb.lineage_of(dom.id)
    assert int(path[0]["id"]) == dom.id and int(path[-1]["parent_id"]) == 0 and int(path[-1]["depth"]) == 0
    assert [int(r["depth"]) for r in path] == list(range(len(path) - 1, -1, -1))
    assert arb.dominant_row(60)[11] == len(path) - 1
    for a, c in zip(path[:-1], path[1:]):
        sa, sc = store.sequence(int(a["id"])), store.sequence(int(c["id"]))
        assert int(a["genotype_key"]) != int(c["genotype_key"])
        if sa is not None and sc is not None:
            assert sa != sc
    b.close()
