"""Pin the insertion, deletion and all-pairs specifications
(avida_amd.landscape.spec_indel / spec_pairs over the CPU oracle).

The reference ships no expected files for InsertionLandscape, DeletionLandscape
and PairTestLandscape, so the pins are: counts computed once by an independent
script over the same oracle (the constants below), the golden land-dump.dat
line, which the one-step half of the all-pairs test must reproduce
(BuildFitnessChart is a one-step pass through ProcessGenome), and
tests/golden/landscape/land-pairs-exact.json, the all-pairs record written
once by the specification (integers as integers, doubles as hex floats).

Every sequence is in the order of instset-classic.cfg.
"""
import json
import math
import os

import pytest

from avida_amd import capi, files, landscape
import oracle_lib as ol
from test_landscape_spec import SEQ, exact_of, lineage_rows

INSERT, DELETE = landscape.INSERT, landscape.DELETE


@pytest.fixture(scope="module")
def orc(golden):
    iset = files.read_instset(os.path.join(golden, "instset-classic.cfg"))
    env = files.read_environment(os.path.join(golden, "environment-logic9.cfg"))
    cfg = capi.cfg_from_avida(files.read_avida_cfg(None))
    b = ol.Backend("oracle", cfg, iset, env, ncells=1)
    yield b, iset
    b.close()


@pytest.fixture(scope="module")
def insertion(orc):
    b, iset = orc
    return landscape.spec_indel(b.test_genomes, iset.parse_sequence(SEQ), len(iset.names), INSERT)


def _land(golden, name):
    return os.path.join(golden, "landscape", name)


def classes(ls):
    return ls.dead_count, ls.neg_count, ls.neut_count, ls.pos_count


def test_insertion(insertion):
    ls = insertion
    assert (ls.genome_length, ls.num_insts, ls.distance, ls.total_count) == (49, 26, 1, 1300)
    assert classes(ls) == (1279, 6, 2, 13)
    assert (ls.peak_fitness, ls.peak_rank) == (3317.4214876033056, 1062)
    assert divmod(ls.peak_rank, 26) == (40, 22)
    assert ls.gestations == [1300, 1017, 4]
    assert len(ls.site_count) == 50 and sum(ls.site_count) == 2 + 13
    assert (ls.total_entropy, ls.complexity) == (0.0, 0.0)
    assert "%g" % ls.base_fitness == "893.673"


def test_deletion(orc):
    b, iset = orc
    ls = landscape.spec_indel(b.test_genomes, iset.parse_sequence(SEQ), len(iset.names), DELETE)
    assert (ls.genome_length, ls.distance, ls.total_count) == (49, 1, 49)
    assert classes(ls) == (48, 1, 0, 0)
    assert (ls.peak_rank, ls.peak_fitness) == (-1, ls.base_fitness)
    assert ls.gestations == [49, 7, 0]
    assert ls.site_count == [0] * 49
    assert (ls.total_entropy, ls.complexity) == (0.0, 0.0)


def test_lineage_totals(golden, orc):
    """class totals over the 90 lineage genomes (lengths 46-56, two bases of fitness 0)"""
    b, iset = orc
    ins, dele = [0] * 4, [0] * 4
    for row in lineage_rows(golden):
        g = iset.parse_sequence(row[20])
        for kind, acc in ((INSERT, ins), (DELETE, dele)):
            ls = landscape.spec_indel(b.test_genomes, g, len(iset.names), kind)
            assert ls.total_count == ((len(g) + 1) * 26 if kind == INSERT else len(g))
            assert sum(classes(ls)) == ls.total_count
            for k, c in enumerate(classes(ls)):
                acc[k] += c
    assert ins == [43827, 56995, 585, 16919]
    assert dele == [1670, 1152, 35, 1604]


def test_refused_kinds(orc):
    b, iset = orc
    with pytest.raises(ValueError):
        landscape.spec_indel(b.test_genomes, iset.parse_sequence(SEQ), 26, 0)
    with pytest.raises(ValueError):
        landscape.spec_indel(b.test_genomes, b"\0", 26, DELETE)
    with pytest.raises(ValueError):
        landscape.spec_pairs(b.test_genomes, b"\0", 26)


def pairs_exact_of(ls, ep):
    """the fields land-pairs-exact.json holds"""
    d = exact_of(ls)
    del d["site_count"]
    d["chart"] = [[float(x).hex() for x in row] for row in ls.chart]
    for f in landscape.Epistasis.INT_FIELDS:
        d[f] = getattr(ep, f)
    d["epi_gestations"] = ep.gestations
    for f in landscape.Epistasis.SUM_FIELDS:
        d[f] = float(getattr(ep, f)).hex()
    return d


@pytest.mark.slow
def test_all_pairs(golden, orc):
    b, iset = orc
    genome = iset.parse_sequence(SEQ)
    ls, ep = landscape.spec_pairs(b.test_genomes, genome, len(iset.names))
    assert ep.total_epi_count == 735000
    assert (ep.dead_epi_count, ep.neg_epi_count, ep.pos_epi_count, ep.no_epi_count) == (427855, 15316, 139968, 151861)
    assert ep.neg_epi_size == 1355.8577539675525
    assert ep.pos_epi_size == 6182.50258460287
    assert ep.no_epi_size == 21122.127486377052
    assert ep.gestations == [735000, 98545, 983]        # the mutants of the two-step landscape
    # the Landscape half is the one-step landscape but for what Process sets
    one = landscape.spec(b.test_genomes, genome, len(iset.names), 1)
    assert (ls.distance, ls.total_entropy, ls.complexity, ls.site_count) == (0, 0.0, 0.0, [])
    for f in landscape.Landscape.INT_FIELDS + landscape.Landscape.SUM_FIELDS + \
            ("base_fitness", "base_merit", "peak_fitness", "gestations", "chart"):
        if f != "distance":
            assert getattr(ls, f) == getattr(one, f), f
    exp, = landscape.data_tokens(_land(golden, "land-dump.dat"))
    assert landscape.stats_tokens(ls, dump=True, epi=None) == exp
    with open(_land(golden, "land-pairs-exact.json")) as f:
        assert pairs_exact_of(ls, ep) == json.load(f)


def test_epistasis_getters():
    ep = landscape.Epistasis()
    assert math.isnan(ep.prob_epi_dead()) and ep.av_pos_epi_size() == 0.0
    ep.total_epi_count, ep.dead_epi_count, ep.neg_epi_count, ep.pos_epi_count, ep.no_epi_count = 10, 4, 1, 2, 3
    ep.neg_epi_size, ep.pos_epi_size, ep.no_epi_size = 0.5, 3.0, 1.5
    assert (ep.prob_epi_dead(), ep.prob_epi_neg(), ep.prob_epi_pos(), ep.prob_no_epi()) == (0.4, 0.1, 0.2, 0.3)
    assert (ep.av_neg_epi_size(), ep.av_pos_epi_size(), ep.av_no_epi_size()) == (0.5, 1.5, 0.5)


def test_writers(orc, insertion, tmp_path):
    b, iset = orc
    genome = iset.parse_sequence(SEQ)
    ep = landscape.Epistasis()
    ep.total_epi_count, ep.dead_epi_count, ep.neg_epi_count, ep.pos_epi_count, ep.no_epi_count = 8, 1, 2, 4, 1
    ep.neg_epi_size, ep.pos_epi_size, ep.no_epi_size = 0.5, 6.0, 0.75
    plain = landscape.stats_tokens(insertion)
    assert plain[17:] == ["0"] * 8 and plain[7:9] == ["1300", "1"]
    landscape.write_stats(insertion, tmp_path / "land-pairs.dat", epi=ep)
    got, = landscape.data_tokens(tmp_path / "land-pairs.dat")
    assert got[:17] == plain[:17]
    # lethal, synergistic, antagonistic, none; the three sizes in the same order; the count
    assert got[17:] == ["0.125", "0.5", "0.25", "0.125", "1.5", "0.25", "0.75", "8"]
    # a base of fitness 0 under the all-pairs test: nothing counted, 0 / 0 printed as nan
    dead = landscape.Landscape()
    toks = landscape.stats_tokens(dead, dump=True, epi=landscape.Epistasis())
    assert toks[1:5] == ["nan"] * 4 and toks[17:21] == ["nan"] * 4 and toks[21:] == ["0"] * 4
    # PrintSiteCount: the base genome's L sites, entry L of the insertion landscape left out
    landscape.write_site_count(insertion, tmp_path / "site.dat")
    with open(tmp_path / "site.dat") as f:
        assert f.readline() == "# Site Counts\n"
    rows = landscape.data_tokens(tmp_path / "site.dat")
    assert rows == [[str(c) for c in insertion.site_count[:49]]]
    # one uphill step
    peak = landscape.peak_genome(insertion, genome, INSERT)
    assert peak == genome[:40] + bytes([22]) + genome[40:] and len(peak) == 50
    (f, _m, _t), = landscape.colony(b.test_genomes, [peak])
    assert f == insertion.peak_fitness
    base = landscape.Landscape()
    base.peak_rank = -1
    assert landscape.peak_genome(base, genome, DELETE) == bytes(genome)
