"""Pin the landscape specification (avida_amd.landscape.spec over the CPU
oracle) to the reference's own golden landscape outputs, tests/golden/landscape/:

* land-1step.dat, land-2step.dat: analyze-mode FullLandscape of one 49-site
  genome at distance 1 and 2 (avida-core/tests/analyze_fulllandscape_{1,2}step);
* land-dump.dat, org-Seq1.land: DumpLandscape of the same genome
  (tests/analyze_dumplandscape);
* detail.dat: the five landscape columns PrecalcLandscape gives the 90
  genotypes of a lineage (tests/analyze_truncate_lineage_fulllandscape);
* land-2step-exact.json: the two-step landscape's integer fields and its sums
  as hex floats, written once by the specification over the oracle.

Every sequence is in the order of instset-classic.cfg.
"""
import json
import os

import pytest

from avida_amd import capi, files, landscape
import oracle_lib as ol

SEQ = "sirzaqcppqqbadpncqblcoqvcecpqcgptcbpfcoqutttycsva"


@pytest.fixture(scope="module")
def orc(golden):
    iset = files.read_instset(os.path.join(golden, "instset-classic.cfg"))
    env = files.read_environment(os.path.join(golden, "environment-logic9.cfg"))
    cfg = capi.cfg_from_avida(files.read_avida_cfg(None))
    b = ol.Backend("oracle", cfg, iset, env, ncells=1)
    yield b, iset
    b.close()


@pytest.fixture(scope="module")
def one_step(orc):
    b, iset = orc
    return landscape.spec(b.test_genomes, iset.parse_sequence(SEQ), len(iset.names), 1)


def _land(golden, name):
    return os.path.join(golden, "landscape", name)


def test_one_step_stats_line(golden, one_step, tmp_path):
    ls = one_step
    assert (ls.genome_length, ls.num_insts, ls.total_count) == (49, 26, 1225)
    assert ("%g" % ls.base_fitness, ls.base_merit, ls.base_gestation) == ("893.673", 98304.0, 110)
    assert ls.gestations == [1225, 115, 1]
    exp, = landscape.data_tokens(_land(golden, "land-1step.dat"))
    assert landscape.stats_tokens(ls) == exp
    landscape.write_stats(ls, tmp_path / "land.dat")
    assert landscape.data_tokens(tmp_path / "land.dat") == [exp]


def test_dump(golden, orc, one_step, tmp_path):
    _, iset = orc
    exp, = landscape.data_tokens(_land(golden, "land-dump.dat"))
    assert landscape.stats_tokens(one_step, dump=True) == exp
    rows = landscape.data_tokens(_land(golden, "org-Seq1.land"))
    assert len(rows) == 49 and all(len(r) == 27 for r in rows)
    assert landscape.dump_rows(one_step, iset.parse_sequence(SEQ)) == rows
    landscape.write_dump(one_step, iset.parse_sequence(SEQ), tmp_path / "org.land")
    assert landscape.data_tokens(tmp_path / "org.land") == rows


def lineage_rows(golden):
    rows = landscape.data_tokens(_land(golden, "detail.dat"))
    assert len(rows) == 90
    return rows


def test_lineage_columns(golden, orc):
    """columns 16-20 of all 90 rows (column 5 is the population file's value)"""
    b, iset = orc
    zero_base = 0
    for row in lineage_rows(golden):
        ls = landscape.spec(b.test_genomes, iset.parse_sequence(row[20]), len(iset.names), 1)
        assert ls.genome_length == int(row[2])
        assert landscape.lineage_columns(ls) == row[15:20], row[0]
        if ls.base_fitness == 0:
            # f > 0 is beneficial against a dead base; nothing is deleterious or neutral
            zero_base += 1
            assert ls.neg_count == 0 and ls.neut_count == 0
            assert ls.pos_count == ls.total_count - ls.dead_count and ls.pos_count > 0
            assert ls.peak_rank >= 0
    assert zero_base == 2          # genotypes 356505 and 388509


# the recursion cases of the two-step landscape, counted on the oracle
CASES_2STEP = {0: {"runs": 735000, "no_divide": 331985, "copy_true": 304470, "ancestor": 0},
               1: {"runs": 98545, "no_divide": 97479, "copy_true": 82, "ancestor": 1},
               2: {"runs": 983, "no_divide": 249, "copy_true": 29, "ancestor": 507},
               "exhausted": 198}


def exact_of(ls):
    """the fields land-2step-exact.json holds"""
    d = {f: getattr(ls, f) for f in ("total_count", "dead_count", "neg_count", "neut_count", "pos_count",
                                     "peak_rank", "base_gestation", "gestations", "site_count")}
    for f in ("base_fitness", "base_merit", "peak_fitness") + landscape.Landscape.SUM_FIELDS:
        d[f] = float(getattr(ls, f)).hex()
    return d


@pytest.mark.slow
def test_two_step(golden, orc):
    b, iset = orc
    ls = landscape.spec(b.test_genomes, iset.parse_sequence(SEQ), len(iset.names), 2)
    exp, = landscape.data_tokens(_land(golden, "land-2step.dat"))
    assert landscape.stats_tokens(ls) == exp
    assert ls.cases == CASES_2STEP
    with open(_land(golden, "land-2step-exact.json")) as f:
        assert exact_of(ls) == json.load(f)
