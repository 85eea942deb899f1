"""The specification of the genetic distances and the consensus genome
(avida_amd/distance.py): spec_edit (the reference's two-row chart with its
front / end trimming, core/InstructionSequence.cc:547-613) against a textbook
full-matrix Levenshtein and the numpy row form, known answers, the trimming
edge cases, cHistogram's mode / variance / entropy as CalcConsensus uses them,
and the three actions' files through a Driver run on the oracle backend, their
rows recomputed here from world.states."""
import math
import os
import random
import shutil

import numpy as np
import pytest

from avida_amd import capi, datafiles, distance, driver, files
import oracle_lib as ol


def textbook(a, b):
    """Wagner-Fischer, the whole matrix"""
    d = [[0] * (len(a) + 1) for _ in range(len(b) + 1)]
    for j in range(len(a) + 1):
        d[0][j] = j
    for i in range(1, len(b) + 1):
        d[i][0] = i
        for j in range(1, len(a) + 1):
            d[i][j] = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[j - 1] != b[i - 1]))
    return d[len(b)][len(a)]


@pytest.mark.parametrize("alphabet", [2, 3, 26])
def test_edit_all_pairs(alphabet):
    rnd = random.Random(1000 + alphabet)
    genomes = [bytes(rnd.randrange(alphabet) for _ in range(rnd.randint(1, 70))) for _ in range(40)]
    for a in genomes:
        for b in genomes:
            want = textbook(a, b)
            assert distance.spec_edit(a, b) == want == distance.spec_edit_fast(a, b), (a, b)
            ham = distance.spec_hamming(a, b)
            assert ham == abs(len(a) - len(b)) + sum(x != y for x, y in zip(a, b)) and ham >= want


def _ops(word):
    return bytes(ord(c) - ord("a") for c in word)


@pytest.mark.parametrize("a, b, ham, edit", [
    ("kitten", "sitting", 3, 3), ("saturday", "sunday", 7, 3), ("flaw", "lawn", 4, 2),
    ("intention", "execution", 5, 5), ("a", "b", 1, 1), ("ab", "ba", 2, 2), ("abc", "c", 3, 2)])
def test_known_answers(a, b, ham, edit):
    a, b = _ops(a), _ops(b)
    for f in (distance.spec_edit, distance.spec_edit_fast, textbook):
        assert f(a, b) == edit == f(b, a)
    assert distance.spec_hamming(a, b) == ham == distance.spec_hamming(b, a)


def test_trimming_edges():
    g = _ops("thequickbrownfox")
    cases = [(g, g, 0), (g, g[:9], 7), (g, g[5:], 5),           # equal, a prefix, a suffix
             (b"\1" * 3, b"\1" * 5, 2), (b"\1" * 5, b"\1" * 3, 2),   # front and end matches overlap
             (_ops("aaaa"), _ops("bbbbbb"), 6),                 # no common site
             (g, b"", len(g)), (b"", b"", 0)]
    for a, b, want in cases:
        for f in (distance.spec_edit, distance.spec_edit_fast, textbook):
            assert f(a, b) == want == f(b, a), (a, b)


def _hist(rows):
    h = np.zeros((distance.MAX_GENOME_LENGTH, distance.HIST_COLS), dtype=np.int32)
    total = sum(rows[0])
    h[:, 0] = total
    for j, r in enumerate(rows):
        h[j, :len(r)] = r
    return h


def test_consensus_ties_and_ends():
    n_ops = 3                       # bins -1, 0, 1, 2, 3: five of them, the last never filled
    rows = [[0, 1, 5, 0, 0],        # op 1
            [0, 3, 3, 0, 0],        # a tie: the lower bin, op 0
            [1, 2, 0, 3, 0],        # op 2, one organism has ended
            [3, 3, 0, 0, 0],        # -1 beats op 0 on a tie: the consensus genome ends here
            [5, 0, 0, 1, 0],        # ... though organisms go on
            [6, 0, 0, 0, 0]]        # every organism has ended: the loop stops
    con = distance.consensus(_hist(rows), n_ops)
    assert (con.length, con.genome, con.lines) == (3, bytes([1, 0, 2]), 5)
    assert con.mode == [1, 0, 2, -1, -1] and con.count == [5, 3, 3, 3, 5]

    def ent(r):
        e = 0.0
        for x in r:
            p = x / 6.0
            if p != 0.0:
                e -= p * math.log(p)
        return e / math.log(5.0)

    def var(r):
        v = 0.0
        for x in r:
            v += (x - 6.0 / 5.0) * (x - 6.0 / 5.0)
        return v / 4

    assert con.entropy == [ent(r) for r in rows[:5]] and con.variance == [var(r) for r in rows[:5]]
    assert con.total_entropy == ent(rows[0]) + ent(rows[1]) + ent(rows[2])
    assert con.entropy[1] == math.log(2.0) / math.log(5.0)
    # a site where every organism ends at once: the last line is the one before
    con = distance.consensus(_hist([[0, 0, 6, 0, 0], [6, 0, 0, 0, 0]]), n_ops)
    assert (con.length, con.genome, con.lines, con.entropy, con.total_entropy) == (1, bytes([1]), 1, [0.0], 0.0)
    # the bin that stays zero counts in the divisor and the variance: 64 ops, the op-64 bin has no column
    h = np.zeros((distance.MAX_GENOME_LENGTH, distance.HIST_COLS), dtype=np.int32)
    h[:, 0] = 4
    h[0] = 0
    h[0, 64] = 4
    con = distance.consensus(h, 64)
    assert (con.length, con.genome, con.entropy) == (1, bytes([63]), [0.0])
    mean, v = 4.0 / 66.0, 0.0
    for x in [0.0] * 64 + [4.0, 0.0]:
        v += (x - mean) * (x - mean)
    assert con.variance == [v / 65]


def test_site_histogram_spec():
    ops = [bytes([0, 1, 2]), bytes([0, 2]), bytes([1, 1, 1, 1]), bytes([2])]
    hist, living = distance.spec_site_histogram(ops, [3, 2, 4, 1], [True, True, False, True], 3)
    assert living == 3 and (hist.sum(axis=1) == 3).all()
    assert hist[0].tolist()[:4] == [0, 2, 0, 1] and hist[1].tolist()[:4] == [1, 0, 1, 1]
    assert hist[2].tolist()[:4] == [2, 0, 0, 1] and hist[3].tolist()[:4] == [3, 0, 0, 0]


# ---- the writers, through the driver on the oracle backend -------------------

EVENTS = ("u begin InjectAll default-heads.org\n"
          "u 10:20:30 PrintGeneticDistanceData default-heads.org\n"
          "u 10:20:30 PrintPopulationDistanceData default-heads.org\n"
          "u 10:20:30 CalcConsensus 120\n")
FILES = ("genetic_distance.dat", "consensus.dat", "consensus-abundance.dat", "consensus-var.dat",
         "consensus-entropy.dat")


def make_config(golden, path, last):
    path.mkdir()
    with open(os.path.join(golden, "heads_default_100u", "avida.cfg")) as f:
        (path / "avida.cfg").write_text(f.read() + "\nWORLD_X 8\nWORLD_Y 8\n")
    shutil.copy(os.path.join(golden, "instset-heads.cfg"), path / "instset-heads.cfg")
    shutil.copy(os.path.join(golden, "environment-logic9.cfg"), path / "environment.cfg")
    shutil.copy(os.path.join(golden, "default-heads.org"), path / "default-heads.org")
    (path / "events.cfg").write_text(EVENTS + f"u {last} Exit\n")


def rows_of(path):
    return [l.split() for l in open(path) if l.strip() and not l.startswith("#")]


def legend_of(path):
    return [l.split(": ", 1)[1].strip() for l in open(path) if l.startswith("# ") and ": " in l[:7]]


def fmt(values):
    return [datafiles.fmt(v) for v in values]


def check_files(d, out, update, row):
    """row `row` of the static files and pop_distance-<update>.dat against the
    world's states at the end of the run (the driver stopped at `update`)"""
    w, iset, arb = d.world, d.iset, d.arbiter
    n_ops = len(iset.names)
    ref = open_org(d)
    cap = capi.MAX_GENOME
    st, ops, _ = w.states(0, w.ncells, cap)
    genome = {c: ops[c * cap:c * cap + st[c].birth_length] for c in range(w.ncells) if st[c].alive}
    ids = np.asarray(arb.ids)
    order = np.argsort(ids)
    units = np.asarray(arb.units)[order]
    first = np.asarray(arb.table["first_cell"])[order]
    keys = np.asarray(arb.keys)[order]
    assert int(units.sum()) == len(genome) and len(ids) >= 1
    dom = int(np.flatnonzero(keys == np.uint64(arb.best_key))[0])
    gen = [genome[int(c)] for c in first]
    ham = [distance.spec_hamming(ref, g) for g in gen]
    edit = [textbook(ref, g) for g in gen]
    # genetic_distance.dat: sums per genotype over the count of organisms
    count = float(units.sum())
    m1, m2 = sum(ham) / count, sum(h * h for h in ham) / count
    se = (m2 - m1 * m1) / count
    want = [update, m1, math.sqrt(se) if se >= 0 else "-nan", float(ham[dom])]
    assert rows_of(out / "genetic_distance.dat")[row] == fmt(want)
    assert legend_of(out / "genetic_distance.dat") == ["Update", "Average Hamming Distance", "Standard Error",
                                                        "Best Genotype Hamming Distance"]
    # pop_distance-<update>.dat: a row per genotype by id, then the trailer
    got = rows_of(out / f"pop_distance-{update}.dat")
    assert len(got) == len(ids)
    sum_fit = 0.0
    for j, r in enumerate(got):
        g = arb.active[int(keys[j])]
        fit = float(arb.genotype_averages(g)[2])
        sum_fit += fit * int(units[j])
        assert r == fmt([g.name, fit, int(units[j]), ham[j], edit[j], iset.to_sequence(gen[j])])
    text = open(out / f"pop_distance-{update}.dat").read()
    assert text.endswith("# ave fitness from Test CPU's: %s\n\n" % datafiles.fmt(sum_fit / count))
    # consensus.dat and its three per-site files
    hist = np.zeros((distance.MAX_GENOME_LENGTH, distance.HIST_COLS), dtype=np.int64)
    for g in genome.values():
        for j, op in enumerate(g):
            hist[j, 1 + op] += 1
        hist[len(g):, 0] += 1
    con = distance.consensus(hist, n_ops)
    assert con.length > 0
    for j in range(con.length):                       # the mode of every site, by hand
        col = hist[j, :n_ops + 1]
        assert con.genome[j] + 1 == int(np.argmax(col)) and col[con.genome[j] + 1] == col.max()
    cd = [textbook(con.genome, g) for g in gen]
    s1 = sum(float(x) * float(u) for x, u in zip(cd, units))
    s2 = sum((float(x) * float(u)) ** 2 for x, u in zip(cd, units))
    ave, var = s1 / count, ((s2 - s1 * s1 / count) / (count - 1.0) if count > 1 else 0.0)
    (res, _f, _c), = w.test_genomes([con.genome])
    assert res.divided and res.copy_true               # the consensus of this short run is viable at depth 0
    want = [update, float(res.merit), int(res.gestation_time), float(res.fitness), 1.0 / (0.1 + res.gestation_time),
            con.length, int(res.copied_size), int(res.executed_size), 0, 0, 0, 0, -1, -1, 0, cd[dom], ave, var,
            con.total_entropy, float(con.length) - con.total_entropy]
    assert rows_of(out / "consensus.dat")[row] == fmt(want)
    assert len(legend_of(out / "consensus.dat")) == 20
    lines = min(120, con.lines)
    assert rows_of(out / "consensus-abundance.dat")[row] == fmt(con.count[:lines])
    assert rows_of(out / "consensus-var.dat")[row] == fmt(con.variance[:lines])
    assert rows_of(out / "consensus-entropy.dat")[row] == fmt(con.entropy[:lines])
    assert open(out / "consensus-var.dat").read().startswith("\n")      # an anonymous file: no legend


def open_org(d):
    return files.read_org(os.path.join(d.config_dir, "default-heads.org"), d.iset)


def run_driver(golden, tmp_path, last, **kw):
    cfgdir, out = tmp_path / f"config{last}", tmp_path / f"data{last}"
    make_config(golden, cfgdir, last)
    d = driver.Driver(str(cfgdir), str(out), **kw)
    assert d.run() == last
    return d, out


def test_driver_writes_the_three_files_on_the_oracle(golden, tmp_path):
    mk = lambda cfg, iset, env: ol.Backend("oracle", cfg, iset, env)     # noqa: E731
    d30, out30 = run_driver(golden, tmp_path, 30, make_world=mk)
    assert not distance.on_device(d30.world)
    for name in FILES:
        assert len(rows_of(out30 / name)) == 2, name
    check_files(d30, out30, 30, 1)
    assert len(np.asarray(d30.arbiter.ids)) > 1          # mutants: more than the ancestor's genotype
    d30.world.close()
    # the rows of update 10 are those of a run that stops there
    d10, out10 = run_driver(golden, tmp_path, 10, make_world=mk)
    check_files(d10, out10, 10, 0)
    d10.world.close()
    for name in FILES:
        assert rows_of(out10 / name)[0] == rows_of(out30 / name)[0], name
    assert open(out10 / "pop_distance-10.dat").read() == open(out30 / "pop_distance-10.dat").read()
