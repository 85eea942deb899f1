"""Mutational landscapes (main/cLandscape.cc:97-213 of the reference).

Every one-step (or two-step) substitution mutant of a genome is run through
the test CPU, classified against the base genome's colony fitness and summed
up.  Two routes give the same numbers:

* ``spec``: the specification in plain Python over any ``test_genomes``
  callable (the tests' oracle Backend, or the product's avgpu_test_genomes
  wrapped the same way): the viability recursion, the rank order, the
  classification, ``gestations``, ``site_count`` and the chart.  It is what
  the device is tested against and the path for worlds without the call.
* ``full``: avgpu_landscapes -- mutants made, run, judged and reduced on the
  device, nothing but the accumulators copied back.

Rank order.  Distance 1: rank = site * (I - 1) + j, j counting the op codes
in ascending order with the original skipped (I = instruction set size).
Distance 2: the reference's recursion order -- first site ascending, its op
ascending, second site (> first) ascending, its op ascending.

The writers print the reference's files: ``write_stats`` the 25-column
land-*.dat line (cLandscape::PrintStats, :952-980), ``write_dump`` org-*.land
(ProcessDump, :217-261), ``lineage_columns`` the five landscape columns of an
analyze-mode DETAIL file (frac_pos frac_neg frac_neut frac_dead land_fitness).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import capi

GENERATION_TESTS = 3      # cCPUTestInfo's generation_tests: recursion depths 0..2
SPEC_BATCH = 65536        # genomes per test_genomes call of the specification


class Landscape:
    """cLandscape's accumulators for one base genome (avgpu_landscape's
    fields), its per-site counts and, at distance 1, the fitness chart."""

    INT_FIELDS = ("total_count", "dead_count", "neg_count", "neut_count", "pos_count", "peak_rank",
                  "base_gestation", "distance", "genome_length", "num_insts")
    SUM_FIELDS = ("total_fitness", "total_sqr_fitness", "pos_size", "neg_size")

    def __init__(self):
        for f in self.INT_FIELDS:
            setattr(self, f, 0)
        for f in self.SUM_FIELDS + ("base_fitness", "base_merit", "peak_fitness", "total_entropy", "complexity"):
            setattr(self, f, 0.0)
        self.gestations = [0, 0, 0]
        self.site_count = []
        self.chart = None          # [site][op] at distance 1
        self.cases = None          # the specification's recursion-case counts

    # cLandscape.h:134-143
    def prob(self, name):
        return getattr(self, name + "_count") / self.total_count

    def av_pos_size(self):
        return self.pos_size / self.pos_count if self.pos_count else 0.0

    def av_neg_size(self):
        return self.neg_size / self.neg_count if self.neg_count else 0.0

    def ave_fitness(self):
        return self.total_fitness / self.total_count

    def ave_sqr_fitness(self):
        return self.total_sqr_fitness / self.total_count


def entropy(site_count, num_insts):
    """(total_entropy, complexity) of cLandscape::Process (:158-169): a site's
    entropy is the log of its legal states, the unmutated one included"""
    max_ent = math.log(float(num_insts))
    total = 0.0
    for c in site_count:
        total += math.log(float(c) + 1) / max_ent
    return total, len(site_count) - total


def num_mutants(length, num_insts, distance):
    k = num_insts - 1
    return length * k if distance == 1 else length * (length - 1) // 2 * k * k


def mutants(genome, num_insts, distance):
    """(mutant genome, site the reference counts it under) in rank order"""
    g = bytearray(genome)
    L = len(g)
    if distance == 1:
        for s in range(L):
            o = g[s]
            for k in range(num_insts):
                if k != o:
                    g[s] = k
                    yield bytes(g), s
            g[s] = o
    else:
        for s1 in range(L - 1):
            o1 = g[s1]
            for k1 in range(num_insts):
                if k1 == o1:
                    continue
                g[s1] = k1
                for s2 in range(s1 + 1, L):
                    o2 = g[s2]
                    for k2 in range(num_insts):
                        if k2 != o2:
                            g[s2] = k2
                            yield bytes(g), s2       # Process_Body:204 counts the innermost site
                    g[s2] = o2
            g[s1] = o1


def colony(test_genomes, genomes, gestations=None, cases=None):
    """cTestCPU::TestGenome_Body (cpu/cTestCPU.cc:233-326) over a batch:
    per genome (colony fitness, colony organism's merit, its gestation time).
    At depth d an organism that does not divide has fitness 0; one whose
    offspring equals the genome it ran, or a genome of a depth below, gives
    its own fitness; any other offspring is run at depth d + 1; past the last
    depth the fitness is 0."""
    out = [(0.0, 0.0, 0)] * len(genomes)
    pending = [(i, [bytes(g)]) for i, g in enumerate(genomes)]
    for depth in range(GENERATION_TESTS):
        if not pending:
            break
        if gestations is not None:
            gestations[depth] += len(pending)
        res = test_genomes([chain[-1] for _, chain in pending])
        nxt = []
        for (i, chain), (r, _flags, child) in zip(pending, res):
            if cases is not None:
                cases[depth]["runs"] += 1
            if not r.divided:
                if cases is not None:
                    cases[depth]["no_divide"] += 1
                continue
            child = bytes(child)
            if child == chain[-1] or child in chain[:-1]:
                if cases is not None:
                    cases[depth]["copy_true" if child == chain[-1] else "ancestor"] += 1
                out[i] = (float(r.fitness), float(r.merit), int(r.gestation_time))
                continue
            nxt.append((i, chain + [child]))
        pending = nxt
    if cases is not None:
        cases["exhausted"] += len(pending)
    return out


def spec(test_genomes, genome, num_insts, distance):
    """The landscape of `genome` (op codes) by the specification."""
    if distance not in (1, 2):
        raise ValueError("distance must be 1 or 2")
    genome = bytes(genome)
    L = len(genome)
    ls = Landscape()
    ls.distance, ls.genome_length, ls.num_insts = distance, L, num_insts
    ls.cases = {d: {"runs": 0, "no_divide": 0, "copy_true": 0, "ancestor": 0} for d in range(GENERATION_TESTS)}
    ls.cases["exhausted"] = 0
    # ProcessBase (:125-142); FITNESS_NEUTRAL_RANGE 0: neut_min = neut_max = base
    (ls.base_fitness, ls.base_merit, ls.base_gestation), = colony(test_genomes, [genome])
    base = ls.base_fitness
    ls.peak_fitness, ls.peak_rank = base, -1
    ls.site_count = [0] * L
    if distance == 1:
        ls.chart = [[base] * num_insts for _ in range(L)]
    fits, pos, neg = [], [], []

    def run(batch, rank0):
        res = colony(test_genomes, [g for g, _ in batch], ls.gestations, ls.cases)
        for k, ((g, site), (f, _m, _t)) in enumerate(zip(batch, res)):
            rank = rank0 + k
            fits.append(f)
            ls.total_count += 1
            if f == 0:                      # ProcessGenome (:97-123)
                ls.dead_count += 1
            elif f < base:
                ls.neg_count += 1
                neg.append(f)
            elif f <= base:
                ls.neut_count += 1
            else:
                ls.pos_count += 1
                pos.append(f)
                if f > ls.peak_fitness:
                    ls.peak_fitness, ls.peak_rank = f, rank
            if f >= base:
                ls.site_count[site] += 1
            if distance == 1:
                ls.chart[site][g[site]] = f

    batch, rank0 = [], 0
    for item in mutants(genome, num_insts, distance):
        batch.append(item)
        if len(batch) == SPEC_BATCH:
            run(batch, rank0)
            rank0 += len(batch)
            batch = []
    if batch:
        run(batch, rank0)
    ls.total_fitness = math.fsum(fits)
    ls.total_sqr_fitness = math.fsum(f * f for f in fits)
    ls.pos_size = math.fsum(pos)
    ls.neg_size = math.fsum(neg)
    ls.total_entropy, ls.complexity = entropy(ls.site_count, num_insts)
    return ls


# ---- the device route -------------------------------------------------------

def call(world, genomes, distance, chart=None):
    """avgpu_landscapes as it returns: (rows, site_count, chart) -- numpy
    arrays of capi.LANDSCAPE_DTYPE rows, the per-site counts of all genomes
    back to back and (or None) the charts back to back, [site][op] each.
    `world` is a product world (an object with .lib and .h).  chart: None =
    at distance 1 only."""
    lib, h = world.lib, world.h
    n = len(genomes)
    want_chart = (distance == 1) if chart is None else bool(chart)
    blob = b"".join(bytes(g) for g in genomes)
    buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(blob or b"\0")
    lens = np.array([len(g) for g in genomes], dtype=np.int32)
    out = np.zeros(max(1, n), dtype=capi.LANDSCAPE_DTYPE)
    total = int(lens.sum())
    sc = np.zeros(max(1, total), dtype=np.int32)
    ch = None
    if want_chart:
        # the chart's stride is the instruction set's size, which comes back
        # in the rows: room for the largest set
        ch = np.zeros(max(1, total * capi.MAX_INST), dtype=np.float64)
    rc = lib.avgpu_landscapes(h, n, buf, lens.ctypes.data_as(C.POINTER(C.c_int32)), distance,
                              out.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.POINTER(C.c_int32)),
                              ch.ctypes.data_as(C.POINTER(C.c_double)) if ch is not None else None)
    if rc < 0:
        raise RuntimeError(f"avgpu_landscapes: {lib.avgpu_last_error().decode()}")
    if ch is not None:
        ch = ch[:total * int(out[0]["num_insts"])]
    return out[:n], sc[:total], ch


def full(world, genomes, distance, chart=None):
    """Landscapes of `genomes` (op-code byte strings) on the device: a list
    of Landscape"""
    out, sc, ch = call(world, genomes, distance, chart)
    res, off = [], 0
    for i, g in enumerate(genomes):
        ni, ln = int(out[i]["num_insts"]), len(g)
        res.append(from_row(out[i], sc[off:off + ln], None if ch is None else ch[off * ni:(off + ln) * ni]))
        off += ln
    return res


def set_chunk(world, cells):
    """avgpu_set_landscape_chunk: cells of the scratch test world"""
    if world.lib.avgpu_set_landscape_chunk(world.h, cells) < 0:
        raise ValueError(world.lib.avgpu_last_error().decode())


def last_timing(world):
    """(device ms, mutants, test-CPU runs) of the last avgpu_landscapes"""
    ms, m, r = C.c_double(), C.c_int64(), C.c_int64()
    world.lib.avgpu_last_landscape_ms(world.h, C.byref(ms), C.byref(m), C.byref(r))
    return ms.value, m.value, r.value


def from_row(row, site_count, chart=None):
    """Landscape of one avgpu_landscape row (capi.LANDSCAPE_DTYPE)"""
    ls = Landscape()
    for f in Landscape.INT_FIELDS:
        setattr(ls, f, int(row[f]))
    for f in Landscape.SUM_FIELDS + ("base_fitness", "base_merit", "peak_fitness", "total_entropy", "complexity"):
        setattr(ls, f, float(row[f]))
    ls.gestations = [int(x) for x in row["gestations"]]
    ls.site_count = [int(x) for x in site_count]
    if chart is not None:
        ls.chart = np.asarray(chart, dtype=np.float64).reshape(ls.genome_length, ls.num_insts).tolist()
    return ls


# ---- the reference's files --------------------------------------------------

STATS_COLUMNS = [
    "Update", "Probability Lethal", "Probability Deleterious", "Probability Neutral",
    "Probability Beneficial", "Average Beneficial Size", "Average Deleterious Size", "Total Mutants",
    "Distance", "Base Fitness", "Base Merit", "Base Gestation", "Peak Fitness", "Average Fitness",
    "Average Square Fitness", "Total Entropy", "Total Complexity", "Probability Lethal Epistasis",
    "Probability Synergistic Epistasis", "Probability Antagonistic Epistasis", "Probability No Epistasis",
    "Average Synergistic Epistasis Size", "Average Antagonistic Epistasis Size",
    "Average Size - No Epistasis", "Total Epistasis Count"]


def _g(x):
    # Avida::Output::File prints doubles at the default ostream precision
    return "%g" % x if isinstance(x, float) else str(x)


def stats_tokens(ls, dump=False):
    """The 25 columns of cLandscape::PrintStats; update -1, no epistasis
    (TestPairs is not on this path).  dump: the line DumpLandscape prints
    (ProcessDump sets neither the distance nor the entropy: all 0)."""
    v = [-1, ls.prob("dead"), ls.prob("neg"), ls.prob("neut"), ls.prob("pos"), ls.av_pos_size(),
         ls.av_neg_size(), ls.total_count, 0 if dump else ls.distance, ls.base_fitness, ls.base_merit,
         ls.base_gestation, ls.peak_fitness, ls.ave_fitness(), ls.ave_sqr_fitness(),
         0 if dump else ls.total_entropy, 0 if dump else ls.complexity, 0, 0, 0, 0, 0, 0, 0, 0]
    return [_g(x) for x in v]


def _legend(f, names):
    for i, name in enumerate(names):
        f.write("# %2d: %s\n" % (i + 1, name))
    f.write("\n")


def write_stats(ls, path, dump=False):
    """land-*.dat: the legend and one PrintStats line"""
    with open(path, "w") as f:
        _legend(f, STATS_COLUMNS)
        f.write(" ".join(stats_tokens(ls, dump)) + " \n")


def dump_rows(ls, genome):
    """org-*.land rows: the original op code, then the fitness of every op at
    the site (the original's entry is the base fitness)"""
    return [[_g(int(genome[s]))] + [_g(float(x)) for x in ls.chart[s]] for s in range(ls.genome_length)]


def write_dump(ls, genome, path):
    with open(path, "w") as f:
        f.write("# Detailed dump of the per-site, per-instruction fitness\n")
        f.write("# values for the entire single-step landscape.\n")
        _legend(f, ["Original Instruction"] +
                ["Mutation Fitness (instruction = column_number - 2)"] * ls.num_insts)
        for row in dump_rows(ls, genome):
            f.write(" ".join(row) + " \n")


def lineage_columns(ls):
    """frac_pos frac_neg frac_neut frac_dead land_fitness of an analyze-mode
    DETAIL line (cAnalyzeGenotype's landscape statistics, PrecalcLandscape)"""
    return [_g(ls.prob("pos")), _g(ls.prob("neg")), _g(ls.prob("neut")), _g(ls.prob("dead")),
            _g(ls.ave_fitness())]


def data_tokens(path):
    """token lists of a reference data file's lines, '#' and blank lines skipped"""
    with open(path) as f:
        return [l.split() for l in f if l.strip() and not l.startswith("#")]
