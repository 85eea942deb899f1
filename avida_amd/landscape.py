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

The same two routes exist for the insertion and deletion landscapes
(cLandscape::ProcessInsert / ProcessDelete, :265-330): ``spec_indel`` and
``full_indel`` (avgpu_landscapes_indel); insertion rank = line * I + op with
line 0..L, deletion rank = line -- and for the all-pairs epistasis test
(TestAllPairs / TestMutPair, :788-825, :909-949): ``spec_pairs`` and
``full_pairs`` (avgpu_landscape_pairs), which return a Landscape (the
one-step pass of BuildFitnessChart) and an ``Epistasis``.

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
    ls = _based(test_genomes, genome, num_insts, distance)
    base = ls.base_fitness
    ls.site_count = [0] * L
    if distance == 1:
        ls.chart = [[base] * num_insts for _ in range(L)]
    _process(test_genomes, ls, mutants(genome, num_insts, distance), chart=distance == 1)
    ls.total_entropy, ls.complexity = entropy(ls.site_count, num_insts)
    return ls


def _process(test_genomes, ls, items, chart=False):
    """cLandscape::ProcessGenome (:97-123) over `items` -- (mutant genome,
    site it is counted under) in rank order -- into ls, whose base is set"""
    base = ls.base_fitness
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
            if chart:
                ls.chart[site][g[site]] = f

    batch, rank0 = [], 0
    for item in items:
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
    return fits


def _based(test_genomes, genome, num_insts, distance):
    """a Landscape after Reset and ProcessBase (:49-95, :125-142);
    FITNESS_NEUTRAL_RANGE 0: neut_min = neut_max = base"""
    ls = Landscape()
    ls.distance, ls.genome_length, ls.num_insts = distance, len(genome), num_insts
    ls.cases = {d: {"runs": 0, "no_divide": 0, "copy_true": 0, "ancestor": 0} for d in range(GENERATION_TESTS)}
    ls.cases["exhausted"] = 0
    (ls.base_fitness, ls.base_merit, ls.base_gestation), = colony(test_genomes, [genome])
    ls.peak_fitness, ls.peak_rank = ls.base_fitness, -1
    return ls


INSERT, DELETE = capi.LAND_INSERT, capi.LAND_DELETE


def indel_mutants(genome, num_insts, kind):
    """(mutant genome, line it is counted under) in rank order: insertions
    line * num_insts + op over lines 0..L (ProcessInsert, :318-327), no op
    skipped; deletions by line (ProcessDelete, :285-292)"""
    g = bytes(genome)
    if kind == INSERT:
        for line in range(len(g) + 1):
            for op in range(num_insts):
                yield g[:line] + bytes([op]) + g[line:], line
    elif kind == DELETE:
        for line in range(len(g)):
            yield g[:line] + g[line + 1:], line
    else:
        raise ValueError("kind must be INSERT (1) or DELETE (2)")


def spec_indel(test_genomes, genome, num_insts, kind):
    """The insertion or deletion landscape of `genome` by the specification
    (cLandscape::ProcessInsert / ProcessDelete).  distance 1 (the actions'
    m_dist, which PrintStats prints), no entropy; site_count has L + 1 entries
    for insertions (Reset allocates size + 1), L for deletions."""
    genome = bytes(genome)
    if kind not in (INSERT, DELETE):
        raise ValueError("kind must be INSERT (1) or DELETE (2)")
    if kind == DELETE and len(genome) < 2:
        raise ValueError("a one-site genome has no deletion mutants")
    ls = _based(test_genomes, genome, num_insts, 1)
    ls.site_count = [0] * (len(genome) + (1 if kind == INSERT else 0))
    _process(test_genomes, ls, indel_mutants(genome, num_insts, kind))
    return ls


class Epistasis:
    """cLandscape::TestAllPairs' accumulators (avgpu_epistasis's fields) and
    the getters of main/cLandscape.h:144-162"""

    INT_FIELDS = ("total_epi_count", "dead_epi_count", "neg_epi_count", "pos_epi_count", "no_epi_count")
    SUM_FIELDS = ("neg_epi_size", "pos_epi_size", "no_epi_size")

    def __init__(self):
        for f in self.INT_FIELDS:
            setattr(self, f, 0)
        for f in self.SUM_FIELDS:
            setattr(self, f, 0.0)
        self.gestations = [0, 0, 0]
        self.cases = None

    def _prob(self, count):
        # 0 / 0 where TestAllPairs stopped at a base of fitness 0
        return count / self.total_epi_count if self.total_epi_count else math.nan

    def prob_epi_dead(self):
        return self._prob(self.dead_epi_count)

    def prob_epi_pos(self):
        return self._prob(self.pos_epi_count)

    def prob_epi_neg(self):
        return self._prob(self.neg_epi_count)

    def prob_no_epi(self):
        return self._prob(self.no_epi_count)

    def av_pos_epi_size(self):
        return self.pos_epi_size / self.pos_epi_count if self.pos_epi_count else 0.0

    def av_neg_epi_size(self):
        return self.neg_epi_size / self.neg_epi_count if self.neg_epi_count else 0.0

    def av_no_epi_size(self):
        return self.no_epi_size / self.no_epi_count if self.no_epi_count else 0.0


def spec_pairs(test_genomes, genome, num_insts):
    """cLandscape::TestAllPairs (:788-825) by the specification: (Landscape,
    Epistasis).  The Landscape is BuildFitnessChart's one-step pass (distance
    0, no entropy, site_count untouched); the pair mutants are classified by
    TestMutPair (:909-949) and enter the Epistasis only."""
    genome = bytes(genome)
    L = len(genome)
    if L < 2:
        raise ValueError("a one-site genome has no pairs of sites")
    ls = _based(test_genomes, genome, num_insts, 0)
    ls.site_count = [0] * L
    ep = Epistasis()
    base = ls.base_fitness
    ls.chart = [[base] * num_insts for _ in range(L)]
    if base == 0:                                # TestAllPairs :793
        ls.site_count = []
        return ls, ep
    _process(test_genomes, ls, mutants(genome, num_insts, 1), chart=True)
    ls.site_count = []                           # BuildFitnessChart counts no sites
    ep.cases = {d: {"runs": 0, "no_divide": 0, "copy_true": 0, "ancestor": 0} for d in range(GENERATION_TESTS)}
    ep.cases["exhausted"] = 0
    sizes = {"neg": [], "pos": [], "no": []}

    def run(batch):
        res = colony(test_genomes, [g for g, _ in batch], ep.gestations, ep.cases)
        for (g, (s1, s2)), (f12, _m, _t) in zip(batch, res):
            combo = f12 / base
            m1 = ls.chart[s1][g[s1]] / base
            m2 = ls.chart[s2][g[s2]] / base
            mult = m1 * m2
            ep.total_epi_count += 1
            if (m1 == 0 or m2 == 0) and combo == 0:
                ep.dead_epi_count += 1
            elif combo < mult:
                ep.neg_epi_count += 1
                sizes["neg"].append(combo)
            elif combo > mult:
                ep.pos_epi_count += 1
                sizes["pos"].append(combo)
            else:
                ep.no_epi_count += 1
                sizes["no"].append(combo)

    batch = []
    for item in pair_mutants(genome, num_insts):
        batch.append(item)
        if len(batch) == SPEC_BATCH:
            run(batch)
            batch = []
    if batch:
        run(batch)
    ep.neg_epi_size = math.fsum(sizes["neg"])
    ep.pos_epi_size = math.fsum(sizes["pos"])
    ep.no_epi_size = math.fsum(sizes["no"])
    return ls, ep


def pair_mutants(genome, num_insts):
    """(mutant genome, (s1, s2)) in TestAllPairs' loop order (:807-822):
    s1, s2 > s1, op at s1, op at s2, each ascending, the base's ops skipped"""
    g = bytearray(genome)
    L = len(g)
    for s1 in range(L - 1):
        o1 = g[s1]
        for s2 in range(s1 + 1, L):
            o2 = g[s2]
            for k1 in range(num_insts):
                if k1 == o1:
                    continue
                g[s1] = k1
                for k2 in range(num_insts):
                    if k2 != o2:
                        g[s2] = k2
                        yield bytes(g), (s1, s2)
            g[s1], g[s2] = o1, o2


def peak_genome(ls, genome, kind=0):
    """The genome at ls.peak_rank (the base at -1) of a distance-1
    substitution landscape (kind 0), an insertion or a deletion landscape:
    one uphill step for a host that walks with these calls."""
    g = bytes(genome)
    r, ni = ls.peak_rank, ls.num_insts
    if r < 0:
        return g
    if kind == INSERT:
        line, op = divmod(r, ni)
        return g[:line] + bytes([op]) + g[line:]
    if kind == DELETE:
        return g[:r] + g[r + 1:]
    if kind != 0 or ls.distance not in (0, 1):
        raise ValueError("peak_genome: distance-1 substitution, insertion and deletion ranks only")
    site, j = divmod(r, ni - 1)
    op = j + (1 if j >= g[site] else 0)
    return g[:site] + bytes([op]) + g[site + 1:]


# ---- the device route -------------------------------------------------------

def _call(world, name, *args):
    return capi.call(world.lib, "avgpu_", name, world.h, *args)


def call(world, genomes, distance, chart=None):
    """avgpu_landscapes as it returns: (rows, site_count, chart) -- numpy
    arrays of capi.LANDSCAPE_DTYPE rows, the per-site counts of all genomes
    back to back and (or None) the charts back to back, [site][op] each.
    `world` is a product world (an object with .lib and .h).  chart: None =
    at distance 1 only."""
    n = len(genomes)
    want_chart = (distance == 1) if chart is None else bool(chart)
    buf, lens = capi.pack_genomes(genomes)
    out = np.zeros(max(1, n), dtype=capi.LANDSCAPE_DTYPE)
    total = sum(lens)
    sc = np.zeros(max(1, total), dtype=np.int32)
    ch = None
    if want_chart:
        # the chart's stride is the instruction set's size, which comes back
        # in the rows: room for the largest set
        ch = np.zeros(max(1, total * capi.MAX_INST), dtype=np.float64)
    _call(world, "landscapes", n, buf, lens, distance, out.ctypes.data_as(C.c_void_p),
          sc.ctypes.data_as(C.POINTER(C.c_int32)), ch.ctypes.data_as(C.POINTER(C.c_double)) if ch is not None else None)
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


def call_indel(world, genomes, kind):
    """avgpu_landscapes_indel as it returns: (rows, site_count) -- the counts
    of all genomes back to back, len + 1 each for insertions, len for deletions"""
    n = len(genomes)
    buf, lens = capi.pack_genomes(genomes)
    out = np.zeros(max(1, n), dtype=capi.LANDSCAPE_DTYPE)
    total = sum(lens) + (n if kind == INSERT else 0)
    sc = np.zeros(max(1, total), dtype=np.int32)
    _call(world, "landscapes_indel", n, buf, lens, kind, out.ctypes.data_as(C.c_void_p),
          sc.ctypes.data_as(C.POINTER(C.c_int32)))
    return out[:n], sc[:total]


def full_indel(world, genomes, kind):
    """Insertion (INSERT) or deletion (DELETE) landscapes of `genomes` on the
    device: a list of Landscape"""
    out, sc = call_indel(world, genomes, kind)
    res, off = [], 0
    for i, g in enumerate(genomes):
        ln = len(g) + (1 if kind == INSERT else 0)
        res.append(from_row(out[i], sc[off:off + ln]))
        off += ln
    return res


def call_pairs(world, genomes, chart=True):
    """avgpu_landscape_pairs as it returns: (rows, epistasis rows, chart) --
    capi.LANDSCAPE_DTYPE, capi.EPISTASIS_DTYPE and (or None) the one-step
    charts back to back, [site][op] each"""
    n = len(genomes)
    buf, lens = capi.pack_genomes(genomes)
    out = np.zeros(max(1, n), dtype=capi.LANDSCAPE_DTYPE)
    epi = np.zeros(max(1, n), dtype=capi.EPISTASIS_DTYPE)
    total = sum(lens)
    ch = np.zeros(max(1, total * capi.MAX_INST), dtype=np.float64) if chart else None
    _call(world, "landscape_pairs", n, buf, lens, out.ctypes.data_as(C.c_void_p), epi.ctypes.data_as(C.c_void_p),
          ch.ctypes.data_as(C.POINTER(C.c_double)) if ch is not None else None)
    if ch is not None:
        ch = ch[:total * int(out[0]["num_insts"])]
    return out[:n], epi[:n], ch


def epistasis_from_row(row):
    """Epistasis of one avgpu_epistasis row (capi.EPISTASIS_DTYPE)"""
    ep = Epistasis()
    for f in Epistasis.INT_FIELDS:
        setattr(ep, f, int(row[f]))
    for f in Epistasis.SUM_FIELDS:
        setattr(ep, f, float(row[f]))
    ep.gestations = [int(x) for x in row["gestations"]]
    return ep


def full_pairs(world, genomes, chart=True):
    """The all-pairs epistasis test of `genomes` on the device: a list of
    (Landscape, Epistasis)"""
    out, epi, ch = call_pairs(world, genomes, chart)
    res, off = [], 0
    for i, g in enumerate(genomes):
        ni, ln = int(out[i]["num_insts"]), len(g)
        ls = from_row(out[i], [], None if ch is None else ch[off * ni:(off + ln) * ni])
        res.append((ls, epistasis_from_row(epi[i])))
        off += ln
    return res


def set_chunk(world, cells):
    """avgpu_set_landscape_chunk: cells of the scratch test world"""
    try:
        _call(world, "set_landscape_chunk", cells)
    except RuntimeError as e:
        raise ValueError(str(e)) from None


def last_timing(world):
    """(device ms, mutants, test-CPU runs) of the last avgpu_landscapes,
    avgpu_landscapes_indel or avgpu_landscape_pairs (the latter: the one-step
    and the pair mutants together)"""
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


def stats_tokens(ls, dump=False, epi=None):
    """The 25 columns of cLandscape::PrintStats; update -1.  dump: the line
    DumpLandscape prints (ProcessDump sets neither the distance nor the
    entropy: all 0).  epi: an Epistasis for columns 18-25 (PairTestLandscape);
    without it they are the zeros every other command prints.  Where the
    all-pairs test stopped at a base of fitness 0 nothing was counted and the
    reference divides 0 by 0: those columns print nan (no file pins them)."""
    def over_total(x):
        return x / ls.total_count if ls.total_count else math.nan

    v = [-1, over_total(ls.dead_count), over_total(ls.neg_count), over_total(ls.neut_count),
         over_total(ls.pos_count), ls.av_pos_size(), ls.av_neg_size(), ls.total_count,
         0 if dump else ls.distance, ls.base_fitness, ls.base_merit,
         ls.base_gestation, ls.peak_fitness, over_total(ls.total_fitness), over_total(ls.total_sqr_fitness),
         0 if dump else ls.total_entropy, 0 if dump else ls.complexity]
    if epi is None:
        v += [0, 0, 0, 0, 0, 0, 0, 0]
    else:
        v += [epi.prob_epi_dead(), epi.prob_epi_pos(), epi.prob_epi_neg(), epi.prob_no_epi(),
              epi.av_pos_epi_size(), epi.av_neg_epi_size(), epi.av_no_epi_size(), epi.total_epi_count]
    return [_g(x) for x in v]


def _legend(f, names):
    for i, name in enumerate(names):
        f.write("# %2d: %s\n" % (i + 1, name))
    f.write("\n")


def write_stats(ls, path, dump=False, epi=None):
    """land-*.dat: the legend and one PrintStats line"""
    with open(path, "w") as f:
        _legend(f, STATS_COLUMNS)
        f.write(" ".join(stats_tokens(ls, dump, epi)) + " \n")


def write_site_count(ls, path):
    """cLandscape::PrintSiteCount (:994-1003): the comment and the counts of
    the base genome's sites -- an insertion landscape's entry L (insertions
    behind the last site) is not printed, as in the reference"""
    with open(path, "w") as f:
        f.write("# Site Counts\n")
        f.write(" ".join(str(int(c)) for c in ls.site_count[:ls.genome_length]) + " \n")


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
