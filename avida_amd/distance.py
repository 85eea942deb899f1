"""Genetic distances and the consensus genome.

The reference measures how far genomes are from each other with
InstructionSequence::FindHammingDistance (core/InstructionSequence.cc:488-504)
and FindEditDistance (:547-613), behind the actions PrintGeneticDistanceData
(actions/PrintActions.cc:2700-2766), PrintPopulationDistanceData (:2773-2852)
and CalcConsensus (:3063-3228).  Two routes give the same integers:

* the specification -- ``spec_hamming`` and ``spec_edit`` restate the two
  functions loop for loop, ``spec_edit_fast`` is a numpy row-wise Levenshtein
  for long genomes, ``spec_site_histogram`` CalcConsensus' histograms.  The
  device is tested against them, and they are the path of worlds without the
  device calls (the oracle backend): ``pair_distances``, ``cell_distances`` and
  ``site_histogram`` fall back to them over ``world.states``.
* the device -- avgpu_genome_distances, avgpu_cell_distances and
  avgpu_site_histogram (include/avida_gpu.h): one wave per pair, one pass over
  the tapes for the histogram, nothing but the results copied back.

A genotype's genome is the tape prefix of birth_length sites of its first
cell, the rule population.save_population uses for a member's genome, so a
genotype's distance is ``cell_distances(...)[first_cell]`` gathered from the
arbiter's table.  Limit of that rule: an organism that copied into its own
first sites no longer shows its birth genome there; save_population looks for
a member whose prefix still hashes to the key, the distances take the first
cell's prefix as it is.

``consensus`` restates cHistogram (tools/cHistogram.h) as CalcConsensus uses
it; from exact integer histograms both routes give the same doubles bit for
bit.  ``Actions`` writes the three actions' files.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import capi, datafiles

MAX_GENOME_LENGTH = capi.MAX_GENOME      # include/public/avida/core/Definitions.h:29
HIST_COLS = capi.MAX_INST + 1            # column 0: "no site", the reference's -1 bin
GENERATION_TESTS = 3                     # cCPUTestInfo's generation_tests


# ---- the specification ------------------------------------------------------

def spec_hamming(seq1, seq2):
    """FindHammingDistance at offset 0 (core/InstructionSequence.cc:488-504):
    whatever protrudes past the overlap, plus the differences inside it"""
    size1, size2 = len(seq1), len(seq2)
    overlap = min(size1, size2)                       # FindOverlap, offset 0 (:484)
    distance = size1 + size2 - 2 * overlap            # :496
    for i in range(overlap):                          # :499-501
        if seq1[i] != seq2[i]:
            distance += 1
    return distance


def spec_edit(seq1, seq2):
    """FindEditDistance (core/InstructionSequence.cc:547-613): matching sites
    at the front and at the end are set aside, the rest goes through a two-row
    chart whose column 0 and row 0 are implied"""
    size1, size2 = len(seq1), len(seq2)
    min_size = min(size1, size2)
    if not min_size:                                  # :554
        return max(size1, size2)
    front = 0                                         # :557-559 (the end count may overlap the front's)
    while front < min_size and seq1[front] == seq2[front]:
        front += 1
    end = 0
    while end < min_size and seq1[size1 - end - 1] == seq2[size2 - end - 1]:
        end += 1
    test1 = size1 - front - end                       # :562-565
    test2 = size2 - front - end
    if test1 <= 0 or test2 <= 0:
        return abs(test1 - test2)
    prev_row = [i + 1 for i in range(test1)]          # :572
    cur_row = [0] * test1
    for i in range(test2):                            # :575
        sym = seq2[front + i]
        if seq1[front] == sym:                        # :577-578
            cur_row[0] = i
        else:
            cur_row[0] = i + 1 if i < prev_row[0] else prev_row[0] + 1
        for j in range(1, test1):                     # :581-595
            if seq1[front + j] == sym:
                cur_row[j] = prev_row[j - 1]
            else:
                best = prev_row[j] if prev_row[j] < prev_row[j - 1] else prev_row[j - 1]
                if cur_row[j - 1] < best:
                    best = cur_row[j - 1]
                cur_row[j] = best + 1
        cur_row, prev_row = prev_row, cur_row         # :600-602
    return prev_row[test1 - 1]                        # :607


def spec_edit_fast(seq1, seq2):
    """The Levenshtein distance, one numpy row at a time.  Row i's entries are
    min over k <= j of (t[k] + j - k), t the row's values from the row above
    alone (with D[i][0] = i as t[0]): a running minimum of t[k] - k."""
    a = np.frombuffer(bytes(seq1), dtype=np.uint8)
    b = bytes(seq2)
    m = len(a)
    if m == 0 or len(b) == 0:
        return max(m, len(b))
    idx = np.arange(m + 1, dtype=np.int64)
    prev = idx.copy()
    t = np.empty(m + 1, dtype=np.int64)
    for i, sym in enumerate(b, 1):
        t[0] = i
        np.minimum(prev[1:] + 1, prev[:-1] + (a != sym), out=t[1:])
        t -= idx
        np.minimum.accumulate(t, out=t)
        t += idx
        prev, t = t, prev
    return int(prev[m])


def spec_site_histogram(ops, birth_lens, alive, n_ops):
    """CalcConsensus' histograms (actions/PrintActions.cc:3088-3114) over
    cells: ops[c] the op codes of cell c's memory (at least birth_lens[c] of
    them), alive[c] whether it holds an organism.  Returns (hist, num_living):
    hist[j][1 + op] the living organisms with op at site j of their
    birth_lens[c]-site genome, hist[j][0] those whose genome ends before j."""
    hist = np.zeros((MAX_GENOME_LENGTH, HIST_COLS), dtype=np.int32)
    living = 0
    for c in range(len(birth_lens)):
        if not alive[c]:
            continue
        living += 1
        n = int(birth_lens[c])
        g = np.frombuffer(bytes(ops[c][:n]), dtype=np.uint8)
        if len(g) != n or (n and int(g.max()) >= n_ops):
            raise ValueError(f"cell {c}: a genome of {len(g)} of {n} sites, or an op outside the instruction set")
        np.add.at(hist, (np.arange(n), 1 + g.astype(np.int64)), 1)
        hist[n:, 0] += 1
    return hist, living


class Consensus:
    """what CalcConsensus derives from the histograms"""

    def __init__(self):
        self.length = 0            # con_length
        self.genome = b""          # the consensus genome, op codes
        self.total_entropy = 0.0   # over the sites of the consensus genome
        self.lines = 0             # sites before the one where every organism has ended
        self.mode = []             # per line: the mode (-1: no site), its count, the count variance, the entropy
        self.count = []
        self.variance = []
        self.entropy = []


def consensus(hist, n_ops):
    """cHistogram as CalcConsensus uses it (actions/PrintActions.cc:3122-3154).
    Every site's histogram has the bins -1 .. n_ops -- Resize(num_inst, -1),
    tools/cHistogram.cc:45, so n_ops + 2 of them, the last never filled.
    GetMode (tools/cHistogram.h:130-139): the first maximum, bins in the order
    -1, 0, 1, ...; con_length: the first site whose mode is -1;
    GetCountVariance (:159-173) and GetNormEntropy (:202-215, divided by
    log(n_ops + 2)) in the reference's order of operations.  The loop stops at
    the first site where every organism has ended."""
    num_bins = n_ops + 2
    con = Consensus()
    rows = []
    for i in range(MAX_GENOME_LENGTH):
        bins = [int(x) for x in hist[i][:num_bins]]
        bins += [0] * (num_bins - len(bins))
        mode = 0
        for k in range(1, num_bins):
            if bins[k] > bins[mode]:
                mode = k
        rows.append((bins, mode - 1))
    con.length = MAX_GENOME_LENGTH
    for i, (_, mode) in enumerate(rows):
        if mode == -1:
            con.length = i
            break
    genome = []
    for i, (bins, mode) in enumerate(rows):
        count = bins[mode + 1]
        total = 0
        for x in bins:
            total += x
        entropy = 0.0                                   # GetNormEntropy
        for x in bins:
            prob = float(x) / float(total) if total else math.nan
            if prob != 0.0:
                entropy -= prob * math.log(prob)
        entropy = entropy / math.log(float(num_bins))
        if i < con.length:
            con.total_entropy += entropy
        if mode == -1 and count == total:
            break
        if i < con.length:
            genome.append(mode)
        mean = float(total) / float(num_bins)           # GetCountVariance
        var = 0.0
        for x in bins:
            value = float(x) - mean
            var += value * value
        var /= num_bins - 1
        con.mode.append(mode)
        con.count.append(count)
        con.variance.append(var)
        con.entropy.append(entropy)
    con.lines = len(con.mode)
    con.genome = bytes(genome)
    return con


# ---- the two routes ---------------------------------------------------------

def on_device(world):
    """does `world` answer the distance calls on the device?"""
    return getattr(world, "p", None) == "avgpu_" and hasattr(world.lib, "avgpu_genome_distances")


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _call(world, name, *args):
    return capi.call(world.lib, "avgpu_", name, world.h, *args)


def _edit(a, b):
    return spec_edit_fast(a, b) if len(a) * len(b) > 4096 else spec_edit(a, b)


def pair_distances(world, genomes, pairs, hamming=True, edit=True, device=None):
    """(hamming, edit) of the pairs (i, j) among `genomes` (op-code byte
    strings): int32 arrays, None for a distance not asked for"""
    genomes = [bytes(g) for g in genomes]
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    if not (on_device(world) if device is None else device):
        h = np.array([spec_hamming(genomes[i], genomes[j]) for i, j in pairs], dtype=np.int32) if hamming else None
        e = np.array([_edit(genomes[i], genomes[j]) for i, j in pairs], dtype=np.int32) if edit else None
        return h, e
    buf, lens = capi.pack_genomes(genomes)
    pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    h = np.zeros(max(1, len(pairs)), dtype=np.int32) if hamming else None
    e = np.zeros(max(1, len(pairs)), dtype=np.int32) if edit else None
    _call(world, "genome_distances", len(genomes), buf, lens, len(pairs), _i32p(pa), _i32p(pb),
          None if h is None else _i32p(h), None if e is None else _i32p(e))
    return (None if h is None else h[:len(pairs)]), (None if e is None else e[:len(pairs)])


def to_reference(world, genomes, ref, hamming=True, edit=True, device=None):
    """(hamming, edit) of every genome to `ref`: the pairs (0, i) with the
    reference in front"""
    pairs = [(0, i + 1) for i in range(len(genomes))]
    return pair_distances(world, [bytes(ref)] + list(genomes), pairs, hamming, edit, device)


def _cell_genomes(world, first, count):
    """(genomes, alive) of a cell range from world.states: each organism's
    op-code prefix of birth_length sites, the rule of save_population"""
    cap = capi.MAX_GENOME
    st, ops, _ = world.states(first, count, cap)
    genomes = [ops[i * cap:i * cap + st[i].birth_length] for i in range(count)]
    return genomes, [bool(st[i].alive) for i in range(count)]


def cell_distances(world, ref, first=0, count=None, hamming=True, edit=True, device=None):
    """(hamming, edit) of the organisms of cells first .. first+count-1 to the
    genome `ref` (op codes): int32 arrays, -1 for an empty cell"""
    ref = bytes(ref)
    count = world.ncells - first if count is None else count
    if not (on_device(world) if device is None else device):
        genomes, alive = _cell_genomes(world, first, count)
        h = np.full(count, -1, dtype=np.int32) if hamming else None
        e = np.full(count, -1, dtype=np.int32) if edit else None
        memo = {}
        for i, g in enumerate(genomes):
            if alive[i]:
                if g not in memo:
                    memo[g] = (spec_hamming(g, ref) if hamming else 0, _edit(g, ref) if edit else 0)
                if hamming:
                    h[i] = memo[g][0]
                if edit:
                    e[i] = memo[g][1]
        return h, e
    buf, _ = capi.pack_genomes([ref])
    h = np.zeros(max(1, count), dtype=np.int32) if hamming else None
    e = np.zeros(max(1, count), dtype=np.int32) if edit else None
    _call(world, "cell_distances", first, count, buf, len(ref), None if h is None else _i32p(h),
          None if e is None else _i32p(e))
    return (None if h is None else h[:count]), (None if e is None else e[:count])


def site_histogram(world, first=0, count=None, n_ops=None, device=None):
    """(hist, num_living) over the organisms of a cell range: hist
    [MAX_GENOME_LENGTH][MAX_INST + 1] int32, column 0 "no site", column
    1 + op the organisms with op at the site"""
    count = world.ncells - first if count is None else count
    if not (on_device(world) if device is None else device):
        genomes, alive = _cell_genomes(world, first, count)
        return spec_site_histogram(genomes, [len(g) for g in genomes], alive, capi.MAX_INST if n_ops is None else n_ops)
    hist = np.zeros((MAX_GENOME_LENGTH, HIST_COLS), dtype=np.int32)
    living = C.c_int64()
    _call(world, "site_histogram", first, count, _i32p(hist), C.byref(living))
    return hist, living.value


def last_timing(world):
    """(device ms, pairs, cells) of the last distance or histogram call on the device"""
    ms, p, c = C.c_double(), C.c_int64(), C.c_int64()
    _call(world, "last_distance_ms", C.byref(ms), C.byref(p), C.byref(c))
    return ms.value, p.value, c.value


# ---- the actions' files -----------------------------------------------------

def _test_genomes(world, genomes):
    """[(result, offspring op codes)] of the test CPU: the world's own
    test_genomes, or on a product world avgpu_test_genomes with the offspring
    handed out (driver.ProductWorld.test_genomes drops them)"""
    if getattr(world, "p", None) != "avgpu_":
        return [(r, bytes(child)) for r, _f, child in world.test_genomes(genomes)]
    n = len(genomes)
    buf, lens = capi.pack_genomes(genomes)
    res = (capi.AvgpuTestResult * n)()
    off = (C.c_uint8 * (n * capi.MAX_GENOME))()
    _call(world, "test_genomes", n, buf, lens, res, None, 0, off)
    offb = bytes(off)
    return [(res[i], offb[i * capi.MAX_GENOME:i * capi.MAX_GENOME + res[i].offspring_len]) for i in range(n)]


def colony_organism(world, genome):
    """The test result of cCPUTestInfo::GetColonyOrganism (cpu/cCPUTestInfo.h:
    133-137) after cTestCPU::TestGenome (cpu/cTestCPU.cc:233-326): the
    organism of the depth at which the genome proved viable -- its offspring
    equals the genome it ran or one of a depth below -- else the depth-0
    organism."""
    chain = [bytes(genome)]
    first = None
    for _ in range(GENERATION_TESTS):
        (r, child), = _test_genomes(world, [chain[-1]])
        first = first if first is not None else r
        if not r.divided:
            break
        if child in chain:
            return r
        chain.append(child)
    return first


def _minus_nan_sqrt(x):
    # std::sqrt of a negative double is the default NaN, which ostream prints as "-nan"
    return math.sqrt(x) if x >= 0 else "-nan"


class Actions:
    """PrintGeneticDistanceData, PrintPopulationDistanceData and CalcConsensus
    for the driver.  `device`: None = where the world answers the calls, False
    = the specification over world.states (what a world without them gets)."""

    NAMES = ("PrintGeneticDistanceData", "PrintPopulationDistanceData", "CalcConsensus")

    def __init__(self, world, iset, data_dir, config_dir, device=None):
        self.world, self.iset = world, iset
        self.data_dir, self.config_dir = data_dir, config_dir
        self.device = device
        self.files = {}          # the reference's static files: opened once, a row per call
        self.refs = {}

    def _static(self, name, columns):
        if name not in self.files:
            os.makedirs(self.data_dir, exist_ok=True)
            self.files[name] = datafiles.DataFile(os.path.join(self.data_dir, name), [], columns)
        return self.files[name]

    def close(self):
        for f in self.files.values():
            f.close()
        self.files = {}

    def _reference(self, name):
        if name not in self.refs:
            from . import files
            self.refs[name] = files.read_org(os.path.join(self.config_dir, name), self.iset)
        return self.refs[name]

    def _genotypes(self, arbiter):
        """(ids, units, first cells, keys) of the active genotypes in id
        order, and the dominant's position among them"""
        ids = np.asarray(arbiter.ids, dtype=np.int64)
        o = np.argsort(ids, kind="stable")
        keys = np.asarray(arbiter.keys, dtype=np.uint64)[o]
        units = np.asarray(arbiter.units, dtype=np.int64)[o]
        first = np.asarray(arbiter.table["first_cell"], dtype=np.int64)[o]
        best = arbiter.best_key
        dom = int(np.flatnonzero(keys == np.uint64(best))[0]) if best is not None and len(keys) else -1
        return ids[o], units, first, keys, dom

    def run(self, action, args, arbiter, update):
        if action == "PrintGeneticDistanceData":
            self.genetic_distance(arbiter, update, self._reference(args[0]), *args[1:2])
        elif action == "PrintPopulationDistanceData":
            self.population_distance(arbiter, update, self._reference(args[0]), *args[1:2])
        elif action == "CalcConsensus":
            self.calc_consensus(arbiter, update, int(args[0]) if args else 0)
        else:
            raise ValueError(action)

    def genetic_distance(self, arbiter, update, ref, name="genetic_distance.dat"):
        """genetic_distance.dat (actions/PrintActions.cc:2725-2765), quirks
        restated: the distance sums run once per GENOTYPE while `count` sums
        the genotypes' units, so the "average" is the genotypes' sum over the
        organisms; the "Standard Error" is sqrt((m2 - m1^2) / count) of those
        two quotients (negative under the root prints as the reference's
        "-nan").  With no organism the reference dereferences an empty list:
        no row is written."""
        _ids, units, first, _keys, dom = self._genotypes(arbiter)
        if dom < 0:
            return
        ham = cell_distances(self.world, ref, edit=False, device=self.device)[0][first]
        m1 = m2 = 0.0
        count = 0
        for d, u in zip(ham.tolist(), units.tolist()):
            m1 += d
            m2 += d * d
            count += u
        m1 /= float(count)
        m2 /= float(count)
        f = self._static(name, ["Update", "Average Hamming Distance", "Standard Error",
                                "Best Genotype Hamming Distance"])
        f.row([update, m1, _minus_nan_sqrt((m2 - m1 * m1) / float(count)), float(ham[dom])])

    def population_distance(self, arbiter, update, ref, name=None):
        """pop_distance-<update>.dat (actions/PrintActions.cc:2792-2851): per
        genotype its name, fitness, abundance, Hamming and Levenshtein distance
        to the reference and its genome; rows by genotype id (the reference
        walks its abundance-ordered list).  Two deviations: the reference
        computes the file name but passes the empty m_filename to
        CreateWithPath -- the computed name is used here; its trailer prints
        the double with %d -- datafiles.fmt prints it here.  The trailer's
        WriteRaw adds a second newline, as there."""
        ids, units, first, keys, _dom = self._genotypes(arbiter)
        ham, edit = cell_distances(self.world, ref, device=self.device)
        os.makedirs(self.data_dir, exist_ok=True)
        f = datafiles.DataFile(os.path.join(self.data_dir, name or f"pop_distance-{update}.dat"), [],
                               ["Genotype Name", "Fitness", "Abundance", "Hamming distance to reference",
                                "Levenstein distance to reference", "Genome"])
        sum_fitness, sum_orgs = 0.0, 0
        cap = capi.MAX_GENOME
        for j in range(len(ids)):
            g = arbiter.active[int(keys[j])]
            fitness = float(arbiter.genotype_averages(g)[2])
            st, ops, _ = self.world.states(int(first[j]), 1, cap)
            sum_fitness += fitness * int(units[j])
            sum_orgs += int(units[j])
            f.row([g.name, fitness, int(units[j]), int(ham[first[j]]), int(edit[first[j]]),
                   self.iset.to_sequence(ops[:st[0].birth_length])])
        if sum_orgs:
            f.f.write("# ave fitness from Test CPU's: %s\n\n" % datafiles.fmt(sum_fitness / sum_orgs))
        f.close()

    def calc_consensus(self, arbiter, update, lines_saved=0):
        """consensus.dat (actions/PrintActions.cc:3203-3223) and, with
        lines_saved > 0, consensus-abundance.dat, consensus-var.dat and
        consensus-entropy.dat (:3149-3161).  The histograms count every living
        organism at its own genome, which is the reference's per-genotype
        Insert(op, num_units); the distances to the consensus genome are
        cDoubleSum's weighted average and variance (tools/cDoubleSum.h:47-60,
        Add(value, weight) squares value x weight); the colony values are the
        test CPU's for the consensus genome.  Births, breed counts, abundance
        are 0 and depth and id -1 as in the reference, which looks up no
        consensus genotype.  The archive/*.gen print is left out.  With no
        organism the reference dereferences an empty list: nothing is written."""
        ids, units, first, _keys, dom = self._genotypes(arbiter)
        if dom < 0:
            return
        n_ops = len(self.iset.names)
        hist, _living = site_histogram(self.world, n_ops=n_ops, device=self.device)
        con = consensus(hist, n_ops)
        if lines_saved > 0:
            for name, values in (("consensus-abundance.dat", con.count), ("consensus-var.dat", con.variance),
                                 ("consensus-entropy.dat", con.entropy)):
                self._static(name, []).row(values[:lines_saved])
        if con.length:
            dist = cell_distances(self.world, con.genome, hamming=False, device=self.device)[1][first]
            r = colony_organism(self.world, con.genome)
            merit, gest, fitness = float(r.merit), int(r.gestation_time), float(r.fitness)
            copied, executed = int(r.copied_size), int(r.executed_size)
        else:                      # FindEditDistance of an empty genome: the other one's size
            dist = np.asarray(arbiter.table["genome_length"])[np.argsort(np.asarray(arbiter.ids), kind="stable")]
            merit, gest, fitness, copied, executed = 0.0, 0, 0.0, 0, 0
        s1 = s2 = n = 0.0                                # cDoubleSum
        for d, u in zip(dist.tolist(), units.tolist()):
            w_val = float(d) * float(u)
            n += float(u)
            s1 += w_val
            s2 += w_val * w_val
        ave = s1 / n if n > 0.0 else 0.0
        var = (s2 - s1 * s1 / n) / (n - 1.0) if n > 1.0 else 0.0
        f = self._static("consensus.dat", [
            "Update", "Merit", "Gestation Time", "Fitness", "Reproduction Rate", "Length", "Copied Size",
            "Executed Size", "Get Births", "Breed True", "Breed In", "Abundance", "Tree Depth", "Genotype ID",
            "Age (in updates)", "Best Distance", "Average Distance", "Var Distance", "Total Entropy", "Complexity"])
        f.row([update, merit, gest, fitness, 1.0 / (0.1 + gest), con.length, copied, executed, 0, 0, 0, 0, -1, -1, 0,
               int(dist[dom]), ave, var, con.total_entropy, float(con.length) - con.total_entropy])
