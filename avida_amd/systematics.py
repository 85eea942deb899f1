"""Genotype classification on the host.

The reference files every newborn under the genotype whose instruction
sequence equals its birth genome (Systematics::GenotypeArbiter::
ClassifyNewUnit, systematics/GenotypeArbiter.cc:280-380), keeps genotypes in
abundance-ordered lists (AdjustGenotype, :423-468), names a genotype when it
reaches THRESHOLD organisms or becomes the most abundant (nameGenotype,
:482-497: "%03d-" + five base-26 letters counted per genome size) and drops it
when its last organism dies (removeGenotype, :499-530).

Here the device keys each birth genome once at activation (avgpu_census,
include/avida_gpu.h) and groups the living cells by key into a genotype table
(avgpu_get_genotypes: one row per key with its abundance, first cell and
sums; table_from_census is the same table in numpy, for worlds without the
device call).  GenotypeArbiter.update_table classifies one table after each
update; update(census) does the same from a census and also keeps every
genotype's cells.  It is a batch restatement: births and deaths of one update are
applied together, in cell order, because the batch world itself places and
activates an update's offspring together.
DeviceGenotypeArbiter is the same arbiter kept on the device
(avgpu_classify_genotypes): update_table is its specification,
and only a summary returns per classification.  Rules:

* a key not among the active genotypes becomes a new genotype; new ids are
  handed out in order of the first cell holding the key;
* a genotype whose abundance falls to 0 is removed from the active set; a
  later organism with the same genome starts a new genotype, as in the
  reference once the old one left the active hash;
* ancestry (GenotypeArbiter(threshold, lineage=True)): the
  device hands every organism its parent's genotype key (avgpu_get_parent_keys),
  and LineageStore keeps one row per genotype ever classified -- parent id,
  depth = the parent's + 1 (systematics/Genotype.cc:139-176), the update it
  was deactivated -- until prune() drops the dead genotypes with no living
  descendant (the passive references of :159 and GenotypeArbiter.cc:499-530);
* threshold: abundance >= THRESHOLD, or the genotype is the most abundant
  (GenotypeArbiter.cc:320-328, :459-467); names are given in id order among
  the genotypes that cross it in one update;
* dominant (GenotypeArbiter::Begin -> getBest): the most abundant; on a tie
  the previous dominant stays (the "keep the current best" special case,
  :450-453), otherwise the lowest id.

Genotype averages (merit, gestation time, fitness, repro rate, copied size)
are the means, over the genotype's living organisms that carry a completed
gestation (gestation_time > 0: a divided parent or an offspring, which
inherits its parent's last gestation values, main/cPhenotype.cc:349-420), of
the values Genotype::HandleUnitGestation (systematics/Genotype.cc:289-301)
accumulates per gestation; the reference averages over all gestations the
genotype ever had, so the two agree while the genotype's members share their
phenotype (always for a clonal lineage), and are statistically close
otherwise.  "Executed Size of Dominant Genotype" is 0 in the reference: the
organism publishes "last_exectuted_size" (main/cOrganism.cc:67) while the
genotype reads "last_executed_size" (systematics/Genotype.cc:38, :294); it is
written as 0 here too.  With no gestation recorded the averages are 0 and max
fitness is DBL_MIN (an empty cDoubleSum, as the reference's first rows show).
"""
from __future__ import annotations

import sys
from collections.abc import Mapping

import numpy as np

from . import capi

GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
DBL_MIN = sys.float_info.min


def _mix(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def genome_key(codes) -> int:
    """Genome key of a birth genome given as canonical instruction codes
    (the device's gk_* in avida_amd/csrc/device.h; oracle genome_key)."""
    codes = bytes(codes)
    n = len(codes)
    s = 0
    for w in range((n + 3) // 4):
        v = 0
        for j in range(4):
            if 4 * w + j < n:
                v |= (codes[4 * w + j] & 0x3F) << (8 * j)
        s = (s + _mix(((w + 1) << 32) | v)) & M64
    k = _mix(s ^ ((n * GOLD) & M64))
    return k or 1


def name_letters(num: int) -> str:
    """nameGenotype's five base-26 letters (GenotypeArbiter.cc:482-497)"""
    a = []
    for _ in range(5):
        a.append(chr(ord("a") + num % 26))
        num //= 26
    return "".join(reversed(a))


def _totals(num_organisms=0, num_genotypes=0, sum_copied=0, sum_executed=0):
    t = capi.GENOTYPE_TOTALS()
    t.num_organisms, t.num_genotypes = int(num_organisms), int(num_genotypes)
    t.sum_copied_size, t.sum_executed_size = int(sum_copied), int(sum_executed)
    return t


def table_from_census(census):
    """The genotype table of a census, (table, totals): the numpy statement of
    avgpu_get_genotypes (include/avida_gpu.h), the same fields
    (capi.GENOTYPE_DTYPE) in the same order -- one row per distinct non-zero
    key, keys ascending.  The device table is tested against it, and worlds
    without a device table (the oracle) feed the arbiter through it.

    Summation: every double sum is accumulated one member at a time in
    ascending cell order (numpy.bincount with weights).  The device adds the
    same members in a tree, so the two agree to num_gestated * 2^-52
    relative (all terms >= 0), not bit for bit; integers and max_fitness are
    exact.  A census row counts as living when its key is non-zero."""
    key = census["genotype_key"]
    alive = np.flatnonzero(key != 0)
    uk, first, inv, counts = np.unique(key[alive], return_index=True, return_inverse=True,
                                       return_counts=True)
    m = len(uk)
    table = np.zeros(m, dtype=capi.GENOTYPE_DTYPE)
    totals = _totals(len(alive), m, census["copied_size"][alive].sum(dtype=np.int64),
                     census["executed_size"][alive].sum(dtype=np.int64))
    if m == 0:
        return table, totals
    inv = inv.reshape(-1)
    first_cell = alive[first]
    table["genotype_key"] = uk
    table["first_cell"] = first_cell
    table["num_units"] = counts
    table["genome_length"] = census["genome_length"][first_cell]
    gest = census["gestation_time"][alive]
    done = gest > 0
    gi, rows = inv[done], census[alive[done]]
    gt = rows["gestation_time"].astype(np.float64)
    table["num_gestated"] = np.bincount(gi, minlength=m)
    table["sum_merit"] = np.bincount(gi, weights=rows["merit"], minlength=m)
    table["sum_fitness"] = np.bincount(gi, weights=rows["fitness"], minlength=m)
    table["sum_repro_rate"] = np.bincount(gi, weights=1.0 / gt, minlength=m)
    sg, sc = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    np.add.at(sg, gi, rows["gestation_time"])
    np.add.at(sc, gi, rows["copied_size"])
    table["sum_gestation"], table["sum_copied"] = sg, sc
    if len(gi):
        o = np.lexsort((rows["fitness"], gi))            # by genotype, fitness ascending
        gs = gi[o]
        last = np.flatnonzero(np.r_[gs[1:] != gs[:-1], True])
        table["max_fitness"][gs[last]] = rows["fitness"][o][last]
    return table, totals


def cells_by_key(census):
    """(keys ascending, order, bounds): the living cells of key keys[j] are
    order[bounds[j]:bounds[j + 1]], ascending -- one stable argsort"""
    alive = np.flatnonzero(census["genotype_key"] != 0)
    k = census["genotype_key"][alive]
    o = np.argsort(k, kind="stable")
    ks = k[o]
    heads = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]]) if len(ks) else np.zeros(0, dtype=np.int64)
    return ks[heads], alive[o], np.r_[heads, len(ks)]


def _align16(n):
    return (n + 15) & ~15


class LineageStore:
    """The ancestry of every genotype classified since the arbiter was new
    (DESIGN.md 10.6): `rows` (capi.LINEAGE_ROW_DTYPE, ascending by id -- ids
    are handed out consecutively, so appending keeps them sorted and a lookup
    is a binary search) and `arena`, the captured birth genomes as canonical
    codes at 16-B aligned offsets in id order.  Integers only; every rule is
    order-free."""

    def __init__(self):
        self.rows = np.zeros(0, dtype=capi.LINEAGE_ROW_DTYPE)
        self.arena = bytearray()
        self.num_orphans = 0
        self.num_unsequenced = 0
        self.dropped_last_prune = 0

    def index(self, gid):
        """the row of genotype id `gid`, -1 when the store has none"""
        ids = self.rows["id"]
        j = int(np.searchsorted(ids, gid))
        return j if j < len(ids) and int(ids[j]) == int(gid) else -1

    def summary(self):
        r = self.rows
        return dict(rows=len(r), active_rows=int((r["update_deactivated"] < 0).sum()), arena_bytes=len(self.arena),
                    num_orphans=self.num_orphans, num_unsequenced=self.num_unsequenced,
                    max_depth=int(r["depth"].max()) if len(r) else 0, dropped_last_prune=self.dropped_last_prune)

    def deactivate(self, ids, update):
        """rule 1: the genotypes `ids` left the active set at `update`"""
        if len(ids):
            j = np.searchsorted(self.rows["id"], ids)
            self.rows["update_deactivated"][j] = update

    def append(self, new, old_keys, old_ids, update):
        """rules 2 and 3: `new` = (key, id, parent key, genome length,
        generation, sequence or None) per new genotype, ascending by id;
        old_keys (ascending) / old_ids: the genotypes active BEFORE this
        classification, those it deactivates included"""
        add = np.zeros(len(new), dtype=capi.LINEAGE_ROW_DTYPE)
        for k, (key, gid, pk, length, gen, seq) in enumerate(new):
            parent_id, depth = 0, 0
            if pk != 0:
                j = int(np.searchsorted(old_keys, np.uint64(pk)))
                if j < len(old_keys) and int(old_keys[j]) == int(pk):
                    parent_id = int(old_ids[j])
                    depth = int(self.rows["depth"][self.index(parent_id)]) + 1
                else:            # born and gone between two classifications, or the key itself
                    parent_id = -1
                    self.num_orphans += 1
            off = -1
            if seq is not None and len(seq) == length and genome_key(seq) == int(key):
                off = len(self.arena)
                self.arena += bytes(c & 0x3F for c in seq) + bytes(_align16(length) - length)
            else:
                self.num_unsequenced += 1
            add[k] = (key, gid, parent_id, off, update, -1, depth, length, gen, 0)
        self.rows = np.concatenate([self.rows, add])

    def kept_by_prune(self):
        """the rows a prune keeps: the active ones and every row on the
        parent_id chain of one (a closure: independent of the order walked)"""
        r = self.rows
        keep = r["update_deactivated"] < 0
        for j in np.flatnonzero(keep):
            p = int(r["parent_id"][j])
            while p > 0:
                q = self.index(p)
                if q < 0 or keep[q]:
                    break            # absent (pruned before), or already marked: its chain is, or will be
                keep[q] = True
                p = int(r["parent_id"][q])
        return keep

    def prune(self):
        """rule 4: drop the dead genotypes without a living descendant; rows
        and arena compacted stably (same order, offsets recomputed)"""
        keep = self.kept_by_prune()
        rows = self.rows[keep].copy()
        arena = bytearray()
        for j in range(len(rows)):
            off = int(rows["seq_off"][j])
            if off >= 0:
                n = _align16(int(rows["genome_length"][j]))
                rows["seq_off"][j] = len(arena)
                arena += self.arena[off:off + n]
        self.dropped_last_prune = int(len(self.rows) - len(rows))
        self.rows, self.arena = rows, arena
        return self.dropped_last_prune

    def sequence(self, gid):
        """the captured birth genome of genotype `gid` (canonical codes), or None"""
        j = self.index(gid)
        if j < 0 or self.rows["seq_off"][j] < 0:
            return None
        off = int(self.rows["seq_off"][j])
        return bytes(self.arena[off:off + int(self.rows["genome_length"][j])])

    def lineage_of(self, gid):
        """the rows from genotype `gid` up to its root: each one's parent
        follows it, until a row without a stored parent (parent_id 0: an
        injected genotype; -1: an orphan; or a parent pruned away)"""
        out = []
        j = self.index(gid)
        while j >= 0:
            out.append(self.rows[j])
            p = int(self.rows["parent_id"][j])
            j = self.index(p) if p > 0 else -1
        return np.array(out, dtype=capi.LINEAGE_ROW_DTYPE)


class Genotype:
    """One active genotype, read through the arbiter's arrays.  The object
    for a key stays the same while the genotype lives; after its removal it
    keeps its last values with num_units 0."""
    __slots__ = ("_a", "id", "key", "length", "update_born", "_gone")

    def __init__(self, arbiter, key, j):
        self._a, self.key = arbiter, key
        self.id, self.length = int(arbiter.ids[j]), int(arbiter.lengths[j])
        self.update_born = int(arbiter.born[j])
        self._gone = None

    def _j(self):
        return self._a._index(self.key)

    def _retire(self):
        """called before the arbiter drops the genotype"""
        self._gone = (self.total_units, self.threshold, self.name)

    @property
    def num_units(self):
        return 0 if self._gone else int(self._a.units[self._j()])

    @property
    def total_units(self):
        return self._gone[0] if self._gone else int(self._a.total[self._j()])

    @property
    def threshold(self):
        return self._gone[1] if self._gone else bool(self._a.thr[self._j()])

    @property
    def name(self):
        if self._gone:
            return self._gone[2]
        k = int(self._a.name_no[self._j()])
        return "%03d-%s" % (self.length, name_letters(k - 1)) if k else "%03d-no_name" % self.length

    @property
    def cells(self):
        a = self._a
        if self._gone or a.cell_order is None:
            return None
        j = self._j()
        return a.cell_order[a.cell_bounds[j]:a.cell_bounds[j + 1]]


class _Active(Mapping):
    """key -> Genotype over the arbiter's sorted key array"""

    def __init__(self, arbiter):
        self._a = arbiter

    def __len__(self):
        return len(self._a.keys)

    def __iter__(self):
        return (int(k) for k in self._a.keys)

    def __contains__(self, key):
        return self._a._index(key) >= 0

    def __getitem__(self, key):
        a = self._a
        j = a._index(key)
        if j < 0:
            raise KeyError(key)
        g = a._views.get(int(key))
        if g is None:
            g = a._views[int(key)] = Genotype(a, int(key), j)
        return g


class GenotypeArbiter:
    """Batch restatement of Systematics::GenotypeArbiter over genotype
    tables.  The active genotypes are parallel arrays in ascending key order
    (the table's order): matching a table against them, abundances, totals and
    the dominant are array operations; Python runs per genotype only for
    those that cross the threshold (names) and for Genotype objects a caller
    asked for."""

    def __init__(self, threshold=3, lineage=False):
        self.threshold = threshold
        self.lineage = LineageStore() if lineage else None
        self.keys = np.zeros(0, dtype=np.uint64)
        self.ids = np.zeros(0, dtype=np.int64)
        self.lengths = np.zeros(0, dtype=np.int32)
        self.born = np.zeros(0, dtype=np.int64)
        self.units = np.zeros(0, dtype=np.int64)
        self.total = np.zeros(0, dtype=np.int64)
        self.thr = np.zeros(0, dtype=bool)
        self.name_no = np.zeros(0, dtype=np.int64)   # 1 + the name's number within its size, 0 = unnamed
        self.active = _Active(self)
        self._views = {}
        self.next_id = 1
        self.sz_count = {}        # genome size -> names handed out
        self.tot_genotypes = 0
        self.tot_threshold = 0
        self.best_key = None
        self.table = None         # the last table: row j describes keys[j]
        self.totals = None
        self.census = None        # set by update(census) only
        self.cell_order = self.cell_bounds = None

    def _index(self, key):
        j = int(np.searchsorted(self.keys, np.uint64(key)))
        return j if j < len(self.keys) and int(self.keys[j]) == int(key) else -1

    def _name(self, size):
        """the next name number of a genome size, plus 1"""
        k = self.sz_count.get(size, 0)
        self.sz_count[size] = k + 1
        return k + 1

    def update_table(self, table, totals, update, parent_keys=None, sequences=None, generations=None):
        """Classify one genotype table (capi.GENOTYPE_DTYPE rows, keys
        ascending; table_from_census or capi.get_genotypes).  With lineage on,
        per table row: parent_keys = the parent key of its first cell
        (avgpu_get_parent_keys), sequences = that cell's tape prefix of
        birth_len sites as canonical codes (or None), generations = its census
        generation; only the new genotypes' entries are read."""
        if self.lineage is not None and parent_keys is None:
            raise ValueError("lineage is on: update_table needs the table rows' parent keys")
        tk = table["genotype_key"]
        m, old = len(tk), len(self.keys)
        pos = np.searchsorted(self.keys, tk)
        found = np.zeros(m, dtype=bool)
        if old:
            found = self.keys[np.minimum(pos, old - 1)] == tk
        dst = np.flatnonzero(found)
        src = pos[dst]
        fresh = np.flatnonzero(~found)
        old_keys, old_ids = self.keys, self.ids
        if self.lineage is not None and len(src) < old:
            gone = np.ones(old, dtype=bool)
            gone[src] = False
            self.lineage.deactivate(np.sort(old_ids[gone]), update)
        if self._views and len(src) < old:            # genotypes that disappear
            gone = np.ones(old, dtype=bool)
            gone[src] = False
            for k in self.keys[gone]:
                g = self._views.pop(int(k), None)
                if g is not None:
                    g._retire()
        units = table["num_units"].astype(np.int64)

        def carry(a, fill):
            out = np.full(m, fill, dtype=a.dtype)
            out[dst] = a[src]
            return out
        ids, lengths, born = carry(self.ids, 0), carry(self.lengths, 0), carry(self.born, update)
        prev, total = carry(self.units, 0), carry(self.total, 0)
        thr, name_no = carry(self.thr, False), carry(self.name_no, 0)
        # new ids in order of the first cell holding the key
        by_cell = fresh[np.argsort(table["first_cell"][fresh], kind="stable")]
        ids[by_cell] = self.next_id + np.arange(len(fresh))
        lengths[fresh] = table["genome_length"][fresh]
        if self.lineage is not None and len(fresh):
            self.lineage.append([(int(tk[j]), int(ids[j]), int(parent_keys[j]), int(lengths[j]),
                                  int(generations[j]) if generations is not None else 0,
                                  sequences[j] if sequences is not None else None) for j in by_cell],
                                old_keys, old_ids, update)
        self.next_id += len(fresh)
        self.tot_genotypes += len(fresh)
        total += np.maximum(0, units - prev)
        self.keys, self.ids, self.lengths, self.born = tk.copy(), ids, lengths, born
        self.units, self.total, self.thr, self.name_no = units, total, thr, name_no
        self.table, self.totals = table, totals
        self.census = self.cell_order = self.cell_bounds = None
        if m == 0:
            self.best_key = None
            return
        top = units.max()
        bj = self._index(self.best_key) if self.best_key is not None else -1
        if bj < 0 or units[bj] != top:
            cand = np.flatnonzero(units == top)
            bj = int(cand[np.argmin(ids[cand])])
            self.best_key = int(tk[bj])
        cross = ~thr & (units >= self.threshold)
        cross[bj] = not thr[bj]
        cj = np.flatnonzero(cross)
        for j in cj[np.argsort(ids[cj])]:              # names in id order
            thr[j] = True
            name_no[j] = self._name(int(lengths[j]))
            self.tot_threshold += 1

    def update(self, census, update):
        """Classify one census (capi.CENSUS_DTYPE rows, one per cell); the
        genotypes then know their cells."""
        table, totals = table_from_census(census)
        self.update_table(table, totals, update)
        self.census = census
        self.set_cells(census)

    def set_cells(self, census):
        """give the genotypes of the last table their cell lists from a
        census of the same world state"""
        keys, self.cell_order, self.cell_bounds = cells_by_key(census)
        if not np.array_equal(keys, self.keys):
            raise ValueError("the census does not hold the genotypes of the last table")

    # ---- cStats / data-file views ----
    def num_genotypes(self):
        return len(self.keys)

    def num_threshold(self):
        return int(self.thr.sum())

    def dominant(self):
        return self.active[self.best_key] if self.best_key is not None else None

    @property
    def best(self):
        return self.dominant()

    # ---- ancestry (lineage=True) ----
    def _store(self):
        if self.lineage is None:
            raise ValueError("this arbiter keeps no lineage (GenotypeArbiter(threshold, lineage=True))")
        return self.lineage

    def prune(self):
        """drop the dead genotypes without a living descendant; returns how many"""
        return self._store().prune()

    def lineage_of(self, gid):
        """the store's rows from genotype `gid` up to its root"""
        return self._store().lineage_of(gid)

    def depth_of(self, gid):
        j = self._store().index(gid)
        return int(self.lineage.rows["depth"][j]) if j >= 0 else 0

    def genotype_averages(self, g):
        """(merit, gestation, fitness, repro rate, copied size, max fitness)
        over g's organisms with a completed gestation: the table's sums over
        num_gestated"""
        r = self.table[self._index(g.key)]
        n = int(r["num_gestated"])
        if n == 0:
            return 0.0, 0.0, 0.0, 0.0, 0.0, DBL_MIN
        return (float(r["sum_merit"]) / n, int(r["sum_gestation"]) / n, float(r["sum_fitness"]) / n,
                float(r["sum_repro_rate"]) / n, int(r["sum_copied"]) / n, float(r["max_fitness"]))

    def dominant_row(self, update):
        """One PrintDominantData row (actions/PrintActions.cc:5405-5440), or
        None with no organisms (the reference writes nothing then)."""
        g = self.dominant()
        if g is None:
            return None
        merit, gest, fit, repro, copied, maxfit = self.genotype_averages(g)
        # births / breed true / breed in need per-genotype birth records: 0;
        # the depth comes from the lineage store where one is kept
        depth = self.depth_of(g.id) if self.lineage is not None else 0
        return [update, merit, gest, fit, repro, g.length, copied, 0.0, g.num_units,
                0, 0, depth, 0, maxfit, g.id, g.name]


def classify_with_lineage(arbiter, world, update, handlers, cap=capi.MAX_GENOME):
    """One classification of `world` by a host GenotypeArbiter(lineage=True),
    the specification run beside a device store to check it (it drags the
    parent-key row and a census to the host: not a production path; the
    device keeps the store itself, DeviceGenotypeArbiter(lineage=True)).
    Fed from the device: the genotype table (world.genotypes), the parent key
    and census generation of each row's first cell (world.parent_keys,
    world.census) and, for the new genotypes only, that cell's tape prefix of
    birth_length sites as canonical codes (world.states; `handlers` =
    InstSet.handlers, op -> canonical code).  A world without parent_keys (the
    oracle backend keeps no ancestry) raises."""
    if not hasattr(world, "parent_keys"):
        raise ValueError("lineage needs a world that records parent keys (avgpu_get_parent_keys): "
                         f"{type(world).__name__} has none")
    table, totals = world.genotypes() if hasattr(world, "genotypes") else table_from_census(world.census())
    first = table["first_cell"]
    pk = world.parent_keys()[first]
    gens = world.census()["generation"][first]
    tk = table["genotype_key"]
    old = len(arbiter.keys)
    pos = np.minimum(np.searchsorted(arbiter.keys, tk), max(old - 1, 0))
    known = arbiter.keys[pos] == tk if old else np.zeros(len(tk), dtype=bool)
    seqs = [None] * len(tk)
    for j in np.flatnonzero(~known):
        st, ops, _ = world.states(int(first[j]), 1, cap)
        seqs[j] = bytes(handlers[x] for x in ops[:min(st[0].birth_length, cap)])
    arbiter.update_table(table, totals, update, parent_keys=pk, sequences=seqs, generations=gens)


class GenotypeSnapshot:
    """One active genotype of a DeviceGenotypeArbiter, as the classification
    it was fetched from left it: plain values, not a live view.  After the
    next classify() it still shows the old values; ask the arbiter again."""
    __slots__ = ("_a", "_gen", "_j", "id", "key", "length", "update_born", "num_units", "total_units",
                 "threshold", "name")

    def __init__(self, arbiter, row, j):
        self._a, self._gen, self._j = arbiter, arbiter._generation, j
        self.key, self.id, self.length = int(row["genotype_key"]), int(row["id"]), int(row["genome_length"])
        self.update_born, self.num_units = int(row["update_born"]), int(row["num_units"])
        self.total_units, self.threshold = int(row["total_units"]), bool(row["threshold"])
        k = int(row["name_no"])
        self.name = "%03d-%s" % (self.length, name_letters(k - 1)) if k else "%03d-no_name" % self.length

    @property
    def cells(self):
        a = self._a
        if a._generation != self._gen or a.cell_order is None:
            return None
        j = self._j if self._j is not None else a._index(self.key)
        return a.cell_order[a.cell_bounds[j]:a.cell_bounds[j + 1]]


class _DeviceActive(_Active):
    """key -> GenotypeSnapshot over the fetched state of a DeviceGenotypeArbiter"""

    def __getitem__(self, key):
        a = self._a
        j = a._index(key)
        if j < 0:
            raise KeyError(key)
        g = a._views.get(int(key))
        if g is None:
            g = a._views[int(key)] = GenotypeSnapshot(a, a.rows[j], j)
        return g


class DeviceGenotypeArbiter:
    """The arbiter kept on the device (avgpu_classify_genotypes; DESIGN.md
    10.5): classify() runs one classification there and keeps its summary.
    The counts, the totals, the dominant and its data-file row come from the
    summary alone.  Everything per genotype (keys, ids, ... table, active[...],
    set_cells, genotype_averages of any genotype) is fetched lazily by one
    avgpu_get_arbiter and cached until the next classify(), with the names
    and meanings GenotypeArbiter gives them.

    Genotype objects of this class (GenotypeSnapshot) are snapshots of the
    classification they were fetched from; they do not follow the genotype
    through later classifications as GenotypeArbiter's views do."""

    census = None             # never fed a census

    def __init__(self, threshold=3, lineage=False):
        self.threshold = threshold
        self.lineage = bool(lineage) or None     # (dominant_row: None = no depth column)
        self._lin = None
        self.active = _DeviceActive(self)
        self.world = None
        self.summary = np.zeros(1, dtype=capi.ARBITER_SUMMARY_DTYPE)[0]
        self.summary["next_id"], self.summary["dominant_row"] = 1, -1
        self._generation = 0
        self._drop()

    def _drop(self):
        self._generation += 1
        self._state = None
        self._lin = None
        self._views = {}
        self._dominant = None
        self.cell_order = self.cell_bounds = None

    def classify(self, world, update):
        """one classification of `world` (driver.ProductWorld) after `update`"""
        self.world = world
        self.summary = world.classify_genotypes(update, self.threshold)
        self._drop()
        if self.lineage:                         # prune when the store exceeds twice the active rows
            s = world.lineage_state(summary_only=True)[2]
            if int(s["rows"]) > 2 * int(s["active_rows"]):
                world.prune_lineage()
        return self.summary

    # ---- ancestry: the device store (lineage=True), fetched lazily ----
    def enable(self, world, rows_hint=0, arena_hint=0):
        """turn the world's store on (a new world, or after avgpu_reset_arbiter)"""
        self.world = world
        world.enable_lineage(True, rows_hint, arena_hint)

    def lineage_store(self):
        """the store as a host LineageStore (one avgpu_get_lineage, cached
        until the next classify)"""
        if not self.lineage or self.world is None:
            raise ValueError("this arbiter keeps no lineage (DeviceGenotypeArbiter(threshold, lineage=True))")
        if self._lin is None:
            rows, arena, s = self.world.lineage_state()
            st = LineageStore()
            st.rows, st.arena = rows, bytearray(arena.tobytes())
            st.num_orphans, st.num_unsequenced = int(s["num_orphans"]), int(s["num_unsequenced"])
            st.dropped_last_prune = int(s["dropped_last_prune"])
            self._lin = st
        return self._lin

    def lineage_of(self, gid):
        return self.lineage_store().lineage_of(gid)

    def depth_of(self, gid):
        st = self.lineage_store()
        j = st.index(gid)
        return int(st.rows["depth"][j]) if j >= 0 else 0

    def prune(self):
        self._lin = None
        return int(self.world.prune_lineage()["dropped_last_prune"])

    def attach(self, world):
        """take over the state `world` holds (after a restore)"""
        self.world = world
        self._drop()
        self._state = world.arbiter_state()
        self.summary = self._state[2]

    # ---- from the summary alone ----
    def num_genotypes(self):
        return int(self.summary["num_genotypes"])

    def num_threshold(self):
        return int(self.summary["num_threshold"])

    @property
    def tot_genotypes(self):
        return int(self.summary["tot_genotypes"])

    @property
    def tot_threshold(self):
        return int(self.summary["tot_threshold"])

    @property
    def next_id(self):
        return int(self.summary["next_id"])

    @property
    def best_key(self):
        s = self.summary
        return int(s["dominant_state"]["genotype_key"]) if s["dominant_row"] >= 0 else None

    @property
    def totals(self):
        s = self.summary
        return _totals(s["num_organisms"], s["num_genotypes"], s["sum_copied_size"], s["sum_executed_size"])

    def dominant(self):
        s = self.summary
        if s["dominant_row"] < 0:
            return None
        if self._dominant is None:
            self._dominant = GenotypeSnapshot(self, s["dominant_state"], int(s["dominant_row"]))
        return self._dominant

    @property
    def best(self):
        return self.dominant()

    def genotype_averages(self, g):
        s = self.summary
        if s["dominant_row"] >= 0 and int(s["dominant_state"]["genotype_key"]) == g.key:
            r = s["dominant"]
        else:
            r = self.table[self._index(g.key)]
        n = int(r["num_gestated"])
        if n == 0:
            return 0.0, 0.0, 0.0, 0.0, 0.0, DBL_MIN
        return (float(r["sum_merit"]) / n, int(r["sum_gestation"]) / n, float(r["sum_fitness"]) / n,
                float(r["sum_repro_rate"]) / n, int(r["sum_copied"]) / n, float(r["max_fitness"]))

    dominant_row = GenotypeArbiter.dominant_row

    # ---- per genotype: one avgpu_get_arbiter, cached ----
    def _fetch(self):
        if self._state is None:
            if self.world is None:
                z = np.zeros(0, dtype=capi.ARBITER_ROW_DTYPE), np.zeros(0, dtype=capi.GENOTYPE_DTYPE)
                self._state = (*z, self.summary, np.zeros(capi.MAX_GENOME + 1, dtype=np.int64))
            else:
                self._state = self.world.arbiter_state()
        return self._state

    @property
    def rows(self):
        return self._fetch()[0]

    @property
    def table(self):
        return self._fetch()[1]

    @property
    def sz_count(self):
        """genome size -> names handed out (the sizes with any)"""
        sz = self._fetch()[3]
        return {int(k): int(sz[k]) for k in np.flatnonzero(sz)}

    keys = property(lambda self: self.rows["genotype_key"])
    ids = property(lambda self: self.rows["id"])
    lengths = property(lambda self: self.rows["genome_length"])
    born = property(lambda self: self.rows["update_born"])
    units = property(lambda self: self.rows["num_units"].astype(np.int64))
    total = property(lambda self: self.rows["total_units"])
    thr = property(lambda self: self.rows["threshold"] != 0)
    name_no = property(lambda self: self.rows["name_no"].astype(np.int64))

    _index = GenotypeArbiter._index
    set_cells = GenotypeArbiter.set_cells
