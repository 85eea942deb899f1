"""The genotype table (include/avida_gpu.h avgpu_get_genotypes).

CPU: systematics.table_from_census, the numpy statement of the table, on
hand-built censuses; GenotypeArbiter.update_table against update() and against
the dictionary arbiter it replaced (restated here), over the five-step rule
sequence and 50 random sequences.

GPU: the device table against table_from_census(census of the same world).
Integer fields, first_cell, max_fitness, the totals and the row order match
exactly; each double sum lies within num_gestated * 2^-52 relative of
math.fsum over the same members (all terms are >= 0, so any summation order
stays inside that).
"""
import ctypes as C
import math
import os
import shutil

import numpy as np
import pytest

from avida_amd import capi, driver, files, systematics
import oracle_lib as ol
import parity_util as pu

EPS = 2.0 ** -52
INT_FIELDS = ["genotype_key", "first_cell", "num_units", "genome_length", "num_gestated", "reserved",
              "sum_gestation", "sum_copied", "max_fitness"]
SUMS = [("sum_merit", "merit"), ("sum_fitness", "fitness"), ("sum_repro_rate", None)]
TOTALS = ["num_organisms", "num_genotypes", "sum_copied_size", "sum_executed_size"]


def _census(keys, gest=None, lens=None):
    c = np.zeros(len(keys), dtype=capi.CENSUS_DTYPE)
    c["genotype_key"] = keys
    c["genome_length"] = lens if lens is not None else 100
    if gest is not None:
        c["gestation_time"] = gest
    return c


def _tot(t):
    return [getattr(t, f) for f in TOTALS]


def check_table(table, totals, census):
    """`table` is the genotype table of `census` under the rules above"""
    ref, rtot = systematics.table_from_census(census)
    assert _tot(totals) == _tot(rtot)
    assert len(table) == len(ref) == totals.num_genotypes
    for f in INT_FIELDS:
        assert np.array_equal(table[f], ref[f]), f
    keys, order, bounds = systematics.cells_by_key(census)
    assert np.array_equal(keys, table["genotype_key"])
    for j in range(len(table)):
        rows = census[order[bounds[j]:bounds[j + 1]]]
        rows = rows[rows["gestation_time"] > 0]
        n = len(rows)
        assert n == table["num_gestated"][j]
        for f, src in SUMS:
            terms = rows[src] if src else 1.0 / rows["gestation_time"].astype(np.float64)
            exact = math.fsum(terms.tolist())
            for t in (table, ref):
                assert abs(float(t[f][j]) - exact) <= n * EPS * exact, (f, j, float(t[f][j]), exact)


# ---- table_from_census ------------------------------------------------------
def test_table_from_census_hand_built():
    c = _census([9, 0, 4, 9, 4, 9, 0, 2], gest=[0, 7, 10, 20, 0, 40, 0, 0],
                lens=[11, 99, 22, 12, 23, 13, 99, 33])
    c["merit"] = [1.0, 50.0, 2.0, 3.0, 4.0, 5.0, 60.0, 6.0]
    c["fitness"] = [0.1, 5.0, 0.2, 0.9, 0.4, 0.5, 6.0, 0.6]
    c["copied_size"] = [1, 1000, 2, 3, 4, 5, 1000, 6]
    c["executed_size"] = [10, 1000, 20, 30, 40, 50, 1000, 60]
    t, tot = systematics.table_from_census(c)
    assert t.dtype == capi.GENOTYPE_DTYPE
    assert t["genotype_key"].tolist() == [2, 4, 9]                   # keys ascending, empty cells ignored
    assert t["first_cell"].tolist() == [7, 2, 0]                     # lowest cell
    assert t["num_units"].tolist() == [1, 2, 3]
    assert t["genome_length"].tolist() == [33, 22, 11]               # of the first cell
    assert t["num_gestated"].tolist() == [0, 1, 2]
    assert t["sum_merit"].tolist() == [0.0, 2.0, 8.0]                # gestated members only
    assert t["sum_fitness"].tolist() == [0.0, 0.2, 0.9 + 0.5]
    assert t["sum_repro_rate"].tolist() == [0.0, 1.0 / 10, 1.0 / 20 + 1.0 / 40]
    assert t["max_fitness"].tolist() == [0.0, 0.2, 0.9]
    assert t["sum_gestation"].tolist() == [0, 10, 60]
    assert t["sum_copied"].tolist() == [0, 2, 8]
    assert t["reserved"].tolist() == [0, 0, 0]
    # the totals run over all living cells, gestated or not; the dead cells' values are not counted
    assert _tot(tot) == [6, 3, 21, 210]
    check_table(t, tot, c)


def test_table_from_census_empty_and_large_keys():
    t, tot = systematics.table_from_census(_census([0, 0, 0]))
    assert len(t) == 0 and _tot(tot) == [0, 0, 0, 0]
    big = (1 << 64) - 1
    t, tot = systematics.table_from_census(_census([big, 1, big, 1 << 63]))
    assert t["genotype_key"].tolist() == [1, 1 << 63, big] and t["first_cell"].tolist() == [1, 3, 0]
    assert _tot(tot)[:2] == [4, 3]


# ---- update_table against update() and the dictionary arbiter ----------------
class _RefGenotype:
    def __init__(self, gid, key, length, update_born):
        self.id, self.key, self.length, self.update_born = gid, key, length, update_born
        self.num_units = self.total_units = 0
        self.threshold = False
        self.name = "%03d-no_name" % length
        self.cells = None


class _RefArbiter:
    """the per-genotype dictionary arbiter GenotypeArbiter.update was before
    it consumed tables: the rules of systematics' module docstring, one
    Python step per living genotype"""

    def __init__(self, threshold=3):
        self.threshold, self.active, self.next_id, self.sz_count = threshold, {}, 1, {}
        self.best = self.census = None

    def update(self, census, update):
        self.census = census
        alive = np.nonzero(census["genotype_key"] != 0)[0]
        keys = census["genotype_key"][alive]
        uk, first, inv, counts = np.unique(keys, return_index=True, return_inverse=True, return_counts=True)
        order = np.argsort(inv.reshape(-1), kind="stable")
        bounds = np.concatenate([[0], np.cumsum(counts)])
        present = {}
        for j in np.argsort(first, kind="stable"):
            k = int(uk[j])
            g = self.active.get(k)
            if g is None:
                g = _RefGenotype(self.next_id, k, int(census["genome_length"][alive[first[j]]]), update)
                self.next_id += 1
                self.active[k] = g
            prev, g.num_units = g.num_units, int(counts[j])
            g.total_units += max(0, g.num_units - prev)
            g.cells = alive[order[bounds[j]:bounds[j + 1]]]
            present[k] = g
        for k in [k for k in self.active if k not in present]:
            if self.best is self.active.pop(k):
                self.best = None
        if not present:
            self.best = None
            return
        top = max(g.num_units for g in present.values())
        if self.best is None or self.best.num_units != top:
            self.best = min((g for g in present.values() if g.num_units == top), key=lambda g: g.id)
        for g in sorted(present.values(), key=lambda g: g.id):
            if not g.threshold and (g.num_units >= self.threshold or g is self.best):
                g.threshold = True
                k = self.sz_count.get(g.length, 0)
                self.sz_count[g.length] = k + 1
                g.name = "%03d-%s" % (g.length, systematics.name_letters(k))

    def dominant_row(self, update):
        g = self.best
        if g is None:
            return None
        rows = self.census[g.cells]
        rows = rows[rows["gestation_time"] > 0]
        if len(rows) == 0:
            avg = (0.0, 0.0, 0.0, 0.0, 0.0, systematics.DBL_MIN)
        else:
            gest = rows["gestation_time"].astype(np.float64)
            avg = (float(rows["merit"].mean()), float(gest.mean()), float(rows["fitness"].mean()),
                   float((1.0 / gest).mean()), float(rows["copied_size"].astype(np.float64).mean()),
                   float(rows["fitness"].max()))
        return [update, *avg[:4], g.length, avg[4], 0.0, g.num_units, 0, 0, 0, 0, avg[5], g.id, g.name]


def _same_state(ref, a, update):
    """arbiter `a` (GenotypeArbiter) stands where the dictionary arbiter stands"""
    assert sorted(ref.active) == sorted(a.active) and len(a.active) == a.num_genotypes() == len(ref.active)
    for k, r in ref.active.items():
        g = a.active[k]
        assert (g.id, g.key, g.length, g.update_born, g.name, g.threshold, g.num_units, g.total_units) == \
               (r.id, r.key, r.length, r.update_born, r.name, r.threshold, r.num_units, r.total_units), k
    assert a.num_threshold() == sum(1 for r in ref.active.values() if r.threshold)
    if ref.best is None:
        assert a.dominant() is None and a.dominant_row(update) is None
        return
    assert a.dominant() is a.active[ref.best.key] and a.dominant().id == ref.best.id
    want, got = ref.dominant_row(update), a.dominant_row(update)
    for i in (0, 5, 8, 9, 10, 11, 12, 14, 15):                      # integers and the name
        assert got[i] == want[i] and type(got[i]) is type(want[i]), i
    assert got[13] == want[13]                                      # max fitness (or DBL_MIN)
    n = int(a.table["num_gestated"][a._index(ref.best.key)])
    for i in (1, 2, 3, 4, 6):
        assert abs(got[i] - want[i]) <= n * EPS * abs(want[i]), (i, got[i], want[i])


def _run_both(censuses):
    ref, by_census, by_table = _RefArbiter(3), systematics.GenotypeArbiter(3), systematics.GenotypeArbiter(3)
    for u, c in enumerate(censuses):
        ref.update(c, u)
        by_census.update(c, u)
        by_table.update_table(*systematics.table_from_census(c), u)
        _same_state(ref, by_census, u)
        _same_state(ref, by_table, u)
        for k, r in ref.active.items():                             # update() also keeps the cells
            assert np.array_equal(by_census.active[k].cells, r.cells)
            assert by_table.active[k].cells is None
    return by_table


def test_update_table_rule_sequence():
    a = _run_both([_census([7, 0, 0, 0]), _census([7, 9, 9, 5], lens=[100, 100, 100, 99]),
                   _census([5, 5, 5, 9]), _census([5, 5, 9, 9]), _census([7, 0, 0, 0])])
    assert a.active[7].id == 4 and a.num_genotypes() == 1 and a.tot_genotypes == 4
    b = systematics.GenotypeArbiter(threshold=3)
    tab = lambda *x, **k: systematics.table_from_census(_census(*x, **k))   # noqa: E731
    b.update_table(*tab([7, 0, 0, 0]), 0)
    g7 = b.dominant()
    assert (g7.id, g7.name, g7.num_units) == (1, "100-aaaaa", 1)
    b.update_table(*tab([7, 9, 9, 5], lens=[100, 100, 100, 99]), 1)
    assert b.active[9].id == 2 and b.active[5].id == 3 and b.dominant() is b.active[9]
    assert b.active[9].name == "100-aaaab" and b.active[5].name == "099-no_name"
    assert (b.num_genotypes(), b.num_threshold()) == (3, 2)
    b.update_table(*tab([5, 5, 5, 9]), 2)
    assert 7 not in b.active and g7.num_units == 0 and b.active[5].name == "099-aaaaa"
    b.update_table(*tab([5, 5, 9, 9]), 3)
    assert b.dominant() is b.active[5]                              # tie: the dominant stays
    b.update_table(*tab([0, 0, 0, 0]), 4)
    assert b.dominant() is None and b.num_genotypes() == 0 and b.dominant_row(4) is None


@pytest.mark.parametrize("block", range(5))
def test_update_table_random_sequences(block):
    """50 sequences (10 a case) of 20 censuses over 200 cells, keys from a
    pool of 30: ties, removals and returning genomes in every sequence"""
    for seed in range(10 * block, 10 * block + 10):
        rng = np.random.default_rng(seed)
        pool = rng.integers(1, 1 << 63, size=30, dtype=np.uint64) * np.uint64(2) + np.uint64(seed % 2)
        length = {int(k): 50 + i % 3 for i, k in enumerate(pool)}
        seq = []
        for _ in range(20):
            allowed = pool[rng.random(30) < rng.uniform(0.1, 0.6)]
            keys = np.zeros(200, dtype=np.uint64)
            if len(allowed):
                keys = allowed[rng.integers(0, len(allowed), size=200)]
                keys[rng.random(200) < rng.uniform(0.0, 0.7)] = 0
            c = _census(keys, lens=[length.get(int(k), 0) for k in keys])
            live = keys != 0
            c["gestation_time"] = np.where(live & (rng.random(200) < 0.7), rng.integers(1, 600, size=200), 0)
            c["merit"] = np.where(live, rng.random(200) * 1e3, 0.0)
            c["fitness"] = np.where(live, rng.random(200), 0.0)
            c["copied_size"] = np.where(live, rng.integers(1, 200, size=200), 0)
            seq.append(c)
        _run_both(seq)


def test_save_population_cells_from_table(golden, tmp_path):
    """an arbiter fed tables carries no cell lists: set_cells derives them
    from a census with one argsort, as save_population does"""
    c = _census([5, 9, 5, 0, 9, 5])
    a = systematics.GenotypeArbiter()
    a.update_table(*systematics.table_from_census(c), 0)
    assert a.active[5].cells is None and a.census is None
    a.set_cells(c)
    assert a.active[5].cells.tolist() == [0, 2, 5] and a.active[9].cells.tolist() == [1, 4]
    with pytest.raises(ValueError):
        a.set_cells(_census([5, 5, 5, 0, 0, 0]))


# ---- the device table -----------------------------------------------------------
def _gpu(golden, n, overrides=None, seed=7):
    import torch
    assert torch.cuda.is_available()
    iset, env, cfg = pu.load_env(golden, overrides=overrides, seed=seed)
    return ol.Backend("gpu", cfg, iset, env, ncells=n)


def _set_keys(b, keys):
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    b._call("set_genotype_keys", b.h, 0, len(k), k.ctypes.data_as(C.c_void_p))


def _populate(b, n, rng, kill=True):
    """one-instruction organisms in every cell, a seeded third killed (unless
    kill is False), the living given phenotype values (gestation times with
    zeros among them, merits, fitnesses, sizes) through avgpu_set_states"""
    b.set_orgs(0, [bytes([0])] * n)
    dead = np.flatnonzero(rng.random(n) < 1.0 / 3.0) if kill else np.zeros(0, dtype=np.int64)
    for c in dead:
        b.kill(int(c))
    st = (capi.AvgpuCpuState * n)()
    ops, fl = (C.c_uint8 * n)(), (C.c_uint8 * n)()
    b._call("get_states", b.h, 0, n, st, ops, fl, 1)
    for i in range(n):
        if st[i].alive:
            st[i].gestation_time = int(rng.integers(1, 900)) if rng.random() < 0.75 else 0
            st[i].merit = float(rng.random() * 1e4)
            st[i].fitness = float(rng.random() * 30)
            st[i].copied_size = int(rng.integers(1, 300))
            st[i].executed_size = int(rng.integers(1, 300))
    b._call("set_states", b.h, 0, n, st, ops, fl, 1)
    return dead


def _device_table(b):
    return capi.get_genotypes(b.lib, b.h)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_gpu_table_shapes(golden, n):
    """key pools of 1 (one segment spanning the world), 3, n/4 and n (every
    cell its own genotype) over worlds around the wave and tile sizes"""
    rng = np.random.default_rng(n)
    b = _gpu(golden, n)
    dead = _populate(b, n, rng)
    for pool in sorted({1, min(3, n), max(1, n // 4), n}):
        keys = rng.integers(1, 1 << 63, size=pool, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        cell_keys = keys[rng.permutation(n) % pool] if pool == n else keys[rng.integers(0, pool, size=n)]
        _set_keys(b, cell_keys)
        census = b.census()
        assert (census["genotype_key"][dead] == 0).all() and (census["genotype_key"] != 0).sum() == n - len(dead)
        assert n < 64 or (census["gestation_time"] > 0).any()
        table, totals = _device_table(b)
        check_table(table, totals, census)
    b.close()


@pytest.mark.gpu
def test_gpu_table_many_tiles(golden):
    """150000 cells, 144990 living: more than 512 segment tiles (the carry
    kernel's second chunk) and 37 sort tiles.  One genotype holding every
    living cell crosses the chunk boundary; 1000 genotypes put segment ends
    on both sides of it."""
    n = 150000
    rng = np.random.default_rng(5)
    b = _gpu(golden, n)
    b.set_orgs(0, [bytes([0])] * 70000)
    b.set_orgs(75000, [bytes([0])] * 75000)
    for c in rng.integers(0, 70000, size=10):
        b.kill(int(c))
    st = (capi.AvgpuCpuState * n)()
    ops, fl = (C.c_uint8 * n)(), (C.c_uint8 * n)()
    b._call("get_states", b.h, 0, n, st, ops, fl, 1)
    s = np.frombuffer(st, dtype=np.dtype(capi.AvgpuCpuState))
    live = s["alive"] != 0
    s["gestation_time"] = np.where(live & (rng.random(n) < 0.75), rng.integers(1, 900, size=n), 0)
    s["merit"] = np.where(live, rng.random(n) * 1e4, 0.0)
    s["fitness"] = np.where(live, rng.random(n) * 30, 0.0)
    s["copied_size"] = np.where(live, rng.integers(1, 300, size=n), 0)
    b._call("set_states", b.h, 0, n, st, ops, fl, 1)
    for pool in (1, 1000):
        keys = rng.integers(1, 1 << 63, size=pool, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        _set_keys(b, keys[rng.integers(0, pool, size=n)])
        census = b.census()
        assert 144980 <= (census["genotype_key"] != 0).sum() <= 144990
        table, totals = _device_table(b)
        assert len(table) == pool
        check_table(table, totals, census)
    b.close()


@pytest.mark.gpu
def test_gpu_table_empty_world(golden):
    b = _gpu(golden, 300)
    table, totals = _device_table(b)
    assert len(table) == 0 and _tot(totals) == [0, 0, 0, 0]
    b.close()


@pytest.mark.gpu
def test_gpu_table_radix_digits(golden):
    """keys that differ in one byte only, for every byte of the key, beside
    the extreme keys: every pass of the sort has to order some pair"""
    n = 4099
    rng = np.random.default_rng(99)
    keys = [1, (1 << 64) - 1, 1 << 56, 1 << 8]
    base = 0x6A09E667F3BCC908
    for byte in range(8):
        k = (base * (byte + 1)) & ((1 << 64) - 1)
        keys += [k, k ^ (0xA5 << (8 * byte))]
    keys = np.array(keys, dtype=np.uint64)
    assert len(set(keys.tolist())) == 20
    b = _gpu(golden, n)
    _populate(b, n, rng)
    # random multiplicities, every key on at least 12 cells (a third of the cells is dead)
    weights = rng.random(len(keys)) ** 3
    pick = np.r_[np.repeat(np.arange(len(keys)), 12),
                 rng.choice(len(keys), size=n - 12 * len(keys), p=weights / weights.sum())]
    _set_keys(b, keys[rng.permutation(pick)])
    census = b.census()
    assert len(np.unique(census["genotype_key"])) == 21          # the 20 keys and the empty cells' 0
    table, totals = _device_table(b)
    assert len(table) == 20 and table["genotype_key"].tolist() == sorted(keys.tolist())
    check_table(table, totals, census)
    b.close()


@pytest.mark.gpu
def test_gpu_table_free_running_world(golden):
    """the world of test_systematics.test_gpu_census_equals_oracle: seed 11,
    one ancestor, 200 updates"""
    iset, env, cfg = pu.load_env(golden, seed=11)
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    n = cfg.world_x * cfg.world_y
    b = _gpu(golden, n, seed=11)
    b.set_orgs(n // 2 + cfg.world_x // 2, [anc], deterministic=False)
    for _ in range(200):
        b.run_update()
    census = b.census()
    assert (census["genotype_key"] != 0).sum() > 100 and (census["gestation_time"] > 0).sum() > 50
    t1, tot1 = _device_table(b)
    check_table(t1, tot1, census)
    t2, tot2 = _device_table(b)
    assert t1.tobytes() == t2.tobytes() and _tot(tot1) == _tot(tot2)      # a function of the world alone
    # the table and the census drive two arbiters to the same place
    at, ac = systematics.GenotypeArbiter(), systematics.GenotypeArbiter()
    at.update_table(t1, tot1, 200)
    ac.update(census, 200)
    b.run_update()                                                       # scratch reused on a changed population
    census = b.census()
    t3, tot3 = _device_table(b)
    check_table(t3, tot3, census)
    at.update_table(t3, tot3, 201)
    ac.update(census, 201)
    assert np.array_equal(at.keys, ac.keys) and np.array_equal(at.ids, ac.ids)
    assert at.dominant().id == ac.dominant().id and at.num_threshold() == ac.num_threshold()
    rt, rc = at.dominant_row(201), ac.dominant_row(201)
    ng = int(at.table["num_gestated"][at._index(at.best_key)])
    for i, (x, y) in enumerate(zip(rt, rc)):
        if i in (1, 2, 3, 4, 6):
            assert abs(x - y) <= ng * EPS * abs(y), (i, x, y)
        else:
            assert x == y, (i, x, y)
    b.close()


@pytest.mark.gpu
def test_gpu_table_behind_queued_updates(golden):
    """five updates queued without a sync, then the table: it is the table of
    the world those updates leave"""
    iset, env, cfg = pu.load_env(golden, seed=11)
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    n = cfg.world_x * cfg.world_y
    b = _gpu(golden, n, seed=11)
    b.set_orgs(0, [anc] * 40, deterministic=False)
    for _ in range(60):
        b.run_update()
    before = b.census()
    for _ in range(5):
        assert b.lib.avgpu_run_update(b.h, None) == 0, b.lib.avgpu_last_error().decode()
    table, totals = _device_table(b)
    after = b.census()
    assert not np.array_equal(before, after)
    check_table(table, totals, after)
    b.close()


@pytest.mark.gpu
def test_gpu_table_sizing_and_refusals(golden):
    n = 600
    rng = np.random.default_rng(3)
    b = _gpu(golden, n)
    _populate(b, n, rng)
    _set_keys(b, rng.integers(1, 40, size=n, dtype=np.uint64))
    census = b.census()
    rows = len(np.unique(census["genotype_key"][census["genotype_key"] != 0]))
    dig = b.digests()
    lib = b.lib
    # count only: NULL / cap 0
    tot = capi.GENOTYPE_TOTALS()
    assert lib.avgpu_get_genotypes(b.h, None, 0, C.byref(tot)) == 0 and tot.num_genotypes == rows
    buf =np.zeros(rows, dtype=capi.GENOTYPE_DTYPE)
    buf["num_units"] = -7
    tot = capi.GENOTYPE_TOTALS()
    assert lib.avgpu_get_genotypes(b.h, buf.ctypes.data_as(C.c_void_p), 0, C.byref(tot)) == 0
    assert tot.num_genotypes == rows and (buf["num_units"] == -7).all()
    # one row short: refused with the count needed, the buffer and the world untouched
    tot = capi.GENOTYPE_TOTALS()
    rc = lib.avgpu_get_genotypes(b.h, buf.ctypes.data_as(C.c_void_p), rows - 1, C.byref(tot))
    assert rc == -1 and str(rows) in lib.avgpu_last_error().decode()         # AVGPU_EINVAL
    assert tot.num_genotypes == rows and tot.num_organisms == (census["genotype_key"] != 0).sum()
    assert (buf["num_units"] == -7).all() and np.array_equal(b.digests(), dig)
    # exactly enough, totals not asked for
    assert lib.avgpu_get_genotypes(b.h, buf.ctypes.data_as(C.c_void_p), rows, None) == rows
    check_table(buf, tot, census)
    assert np.array_equal(b.digests(), dig) and np.array_equal(b.census(), census)
    b.close()
    # a strip tile is refused
    t = _gpu(golden, 512, overrides={"WORLD_X": 64, "WORLD_Y": 64})
    t._call("set_tile", t.h, C.c_int64(0), C.c_int64(0))
    assert lib.avgpu_get_genotypes(t.h, None, 0, C.byref(tot)) == -5         # AVGPU_EUNSUPPORTED
    assert "genotype table on strip tiles" in lib.avgpu_last_error().decode()
    t.close()


@pytest.mark.gpu
def test_gpu_table_row_buffer_regrows(golden):
    """1536 living cells.  8 genotypes, then every cell its own genotype: by
    the size policy (held to literals in tests/test_host_growth.py; no call
    reports a capacity, so not asserted here) the row buffer is made at its
    floor of 1024 rows, and the second table's 1536 rows need a new one, cut to
    a row per cell.  Asserted: both tables are the census's, and the library
    owns as much after the second call as after the first -- a buffer
    replaced, none added."""
    n = 1536
    rng = np.random.default_rng(1536)
    b = _gpu(golden, n)
    _populate(b, n, rng, kill=False)
    counts = []
    for pool in (8, n):
        keys = rng.integers(1, 1 << 63, size=pool, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        assert len(np.unique(keys)) == pool
        _set_keys(b, keys[rng.permutation(n) % pool])
        census = b.census()
        assert (census["genotype_key"] != 0).all()
        table, totals = _device_table(b)
        assert len(table) == pool
        check_table(table, totals, census)
        counts.append(capi.live_objects(b.lib))
    assert counts[1] == counts[0]
    b.close()


def _rows(path):
    return [l.split() for l in open(path) if l.strip() and not l.startswith("#")]


@pytest.mark.gpu
def test_gpu_driver_files_device_table_vs_census(golden, tmp_path):
    """heads_default_100u for 30 updates, once on the product (the arbiter
    fed by avgpu_get_genotypes) and once on the oracle (fed by the census
    through table_from_census): dominant.dat, count.dat and average.dat agree
    row for row -- integers and names exactly, floats to 1e-5 (the files print
    6 significant digits)"""
    import torch
    assert torch.cuda.is_available()
    cfgdir = tmp_path / "config"
    cfgdir.mkdir()
    shutil.copy(os.path.join(golden, "heads_default_100u", "avida.cfg"), cfgdir / "avida.cfg")
    shutil.copy(os.path.join(golden, "instset-heads.cfg"), cfgdir / "instset-heads.cfg")
    shutil.copy(os.path.join(golden, "environment-logic9.cfg"), cfgdir / "environment.cfg")
    shutil.copy(os.path.join(golden, "default-heads.org"), cfgdir / "default-heads.org")
    (cfgdir / "events.cfg").write_text("u begin Inject default-heads.org\n"
                                       "u 0:10:end PrintDominantData\nu 0:10:end PrintCountData\n"
                                       "u 0:10:end PrintAverageData\nu 30 Exit\n")
    dp = driver.Driver(str(cfgdir), str(tmp_path / "product"))
    assert hasattr(dp.world, "genotypes")
    dp.run()
    assert dp.arbiter.census is None and dp.arbiter.totals is not None     # tables all the way
    dp.world.close()
    do = driver.Driver(str(cfgdir), str(tmp_path / "oracle"),
                       make_world=lambda cfg, iset, env: ol.Backend("oracle", cfg, iset, env))
    assert not hasattr(do.world, "genotypes")
    do.run()
    do.world.close()
    for name in ("dominant.dat", "count.dat", "average.dat"):
        got, want = _rows(tmp_path / "product" / name), _rows(tmp_path / "oracle" / name)
        assert len(got) == len(want) == 4 and [r[0] for r in got] == ["0", "10", "20", "30"], name
        for rg, rw in zip(got, want):
            assert len(rg) == len(rw)
            for x, y in zip(rg, rw):
                try:
                    int(y)
                    assert x == y, (name, rg, rw)
                except ValueError:
                    try:
                        fy = float(y)
                    except ValueError:
                        assert x == y, (name, rg, rw)                     # the genotype's name
                    else:
                        assert abs(float(x) - fy) <= 1e-5 * abs(fy), (name, rg, rw)
