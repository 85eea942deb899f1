"""Population events: kills, bottlenecks, serial transfer.

The events an experiment schedules beside its Print and Save actions are the
population actions of actions/PopulationActions.cc: KillProb / KillRate
(:1166-1187), ApplyBottleneck (:1195-1224), KillDominantGenotype (:1226-1258),
KillProbSequence (:1261-1299), KillRectangle (:1754-1815) and SerialTransfer
(:1833-1854, cPopulation::SerialTransfer, main/cPopulation.cc:7553-7585).  Two
routes kill the same cells:

* the specification -- ``kill_prob``, ``kill_rect``, ``kill_genotypes`` and
  ``keep_sample`` return the sorted array of cells to kill from an alive mask
  (and the cells' genotype keys where they matter), written from the
  reference's loops.  The device is tested against them, and they are the path
  of worlds without the device calls (the oracle backend): the wrappers below
  compute the set from ``world.census()`` and kill cell by cell.
* the device -- avgpu_kill_cells, avgpu_kill_prob, avgpu_kill_rect,
  avgpu_kill_genotypes and avgpu_keep_sample (include/avida_gpu.h): the control
  words never leave HBM.

Where the reference draws from the world's random stream, an event here draws
statelessly: the world's seed, the event's 64-bit key and a
cell's global id give the cell one 32-bit word h, u = h / 2^32.  No organism's
stream moves.  ``lowbias32`` is a bijection, so within one event no two cells
draw the same h and ranks of h need no tie rule.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

SALT_EVENT = 0x0E7E47D5
M32 = 0xFFFFFFFF


# ---- the draw ----------------------------------------------------------------

def lowbias32(x):
    """device.h lowbias32 over a numpy uint32 array (or an int)"""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def event_base(seed, key):
    """the part of the draw every cell of event `key` shares (device.h event_base)"""
    seed, key = int(seed), int(key)
    seed_lo, seed_hi = seed & M32, (seed >> 32) & M32
    key_lo, key_hi = key & M32, (key >> 32) & M32
    a = int(lowbias32((key_hi * 0x85EBCA6B + seed_hi) & M32))
    b = int(lowbias32(a ^ key_lo ^ SALT_EVENT))
    return int(lowbias32((b + seed_lo) & M32))


def event_draw(seed, key, cells):
    """h of the (global) cell ids `cells` in event `key` of a world seeded
    `seed` (avgpu_update_stats.seed): numpy uint32"""
    cells = np.asarray(cells, dtype=np.uint64) & np.uint64(M32)
    return lowbias32(np.uint64(event_base(seed, key)) ^ cells)


def _check_p(p):
    p = float(p)
    if not 0.0 <= p <= 1.0:          # (NaN fails both comparisons)
        raise ValueError(f"kill probability {p} outside [0, 1]")
    return p


def _below(h, p):
    """u < p, u = h 2^-32 (exact in doubles)"""
    return h.astype(np.float64) * 2.0 ** -32 < p


# ---- the specification ---------------------------------------------------------

def kill_prob(alive, seed, key, p):
    """cActionKillProb::Process (actions/PopulationActions.cc:1181-1185): every
    occupied cell dies when P(p) says so -- here u < p of the cell's draw"""
    alive = np.asarray(alive, dtype=bool)
    h = event_draw(seed, key, np.arange(len(alive)))
    return np.flatnonzero(alive & _below(h, _check_p(p)))


def rect_cells(world_x, world_y, x1, y1, x2, y2):
    """the cells cActionKillRectangle visits, ascending: its constructor's
    clamps and wraps (actions/PopulationActions.cc:1770-1798), then its two
    loops (:1806-1808)"""
    x1 = min(max(x1, 0), world_x - 1)                   # :1771-1775
    x2 = min(max(x2, 0), world_x - 1)                   # :1776-1780
    y1 = min(max(y1, 0), world_y - 1)                   # :1781-1785
    y2 = min(max(y2, 0), world_y - 1)                   # :1786-1790
    if x2 < x1:                                         # :1793-1795
        x2 += world_x
    if y2 < y1:                                         # :1796-1798
        y2 += world_y
    rows = (np.arange(y1, y2 + 1, dtype=np.int64) % world_y) * world_x
    cols = np.arange(x1, x2 + 1, dtype=np.int64) % world_x
    return np.unique((rows[:, None] + cols[None, :]).ravel())


def kill_rect(alive, world_x, world_y, x1=0, y1=0, x2=0, y2=0):
    """cActionKillRectangle::Process (:1803-1812): the occupied cells of the rectangle"""
    alive = np.asarray(alive, dtype=bool)
    if len(alive) != world_x * world_y:
        raise ValueError("the alive mask is not WORLD_X x WORLD_Y cells")
    cells = rect_cells(world_x, world_y, x1, y1, x2, y2)
    return cells[alive[cells]]


def kill_genotypes(alive, gkeys, seed, key, keys, p=1.0):
    """The living cells whose genotype key is among `keys`, each with
    probability p from kill_prob's draw: cActionKillDominantGenotype (:1249-1255,
    p = 1, the dominant's key), cActionProbKillSequence (:1289-1296: genome
    equal AND P(p)), and SerialTransfer's "ignore deads" loop
    (main/cPopulation.cc:7559-7564, p = 1, the keys of test fitness 0)"""
    alive = np.asarray(alive, dtype=bool)
    listed = np.isin(np.asarray(gkeys, dtype=np.uint64), np.asarray(list(keys), dtype=np.uint64))
    h = event_draw(seed, key, np.arange(len(alive)))
    return np.flatnonzero(alive & listed & _below(h, _check_p(p)))


def keep_sample(alive, seed, key, keep):
    """The removal loops of cPopulation::SerialTransfer (main/cPopulation.cc:
    7568-7584: swap-remove draws from the pool of occupied cells until `keep`
    are left) and cActionApplyBottleneck (actions/PopulationActions.cc:
    1211-1222: rejection draws over all cells): both leave a uniform sample of
    min(keep, living) survivors.  Here the survivors are the living cells with
    the `keep` smallest h -- the ranks of distinct uniform words are a uniform
    sample without replacement as well."""
    if keep < 0:
        raise ValueError("keep < 0")
    alive = np.asarray(alive, dtype=bool)
    living = np.flatnonzero(alive)
    if keep >= len(living):                             # :7568 / num_to_kill <= 0
        return living[:0]
    h = event_draw(seed, key, living)
    order = np.argsort(h, kind="stable")                # (no ties: lowbias32 is a bijection)
    return np.sort(living[order[keep:]])


# ---- the two routes ------------------------------------------------------------

def on_device(world):
    """does `world` decide the events on the device?"""
    return getattr(world, "p", None) == "avgpu_" and hasattr(world.lib, "avgpu_kill_cells")


def world_seed(world):
    """the seed the world's statistics report (avgpu_update_stats.seed): the
    one the device draws with, on either backend"""
    st = capi.AvgpuUpdateStats()
    capi.call(world.lib, world.p, "get_stats", world.h, C.byref(st))
    return int(st.seed) or int(world.cfg.seed)      # (a world that has run no update reports 0: the configured seed)


def alive_mask(world):
    """(alive, genotype keys) from the census: alive means genome_length > 0"""
    census = world.census()
    return census["genome_length"] > 0, census["genotype_key"]


def _kill_each(world, cells):
    for c in cells:
        world.kill(int(c))
    return len(cells)


def kill_cells(world, cells, device=None):
    """kill the listed cells (any order, duplicates allowed); returns the
    living organisms killed"""
    cells = np.ascontiguousarray(cells, dtype=np.int64).ravel()
    if not (on_device(world) if device is None else device):
        if len(cells) and (cells.min() < 0 or cells.max() >= world.ncells):
            raise ValueError("a cell outside the world")
        alive, _ = alive_mask(world)
        victims = np.unique(cells)
        return _kill_each(world, victims[alive[victims]])
    killed = C.c_int64()
    capi.call(world.lib, "avgpu_", "kill_cells", world.h, cells.ctypes.data_as(C.c_void_p), len(cells), C.byref(killed))
    return killed.value


def _run(world, name, spec, device, *args):
    """avgpu_`name`(*args) on the device, else spec(alive, keys) killed cell by cell"""
    if not (on_device(world) if device is None else device):
        alive, gkeys = alive_mask(world)
        return _kill_each(world, spec(alive, gkeys))
    killed = C.c_int64()
    capi.call(world.lib, "avgpu_", name, world.h, *args, C.byref(killed))
    return killed.value


def apply_kill_prob(world, p, key, device=None):
    return _run(world, "kill_prob", lambda a, g: kill_prob(a, world_seed(world), key, p), device,
                C.c_double(_check_p(p)), C.c_uint64(key))


def apply_kill_rect(world, x1=0, y1=0, x2=0, y2=0, device=None):
    wx, wy = world.cfg.world_x, world.cfg.world_y
    return _run(world, "kill_rect", lambda a, g: kill_rect(a, wx, wy, x1, y1, x2, y2), device,
                int(x1), int(y1), int(x2), int(y2))


def apply_kill_genotypes(world, keys, p, key, device=None):
    keys = np.ascontiguousarray(list(keys), dtype=np.uint64)
    return _run(world, "kill_genotypes",
                lambda a, g: kill_genotypes(a, g, world_seed(world), key, keys, p), device,
                keys.ctypes.data_as(C.c_void_p), len(keys), C.c_double(_check_p(p)), C.c_uint64(key))


def apply_keep_sample(world, keep, key, device=None):
    if keep < 0:
        raise ValueError("keep < 0")
    return _run(world, "keep_sample", lambda a, g: keep_sample(a, world_seed(world), key, keep), device,
                C.c_int64(keep), C.c_uint64(key))


def last_timing(world):
    """(device ms, control words read) of the last event call on the device"""
    ms, cells = C.c_double(), C.c_int64()
    capi.call(world.lib, "avgpu_", "last_event_ms", world.h, C.byref(ms), C.byref(cells))
    return ms.value, cells.value


# ---- SerialTransfer's "ignore deads" leg -----------------------------------------

def dead_genotype_keys(world, iset, cap=None):
    """(keys, unsequenced): the genotype keys among the living whose genome has
    test fitness 0 (cPopulation::SerialTransfer, main/cPopulation.cc:7559-7564:
    GetTestFitness == 0.0), and the number of genotypes left alone because no
    sequence could be had for them.  A genotype's sequence is obtained as
    population.save_population obtains it: the birth_length-site prefix of a
    member's memory that still hashes to the key; a genotype all of whose
    members have copied into their own first sites has none."""
    from . import systematics
    cap = cap or capi.MAX_GENOME
    alive, gkeys = alive_mask(world)
    st, ops, _ = world.states(0, len(alive), cap)
    handlers = iset.handlers
    seqs = {}
    for c in np.flatnonzero(alive).tolist():
        k = int(gkeys[c])
        if seqs.get(k) is None:
            prefix = ops[c * cap:c * cap + st[c].birth_length]
            seqs[k] = prefix if systematics.genome_key(bytes(handlers[x] for x in prefix)) == k else None
    have = [(k, g) for k, g in sorted(seqs.items()) if g is not None]
    dead = []
    if have:
        res = world.test_genomes([g for _, g in have])
        dead = [k for (k, _), r in zip(have, res) if r[0].fitness == 0.0]
    return dead, len(seqs) - len(have)
