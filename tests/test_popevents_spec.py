"""The specification of the population events (avida_amd/popevents.py): the
rectangle against a literal restatement of cActionKillRectangle's constructor
and loops (actions/PopulationActions.cc:1762-1812), the sample's sizes, the
draw shared by the keyed and the unkeyed kill, its distinctness and uniformity,
and a Driver run on the oracle backend whose population after every event is
the specification's."""
import math
import os
import shutil

import numpy as np
import pytest

from avida_amd import driver, popevents
import oracle_lib as ol

SEED = 101


def literal_rectangle(world_x, world_y, m_x1, m_y1, m_x2, m_y2):
    """cActionKillRectangle, statement for statement"""
    if m_x1 < 0:
        m_x1 = 0
    elif m_x1 > world_x - 1:
        m_x1 = world_x - 1
    if m_x2 < 0:
        m_x2 = 0
    elif m_x2 > world_x - 1:
        m_x2 = world_x - 1
    if m_y1 < 0:
        m_y1 = 0
    elif m_y1 > world_y - 1:
        m_y1 = world_y - 1
    if m_y2 < 0:
        m_y2 = 0
    elif m_y2 > world_y - 1:
        m_y2 = world_y - 1
    if m_x2 < m_x1:
        m_x2 = m_x2 + world_x
    if m_y2 < m_y1:
        m_y2 = m_y2 + world_y
    visited = []
    for i in range(m_y1, m_y2 + 1):
        for j in range(m_x1, m_x2 + 1):
            visited.append((i % world_y) * world_x + (j % world_x))
    return visited


RECTS = [(1, 1, 4, 3),            # inside the world
         (5, 1, 1, 3),            # crossing x = 0
         (1, 3, 4, 0),            # crossing y = 0
         (5, 4, 0, 1),            # crossing both
         (-50, 1, 3, 2), (2, -50, 3, 2), (2, 1, 900, 2), (2, 1, 3, 900), (-9, -9, 99, 99), (99, 99, -9, -9),
         (3, 0, 3, 4),            # x1 == x2
         (0, 0, 0, 0)]


@pytest.mark.parametrize("world", [(7, 5), (1, 1)])
def test_rectangle(world):
    wx, wy = world
    rnd = np.random.default_rng(3)
    for rect in RECTS:
        visited = literal_rectangle(wx, wy, *rect)
        assert len(visited) == len(set(visited)), rect          # the loops visit no cell twice
        cells = popevents.rect_cells(wx, wy, *rect)
        assert cells.tolist() == sorted(visited), rect
        for alive in (np.ones(wx * wy, dtype=bool), rnd.random(wx * wy) < 0.6, np.zeros(wx * wy, dtype=bool)):
            want = sorted(c for c in visited if alive[c])
            assert popevents.kill_rect(alive, wx, wy, *rect).tolist() == want, rect


def test_sample_sizes():
    rnd = np.random.default_rng(4)
    alive = rnd.random(500) < 0.7
    living = int(alive.sum())
    for key in (1, (9 << 32) | 4):
        for keep in (0, 1, living - 1, living, living + 3):
            dead = popevents.keep_sample(alive, SEED, key, keep)
            assert dead.tolist() == sorted(set(dead.tolist())) and alive[dead].all()
            assert living - len(dead) == min(keep, living), keep
            if 0 < keep < living:                  # the survivors hold the smallest words
                h = popevents.event_draw(SEED, key, np.arange(500))
                left = alive.copy()
                left[dead] = False
                assert h[left].max() < h[dead].min()
        assert len(popevents.keep_sample(np.zeros(40, dtype=bool), SEED, key, 3)) == 0
        assert len(popevents.keep_sample(np.zeros(0, dtype=bool), SEED, key, 0)) == 0
    with pytest.raises(ValueError):
        popevents.keep_sample(alive, SEED, 1, -1)


def test_keyed_kills_share_the_draw():
    rnd = np.random.default_rng(5)
    n = 4000
    alive = rnd.random(n) < 0.8
    gkeys = rnd.integers(1, 12, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    present = np.unique(gkeys)
    listed = [int(present[0]), int(present[3]), int(present[3]), 12345, int(present[7])]   # a duplicate, an absent key
    member = np.isin(gkeys, np.array(listed, dtype=np.uint64))
    key = (17 << 32) | 2
    assert popevents.kill_genotypes(alive, gkeys, SEED, key, listed, 1.0).tolist() == np.flatnonzero(alive & member).tolist()
    half = popevents.kill_genotypes(alive, gkeys, SEED, key, listed, 0.5)
    unkeyed = popevents.kill_prob(alive, SEED, key, 0.5)
    assert half.tolist() == [c for c in unkeyed.tolist() if member[c]]
    assert 0 < len(half) < int((alive & member).sum())
    assert len(popevents.kill_genotypes(alive, gkeys, SEED, key, [], 1.0)) == 0
    assert len(popevents.kill_prob(alive, SEED, key, 0.0)) == 0
    assert popevents.kill_prob(alive, SEED, key, 1.0).tolist() == np.flatnonzero(alive).tolist()
    for bad in (float("nan"), 1.5, -0.1):
        with pytest.raises(ValueError):
            popevents.kill_prob(alive, SEED, key, bad)


def test_distinct_draws():
    cells = np.arange(65536)
    for k in range(64):
        key = ((k * 7919) << 32) | (k * 31 + 1)
        assert len(np.unique(popevents.event_draw(SEED, key, cells))) == 65536
    # the key's halves and the seed's halves all matter
    base = popevents.event_draw(SEED, (7 << 32) | 3, cells[:64])
    for seed, key in ((SEED, (7 << 32) | 4), (SEED, (8 << 32) | 3), (SEED + 1, (7 << 32) | 3), (SEED + (1 << 32), (7 << 32) | 3)):
        assert (popevents.event_draw(seed, key, cells[:64]) != base).any()
    # the formula of DESIGN.md 3 in plain integers
    def lb(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)

    seed, key = 0xFEDCBA9876543210, 0x0123456789ABCDEF
    a = lb(((key >> 32) * 0x85EBCA6B + (seed >> 32)) & 0xFFFFFFFF)
    b = lb(a ^ (key & 0xFFFFFFFF) ^ 0x0E7E47D5)
    c = lb((b + (seed & 0xFFFFFFFF)) & 0xFFFFFFFF)
    got = popevents.event_draw(seed, key, [0, 1, 65535, 0xFFFFFFFF])
    assert got.dtype == np.uint32 and got.tolist() == [lb(c ^ x) for x in (0, 1, 65535, 0xFFFFFFFF)]


def test_uniformity():
    """A condition on the draw: each of 12 living cells of a 15-cell world
    survives a keep_sample(4) in a third of 20000 events, every kill_prob
    fraction over 2^20 cells is its p -- all within 4.5 standard deviations of
    the binomial."""
    alive = np.ones(15, dtype=bool)
    alive[[2, 7, 11]] = False
    events = 20000
    survived = np.zeros(15, dtype=np.int64)
    for key_lo in range(events):
        left = alive.copy()
        left[popevents.keep_sample(alive, SEED, (7 << 32) | key_lo, 4)] = False
        assert left.sum() == 4
        survived += left
    sd = math.sqrt(events * (1 / 3) * (2 / 3))
    dev = np.abs(survived[alive] - events / 3) / sd
    print("keep_sample survivals", survived.tolist(), "largest deviation %.2f sd" % dev.max())
    assert (survived[~alive] == 0).all() and dev.max() < 4.5
    n = 1 << 20
    everyone = np.ones(n, dtype=bool)
    for p in (0.9, 0.5, 0.001):
        frac = len(popevents.kill_prob(everyone, SEED, (7 << 32) | 3, p)) / n
        sd_p = math.sqrt(p * (1 - p) / n)
        print("kill_prob p = %g: fraction %.6f, %.2f sd" % (p, frac, abs(frac - p) / sd_p))
        assert abs(frac - p) < 4.5 * sd_p


# ---- the driver ----------------------------------------------------------------

EVENTS = ("u begin InjectAll default-heads.org\n"
          "u 0:1:end PrintCountData\n"
          "u 10 KillProb 0.5\n"
          "u 15 KillRectangle 14 14 1 1\n"
          "u 20 SerialTransfer 20 0\n"
          "u 30 Exit\n")


def make_config(golden, path):
    path.mkdir()
    with open(os.path.join(golden, "heads_default_100u", "avida.cfg")) as f:
        (path / "avida.cfg").write_text(f.read() + "\nWORLD_X 16\nWORLD_Y 16\n")
    shutil.copy(os.path.join(golden, "instset-heads.cfg"), path / "instset-heads.cfg")
    shutil.copy(os.path.join(golden, "environment-logic9.cfg"), path / "environment.cfg")
    shutil.copy(os.path.join(golden, "default-heads.org"), path / "default-heads.org")
    (path / "events.cfg").write_text(EVENTS)


class WatchingDriver(driver.Driver):
    """records the alive masks and genotype keys around every population event"""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.seen = []

    def _population_event(self, action, args):
        before, gkeys = popevents.alive_mask(self.world)
        key = (max(self.update, 0) << 32) | self.event_index
        super()._population_event(action, args)
        self.seen.append((action, self.update, key, before, gkeys, popevents.alive_mask(self.world)[0]))


def check_driver_run(d, data_dir):
    """the run of EVENTS: every event killed the specification's set, and count.dat shows it"""
    assert d.run() == 30
    assert [(a, u, k) for a, u, k, *_ in d.seen] == [("KillProb", 10, (10 << 32) | 2), ("KillRectangle", 15, (15 << 32) | 3),
                                                    ("SerialTransfer", 20, (20 << 32) | 4)]
    rows = {int(r.split()[0]): [int(x) for x in r.split()[:9]]
            for r in open(os.path.join(data_dir, "count.dat")) if r.strip() and r[0] != "#"}
    assert sorted(rows) == list(range(31))
    for action, u, key, before, gkeys, after in d.seen:
        if action == "KillProb":
            dead = popevents.kill_prob(before, SEED, key, 0.5)
        elif action == "KillRectangle":
            dead = popevents.kill_rect(before, 16, 16, 14, 14, 1, 1)
            assert set(dead.tolist()) <= {y * 16 + x for y in (14, 15, 0, 1) for x in (14, 15, 0, 1)}
        else:
            dead = popevents.keep_sample(before, SEED, key, 20)
            assert int(after.sum()) == 20
        want = before.copy()
        want[dead] = False
        assert len(dead) > 0 and (after == want).all(), action
        # count.dat, columns 3 and 9: the organisms at the end of an update, its births
        assert rows[u][2] == int(before.sum())
        assert rows[u + 1][2] <= rows[u][2] - len(dead) + rows[u + 1][8] and rows[u + 1][2] < rows[u][2], action


def test_driver_on_the_oracle(golden, tmp_path):
    make_config(golden, tmp_path / "config")
    d = WatchingDriver(str(tmp_path / "config"), str(tmp_path / "data"),
                       make_world=lambda cfg, iset, env: ol.Backend("oracle", cfg, iset, env))
    try:
        assert not popevents.on_device(d.world) and popevents.world_seed(d.world) == SEED
        check_driver_run(d, str(tmp_path / "data"))
    finally:
        d.world.close()


def test_driver_keyed_events(golden, tmp_path):
    """KillDominantGenotype, SerialTransfer with ignore_deads and KillProbSequence on the oracle backend"""
    from avida_amd import files, systematics
    make_config(golden, tmp_path / "config")
    iset = driver.load_config(str(tmp_path / "config"))[1]          # the instruction set of the run's avida.cfg
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    (tmp_path / "config" / "events.cfg").write_text(
        "u begin InjectAll default-heads.org\n"
        "u 14 KillProbSequence %s 0.5\n"
        "u 16 KillDominantGenotype\n"
        "u 18 SerialTransfer 5 1\n"
        "u 20 Exit\n" % iset.to_sequence(anc))
    d = WatchingDriver(str(tmp_path / "config"), str(tmp_path / "data"),
                       make_world=lambda cfg, iset, env: ol.Backend("oracle", cfg, iset, env))
    try:
        assert d.arbiter is not None                       # KillDominantGenotype needs the dominant
        assert d.run() == 20
        anc_key = systematics.genome_key(bytes(iset.handlers[x] for x in anc))
        (a1, u1, k1, b1, g1, after1), (a2, u2, k2, b2, g2, after2), (a3, u3, k3, b3, g3, after3) = d.seen
        assert (a1, u1, a2, u2, a3, u3) == ("KillProbSequence", 14, "KillDominantGenotype", 16, "SerialTransfer", 18)
        dead = popevents.kill_genotypes(b1, g1, SEED, k1, [anc_key], 0.5)
        assert 0 < len(dead) < int((b1 & (g1 == np.uint64(anc_key))).sum())
        assert np.flatnonzero(b1 & ~after1).tolist() == dead.tolist()
        # the dominant: the most abundant key among the living before the event
        keys, counts = np.unique(g2[b2], return_counts=True)
        gone = np.unique(g2[b2 & ~after2])
        assert len(gone) == 1 and counts[keys == gone[0]][0] == counts.max()
        assert not (after2 & (g2 == gone[0])).any() and (after2 == (b2 & (g2 != gone[0]))).all()
        # the transfer: the sterile genotypes go first, then 5 of the rest stay
        assert (after3 <= b3).all() and int(after3.sum()) == 5
        # (mutants that wrote into their own first sites show no birth genome: left alone, and counted)
        print("genotypes without a sequence at the transfer:", d.unsequenced)
        assert 0 <= d.unsequenced < len(np.unique(g3[b3]))
        sterile, _ = popevents.dead_genotype_keys(d.world, d.iset)
        assert sterile == []                               # whoever stayed and shows its genome has a test fitness
    finally:
        d.world.close()
