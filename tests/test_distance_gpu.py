"""avgpu_genome_distances, avgpu_cell_distances and avgpu_site_histogram on the
device against the specification (avida_amd.distance: spec_hamming, spec_edit,
spec_edit_fast, spec_site_histogram; held to a textbook Levenshtein in
test_distance_spec.py).  Every device result is an integer: equality is exact.

The pair lengths put the sites spread over the lanes, m, on both sides of
every column count the systolic wave is built for (C = ceil(m / 64) in 1, 2,
4, 8, 16, 32: m = 64 | 65, 128 | 129, 320 | 321 inside C = 8, 1024 | 1025,
2047 | 2048 the last) and the rows, n, on both sides of the 63-step pipeline
fill.  The cell worlds are checked after 3 updates, as the tapes then carry
copied / executed flags, and again after 20, when the 100-site ancestors have
divided (their gestation takes 13 updates) and offspring sit in the cells."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from avida_amd import capi, distance, driver, files
import oracle_lib as ol
import parity_util as pu
from test_distance_spec import FILES, make_config

pytestmark = pytest.mark.gpu

LENS = (1, 2, 63, 64, 65, 127, 128, 129, 320, 321, 1023, 1024, 1025, 2047, 2048)
MAXG = capi.MAX_GENOME


@pytest.fixture(scope="module")
def setup(golden):
    iset, env, cfg = pu.load_env(golden, "instset-heads.cfg", {"WORLD_X": 16, "WORLD_Y": 16}, seed=23)
    gpu = ol.Backend("gpu", cfg, iset, env, ncells=256)
    yield gpu, iset, env, cfg
    gpu.close()


def rand_genome(rnd, n, alphabet=3):
    return bytes(rnd.randrange(alphabet) for _ in range(n))


def mutate(rnd, g, kind, k):
    g = bytearray(g)
    for _ in range(k):
        p = rnd.randrange(len(g))
        if kind == "sub":
            g[p] = (g[p] + 1 + rnd.randrange(2)) % 3
        elif kind == "ins":
            g.insert(p, rnd.randrange(3))
        elif len(g) > 1:
            del g[p]
    return bytes(g)


def build_pairs():
    """(genomes, pairs): the batch of the pairs test"""
    rnd = random.Random(77)
    genomes, pairs = [], []

    def add(a, b):
        genomes.extend([a, b])
        pairs.append((len(genomes) - 2, len(genomes) - 1))

    ga = {n: rand_genome(rnd, n) for n in LENS}
    gb = {n: rand_genome(rnd, n) for n in LENS}
    for la in LENS:                                   # every length pair
        for lb in LENS:
            add(ga[la], gb[lb])
    for n in LENS:                                    # each length against a mutated copy of itself
        for kind in ("sub", "ins", "del"):
            for k in (1, 2, 3):
                if kind == "ins" and n + k > MAXG:
                    continue
                add(ga[n], mutate(rnd, ga[n], kind, k))
        add(ga[n], ga[n])                             # equal pairs
    g = rand_genome(rnd, 16, 26)
    for a, b in [(g, g[:9]), (g, g[5:]), (b"\1" * 3, b"\1" * 5), (b"\1" * 5, b"\1" * 3),   # the trimming cases
                 (b"\0" * 4, b"\1" * 6), (g[:8] + b"\2" + g[8:], g)]:
        add(a, b)
    add(ga[1], gb[2048])                              # 1 site against 2048, both ways
    add(gb[2048], ga[1])
    pairs.append(pairs[LENS.index(321) * len(LENS) + LENS.index(1025)])    # a pair repeated ...
    a, b = pairs[-1]
    pairs.append((b, a))                              # ... and in the other order
    for _ in range(1100):                             # the bulk: short genomes over 2, 3 and 26 ops
        alpha = rnd.choice((2, 3, 26))
        add(rand_genome(rnd, rnd.randint(1, 130), alpha), rand_genome(rnd, rnd.randint(1, 130), alpha))
    return genomes, pairs


@pytest.fixture(scope="module")
def batch(setup):
    """the batch, its specification and the device's joint answer, computed once"""
    gpu = setup[0]
    genomes, pairs = build_pairs()
    full = sum(1 for i, j in pairs if len(genomes[i]) == len(genomes[j]) == MAXG)
    assert 1400 <= len(pairs) <= 1600 and 1 <= full <= 8, (len(pairs), full)
    memo = {}
    ham, edit = [], []
    for i, j in pairs:
        a, b = genomes[i], genomes[j]
        ham.append(distance.spec_hamming(a, b))
        key = (a, b) if a <= b else (b, a)            # (the distance is symmetric: test_distance_spec)
        if key not in memo:
            memo[key] = distance.spec_edit_fast(a, b)
        edit.append(memo[key])
    h, e = distance.pair_distances(gpu, genomes, pairs)
    timing = distance.last_timing(gpu)
    return genomes, pairs, np.array(ham, dtype=np.int32), np.array(edit, dtype=np.int32), h, e, timing


def test_pairs(batch):
    genomes, pairs, ham, edit, h, e, timing = batch
    bad_h, bad_e = np.flatnonzero(h != ham), np.flatnonzero(e != edit)
    print(f"{len(pairs)} pairs, device {timing[0]:.3f} ms; hamming mismatches {len(bad_h)}, edit {len(bad_e)}")
    for k in bad_e[:10]:
        i, j = pairs[k]
        print(f"pair {k}: lengths {len(genomes[i])} x {len(genomes[j])}: device {e[k]} specification {edit[k]}")
    assert not len(bad_h) and not len(bad_e)
    assert h.dtype == e.dtype == np.int32
    ms, npairs, cells = timing
    assert ms > 0 and (npairs, cells) == (len(pairs), 0)


def test_independence(setup, batch):
    gpu = setup[0]
    genomes, pairs, _ham, _edit, h, e, _ = batch
    k = LENS.index(321) * len(LENS) + LENS.index(1025)
    i, j = pairs[k]
    h1, e1 = distance.pair_distances(gpu, [genomes[i], genomes[j]], [(0, 1)])
    assert (int(h1[0]), int(e1[0])) == (int(h[k]), int(e[k]))
    assert distance.last_timing(gpu)[1:] == (1, 0)
    h_only, none = distance.pair_distances(gpu, genomes, pairs, edit=False)
    assert none is None and h_only.tobytes() == h.tobytes()
    none, e_only = distance.pair_distances(gpu, genomes, pairs, hamming=False)
    assert none is None and e_only.tobytes() == e.tobytes()
    ht, et = distance.to_reference(gpu, [genomes[j], genomes[i]], genomes[i])
    assert (int(ht[0]), int(et[0]), int(ht[1]), int(et[1])) == (int(h[k]), int(e[k]), 0, 0)


# ---- cells and the histogram -------------------------------------------------

def padded(anc, iset, n):
    return anc[:50] + bytes([iset.op_of_name("nop-C")]) * (n - len(anc)) + anc[50:]


def make_world(golden, setup, side, seed):
    """a side x side world set with genomes of 1, 50, 100, 321 and 2048 sites, some cells killed"""
    _, iset, env, _ = setup
    _, _, cfg = pu.load_env(golden, "instset-heads.cfg", {"WORLD_X": side, "WORLD_Y": side}, seed=seed)
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    kinds = [anc[:1], anc[:50], anc, padded(anc, iset, 321), padded(anc, iset, 2048)]
    assert [len(g) for g in kinds] == [1, 50, 100, 321, 2048]
    n = side * side
    rnd = random.Random(seed)
    w = ol.Backend("gpu", cfg, iset, env, ncells=n)
    # (equal merits: the 100-site ancestors get their 30 instructions an update beside the 2048-site organisms)
    w.set_orgs(0, [kinds[2] if rnd.random() < 0.5 else kinds[rnd.randrange(5)] for _ in range(n)], [100.0] * n,
               deterministic=False)
    for c in sorted(set(rnd.sample(range(n), n // 8) + [0, n - 1])):
        w.kill(c)
    return w, kinds


def check_cells(w, kinds, empties):
    n = w.ncells
    st, _, _ = w.states(0, n)
    alive = np.array([bool(st[c].alive) for c in range(n)])
    assert alive.any() and (not empties or not alive.all())
    for ref in (kinds[2], kinds[4]):
        h, e = distance.cell_distances(w, ref)
        assert distance.last_timing(w)[1:] == (0, n) and distance.last_timing(w)[0] > 0
        sh, se = distance.cell_distances(w, ref, device=False)      # the specification over world.states
        assert (h[~alive] == -1).all() and (e[~alive] == -1).all() and (h[alive] >= 0).all()
        assert h.tobytes() == sh.tobytes() and e.tobytes() == se.tobytes()
        for first in (0, 1, n - 1):
            h1, e1 = distance.cell_distances(w, ref, first, 1)
            assert (int(h1[0]), int(e1[0])) == (int(h[first]), int(e[first]))
        h_only, _ = distance.cell_distances(w, ref, edit=False)
        _, e_only = distance.cell_distances(w, ref, hamming=False)
        assert h_only.tobytes() == h.tobytes() and e_only.tobytes() == e.tobytes()
    return int(alive.sum())


def check_hist(w, n_ops, living):
    hist, n = distance.site_histogram(w)
    spec, sn = distance.site_histogram(w, n_ops=n_ops, device=False)
    assert n == sn == living
    assert hist.dtype == np.int32 and hist.shape == (MAXG, capi.MAX_INST + 1)
    assert hist.tobytes() == spec.tobytes()
    assert (hist.sum(axis=1) == living).all()
    again, n2 = distance.site_histogram(w)
    assert again.tobytes() == hist.tobytes() and n2 == n
    assert distance.last_timing(w)[1:] == (0, w.ncells)
    return hist


def test_cells_and_histogram(golden, setup):
    iset = setup[1]
    w, kinds = make_world(golden, setup, 16, seed=5)
    try:
        births = 0
        for updates in (3, 17):
            for _ in range(updates):
                births += w.run_update().births
            living = check_cells(w, kinds, empties=updates == 3)    # (births prefer the empty cells)
            hist = check_hist(w, len(iset.names), living)
            assert hist[2047, 0] < living              # the 2048-site organisms reach the last site
        assert births > 0                              # offspring sit in the cells by now
        st, _, fl = w.states(0, w.ncells)
        assert any(fl)                                 # the tapes carry copied / executed flags
        # a sub-range: its own organisms only
        part, n = distance.site_histogram(w, 64, 100)
        spec, sn = distance.site_histogram(w, 64, 100, n_ops=len(iset.names), device=False)
        assert n == sn and part.tobytes() == spec.tobytes()
    finally:
        w.close()


def test_histogram_crosses_cell_chunks(golden, setup):
    iset = setup[1]
    w, _ = make_world(golden, setup, 32, seed=6)       # 1024 cells: four chunks of 256
    try:
        for _ in range(3):
            w.run_update()
        st, _, _ = w.states(0, w.ncells)
        check_hist(w, len(iset.names), sum(1 for s in st if s.alive))
    finally:
        w.close()


# ---- the driver ----------------------------------------------------------------

class ShadowDriver(driver.Driver):
    """runs every distance action twice on the same world: the fallback over
    the world's own states into a second directory, then the driver's own"""

    def __init__(self, config_dir, data_dir, shadow_dir):
        super().__init__(config_dir, data_dir)
        self.shadow = distance.Actions(self.world, self.iset, shadow_dir, config_dir, device=False)

    def _action(self, action, args):
        if action in distance.Actions.NAMES:
            self.shadow.run(action, args, self.arbiter, max(self.update, 0))
        super()._action(action, args)


def test_driver_device_files_equal_the_fallback(golden, tmp_path):
    make_config(golden, tmp_path / "config", 30)
    d = ShadowDriver(str(tmp_path / "config"), str(tmp_path / "device"), str(tmp_path / "fallback"))
    try:
        assert distance.on_device(d.world) and d.dist.device is None
        assert d.run() == 30
        d.shadow.close()
    finally:
        d.world.close()
    for name in FILES + ("pop_distance-10.dat", "pop_distance-30.dat"):
        got = open(tmp_path / "device" / name, "rb").read()
        assert got == open(tmp_path / "fallback" / name, "rb").read(), name
        assert len(got.splitlines()) > 2, name
    rows = [l.split() for l in open(tmp_path / "device" / "consensus.dat") if l.strip() and l[0] != "#"]
    assert [r[0] for r in rows] == ["10", "30"] and all(int(r[5]) >= 90 for r in rows)     # the consensus length


# ---- the calls as calls ---------------------------------------------------------

def test_world_untouched(golden, setup):
    """calls made between queued updates leave the digests and the next
    update's statistics equal to a twin world's"""
    _, iset, env, _ = setup
    _, _, cfg = pu.load_env(golden, "instset-heads.cfg", {"WORLD_X": 16, "WORLD_Y": 16}, seed=17)
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    a = ol.Backend("gpu", cfg, iset, env, ncells=256)
    b = ol.Backend("gpu", cfg, iset, env, ncells=256)
    try:
        for w in (a, b):
            w.set_orgs(0, [anc] * 256, deterministic=False)
            for _ in range(3):
                w._call("run_update", w.h, None)              # queued: no statistics, no sync
        d0 = a.digests()
        first = distance.cell_distances(a, anc)
        assert (a.digests() == d0).all()
        for w in (a, b):
            for _ in range(2):
                w._call("run_update", w.h, None)
        hist = distance.site_histogram(a)                     # behind the two queued updates
        pd = distance.pair_distances(a, [anc, anc[:60]], [(0, 1)])
        cd = distance.cell_distances(a, anc[:60])
        sa, sb = a.run_update(), b.run_update()
        assert bytes(sa) == bytes(sb)
        assert (a.digests() == b.digests()).all()
        assert (first[0] == 0).all() and (first[1] == 0).all()
        assert hist[1] == 256 and (int(pd[0][0]), int(pd[1][0])) == (40, 40)
        assert (cd[0] == 40).all() and (cd[1] == 40).all()
    finally:
        a.close()
        b.close()


def test_refusals(setup):
    """every refusal is AVGPU_EINVAL and leaves poisoned outputs untouched; the next valid call answers"""
    gpu, iset, _, _ = setup
    lib, h = gpu.lib, gpu.h
    ni = len(iset.names)
    I32P = C.POINTER(C.c_int32)
    p = lambda a: a.ctypes.data_as(I32P)       # noqa: E731
    g = bytes([0, 1, 2, 3, 4])

    def poisoned(n):
        return np.full(n, 0x5A5A5A5A, dtype=np.int32), np.full(n, 0x5A5A5A5A, dtype=np.int32)

    def pairs_refused(world, n, genomes, lens, npairs, pa, pb, outs=(True, True)):
        blob = b"".join(genomes)
        buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(blob or b"\0")
        la, a, b = np.array(lens, dtype=np.int32), np.array(pa, dtype=np.int32), np.array(pb, dtype=np.int32)
        ho, eo = poisoned(8)
        rc = lib.avgpu_genome_distances(world, n, buf, p(la), npairs, p(a), p(b), p(ho) if outs[0] else None,
                                        p(eo) if outs[1] else None)
        assert rc == -1 and lib.avgpu_last_error(), (n, lens, npairs, pa, pb)
        assert (ho == 0x5A5A5A5A).all() and (eo == 0x5A5A5A5A).all()

    long = bytes(MAXG + 1)
    for n in (0, -1):
        pairs_refused(h, n, [g, g], [5, 5], 1, [0], [1])
    for npairs in (0, -1):
        pairs_refused(h, 2, [g, g], [5, 5], npairs, [0], [1])
    pairs_refused(h, 2, [g, g], [5, 0], 1, [0], [1])
    pairs_refused(h, 2, [g, g], [5, -2], 1, [0], [1])
    pairs_refused(h, 2, [g, long], [5, MAXG + 1], 1, [0], [1])
    pairs_refused(h, 2, [g, bytes([0, ni, 0, 0, 0])], [5, 5], 1, [0], [1])
    pairs_refused(h, 2, [g, bytes([0, 255, 0, 0, 0])], [5, 5], 1, [0], [1])
    for pa, pb in (([2], [0]), ([0], [2]), ([-1], [0]), ([0], [-1])):
        pairs_refused(h, 2, [g, g], [5, 5], 1, pa, pb)
    pairs_refused(None, 2, [g, g], [5, 5], 1, [0], [1])
    pairs_refused(h, 2, [g, g], [5, 5], 1, [0], [1], outs=(False, False))

    def cells_refused(world, first, count, ref, ref_len, outs=(True, True)):
        buf = (C.c_uint8 * max(1, len(ref))).from_buffer_copy(ref or b"\0")
        ho, eo = poisoned(512)
        rc = lib.avgpu_cell_distances(world, first, count, buf, ref_len, p(ho) if outs[0] else None,
                                      p(eo) if outs[1] else None)
        assert rc == -1 and lib.avgpu_last_error(), (first, count, ref_len)
        assert (ho == 0x5A5A5A5A).all() and (eo == 0x5A5A5A5A).all()

    for first, count in ((-1, 4), (0, 257), (255, 2), (256, 1), (0, 0), (3, -1)):
        cells_refused(h, first, count, g, 5)
    cells_refused(h, 0, 256, g, 0)
    cells_refused(h, 0, 256, long, MAXG + 1)
    cells_refused(h, 0, 256, bytes([0, ni]), 2)
    cells_refused(None, 0, 256, g, 5)
    cells_refused(h, 0, 256, g, 5, outs=(False, False))

    hist = np.full(MAXG * (capi.MAX_INST + 1), 0x5A5A5A5A, dtype=np.int32)
    living = C.c_int64(-77)
    for world, first, count in ((h, -1, 4), (h, 0, 257), (h, 255, 2), (h, 0, 0), (None, 0, 256)):
        assert lib.avgpu_site_histogram(world, first, count, p(hist), C.byref(living)) == -1
        assert (hist == 0x5A5A5A5A).all() and living.value == -77
    assert lib.avgpu_site_histogram(h, 0, 256, None, C.byref(living)) == -1 and living.value == -77
    assert lib.avgpu_last_distance_ms(None, None, None, None) == -1

    # the next valid calls still answer
    hd, ed = distance.pair_distances(gpu, [g, g[:3]], [(0, 1), (1, 1)])
    assert hd.tolist() == [2, 0] and ed.tolist() == [2, 0]
    hc, ec = distance.cell_distances(gpu, g)
    assert (hc == -1).all() and (ec == -1).all()             # the module's world is empty
    hist2, n = distance.site_histogram(gpu)
    assert n == 0 and not hist2.any()


def test_lifetime(golden, setup):
    """the scratch of all three calls goes with the world"""
    gpu, iset, env, cfg = setup
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    base = capi.live_objects(gpu.lib)
    w = ol.Backend("gpu", cfg, iset, env, ncells=256)
    w.set_orgs(0, [anc] * 16, deterministic=False)
    held = capi.live_objects(gpu.lib)
    distance.pair_distances(w, [anc, anc[:50]], [(0, 1)])
    distance.cell_distances(w, anc)
    distance.site_histogram(w)
    grown = capi.live_objects(gpu.lib)
    assert grown == held + 5                                  # three buffers, two events
    distance.pair_distances(w, [anc] * 64, [(i, 63 - i) for i in range(64)])      # the buffers grow in place
    assert capi.live_objects(gpu.lib) == grown
    w.close()
    assert capi.live_objects(gpu.lib) == base
