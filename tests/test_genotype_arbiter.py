"""The device-resident genotype arbiter (include/avida_gpu.h
avgpu_classify_genotypes).

The reference object is always a host systematics.GenotypeArbiter(threshold)
fed capi.get_genotypes of the same world at the same moments.  Every field of
the arbiter's state is an integer or copied unchanged, so agreement is exact:
np.array_equal on the per-genotype arrays, equal world-level state, equal
dominant.dat rows (types included) and the dominant's table row byte for byte.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from avida_amd import capi, driver, files, systematics
import oracle_lib as ol
import parity_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -5


# ---- CPU: the mirrors ---------------------------------------------------------
def test_arbiter_struct_layouts(tmp_path):
    src = tmp_path / "arb.c"
    src.write_text('#include "avida_gpu.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(avgpu_arbiter_row),'
                   ' sizeof(avgpu_arbiter_summary), offsetof(avgpu_arbiter_row, num_units),'
                   ' offsetof(avgpu_arbiter_summary, dominant_state),'
                   ' offsetof(avgpu_arbiter_summary, dominant)); return 0;}\n')
    exe = tmp_path / "arb"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    row, summary = capi.ARBITER_ROW_DTYPE, capi.ARBITER_SUMMARY_DTYPE
    assert got == [row.itemsize, summary.itemsize, row.fields["num_units"][1],
                   summary.fields["dominant_state"][1], summary.fields["dominant"][1]]
    assert got[:2] == [48, 232]
    assert summary.fields["dominant_state"][0] == row and summary.fields["dominant"][0] == capi.GENOTYPE_DTYPE


def test_arbiter_symbols_are_exported():
    for name in ("avgpu_classify_genotypes", "avgpu_get_arbiter", "avgpu_set_arbiter", "avgpu_reset_arbiter",
                 "avgpu_last_arbiter_ms"):
        assert name in capi.EXPORTED


def _sequence(seed):
    """the key rows of tests/test_genotype_table.py's random sequences: 20
    steps over 200 cells, keys from a pool of 30, 0 = a dead cell"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(1, 1 << 63, size=30, dtype=np.uint64) * np.uint64(2) + np.uint64(seed % 2)
    out = []
    for _ in range(20):
        allowed = pool[rng.random(30) < rng.uniform(0.1, 0.6)]
        keys = np.zeros(200, dtype=np.uint64)
        if len(allowed):
            keys = allowed[rng.integers(0, len(allowed), size=200)]
            keys[rng.random(200) < rng.uniform(0.0, 0.7)] = 0
        out.append(keys)
    return out


SEEDS = [0, 1, 2, 3, 4]


@pytest.mark.parametrize("seed", SEEDS)
def test_random_sequences_cover_the_rules(seed):
    """on the host arbiter alone: every sequence the GPU test replays holds a
    tie for the top, a removed dominant and a returning key"""
    a = systematics.GenotypeArbiter(3)
    tie = removed = back = False
    seen, prev = set(), set()
    for u, keys in enumerate(_sequence(seed)):
        c = np.zeros(200, dtype=capi.CENSUS_DTYPE)
        c["genotype_key"], c["genome_length"] = keys, 1
        t, tot = systematics.table_from_census(c)
        now = set(t["genotype_key"].tolist())
        removed |= a.best_key is not None and len(t) > 0 and a.best_key not in now
        back |= bool((now - prev) & seen)
        a.update_table(t, tot, u)
        tie |= len(t) > 0 and int((t["num_units"] == t["num_units"].max()).sum()) > 1
        seen |= now
        prev = now
    assert tie and removed and back


def test_device_arbiter_before_any_classification():
    d = systematics.DeviceGenotypeArbiter(3)
    assert d.census is None and d.num_genotypes() == 0 and d.num_threshold() == 0 and d.next_id == 1
    assert d.dominant() is None and d.dominant_row(0) is None and d.best_key is None
    assert len(d.keys) == 0 and len(d.active) == 0 and d.sz_count == {}


# ---- GPU ------------------------------------------------------------------------
class _World:
    """what DeviceGenotypeArbiter asks of a world, over a test Backend"""

    def __init__(self, b):
        self.b = b

    def classify_genotypes(self, update, threshold):
        return capi.classify_genotypes(self.b.lib, self.b.h, update, threshold)

    def arbiter_state(self):
        return capi.get_arbiter(self.b.lib, self.b.h)


def _gpu(golden, n, overrides=None, seed=7):
    import torch
    assert torch.cuda.is_available()
    iset, env, cfg = pu.load_env(golden, overrides=overrides, seed=seed)
    return ol.Backend("gpu", cfg, iset, env, ncells=n)


def _set_keys(b, keys):
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    b._call("set_genotype_keys", b.h, 0, len(k), k.ctypes.data_as(C.c_void_p))


def _fill(b, keys, lens=None):
    """every cell refilled with a one-instruction organism (or lens[i]
    instructions), the cells of key 0 killed, the keys set"""
    n = len(keys)
    b.set_orgs(0, [bytes(int(lens[i]) if lens is not None else 1) for i in range(n)])
    for c in np.flatnonzero(np.asarray(keys) == 0):
        b.kill(int(c))
    _set_keys(b, keys)


def _check_summary(s, host, totals, update, before):
    """the summary record against the host arbiter; before = (rows, next_id,
    tot_threshold) of the host ahead of this classification"""
    m = len(host.keys)
    assert int(s["update"]) == update
    assert [int(s[f]) for f in ("num_organisms", "num_genotypes", "sum_copied_size", "sum_executed_size")] == \
           [totals.num_organisms, totals.num_genotypes, totals.sum_copied_size, totals.sum_executed_size]
    assert int(s["num_genotypes"]) == m and int(s["num_threshold"]) == host.num_threshold()
    assert (int(s["tot_genotypes"]), int(s["tot_threshold"]), int(s["next_id"])) == \
           (host.tot_genotypes, host.tot_threshold, host.next_id)
    fresh = host.next_id - before[1]
    assert int(s["num_new"]) == fresh and int(s["num_gone"]) == before[0] - (m - fresh)
    assert int(s["num_crossed"]) == host.tot_threshold - before[2]
    if host.best_key is None:
        assert int(s["dominant_row"]) == -1
        return
    bj = host._index(host.best_key)
    assert int(s["dominant_row"]) == bj and int(s["dominant_state"]["genotype_key"]) == host.best_key
    assert int(s["dominant_state"]["id"]) == int(host.ids[bj])
    assert s["dominant"].tobytes() == host.table[bj].tobytes()


def _check_full(dev, host):
    for name in ("keys", "ids", "lengths", "born", "units", "total", "thr", "name_no"):
        assert np.array_equal(getattr(dev, name), getattr(host, name)), name
    assert (dev.next_id, dev.tot_genotypes, dev.tot_threshold) == (host.next_id, host.tot_genotypes, host.tot_threshold)
    assert dev.sz_count == host.sz_count and dev.best_key == host.best_key
    assert dev.table.tobytes() == host.table.tobytes()
    assert dev.num_genotypes() == host.num_genotypes() and dev.num_threshold() == host.num_threshold()


def _check_dominant_row(dev, host, update):
    dr, hr = dev.dominant_row(update), host.dominant_row(update)
    if hr is None:
        assert dr is None and dev.dominant() is None
        return
    assert len(dr) == len(hr)
    for i, (x, y) in enumerate(zip(dr, hr)):
        assert x == y and type(x) is type(y), (i, x, y)


def _step(b, dev, host, update, full=True):
    """one classification on both sides, compared"""
    before = (len(host.keys), host.next_id, host.tot_threshold)
    table, totals = capi.get_genotypes(b.lib, b.h)
    host.update_table(table, totals, update)
    s = dev.classify(_World(b), update)
    _check_summary(s, host, totals, update, before)
    _check_dominant_row(dev, host, update)
    ms, nbytes = C.c_double(-1.0), C.c_int64(-1)
    assert b.lib.avgpu_last_arbiter_ms(b.h, C.byref(ms), C.byref(nbytes)) == 0
    assert nbytes.value == capi.ARBITER_SUMMARY_DTYPE.itemsize and ms.value >= 0.0
    if full:
        _check_full(dev, host)
    return s


@pytest.mark.gpu
def test_gpu_arbiter_rule_sequence(golden):
    b = _gpu(golden, 4)
    dev, host = systematics.DeviceGenotypeArbiter(3), systematics.GenotypeArbiter(3)
    _fill(b, [7, 0, 0, 0], [100] * 4)
    _step(b, dev, host, 0)
    g7 = dev.dominant()
    assert (g7.id, g7.name, g7.num_units) == (1, "100-aaaaa", 1)
    _fill(b, [7, 9, 9, 5], [100, 100, 100, 99])
    _step(b, dev, host, 1)
    assert dev.active[9].id == 2 and dev.active[5].id == 3 and dev.dominant().key == 9
    assert dev.active[9].name == "100-aaaab" and dev.active[5].name == "099-no_name"
    assert (dev.num_genotypes(), dev.num_threshold()) == (3, 2)
    _fill(b, [5, 5, 5, 9], [100] * 4)
    s = _step(b, dev, host, 2)
    assert 7 not in dev.active and dev.active[5].name == "099-aaaaa" and dev.dominant().key == 5
    assert int(s["num_gone"]) == 1 and int(s["num_crossed"]) == 1
    assert g7.num_units == 1                                          # a snapshot of the classification it came from
    _fill(b, [5, 5, 9, 9], [100] * 4)
    _step(b, dev, host, 3)
    assert dev.dominant().key == 5                                    # tie: the dominant stays
    _fill(b, [0, 0, 0, 0], [100] * 4)
    s = _step(b, dev, host, 4)
    assert dev.dominant() is None and dev.num_genotypes() == 0 and dev.dominant_row(4) is None
    assert int(s["num_gone"]) == 2
    _fill(b, [7, 0, 0, 0], [100] * 4)
    _step(b, dev, host, 5)
    assert dev.active[7].id == 4 and dev.active[7].update_born == 5 and dev.tot_genotypes == 4
    assert dev.active[7].name == "100-aaaac"
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_gpu_arbiter_shapes(golden, n):
    """three classifications per world with key pools of 1, n/4 and n,
    re-drawn in between: matches, new rows and removals on both sides of every
    wave and tile boundary"""
    rng = np.random.default_rng(n)
    b = _gpu(golden, n)
    b.set_orgs(0, [bytes(1)] * n)
    for c in np.flatnonzero(rng.random(n) < 1.0 / 3.0):
        b.kill(int(c))
    dev, host = systematics.DeviceGenotypeArbiter(3), systematics.GenotypeArbiter(3)
    old = np.zeros(0, dtype=np.uint64)
    for u, pool in enumerate((1, max(1, n // 4), n)):
        kept = old[:pool // 2]                            # half of the new pool are keys of the last round
        drawn = rng.integers(1, 1 << 62, size=pool - len(kept), dtype=np.uint64) * np.uint64(4) + np.uint64(u + 1)
        keys = np.concatenate([kept, drawn])
        assert len(np.unique(keys)) == pool
        cell_keys = keys[rng.permutation(n) % pool] if pool == n else keys[rng.integers(0, pool, size=n)]
        _set_keys(b, cell_keys)
        _step(b, dev, host, u)
        old = keys
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_arbiter_random_sequences(golden, seed):
    b = _gpu(golden, 200)
    dev, host = systematics.DeviceGenotypeArbiter(3), systematics.GenotypeArbiter(3)
    for u, keys in enumerate(_sequence(seed)):
        _fill(b, keys)
        _step(b, dev, host, u)
    b.close()


@pytest.mark.gpu
def test_gpu_arbiter_many_tiles(golden):
    """150000 cells: 1000 keys, then all-distinct keys at threshold 1 (145 k
    new rows, every one crossing: ids and names run over many blocks), then
    half of those replaced (72 k removals and 72 k new rows interleaved), then
    one key"""
    n = 150000
    rng = np.random.default_rng(5)
    b = _gpu(golden, n)
    b.set_orgs(0, [bytes(1)] * 70000)
    b.set_orgs(75000, [bytes(1)] * 75000)
    for c in rng.integers(0, 70000, size=10):
        b.kill(int(c))
    dev, host = systematics.DeviceGenotypeArbiter(3), systematics.GenotypeArbiter(3)
    pool = rng.integers(1, 1 << 63, size=1000, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    _set_keys(b, pool[rng.integers(0, 1000, size=n)])
    _step(b, dev, host, 0)
    distinct = rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
    distinct[distinct == 0] = 1
    assert len(np.unique(distinct)) == n
    _set_keys(b, distinct)
    dev.threshold = host.threshold = 1
    s = _step(b, dev, host, 1)
    assert int(s["num_new"]) > 144000 and int(s["num_crossed"]) == int(s["num_new"]) and int(s["num_gone"]) == 1000
    dev.threshold = host.threshold = 3
    half = distinct.copy()
    swap = rng.random(n) < 0.5
    half[swap] = (np.arange(n, dtype=np.uint64)[swap] + np.uint64(n)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
    assert len(np.unique(half)) == n
    _set_keys(b, half)
    s = _step(b, dev, host, 2)
    assert int(s["num_new"]) > 70000 and int(s["num_gone"]) == int(s["num_new"])
    _set_keys(b, np.full(n, half[3], dtype=np.uint64))
    s = _step(b, dev, host, 3)
    assert int(s["num_genotypes"]) == 1 and int(s["num_gone"]) > 144000
    b.close()


@pytest.mark.gpu
def test_gpu_arbiter_free_running_world(golden):
    """seed 11, one ancestor, 200 updates, classified after every update"""
    iset, env, cfg = pu.load_env(golden, seed=11)
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    n = cfg.world_x * cfg.world_y
    b = _gpu(golden, n, seed=11)
    b.set_orgs(n // 2 + cfg.world_x // 2, [anc], deterministic=False)
    dev, host = systematics.DeviceGenotypeArbiter(3), systematics.GenotypeArbiter(3)
    gone = crossed = changes = 0
    last = None
    for u in range(1, 201):
        b.run_update()
        s = _step(b, dev, host, u, full=u in (50, 100, 200))
        gone += int(s["num_gone"])
        crossed += int(s["num_crossed"])
        changes += last is not None and dev.best_key != last
        last = dev.best_key
    assert gone > 0 and crossed > 0 and changes > 0
    b.close()


@pytest.mark.gpu
def test_gpu_arbiter_stream_order_and_purity(golden):
    iset, env, cfg = pu.load_env(golden, seed=11)
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    n = cfg.world_x * cfg.world_y
    worlds = []
    for _ in range(2):
        b = _gpu(golden, n, seed=11)
        b.set_orgs(0, [anc] * 40, deterministic=False)
        for _ in range(60):
            b.run_update()
        worlds.append(b)
    b, b2 = worlds
    dev, host = systematics.DeviceGenotypeArbiter(3), systematics.GenotypeArbiter(3)
    twin = systematics.DeviceGenotypeArbiter(3)
    _step(b, dev, host, 60)
    twin.classify(_World(b2), 60)
    before = b.census()
    for w in worlds:
        for _ in range(5):
            assert w.lib.avgpu_run_update(w.h, None) == 0, w.lib.avgpu_last_error().decode()
    s = dev.classify(_World(b), 65)                       # behind the queued updates
    s2 = twin.classify(_World(b2), 65)
    after, dig = b.census(), b.digests()
    assert not np.array_equal(before, after)
    table, totals = capi.get_genotypes(b.lib, b.h)
    pre = (len(host.keys), host.next_id, host.tot_threshold)
    host.update_table(table, totals, 65)
    _check_summary(s, host, totals, 65, pre)
    _check_full(dev, host)
    # purity: the updates have drained (the snapshot above); one more classification leaves the
    # cells' digests (state, tape, random stream position), the census and the statistics as they were
    stats = capi.AvgpuUpdateStats()
    b._call("get_stats", b.h, C.byref(stats))
    stats = bytes(stats)
    s3 = dev.classify(_World(b), 66)
    twin.classify(_World(b2), 66)
    assert np.array_equal(b.digests(), dig) and np.array_equal(b.census(), after)
    again = capi.AvgpuUpdateStats()
    b._call("get_stats", b.h, C.byref(again))
    assert bytes(again) == stats
    assert (int(s3["num_new"]), int(s3["num_gone"]), int(s3["num_genotypes"])) == (0, 0, len(host.keys))
    pre = (len(host.keys), host.next_id, host.tot_threshold)
    host.update_table(table, totals, 66)
    _check_summary(s3, host, totals, 66, pre)
    _check_full(dev, host)
    s, s2 = dev.summary, twin.summary
    # two worlds built alike: identical bytes
    assert s2.tobytes() == s.tobytes()
    assert twin.rows.tobytes() == dev.rows.tobytes() and twin.table.tobytes() == dev.table.tobytes()
    assert twin.sz_count == dev.sz_count
    for w in worlds:
        w.close()
    # the bytes that cross: the summary alone, on a 600-cell world
    rng = np.random.default_rng(3)
    c = _gpu(golden, 600)
    _fill(c, rng.integers(0, 40, size=600).astype(np.uint64))
    _step(c, systematics.DeviceGenotypeArbiter(3), systematics.GenotypeArbiter(3), 0)
    c.close()


@pytest.mark.gpu
def test_gpu_arbiter_get_set_reset(golden):
    seqs = _sequence(1)
    a, b = _gpu(golden, 200), _gpu(golden, 200)
    dev, host = systematics.DeviceGenotypeArbiter(3), systematics.GenotypeArbiter(3)
    for u in range(10):
        _fill(a, seqs[u])
        _step(a, dev, host, u)
    rows, table, summary, sz = capi.get_arbiter(a.lib, a.h)
    assert rows.tobytes() == dev.rows.tobytes() and table.tobytes() == host.table.tobytes()
    lib = a.lib
    # one row short: refused with the count, the buffers untouched
    m = len(rows)
    assert m > 1
    r2 = np.zeros(m, dtype=capi.ARBITER_ROW_DTYPE)
    t2 = np.zeros(m, dtype=capi.GENOTYPE_DTYPE)
    r2["num_units"], t2["num_units"] = -7, -7
    rc = lib.avgpu_get_arbiter(a.h, r2.ctypes.data_as(C.c_void_p), t2.ctypes.data_as(C.c_void_p), m - 1, None, None)
    assert rc == EINVAL and str(m) in lib.avgpu_last_error().decode()
    assert (r2["num_units"] == -7).all() and (t2["num_units"] == -7).all()
    assert lib.avgpu_get_arbiter(a.h, r2.ctypes.data_as(C.c_void_p), None, m, None, None) == m
    assert r2.tobytes() == rows.tobytes() and (t2["num_units"] == -7).all()
    # hand-over: the second world takes the state and continues alike
    capi.set_arbiter(b.lib, b.h, rows, summary, sz)
    dev_b = systematics.DeviceGenotypeArbiter(3)
    dev_b.attach(_World(b))
    assert dev_b.rows.tobytes() == rows.tobytes() and dev_b.next_id == host.next_id
    assert dev_b.best_key == host.best_key and dev_b.sz_count == host.sz_count
    import copy
    host_b = copy.deepcopy(host)
    for u in range(10, 20):
        _fill(a, seqs[u])
        _fill(b, seqs[u])
        _step(a, dev, host, u)
        _step(b, dev_b, host_b, u)
        assert dev_b.rows.tobytes() == dev.rows.tobytes() and dev_b.summary.tobytes() == dev.summary.tobytes()
    # refusals leave the state as it was
    state = capi.get_arbiter(b.lib, b.h)
    bad = state[0].copy()
    bad["genotype_key"][[0, 1]] = bad["genotype_key"][[1, 0]]
    for rows_bad in (bad, np.concatenate([np.zeros(1, dtype=capi.ARBITER_ROW_DTYPE), state[0]])):
        rc = lib.avgpu_set_arbiter(b.h, len(rows_bad), rows_bad.ctypes.data_as(C.c_void_p),
                                   np.asarray(state[2]).reshape(1).ctypes.data_as(C.c_void_p), None)
        assert rc == EINVAL and "ascending" in lib.avgpu_last_error().decode()
        again = capi.get_arbiter(b.lib, b.h)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again, state))
    for field, value in (("genome_length", capi.MAX_GENOME + 1), ("genome_length", -1), ("name_no", -1),
                         ("num_units", -1), ("total_units", -1), ("id", 0), ("id", int(state[2]["next_id"]))):
        bad = state[0].copy()
        bad[field][1] = value
        rc = lib.avgpu_set_arbiter(b.h, len(bad), bad.ctypes.data_as(C.c_void_p),
                                   np.asarray(state[2]).reshape(1).ctypes.data_as(C.c_void_p), None)
        assert rc == EINVAL and "row 1" in lib.avgpu_last_error().decode(), field
    again = capi.get_arbiter(b.lib, b.h)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, state))
    out = np.zeros(1, dtype=capi.ARBITER_SUMMARY_DTYPE)
    assert lib.avgpu_classify_genotypes(b.h, 20, 0, out.ctypes.data_as(C.c_void_p)) == EINVAL
    assert lib.avgpu_classify_genotypes(b.h, 20, 3, None) == EINVAL
    assert lib.avgpu_classify_genotypes(None, 20, 3, out.ctypes.data_as(C.c_void_p)) == EINVAL
    again = capi.get_arbiter(b.lib, b.h)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, state))
    # a world that never classified reports a new world's state
    fresh = _gpu(golden, 16)
    r0, t0, s0, z0 = capi.get_arbiter(fresh.lib, fresh.h)
    assert len(r0) == 0 and len(t0) == 0 and int(s0["next_id"]) == 1 and int(s0["dominant_row"]) == -1
    assert not z0.any()
    fresh.close()
    # reset: a new world's arbiter
    assert lib.avgpu_reset_arbiter(b.h) == 0
    dev_b, host_b = systematics.DeviceGenotypeArbiter(3), systematics.GenotypeArbiter(3)
    dev_b.attach(_World(b))
    assert dev_b.num_genotypes() == 0 and dev_b.next_id == 1 and dev_b.sz_count == {} and dev_b.best_key is None
    _step(b, dev_b, host_b, 0)
    assert int(dev_b.ids.min()) == 1
    a.close()
    b.close()
    # a strip tile is refused
    t = _gpu(golden, 512, overrides={"WORLD_X": 64, "WORLD_Y": 64})
    t._call("set_tile", t.h, C.c_int64(0), C.c_int64(0))
    assert lib.avgpu_classify_genotypes(t.h, 0, 3, out.ctypes.data_as(C.c_void_p)) == EUNSUPPORTED
    assert "strip tiles" in lib.avgpu_last_error().decode()
    t.close()


# ---- the driver ---------------------------------------------------------------------
class _HostArbiterWorld:
    """a product world that hides the device arbiter: the driver then keeps
    the host arbiter over the device's genotype tables"""

    def __init__(self, w):
        self._w = w

    def __getattr__(self, name):
        if name in ("classify_genotypes", "arbiter_state"):
            raise AttributeError(name)
        return getattr(self._w, name)


STAMP = re.compile(r"^# \w{3} \w{3} \d{2} \d{2}:\d{2}:\d{2} \d{4}$")


def _lines(path):
    return [l for l in open(path).read().splitlines() if not STAMP.match(l)]


def _rows(path):
    return [l.split() for l in open(path) if l.strip() and not l.startswith("#")]


def _config(golden, path, events):
    path.mkdir()
    shutil.copy(os.path.join(golden, "heads_default_100u", "avida.cfg"), path / "avida.cfg")
    shutil.copy(os.path.join(golden, "instset-heads.cfg"), path / "instset-heads.cfg")
    shutil.copy(os.path.join(golden, "environment-logic9.cfg"), path / "environment.cfg")
    shutil.copy(os.path.join(golden, "default-heads.org"), path / "default-heads.org")
    (path / "events.cfg").write_text(events)


PRINTS = ("u 0:10:end PrintDominantData\nu 0:10:end PrintCountData\nu 0:10:end PrintAverageData\n"
          "u 30 SavePopulation\nu 30 Exit\n")
NAMES = ("dominant.dat", "count.dat", "average.dat", "detail-30.spop")


@pytest.mark.gpu
def test_gpu_driver_device_arbiter_vs_host_arbiter(golden, tmp_path):
    import torch
    assert torch.cuda.is_available()
    _config(golden, tmp_path / "config", "u begin Inject default-heads.org\nu 20 SaveCheckpoint ck.npz\n" + PRINTS)
    dd = driver.Driver(str(tmp_path / "config"), str(tmp_path / "device"))
    assert type(dd.arbiter) is systematics.DeviceGenotypeArbiter
    dd.run()
    dd.world.close()
    dh = driver.Driver(str(tmp_path / "config"), str(tmp_path / "host"),
                       make_world=lambda cfg, iset, env: _HostArbiterWorld(driver.ProductWorld(cfg, iset, env)))
    assert type(dh.arbiter) is systematics.GenotypeArbiter
    dh.run()
    dh.world.close()
    for name in NAMES:
        got, want = _lines(tmp_path / "device" / name), _lines(tmp_path / "host" / name)
        assert got == want, name
        assert len(got) + 1 == len(open(tmp_path / "device" / name).read().splitlines())    # one time stamp
    assert len(_rows(tmp_path / "device" / "dominant.dat")) == 4
    assert len(_rows(tmp_path / "device" / "detail-30.spop")) >= 1
    # resume from the checkpoint of update 20 in a fresh world
    _config(golden, tmp_path / "resume", "u begin LoadCheckpoint ck.npz\n" + PRINTS)
    shutil.copy(tmp_path / "device" / "ck.npz", tmp_path / "resume" / "ck.npz")
    dr = driver.Driver(str(tmp_path / "resume"), str(tmp_path / "resumed"))
    assert type(dr.arbiter) is systematics.DeviceGenotypeArbiter
    assert dr.run() == 30
    dr.world.close()
    for name in ("dominant.dat", "count.dat"):
        assert _rows(tmp_path / "resumed" / name) == _rows(tmp_path / "device" / name)[-1:], name
    ids = lambda p: [(r[0], r[16]) for r in _rows(p)]                  # noqa: E731  (id, sequence)
    assert ids(tmp_path / "resumed" / "detail-30.spop") == ids(tmp_path / "device" / "detail-30.spop")
