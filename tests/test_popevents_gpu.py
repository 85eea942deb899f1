"""avgpu_kill_cells, avgpu_kill_prob, avgpu_kill_rect, avgpu_kill_genotypes and
avgpu_keep_sample on the device against the specification
(avida_amd.popevents, held to the reference's loops in test_popevents_spec.py).

Each call is by definition avgpu_kill over the specification's set of cells: a
twin world gets that set through avgpu_kill one by one, and every cell's state
digest must agree -- the event writes nothing but the alive bit.  Worlds: 1 x 1;
3 x 5; 16 x 16 evolved 20 updates from ancestors (dead cells, newborns with
head starts, several genotypes); 67 x 64 = 4288 cells, a partial last 256-cell
block and rows that are no multiple of four words; 256 x 256 one-instruction
organisms of four genotypes, a seeded third dead, so that every pass of the
sample's select sees many populated bins."""
import ctypes as C
import os

import numpy as np
import pytest

from avida_amd import capi, datafiles, files, popevents
import oracle_lib as ol
import parity_util as pu
import test_checkpoint as tc
from test_popevents_spec import SEED, WatchingDriver, check_driver_run, make_config

pytestmark = pytest.mark.gpu

WORLDS = {"1x1": (1, 1), "3x5": (3, 5), "16x16": (16, 16), "67x64": (67, 64), "256x256": (256, 256)}
CALLS = ("cells", "prob", "rect", "genotypes", "sample")
KEYS = ((10 << 32) | 2, 0xC0FFEE1234567)
EINVAL, EUNSUPPORTED = -1, -5


def base_dead(n, seed=11):
    """the seeded third of the cells that is dead before anything is tested"""
    return np.sort(np.random.default_rng(seed).choice(n, n // 3, replace=False))


def make_world(golden, name, kind="gpu"):
    """the world `name` on backend `kind`; built the same way every time, so two of them are twins"""
    X, Y = WORLDS[name]
    n = X * Y
    iset, env, cfg = pu.load_env(golden, "instset-heads.cfg", {"WORLD_X": X, "WORLD_Y": Y}, seed=SEED)
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    w = ol.Backend(kind, cfg, iset, env, ncells=n)
    if name == "16x16":
        for c in range(0, n, 3):                       # a third of the cells: room for the births
            w.set_orgs(c, [anc], deterministic=False)
        for _ in range(20):
            w.run_update()
        return w
    if name == "256x256":
        ops = np.random.default_rng(12).integers(0, 4, n).astype(np.uint8)      # four genotypes of one site
        w.set_orgs_np(0, ops.tobytes(), np.ones(n, dtype=np.int32))
    else:
        w.set_orgs(0, [anc if c % 5 else anc[:60] for c in range(n)], deterministic=False)
    dead = base_dead(n)
    if n > 256:
        assert popevents.kill_cells(w, dead) == len(dead)
    else:
        for c in dead:
            w.kill(int(c))
    alive, _ = popevents.alive_mask(w)
    want = np.ones(n, dtype=bool)
    want[dead] = False
    assert (alive == want).all()                      # (the large worlds' base came through avgpu_kill_cells)
    return w


def call_args(name, call, alive, gkeys):
    """the arguments of `call` on world `name`"""
    X, Y = WORLDS[name]
    n = X * Y
    if call == "cells":
        rnd = np.random.default_rng(13)
        ids = rnd.integers(0, n, max(1, n // 4))
        return (np.concatenate([ids, ids[:max(1, len(ids) // 3)], [0, n - 1]]),)      # duplicates, the dead, both ends
    if call == "prob":
        return 0.5, KEYS[0]
    if call == "rect":
        return (3 * X) // 4, (3 * Y) // 4, X // 4, Y // 4           # crosses x = 0 and y = 0
    if call == "genotypes":
        present = np.unique(gkeys[alive])
        return [int(k) for k in present[::2]] + [int(present[0]), 987654321], 0.5, KEYS[1]   # a duplicate, an absent key
    living = int(alive.sum())
    return living // 2, KEYS[0]


def spec_set(name, call, args, alive, gkeys):
    X, Y = WORLDS[name]
    if call == "cells":
        ids = np.unique(args[0])
        return ids[alive[ids]]
    if call == "prob":
        return popevents.kill_prob(alive, SEED, args[1], args[0])
    if call == "rect":
        return popevents.kill_rect(alive, X, Y, *args)
    if call == "genotypes":
        return popevents.kill_genotypes(alive, gkeys, SEED, args[2], args[0], args[1])
    return popevents.keep_sample(alive, SEED, args[1], args[0])


def device_call(w, call, args):
    f = {"cells": popevents.kill_cells, "prob": popevents.apply_kill_prob, "rect": popevents.apply_kill_rect,
         "genotypes": popevents.apply_kill_genotypes, "sample": popevents.apply_keep_sample}[call]
    assert popevents.on_device(w)
    return f(w, *args)


def check_against_spec(w, name, call, args):
    """the device call on w: the alive mask afterwards and the count are the specification's; returns its set"""
    alive, gkeys = popevents.alive_mask(w)
    dead = spec_set(name, call, args, alive, gkeys)
    killed = device_call(w, call, args)
    after, _ = popevents.alive_mask(w)
    want = alive.copy()
    want[dead] = False
    assert killed == len(dead), (name, call, killed, len(dead))
    assert (after == want).all(), (name, call, np.flatnonzero(after != want)[:10])
    return dead


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("name", list(WORLDS))
def test_set_equality(golden, name, call):
    a, b = make_world(golden, name), make_world(golden, name)
    try:
        assert popevents.world_seed(a) == SEED
        alive, gkeys = popevents.alive_mask(a)
        if name == "16x16":
            assert 0 < alive.sum() < 256 and len(np.unique(gkeys[alive])) >= 3
        args = call_args(name, call, alive, gkeys)
        dead = check_against_spec(a, name, call, args)
        if len(alive) >= 256:
            assert 0 < len(dead) < alive.sum(), (name, call)
        for c in dead:
            b.kill(int(c))
        assert (a.digests() == b.digests()).all()
        ms, cells = popevents.last_timing(a)
        assert ms > 0 and cells > 0
    finally:
        a.close()
        b.close()


RECTS = [(2, 3, 9, 7), (1, 1, 1, 1), (60, 2, 3, 5), (2, 60, 5, 3), (-7, -7, 1000, 1000), (1000, 1000, -7, -7),
         (5, 0, 5, 63), (13, 2, 14, 2), (0, 0, 0, 0)]


@pytest.mark.parametrize("name", ["16x16", "67x64"])
def test_rectangles(golden, name):
    """inside, crossing either edge, far outside, one column, one row: against the specification"""
    w = make_world(golden, name)
    try:
        for rect in RECTS:
            check_against_spec(w, name, "rect", rect)
            if not popevents.alive_mask(w)[0].any():              # (the whole-world rectangles): set again
                w.close()
                w = make_world(golden, name)
    finally:
        w.close()


@pytest.mark.parametrize("call", CALLS)
def test_downstream(golden, call):
    """after an event five more updates run alike on the device and on the
    oracle, which got the specification's set through its per-cell kill"""
    g, o = make_world(golden, "16x16"), make_world(golden, "16x16", kind="oracle")
    try:
        alive, gkeys = popevents.alive_mask(g)
        assert (popevents.alive_mask(o)[0] == alive).all()
        args = call_args("16x16", call, alive, gkeys)
        dead = check_against_spec(g, "16x16", call, args)
        assert len(dead) > 0
        for c in dead:
            o.kill(int(c))
        births = 0
        for _ in range(5):
            sg, so = g.run_update(), o.run_update()
            assert (sg.num_organisms, sg.births) == (so.num_organisms, so.births)
            births += sg.births
        assert births > 0                                          # births landed in the emptied cells
        tc.compare(o, g, 256)
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("which", ["0", "1", "living-1", "living", "living+1"])
@pytest.mark.parametrize("name", ["67x64", "256x256"])
def test_keep_sample(golden, name, which, key):
    """exactly min(keep, living) survive, the specification's; the same call on
    a twin world leaves the same bytes"""
    a, b = make_world(golden, name), make_world(golden, name)
    try:
        living = int(popevents.alive_mask(a)[0].sum())
        keep = {"0": 0, "1": 1, "living-1": living - 1, "living": living, "living+1": living + 1}[which]
        check_against_spec(a, name, "sample", (keep, key))
        assert int(popevents.alive_mask(a)[0].sum()) == min(keep, living)
        popevents.apply_keep_sample(b, keep, key)
        assert a.digests().tobytes() == b.digests().tobytes()
        assert a.census().tobytes() == b.census().tobytes()
    finally:
        a.close()
        b.close()


def test_keep_sample_above_living_and_empty(golden):
    w = make_world(golden, "67x64")
    try:
        living = int(popevents.alive_mask(w)[0].sum())
        d0 = w.digests()
        for key in KEYS:
            assert popevents.apply_keep_sample(w, living + 1, key) == 0
            assert popevents.apply_keep_sample(w, 1 << 40, key) == 0
        assert (w.digests() == d0).all()
        assert popevents.apply_keep_sample(w, 0, KEYS[0]) == living          # nobody is left
        assert not popevents.alive_mask(w)[0].any()
        d1 = w.digests()
        for keep in (0, 1, 5000):
            assert popevents.apply_keep_sample(w, keep, KEYS[1]) == 0
        assert popevents.apply_kill_prob(w, 1.0, KEYS[0]) == 0 and popevents.apply_kill_rect(w, 0, 0, 66, 63) == 0
        assert (w.digests() == d1).all()
    finally:
        w.close()


def test_kill_cells(golden):
    w = make_world(golden, "67x64")
    try:
        n = w.ncells
        alive, _ = popevents.alive_mask(w)
        live, dead = np.flatnonzero(alive), np.flatnonzero(~alive)
        assert popevents.kill_cells(w, []) == 0
        assert popevents.kill_cells(w, dead[:50]) == 0                           # the dead count not at all
        assert popevents.kill_cells(w, [live[0]] * 7 + [dead[0]] + [live[1]] * 2) == 2   # duplicates count once
        assert popevents.kill_cells(w, [live[0], live[1], live[2]]) == 1
        after, _ = popevents.alive_mask(w)
        assert np.flatnonzero(alive != after).tolist() == live[:3].tolist()
        d0 = w.digests()
        for bad in ([live[5], n], [-1], [live[6], live[7], 1 << 40]):
            ids = np.array(bad, dtype=np.int64)
            killed = C.c_int64(-77)
            rc = w.lib.avgpu_kill_cells(w.h, ids.ctypes.data_as(C.c_void_p), len(ids), C.byref(killed))
            assert rc == EINVAL and killed.value == -77 and w.lib.avgpu_last_error()
        assert w.lib.avgpu_kill_cells(w.h, None, 3, None) == EINVAL
        assert w.lib.avgpu_kill_cells(w.h, None, -1, None) == EINVAL
        assert (w.digests() == d0).all()
    finally:
        w.close()


def test_refusals(golden):
    w = make_world(golden, "3x5")
    try:
        lib, h = w.lib, w.h
        d0 = w.digests()
        killed = C.c_int64(-77)
        keys = np.array([1, 2], dtype=np.uint64)
        kp = keys.ctypes.data_as(C.c_void_p)
        for p in (float("nan"), 1.5, -0.25):
            assert lib.avgpu_kill_prob(h, p, 1, C.byref(killed)) == EINVAL
            assert lib.avgpu_kill_genotypes(h, kp, 2, p, 1, C.byref(killed)) == EINVAL
        assert lib.avgpu_keep_sample(h, -1, 1, C.byref(killed)) == EINVAL
        assert lib.avgpu_kill_genotypes(h, kp, -1, 0.5, 1, C.byref(killed)) == EINVAL
        assert lib.avgpu_kill_genotypes(h, None, 2, 0.5, 1, C.byref(killed)) == EINVAL
        for rc in (lib.avgpu_kill_cells(None, None, 0, None), lib.avgpu_kill_prob(None, 0.5, 1, None),
                   lib.avgpu_kill_rect(None, 0, 0, 0, 0, None), lib.avgpu_kill_genotypes(None, kp, 2, 0.5, 1, None),
                   lib.avgpu_keep_sample(None, 1, 1, None), lib.avgpu_last_event_ms(None, None, None)):
            assert rc == EINVAL
        assert killed.value == -77 and (w.digests() == d0).all()
        assert lib.avgpu_kill_genotypes(h, None, 0, 1.0, 1, C.byref(killed)) == 0 and killed.value == 0   # no key: nobody
        assert (w.digests() == d0).all()
    finally:
        w.close()


def test_strip_tile_is_refused(golden):
    iset, env, cfg = pu.load_env(golden, "instset-heads.cfg", {"WORLD_X": 32, "WORLD_Y": 32}, seed=SEED)
    w = ol.Backend("gpu", cfg, iset, env, ncells=512)              # rows 0 .. 15 of 32
    try:
        w._call("set_tile", w.h, 0, 0)
        lib, h = w.lib, w.h
        killed = C.c_int64(-77)
        ids = np.array([1], dtype=np.int64)
        keys = np.array([1], dtype=np.uint64)
        calls = (("avgpu_kill_cells", lambda: lib.avgpu_kill_cells(h, ids.ctypes.data_as(C.c_void_p), 1, C.byref(killed))),
                 ("avgpu_kill_prob", lambda: lib.avgpu_kill_prob(h, 0.5, 1, C.byref(killed))),
                 ("avgpu_kill_rect", lambda: lib.avgpu_kill_rect(h, 0, 0, 3, 3, C.byref(killed))),
                 ("avgpu_kill_genotypes", lambda: lib.avgpu_kill_genotypes(h, keys.ctypes.data_as(C.c_void_p), 1, 1.0, 1,
                                                                           C.byref(killed))),
                 ("avgpu_keep_sample", lambda: lib.avgpu_keep_sample(h, 3, 1, C.byref(killed))))
        for name, call in calls:
            assert call() == EUNSUPPORTED and name in lib.avgpu_last_error().decode(), name
        assert killed.value == -77
    finally:
        w.close()


def test_lifetime(golden):
    """the scratch of every call goes with the world"""
    lib = capi.load_product()
    base = capi.live_objects(lib)
    w = make_world(golden, "16x16")
    try:
        alive, gkeys = popevents.alive_mask(w)
        for call in CALLS:
            device_call(w, call, call_args("16x16", call, alive, gkeys))
        grown = capi.live_objects(lib)
        popevents.last_timing(w)
        for call in CALLS:                                # a second round allocates nothing
            device_call(w, call, call_args("16x16", call, alive, gkeys))
        assert capi.live_objects(lib) == grown > base
    finally:
        w.close()
    assert capi.live_objects(lib) == base


def test_calls_behind_queued_updates(golden):
    """a call with killed == NULL right behind three queued avgpu_run_update(w,
    NULL) acts on the world those updates leave: a twin that waits for every
    update and kills the specification's set cell by cell ends alike"""
    a, b = tc._world("gpu", golden, "logic9"), tc._world("gpu", golden, "logic9")
    X = Y = 32
    try:
        seed = popevents.world_seed(a)
        lib, h = a.lib, a.h
        keys = np.ascontiguousarray(np.unique(popevents.alive_mask(a)[1])[::3], dtype=np.uint64)
        ids = np.array([5, 17, 200, 513, 17], dtype=np.int64)
        steps = [
            ("cells", lambda: lib.avgpu_kill_cells(h, ids.ctypes.data_as(C.c_void_p), len(ids), None),
             lambda al, gk: np.unique(ids)[al[np.unique(ids)]]),
            ("prob", lambda: lib.avgpu_kill_prob(h, 0.3, KEYS[0], None),
             lambda al, gk: popevents.kill_prob(al, seed, KEYS[0], 0.3)),
            ("rect", lambda: lib.avgpu_kill_rect(h, 30, 29, 2, 1, None),
             lambda al, gk: popevents.kill_rect(al, X, Y, 30, 29, 2, 1)),
            ("genotypes", lambda: lib.avgpu_kill_genotypes(h, keys.ctypes.data_as(C.c_void_p), len(keys), 0.7, KEYS[1], None),
             lambda al, gk: popevents.kill_genotypes(al, gk, seed, KEYS[1], keys, 0.7)),
            ("sample", lambda: lib.avgpu_keep_sample(h, 100, KEYS[1], None),
             lambda al, gk: popevents.keep_sample(al, seed, KEYS[1], 100)),
        ]
        for name, queued, spec in steps:
            for _ in range(3):
                assert lib.avgpu_run_update(h, None) == 0          # queued: no statistics, no sync
            assert queued() == 0, lib.avgpu_last_error().decode()
            for _ in range(3):
                b.run_update()
            alive, gkeys = popevents.alive_mask(b)
            dead = spec(alive, gkeys)
            assert len(dead) > 0, name
            for c in dead:
                b.kill(int(c))
            assert (a.digests() == b.digests()).all(), name
        sa, sb = a.run_update(), b.run_update()
        assert (sa.num_organisms, sa.births, sa.insts_executed) == (sb.num_organisms, sb.births, sb.insts_executed)
        assert (a.digests() == b.digests()).all()
    finally:
        a.close()
        b.close()


def test_kill_list_regrows_behind_queued_updates(golden):
    """avgpu_kill_cells with 4 cells, then with 40, each right behind three
    queued updates and nothing synchronised in between: the second list does
    not fit the words made for the first (5 of them), so the call replaces the
    device words and their pinned twin while updates are queued.  A twin that
    waits for every update and kills the specification's sets cell by cell ends
    alike, and the library owns as much after the second call as after the
    first: buffers replaced, none added."""
    a, b = tc._world("gpu", golden, "logic9"), tc._world("gpu", golden, "logic9")
    try:
        lib, h = a.lib, a.h
        lists = [np.array([5, 17, 200, 513], dtype=np.int64),
                 np.sort(np.random.default_rng(40).choice(a.ncells, 40, replace=False)).astype(np.int64)]
        counts = []
        for ids in lists:
            for _ in range(3):
                assert lib.avgpu_run_update(h, None) == 0          # queued: no statistics, no sync
            assert lib.avgpu_kill_cells(h, ids.ctypes.data_as(C.c_void_p), len(ids), None) == 0, \
                lib.avgpu_last_error().decode()
            counts.append(capi.live_objects(lib))
        for ids in lists:
            for _ in range(3):
                b.run_update()
            assert popevents.kill_cells(b, ids, device=False) > 0  # the specification: the living among the list, one by one
        assert (a.digests() == b.digests()).all()
        assert counts[1] == counts[0]
    finally:
        a.close()
        b.close()


def test_driver_files_equal_the_oracle_run(golden, tmp_path, monkeypatch):
    """the driver run of test_popevents_spec on ProductWorld: the device decides
    the events, and the data files are the oracle run's, byte for byte"""
    monkeypatch.setattr(datafiles.StatsRecorder, "_stamp", lambda self: "(time)")     # the header's wall-clock line
    make_config(golden, tmp_path / "config")
    runs = {"device": None, "oracle": lambda cfg, iset, env: ol.Backend("oracle", cfg, iset, env)}
    for name, mk in runs.items():
        d = WatchingDriver(str(tmp_path / "config"), str(tmp_path / name), make_world=mk)
        try:
            assert popevents.on_device(d.world) == (name == "device")
            check_driver_run(d, str(tmp_path / name))
        finally:
            d.world.close()
    names = sorted(os.listdir(tmp_path / "oracle"))
    assert "count.dat" in names and sorted(os.listdir(tmp_path / "device")) == names
    for f in names:
        assert open(tmp_path / "device" / f, "rb").read() == open(tmp_path / "oracle" / f, "rb").read(), f
