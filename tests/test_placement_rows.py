"""Placement on small tori where records collide: the birth record's row
(device.h BI_PARENT .. BI_PRIO), the batched pick loads and the skipped
placement launches against the oracle.

Every world is seeded from detail-50000.pop by bench._genomes_for (the cell
id's hash), default config, seed 101, and runs 60 updates; after EVERY update
the GPU's statistics and every cell's digest must equal the oracle's.

* 16x16, every second row empty: empty-cell claims, lost empty claims and
  re-picks in rounds 1..3 -- placement launches 2 and 3 run in some updates
  and are skipped in others.
* 16x16 and 8x8 full: kill claims; on 8x8 the torus wraps onto few cells and
  many records share a target.
* the half-empty 16x16 world without PREFER_EMPTY, without ALLOW_PARENT, and
  as a bounded grid (edge cells have 3 or 5 neighbours: the validity mask).

The first three may not pass vacuously: the oracle's own statistics must show
overwritten births and cancelled records (divides beyond the births placed,
overwritten or dropped) in enough updates -- a CPU test of its own.
"""
import os

import pytest

from avida_amd import capi, files
import oracle_lib as ol
import parity_util as pu

UPDATES = 60
STAT_FIELDS = ("num_organisms", "insts_executed", "births", "deaths", "divides", "births_dropped",
               "births_overwritten")

# name: (X, Y, every second row empty, config overrides)
CASES = {
    "half16": (16, 16, True, {}),
    "full16": (16, 16, False, {}),
    "full8": (8, 8, False, {}),
    "half16_no_prefer_empty": (16, 16, True, {"PREFER_EMPTY": 0}),
    "half16_no_allow_parent": (16, 16, True, {"ALLOW_PARENT": 0}),
    "half16_bounded": (16, 16, True, {"WORLD_GEOMETRY": 1}),
}
# name: updates (of 60) in which the oracle must show overwritten births /
# cancelled records
NOT_VACUOUS = {"half16": 10, "full16": 10, "full8": 5}

_setup = {}
_oracle = {}


def _world(golden, name):
    """(cfg, iset, env, seeded rows [(first cell, genomes, merits)]) of a case"""
    if name not in _setup:
        import bench
        X, Y, half, over = CASES[name]
        iset, pool = bench._pool(golden)
        env = files.read_environment(os.path.join(golden, "environment-logic9.cfg"))
        cfg = capi.cfg_from_avida(files.read_avida_cfg(None, dict(over, WORLD_X=X, WORLD_Y=Y)), seed=101)
        picks = bench._genomes_for(X * Y, pool)
        rows = []
        for y in range(0, Y, 2 if half else 1):
            row = picks[y * X:(y + 1) * X]
            rows.append((y * X, [g for g, _ in row], [m for _, m in row]))
        _setup[name] = (cfg, iset, env, rows)
    return _setup[name]


def _backend(kind, golden, name):
    cfg, iset, env, rows = _world(golden, name)
    b = ol.Backend(kind, cfg, iset, env, ncells=cfg.world_x * cfg.world_y)
    for first, genomes, merits in rows:
        b.set_orgs(first, genomes, merits=merits, deterministic=False)
    return b


def _oracle_run(golden, name):
    """the oracle's run of a case, computed once: the seeded world's digests,
    then per update ({field: value}, digests)"""
    if name not in _oracle:
        orc = _backend("oracle", golden, name)
        d0 = orc.digests()
        run = []
        for _ in range(UPDATES):
            s = orc.run_update()
            run.append(({f: getattr(s, f) for f in STAT_FIELDS}, orc.digests()))
        orc.close()
        _oracle[name] = (d0, run)
    return _oracle[name]


@pytest.mark.parametrize("name", sorted(NOT_VACUOUS))
def test_oracle_worlds_collide(golden, name):
    """CPU half: the oracle's statistics of the first three worlds show
    overwritten births and cancelled records in enough of the 60 updates"""
    _, run = _oracle_run(golden, name)
    over = sum(1 for s, _ in run if s["births_overwritten"] > 0)
    canc = sum(1 for s, _ in run if s["divides"] > s["births"] + s["births_overwritten"] + s["births_dropped"])
    print(f"{name}: overwritten births in {over} updates, cancelled records in {canc} of {UPDATES}")
    assert over >= NOT_VACUOUS[name], (name, over)
    assert canc >= NOT_VACUOUS[name], (name, canc)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_placement_rows_bit_exact(golden, name):
    d0, run = _oracle_run(golden, name)
    gpu = _backend("gpu", golden, name)
    nbad, cells = pu.compare_digests(d0, gpu.digests())
    assert nbad == 0, f"{name}, seeded world: {nbad} cells differ, first {cells}"
    births = 0
    for u, (so, do) in enumerate(run):
        sg = gpu.run_update()
        for f in STAT_FIELDS:
            assert so[f] == getattr(sg, f), (name, u, f, so[f], getattr(sg, f))
        nbad, cells = pu.compare_digests(do, gpu.digests())
        assert nbad == 0, f"{name}, update {u}: {nbad} cells differ, first {cells}"
        births += sg.births
    assert births > 0
    assert gpu.counters(cumulative=1)[capi.CNT_BAD_RECORD] == 0
    gpu.close()
