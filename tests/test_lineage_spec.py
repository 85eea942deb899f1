"""The host lineage rules (systematics.GenotypeArbiter(threshold, lineage=True),
DESIGN.md 10.6) over synthetic sequences: 200 cells, genomes from a pool of
30, 20 steps, synthetic parent keys, 5 seeds.  The checks keep books of their
own (dicts and sets), apart from the store's arrays."""
import numpy as np
import pytest

from avida_amd import capi, systematics

CELLS, POOL, STEPS, SEEDS = 200, 30, 20, (1, 2, 3, 4, 5)


def _pool(seed):
    rng = np.random.default_rng(1000 + seed)
    genomes = [bytes(rng.integers(0, 26, size=int(rng.integers(10, 60)), dtype=np.uint8)) for _ in range(POOL)]
    return genomes, np.array([systematics.genome_key(g) for g in genomes], dtype=np.uint64)


def _sequence(seed):
    """per step (keys, parent keys, key -> genome): a turnover of half the
    cells; an offspring takes its parent's genome or mutates into one of a
    window of the pool that slides by three per step (old genomes die out and
    later return); one offspring in twenty names a parent nobody saw (its
    parent was born and died between two classifications)"""
    rng = np.random.default_rng(seed)
    genomes, pool = _pool(seed)
    of_key = {int(k): g for k, g in zip(pool, genomes)}
    keys = pool[rng.integers(0, 6, size=CELLS)]
    keys[rng.random(CELLS) < 0.3] = 0
    pk = np.zeros(CELLS, dtype=np.uint64)
    out = [(keys.copy(), pk.copy(), of_key)]
    for t in range(1, STEPS):
        old = keys.copy()
        window = pool[(3 * t + np.arange(5)) % POOL]
        live = np.flatnonzero(old)
        keys[rng.random(CELLS) < 0.25] = 0
        for c in np.flatnonzero(rng.random(CELLS) < 0.5):
            p = int(live[rng.integers(len(live))])
            keys[c] = old[p] if rng.random() < 0.4 else window[rng.integers(len(window))]
            pk[c] = old[p] if rng.random() >= 0.05 else np.uint64(rng.integers(1, 1 << 62))
        pk[keys == 0] = 0
        out.append((keys.copy(), pk.copy(), of_key))
    return out


def _census(keys, step):
    c = np.zeros(CELLS, dtype=capi.CENSUS_DTYPE)
    c["genotype_key"] = keys
    c["genome_length"] = 0
    c["generation"] = step + np.arange(CELLS) % 3
    return c


def _closure(rows):
    """ids a prune must keep, by plain recursion over a dict"""
    parent = {int(r["id"]): int(r["parent_id"]) for r in rows}
    keep = set()
    for r in rows:
        if r["update_deactivated"] < 0:
            g = int(r["id"])
            while g > 0 and g in parent and g not in keep:
                keep.add(g)
                g = parent[g]
    return keep


def _check_invariants(store):
    rows = store.rows
    ids = rows["id"]
    assert (np.diff(ids) > 0).all()
    depth = {int(r["id"]): int(r["depth"]) for r in rows}
    for r in rows:
        p = int(r["parent_id"])
        assert p < int(r["id"])
        if p > 0:
            assert p in depth, (int(r["id"]), p)
            assert int(r["depth"]) == depth[p] + 1
        else:
            assert int(r["depth"]) == 0
    offs = [(int(r["seq_off"]), int(r["genome_length"])) for r in rows if r["seq_off"] >= 0]
    at = 0
    for off, length in offs:                       # 16-B aligned, in id order, no gaps
        assert off == at and off % 16 == 0
        at += (length + 15) & ~15
    assert at == len(store.arena)


def _run(seed, reached):
    arb = systematics.GenotypeArbiter(3, lineage=True)
    store = arb.lineage
    every = {}                                     # id -> key, over the whole run
    prev_keys = np.zeros(CELLS, dtype=np.uint64)
    orphans = unsequenced = 0
    for step, (keys, pk, of_key) in enumerate(_sequence(seed)):
        census = _census(keys, step)
        for k in np.unique(keys[keys != 0]):
            census["genome_length"][keys == k] = len(of_key[int(k)])
        table, totals = systematics.table_from_census(census)
        first = table["first_cell"]
        active_before = {int(k): int(i) for k, i in zip(arb.keys, arb.ids)}
        n_before = len(store.rows)
        # every third new genotype's capture is spoiled: the tape prefix no longer hashes to the key
        seqs = [of_key[int(k)] if j % 3 else of_key[int(k)][::-1] + b"\x01" for j, k in enumerate(table["genotype_key"])]
        arb.update_table(table, totals, step, parent_keys=pk[first], sequences=seqs,
                         generations=census["generation"][first])
        _check_invariants(store)
        new = store.rows[n_before:]
        assert not set(int(i) for i in new["id"]) & set(every) and set(int(i) for i in store.rows["id"][:n_before]) <= set(every)
        assert {int(r["id"]) for r in store.rows if r["update_deactivated"] < 0} == {int(i) for i in arb.ids}
        for r in new:
            gid, key, p = int(r["id"]), int(r["genotype_key"]), int(r["parent_id"])
            assert key not in active_before            # a still-active key never gets a second row
            if key in every.values():
                reached["returning key"] = True
            every[gid] = key
            j = int(np.flatnonzero(table["genotype_key"] == np.uint64(key))[0])
            want_pk = int(pk[first[j]])
            assert int(r["update_born"]) == step and int(r["gen_born"]) == int(census["generation"][first[j]])
            if want_pk == 0:
                assert p == 0
            elif want_pk in active_before:
                assert p == active_before[want_pk]
                if int(store.rows[store.index(p)]["update_deactivated"]) == step:
                    reached["parent deactivated with the child's birth"] = True
            else:
                assert p == -1
                orphans += 1
                reached["orphan"] = True
            seq = store.sequence(gid)
            assert (seq is None) == (seqs[j] != of_key[key])
            unsequenced += seq is None
            assert seq is None or (seq == of_key[key] and systematics.genome_key(seq) == key)
        assert store.num_orphans == orphans
        new_keys = {int(r["genotype_key"]) for r in new}
        changed = np.flatnonzero((keys != prev_keys) & (keys != 0) & (pk != keys))
        if any(int(keys[c]) in active_before and int(keys[c]) not in new_keys for c in changed):
            reached["back-mutation into an active key"] = True
        gone = set(active_before.values()) - {int(i) for i in arb.ids}
        for g in gone:
            assert int(store.rows[store.index(g)]["update_deactivated"]) == step
        if step % 5 == 4:
            before = store.rows.copy()
            want = _closure(before)
            dropped = arb.prune()
            assert {int(i) for i in store.rows["id"]} == want
            assert dropped == len(before) - len(want) == store.summary()["dropped_last_prune"]
            _check_invariants(store)
            for r in store.rows:                       # stable: every kept row unchanged but for its offset
                b = before[int(np.searchsorted(before["id"], r["id"]))]
                for f in capi.LINEAGE_ROW_DTYPE.names:
                    assert f == "seq_off" or r[f] == b[f]
            lost = {int(r["id"]): int(r["parent_id"]) for r in before if int(r["id"]) not in want}
            if any(p in lost and lost[p] in lost for p in lost.values()):   # a row, its parent, its grandparent
                reached["dead chain 3 deep dropped"] = True
            if (store.rows["update_deactivated"] >= 0).any():
                reached["dead ancestor kept"] = True
        prev_keys = keys
    s = store.summary()
    assert s["rows"] == len(store.rows) and s["num_unsequenced"] == unsequenced and s["num_orphans"] == orphans
    assert s["active_rows"] == len(arb.ids) and s["max_depth"] == int(store.rows["depth"].max())
    return arb


def test_host_lineage_rules_over_synthetic_sequences():
    reached = {}
    for seed in SEEDS:
        arb = _run(seed, reached)
        dom = arb.dominant()
        path = arb.lineage_of(dom.id)
        assert int(path[0]["id"]) == dom.id
        for a, b in zip(path[:-1], path[1:]):
            assert int(a["parent_id"]) == int(b["id"]) and int(a["depth"]) == int(b["depth"]) + 1
        assert int(path[-1]["parent_id"]) <= 0 or arb.lineage.index(int(path[-1]["parent_id"])) < 0
        assert arb.dominant_row(STEPS)[11] == int(path[0]["depth"])
    for case in ("parent deactivated with the child's birth", "orphan", "returning key",
                 "back-mutation into an active key", "dead chain 3 deep dropped", "dead ancestor kept"):
        assert reached.get(case), f"the sequences never reach: {case}"


def test_lineage_off_is_unchanged_and_on_needs_parent_keys():
    keys, pk, of_key = _sequence(1)[0]
    table, totals = systematics.table_from_census(_census(keys, 0))
    off = systematics.GenotypeArbiter(3)
    off.update_table(table, totals, 0)
    assert off.lineage is None and off.dominant_row(0)[11] == 0
    with pytest.raises(ValueError):
        off.lineage_of(1)
    on = systematics.GenotypeArbiter(3, lineage=True)
    with pytest.raises(ValueError):
        on.update_table(table, totals, 0)
    on.update_table(table, totals, 0, parent_keys=pk[table["first_cell"]])
    assert np.array_equal(on.ids, off.ids) and np.array_equal(on.keys, off.keys)
    assert on.lineage.summary()["rows"] == len(on.ids) == on.lineage.summary()["num_unsequenced"]
    assert (on.lineage.rows["parent_id"] == 0).all() and (on.lineage.rows["seq_off"] == -1).all()


def test_lineage_row_layout():
    d = capi.LINEAGE_ROW_DTYPE
    assert d.itemsize == 64
    assert [d.fields[n][1] for n in d.names] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60]
