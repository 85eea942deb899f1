"""The lineage store on the device (include/avida_gpu.h avgpu_enable_lineage;
DESIGN.md 10.6) against its specification, the host
systematics.GenotypeArbiter(threshold, lineage=True) fed the same tables,
parent keys and tape prefixes at the same moments.  Every field is an integer
or copied bytes, so agreement is exact: every row, the arena, the summary."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from avida_amd import capi, systematics
import lineage_util as lu
import oracle_lib as ol
import parity_util as pu
from test_lineage_spec import _sequence, SEEDS
from test_lineage_run import _World

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE, EUNSUPPORTED = -1, -3, -5


# ---- CPU: the mirrors ----
def test_lineage_struct_layouts(tmp_path):
    row, summ = capi.LINEAGE_ROW_DTYPE, capi.LINEAGE_SUMMARY_DTYPE
    fields = [("avgpu_lineage_row", n) for n in row.names] + [("avgpu_lineage_summary", n) for n in summ.names]
    src = tmp_path / "lin.c"
    src.write_text('#include "avida_gpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){'
                   'printf("%zu %zu", sizeof(avgpu_lineage_row), sizeof(avgpu_lineage_summary));'
                   + "".join('printf(" %%zu", offsetof(%s, %s));' % f for f in fields) + 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "lin"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:2] == [64, 64] == [row.itemsize, summ.itemsize]
    assert got[2:] == [row.fields[n][1] for n in row.names] + [summ.fields[n][1] for n in summ.names]


def test_lineage_symbols_are_exported():
    for name in ("avgpu_enable_lineage", "avgpu_get_lineage", "avgpu_set_lineage", "avgpu_prune_lineage",
                 "avgpu_last_lineage_ms"):
        assert name in capi.EXPORTED


# ---- GPU ----
def _compare(b, host, where):
    rows, arena, s = capi.get_lineage(b.lib, b.h)
    st = host.lineage
    if rows.tobytes() != st.rows.tobytes():
        bad = [j for j in range(min(len(rows), len(st.rows))) if rows[j] != st.rows[j]][:3]
        raise AssertionError((where, len(rows), len(st.rows), bad, [rows[j] for j in bad], [st.rows[j] for j in bad]))
    assert arena.tobytes() == bytes(st.arena), where
    want = st.summary()
    assert {f: int(s[f]) for f in want} == want, where


class _DevWorld(_World):
    """what DeviceGenotypeArbiter(lineage=True) asks of a world, over a test Backend"""

    def classify_genotypes(self, update, threshold):
        return capi.classify_genotypes(self.b.lib, self.b.h, update, threshold)

    def arbiter_state(self):
        return capi.get_arbiter(self.b.lib, self.b.h)

    def enable_lineage(self, on=True, rows_hint=0, arena_hint=0):
        capi.enable_lineage(self.b.lib, self.b.h, on, rows_hint, arena_hint)

    def lineage_state(self, summary_only=False):
        return capi.get_lineage(self.b.lib, self.b.h, summary_only)

    prunes = 0

    def prune_lineage(self):
        self.prunes += 1
        return capi.prune_lineage(self.b.lib, self.b.h)


def _device_step(b, dev_summary_holder, update):
    return capi.classify_genotypes(b.lib, b.h, update, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_store_equals_host_on_synthetic_sequences(golden, seed):
    """the host test's sequences through avgpu_set_genotype_keys +
    avgpu_set_parent_keys: every capture takes the mismatch path (the tapes are
    not the keys' genomes); a prune every 5th step; hints 1 / 16, so the row
    buffer regrows"""
    seq = _sequence(seed)
    n = len(seq[0][0])
    iset, env, cfg = pu.load_env(golden, seed=7)
    b = ol.Backend("gpu", cfg, iset, env, ncells=n)
    capi.enable_lineage(b.lib, b.h, True, 1, 16)
    host = systematics.GenotypeArbiter(3, lineage=True)
    for step, (keys, pk, of_key) in enumerate(seq):
        lens = [len(of_key[int(k)]) if k else 1 for k in keys]
        b.set_orgs(0, [bytes(x) for x in lens])
        for c in np.flatnonzero(keys == 0):
            b.kill(int(c))
        kk = np.ascontiguousarray(keys, dtype=np.uint64)
        b._call("set_genotype_keys", b.h, 0, n, kk.ctypes.data_as(C.c_void_p))
        lu.set_parent_keys(b, pk)
        table, totals = capi.get_genotypes(b.lib, b.h)
        first = table["first_cell"]
        host.update_table(table, totals, step, parent_keys=pk[first], sequences=None,
                          generations=b.census()["generation"][first])
        _device_step(b, None, step)
        _compare(b, host, (seed, step))
        if step % 5 == 4:
            dropped = host.prune()
            s = capi.prune_lineage(b.lib, b.h)
            assert int(s["dropped_last_prune"]) == dropped
            _compare(b, host, (seed, step, "pruned"))
    assert host.lineage.num_orphans > 0 and host.lineage.num_unsequenced == host.next_id - 1
    ms, pms = C.c_double(-1.0), C.c_double(-1.0)
    assert b.lib.avgpu_last_lineage_ms(b.h, C.byref(ms), C.byref(pms)) == 0 and ms.value >= 0.0 and pms.value >= 0.0
    b.close()


@pytest.mark.gpu
def test_store_equals_host_on_a_real_run_and_through_a_checkpoint(golden, tmp_path):
    """the 16 x 16 world, 60 updates, the store against the host arbiter fed
    from get_genotypes, get_parent_keys and the tape prefixes (captures
    succeed: the arena regrows from 16 bytes); at update 30 a checkpoint is
    restored into a second world, which then runs beside the first: resume ==
    the continuous run, store bytes identical"""
    b, step, _ = lu.make_world("gpu", golden, "torus16_bm0")
    capi.enable_lineage(b.lib, b.h, True, 1, 16)
    w = _World(b)
    host = systematics.GenotypeArbiter(3, lineage=True)
    handlers = b.instset.handlers
    r = step_r = None
    for u in range(0, 61):
        if u:
            step()
            if r is not None:
                step_r()
        systematics.classify_with_lineage(host, w, u, handlers)
        capi.classify_genotypes(b.lib, b.h, u, 3)
        _compare(b, host, u)
        if r is not None:
            capi.classify_genotypes(r.lib, r.h, u, 3)
            _compare(r, host, ("resumed", u))
        if u % 20 == 10:
            host.prune()
            capi.prune_lineage(b.lib, b.h)
            if r is not None:
                capi.prune_lineage(r.lib, r.h)
            _compare(b, host, (u, "pruned"))
        if u == 30:
            path = str(tmp_path / "lin.npz")
            b.checkpoint(path)
            assert {"lin_rows", "lin_genomes", "lin_summary", "pkeys"} <= set(np.load(path).files)
            r, step_r, _ = lu.make_world("gpu", golden, "torus16_bm0")
            capi.enable_lineage(r.lib, r.h, True, 1, 16)
            r.restore(path)
            _compare(r, host, "restored")
    s = host.lineage.summary()
    assert s["rows"] > 50 and s["arena_bytes"] > 16 * 50 and s["max_depth"] >= 2 and s["num_orphans"] == 0, s
    # the device arbiter's view: lazy fetch, lineage_of, the dominant's depth
    dev = systematics.DeviceGenotypeArbiter(3, lineage=True)
    dev.attach(_DevWorld(b))
    dom = host.dominant()
    assert dev.lineage_of(dom.id).tobytes() == host.lineage_of(dom.id).tobytes()
    assert dev.dominant_row(60) == host.dominant_row(60) and dev.dominant_row(60)[11] == host.depth_of(dom.id)
    b.close()
    r.close()


@pytest.mark.gpu
def test_device_arbiter_with_lineage(golden):
    """DeviceGenotypeArbiter(threshold, lineage=True): it turns the store on,
    prunes when the store exceeds twice the active rows, fetches lazily, and
    reports the dominant's lineage and depth"""
    b, step, _ = lu.make_world("gpu", golden, "torus16_bm0")
    w = _DevWorld(b)
    dev = systematics.DeviceGenotypeArbiter(3, lineage=True)
    dev.enable(w, 1, 16)
    dropped = 0
    # 120 updates: ~20 births an update, most founding a genotype, against at most 256 active ones --
    # the store passes twice the active rows several times
    for u in range(120):
        if u:
            step()
        before = w.prunes
        dev.classify(w, u)
        s = capi.get_lineage(b.lib, b.h, True)[2]
        assert int(s["active_rows"]) == dev.num_genotypes()
        # over twice the active rows only right after a prune (what it kept: the ancestors of the living)
        assert int(s["rows"]) <= 2 * int(s["active_rows"]) or w.prunes == before + 1
        dropped += int(s["dropped_last_prune"]) if w.prunes == before + 1 else 0
    assert w.prunes > 0 and dropped > 0
    dom = dev.dominant()
    path = dev.lineage_of(dom.id)
    assert int(path[0]["id"]) == dom.id and int(path[-1]["parent_id"]) == 0 and len(path) >= 2
    assert [int(r["depth"]) for r in path] == list(range(len(path) - 1, -1, -1))
    assert dev.dominant_row(119)[11] == len(path) - 1
    st = dev.lineage_store()
    for r in path:
        seq = st.sequence(int(r["id"]))
        assert seq is None or systematics.genome_key(seq) == int(r["genotype_key"])
    with pytest.raises(ValueError):
        systematics.DeviceGenotypeArbiter(3).lineage_of(1)
    b.close()


@pytest.mark.gpu
def test_lineage_refusals_and_lifetime(golden):
    lib = capi.load_product()
    base = capi.live_objects(lib)
    b, step, _ = lu.make_world("gpu", golden, "torus16_bm0")
    assert lib.avgpu_get_lineage(b.h, None, 0, None, 0, None) == ESTATE          # the store is off
    capi.enable_lineage(lib, b.h, True, 1, 16)
    for u in range(20):
        step()
        capi.classify_genotypes(lib, b.h, u, 3)
    assert lib.avgpu_enable_lineage(b.h, 0, 0, 0) == 0                           # off: the buffers go
    assert lib.avgpu_enable_lineage(b.h, 1, 0, 0) == ESTATE                      # the arbiter holds genotypes
    b._call("reset_arbiter", b.h)
    capi.enable_lineage(lib, b.h, True, 1, 16)
    assert int(capi.get_lineage(lib, b.h, True)[2]["rows"]) == 0
    for u in range(20, 30):
        step()
        capi.classify_genotypes(lib, b.h, u, 3)
    rows, arena, s = capi.get_lineage(lib, b.h)
    assert len(rows) > 10
    small = np.zeros(2, dtype=capi.LINEAGE_ROW_DTYPE)
    assert lib.avgpu_get_lineage(b.h, small.ctypes.data_as(C.c_void_p), 2, None, 0, None) == EINVAL
    assert not small["id"].any()                                                  # nothing written
    bad = rows.copy()
    bad["id"][[0, 1]] = bad["id"][[1, 0]]                                         # ids not ascending
    for wrong in (bad, rows[1:]):                                                 # ... / an active genotype's row missing
        with pytest.raises(RuntimeError):
            capi.set_lineage(lib, b.h, wrong, arena if wrong is bad else arena[:0], s)
    again = capi.get_lineage(lib, b.h)
    assert again[0].tobytes() == rows.tobytes() and again[1].tobytes() == arena.tobytes()   # state unchanged
    capi.set_lineage(lib, b.h, rows, arena, s)                                    # its own state goes back in
    assert capi.get_lineage(lib, b.h)[0].tobytes() == rows.tobytes()
    b._call("reset_arbiter", b.h)                                                 # empties the store
    assert int(capi.get_lineage(lib, b.h, True)[2]["rows"]) == 0
    b.close()
    assert capi.live_objects(lib) == base
    import tile_util as tu
    t, _ = tu.make_tile("gpu", golden, 128, 4, 2, 0, device="cuda")
    assert lib.avgpu_enable_lineage(t.h, 1, 0, 0) == EUNSUPPORTED
    assert lib.avgpu_prune_lineage(t.h, None) == EUNSUPPORTED
    t.close()
