"""A world gives back everything it took: avgpu_live_objects (device buffers,
pinned buffers, events and streams the library owns) returns to where it was
after a world's destruction -- a plain one, one that touched every allocation
made on first use -- and after each refused call on a living world.  The
count is exact and does not depend on the card's free memory.  Other tests of
the process may hold worlds: every case compares against the count it starts
from."""
import ctypes as C
import os

import numpy as np
import pytest

from avida_amd import capi, files, landscape
import oracle_lib as ol
import parity_util as pu

X = Y = 16
N = X * Y


def _live():
    return capi.live_objects(capi.load_product())


def _world(golden, env=None, **overrides):
    ov = {"WORLD_X": X, "WORLD_Y": Y}
    ov.update(overrides)
    iset, env0, cfg = pu.load_env(golden, overrides=ov, seed=11)
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    b = ol.Backend("gpu", cfg, iset, env if env is not None else env0, ncells=N)
    b.set_orgs(0, pu.mutants_of(anc, iset, N // 2, rate=0.02, seed=11), deterministic=False)
    b.anc = anc
    return b


def _plain_cycle(golden):
    b = _world(golden)
    for _ in range(2):
        b.run_update()
    b.close()


@pytest.mark.gpu
def test_plain_world_returns_the_count(golden):
    base = _live()
    b = _world(golden)
    assert _live() > base
    for _ in range(2):
        b.run_update()
    b.close()
    assert _live() == base


@pytest.mark.gpu
def test_ten_cycles_leave_the_count(golden):
    base = _live()
    for _ in range(10):
        _plain_cycle(golden)
    assert _live() == base


@pytest.mark.gpu
def test_batch_world_with_every_lazy_allocation(golden):
    """resources (spatial + CELL entries, loaded twice), recorded streams, the
    genotype table, the arbiter, the test CPU, landscapes over two scratch
    worlds, states, digests, the census: each call checked for success"""
    base = _live()
    env = files.read_environment(os.path.join(golden, "spatial_res_100u", "environment.cfg"))
    assert any(r.geometry != 0 for r in env.resources) and len(env.cells) > 0
    b = _world(golden, env=env)
    lib, h = b.lib, b.h
    b.load_resources(env)                    # again: the CELL entries' buffer is replaced
    b.run_update()
    rnd = np.random.default_rng(3).random(20000)
    b.set_rng_mode(capi.RNG_RECORDED, rnd, np.arange(N, dtype=np.int64) * 11)
    b.run_update()
    b.set_rng_mode(capi.RNG_COUNTER)
    b.run_update()
    rows, totals = capi.get_genotypes(lib, h)
    assert len(rows) >= 2
    capi.classify_genotypes(lib, h, 1, 3)
    capi.classify_genotypes(lib, h, 2, 3)
    arb = capi.get_arbiter(lib, h)
    capi.set_arbiter(lib, h, arb[0], arb[2], arb[3])
    assert lib.avgpu_reset_arbiter(h) == 0
    assert len(b.test_genomes([b.anc, b.anc[:50]])) == 2
    landscape.set_chunk(b, 2048)
    out, sc, chart = landscape.call(b, [b.anc], 1, chart=True)
    assert int(out[0]["total_count"]) > 0 and chart is not None
    landscape.set_chunk(b, 1024)             # the scratch world is re-created
    out, sc = landscape.call_indel(b, [b.anc], landscape.INSERT)
    assert int(out[0]["total_count"]) > 0
    st, ops, fl = b.states(0, N)
    b._call("set_states", h, 0, N, st, (C.c_uint8 * len(ops)).from_buffer_copy(ops),
            (C.c_uint8 * len(fl)).from_buffer_copy(fl), capi.MAX_GENOME)
    assert len(b.digests()) == N
    assert len(b.census()) == N
    b.close()
    assert _live() == base


@pytest.mark.gpu
@pytest.mark.parametrize("birth_method", [4, 5])
def test_serial_world_with_its_lazy_allocations(golden, birth_method):
    """the serial world's state (BIRTH_METHOD 4: the soup; 5: the reaper queue)
    and both recorded streams, set twice so that each is replaced once"""
    base = _live()
    b = _world(golden, BIRTH_METHOD=birth_method)
    for seed in (6, 7):
        sched = np.ascontiguousarray(np.random.default_rng(seed).random(30000))
        ctx = np.ascontiguousarray(np.random.default_rng(seed + 10).random(30000))
        b._call("set_serial_streams", b.h, sched.ctypes.data_as(C.c_void_p), len(sched),
                ctx.ctypes.data_as(C.c_void_p), len(ctx))
    st = b.run_serial_update()
    assert st.num_organisms > 0
    assert len(b.digests()) == N
    b.close()
    assert _live() == base


@pytest.mark.gpu
def test_refused_calls_return_to_the_count(golden):
    """argument refusals on a living world: nothing they allocated stays"""
    b = _world(golden)
    lib, h = b.lib, b.h
    b.run_update()
    rows, totals = capi.get_genotypes(lib, h)        # (its scratch and row buffer exist from here on)
    assert len(rows) >= 2
    st, ops, fl = b.states(0, 1)
    assert st[0].mem_size > 0
    bad_ops = (C.c_uint8 * len(ops)).from_buffer_copy(bytes([255]) + ops[1:])
    flags = (C.c_uint8 * len(fl)).from_buffer_copy(fl)
    one_row = np.zeros(1, dtype=rows.dtype)
    tot = capi.GENOTYPE_TOTALS()
    bad_genome = [bytes([255] * 12)]

    def refused_landscape():
        with pytest.raises(RuntimeError):
            landscape.call(b, bad_genome, 1)
        return -1

    refusals = {
        "get_genotypes, cap below the table": lambda: lib.avgpu_get_genotypes(
            h, one_row.ctypes.data_as(C.c_void_p), 1, C.byref(tot)),
        "set_states, op outside the set": lambda: lib.avgpu_set_states(h, 0, 1, st, bad_ops, flags, capi.MAX_GENOME),
        "landscapes, op outside the set": refused_landscape,
        "step, budget 2^30": lambda: lib.avgpu_step(h, 0, 1, None, 1 << 30, capi.MODE_FROZEN),
    }
    for what, call in refusals.items():
        before = _live()
        assert call() < 0, what
        assert _live() == before, what
    b.run_update()                                   # the world is still alive
    b.close()
