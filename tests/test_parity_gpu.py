"""GPU parity: the HIP interpreter (through the C-ABI) against the CPU oracle
and the reference's golden vectors.  Integer/byte state must match bit for bit;
doubles (merit, bonus, fitness) must match exactly too, because both sides
perform the same IEEE operations without contraction."""
import os

import pytest

from avida_amd import capi, files
import oracle_lib as ol
import parity_util as pu
from res_util import bits

pytestmark = pytest.mark.gpu
CAP = capi.MAX_GENOME


def _pair(golden, n, instset="instset-heads.cfg", overrides=None, seed=7):
    iset, env, cfg = pu.load_env(golden, instset, overrides, seed)
    return (ol.Backend("oracle", cfg, iset, env, ncells=n),
            ol.Backend("gpu", cfg, iset, env, ncells=n), iset)


def _run_compare(orc, gpu, n, chunks, mode=capi.MODE_FROZEN):
    for budget in chunks:
        orc.step(0, n, uniform=budget, mode=mode)
        gpu.step(0, n, uniform=budget, mode=mode)
        a, oa, fa = orc.states(0, n, CAP)
        b, ob, fb = gpu.states(0, n, CAP)
        bad = pu.diff_states(a, b, oa, ob, fa, fb, CAP)
        assert not bad, f"{len(bad)} mismatches after budget {budget}: {bad[:5]}"


def test_test_cpu_detail_recalc_on_gpu(golden):
    """All 1794 golden genomes recalculated by the GPU test-CPU path."""
    iset, env, cfg = pu.load_env(golden, "instset-classic.cfg")
    gpu = ol.Backend("gpu", cfg, iset, env, ncells=16)
    fmt, rows = files.parse_detail_dat(os.path.join(golden, "detail-recalc.dat"))
    genomes = [iset.parse_sequence(r[8]) for r in rows]
    res = ol.recalculate(gpu, genomes)
    bad = []
    for row, (r, flags, viable) in zip(rows, res):
        got = [int(viable), r.copied_size, r.executed_size, "%g" % r.merit, r.gestation_time,
               flags, [int(x) for x in list(r.task_count)[:9]]]
        exp = [int(row[10]), int(row[11]), int(row[12]), "%g" % float(row[13]), int(row[15]),
               row[19], [int(x) for x in row[20:29]]]
        if got != exp:
            bad.append((row[0], exp, got))
    assert not bad, f"{len(bad)} mismatches: {bad[:3]}"


@pytest.mark.parametrize("death", [0, 2])
def test_frozen_population_config2(golden, death):
    """BASELINE config 2: frozen 3600-organism population, mutations off,
    10^4 instructions per organism; per-lane state compared after every chunk."""
    iset_c = files.read_instset(os.path.join(golden, "instset-classic.cfg"))
    genomes = pu.pop_genomes(golden, iset_c)
    anc = files.read_org(os.path.join(golden, "default-heads.org"),
                         files.read_instset(os.path.join(golden, "instset-heads.cfg")))
    # the ancestor re-expressed in classic op codes
    heads = files.read_instset(os.path.join(golden, "instset-heads.cfg"))
    anc_c = bytes(iset_c.op_of_name(heads.names[o]) for o in anc)
    genomes = genomes[:3599] + [anc_c]
    n = len(genomes)
    assert n == 3600
    ov = {"COPY_MUT_PROB": 0.0, "DIVIDE_INS_PROB": 0.0, "DIVIDE_DEL_PROB": 0.0,
          "DEATH_METHOD": death}
    orc, gpu, iset = _pair(golden, n, "instset-classic.cfg", ov)
    orc.set_orgs(0, genomes, deterministic=False)
    gpu.set_orgs(0, genomes, deterministic=False)
    _run_compare(orc, gpu, n, [1, 29, 970, 3000, 6000])


def test_random_genomes_fuzz(golden):
    """Random genomes 8..2048 sites (all LDS size classes, faults): by the
    class view of the oracle's states (parity_util.class_view) organisms of
    every class run a slice in every chunk.  No spills: an organism that has
    not allocated is classed by what h-alloc would grow it to, and no memory
    here shrinks and grows again, so the class view expects none and
    AVGPU_CNT_SPILLS agrees (tests/test_size_classes.py builds the spills)."""
    orc, gpu, iset = _pair(golden, 512, overrides={"DEATH_METHOD": 0})
    g = pu.random_genomes(iset, 384, 8, 300, seed=11) + pu.random_genomes(iset, 128, 300, 2048, seed=12)
    orc.set_orgs(0, g, deterministic=False)
    gpu.set_orgs(0, g, deterministic=False)
    for budget in [1, 7, 500, 1500]:
        before = pu.state_array(orc)
        _run_compare(orc, gpu, len(g), [budget])
        after = pu.state_array(orc)
        _, cls, _ = pu.class_view(before, "step_frozen")
        ran = (before["alive"] != 0) & (after["time_used"] > before["time_used"])
        assert set(cls[ran].tolist()) == {0, 1, 2, 3}, budget
        # the premise of expected_spills, a property of these genomes and not of
        # the product: none divides, so no memory shrinks (fails: pick other seeds)
        assert (after["mem_size"] >= before["mem_size"]).all()
        assert gpu.counters()[capi.CNT_SPILLS] == pu.expected_spills(before, after, "step_frozen").sum(), budget


def test_ancestor_mutants_fuzz(golden):
    """Point mutants of the ancestor with copy mutations ON (FROZEN mode draws
    copy mutations from the per-organism counter stream on both sides)."""
    orc, gpu, iset = _pair(golden, 1024, overrides={"DEATH_METHOD": 0, "COPY_MUT_PROB": 0.02})
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    g = pu.mutants_of(anc, iset, 1024, rate=0.03, seed=5)
    orc.set_orgs(0, g, deterministic=False)
    gpu.set_orgs(0, g, deterministic=False)
    _run_compare(orc, gpu, len(g), [250, 750, 2000])


@pytest.mark.timeout(900)
def test_world_updates_bit_exact(golden):
    """BASELINE.json configs[0] at its stated length: the default avida.cfg
    world (60x60 torus, heads_default, logic-9, default mutation rates), the
    default-heads ancestor injected once, 1000 full batch-synchronous updates
    (allot, interpret with copy/divide mutations, time-ordered placement,
    activation): every update's counters equal, then GPU world == oracle
    world, every cell, every field, and the cell digests."""
    iset, env, cfg = pu.load_env(golden, seed=101)
    n = cfg.world_x * cfg.world_y
    orc = ol.Backend("oracle", cfg, iset, env, ncells=n)
    gpu = ol.Backend("gpu", cfg, iset, env, ncells=n)
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    center = (cfg.world_y // 2) * cfg.world_x + cfg.world_x // 2
    for b in (orc, gpu):
        b.set_orgs(center, [anc], deterministic=False)
    for upd in range(1000):
        so = orc.run_update()
        sg = gpu.run_update()
        for f in ("num_organisms", "insts_executed", "births", "deaths", "divides", "births_dropped",
                  "births_overwritten", "births_cancelled", "cum_insts_executed", "cum_births"):
            assert getattr(so, f) == getattr(sg, f), (upd, f, getattr(so, f), getattr(sg, f))
        assert list(so.task_orgs) == list(sg.task_orgs), upd
    a, oa, fa = orc.states(0, n, CAP)
    b, ob, fb = gpu.states(0, n, CAP)
    bad = pu.diff_states(a, b, oa, ob, fa, fb, CAP)
    assert not bad, f"{len(bad)} mismatches: {bad[:5]}"
    nbad, cells = pu.compare_digests(orc.digests(0, n), gpu.digests(0, n))
    assert nbad == 0, f"{nbad} cell digests differ, first {cells}"
    assert so.num_organisms > 3000 and so.update == 999
    assert gpu.counters(cumulative=1)[capi.CNT_BAD_RECORD] == 0


# cells of test_handed_in_totals_equal_oracle overwritten with random genomes,
# and their lengths: an organism that has not allocated needs a slot for three
# times its size (device.h need_of at OFFSPRING_SIZE_RANGE 2), so 200 / 400 /
# 1700 sites start in list classes 1 / 2 / 3 and stay there after h-alloc
HANDED_IN_LONG = ((700, 200, 41), (1800, 400, 42), (2900, 1700, 43))


def handed_in_world(golden):
    """The world of test_handed_in_totals_equal_oracle: (iset, env, cfg,
    genomes, merits) -- detail-50000.pop's 3599 organisms and the ancestor on
    the default 60x60 torus with the merits the file records (injected without
    them the first offspring hold 10^7 times their neighbours' merit, and the
    world has 35 births in 25 updates), three cells overwritten with long
    random genomes at the population's highest merit, so that every update
    gives them a slice."""
    iset, env, cfg = pu.load_env(golden, "instset-classic.cfg", seed=101)
    genomes = pu.pop_genomes(golden, iset)
    merits = [g.merit for g in files.read_pop(os.path.join(golden, "detail-50000.pop")) for _ in range(g.num_cpus)]
    heads = files.read_instset(os.path.join(golden, "instset-heads.cfg"))
    anc = files.read_org(os.path.join(golden, "default-heads.org"), heads)
    genomes = genomes[:3599] + [bytes(iset.op_of_name(heads.names[o]) for o in anc)]
    merits = merits[:3599] + [0.0]
    assert len(genomes) == len(merits) == cfg.world_x * cfg.world_y == 3600
    for cell, length, seed in HANDED_IN_LONG:
        genomes[cell], = pu.random_genomes(iset, 1, length, length, seed=seed)
        merits[cell] = max(merits)
    return iset, env, cfg, genomes, merits


def handed_in_view(orc, n):
    """the oracle's state records as a numpy array, and each cell's size class
    (device.h need_of / class_of at the default OFFSPRING_SIZE_RANGE 2)"""
    s = pu.state_array(orc, n)
    return s, pu.class_view(s, "update")[1]


def handed_in_ran(s, cls, s2):
    """the size classes of the organisms of s that ran a slice before s2: alive
    in both, the same organism (its RNG key), time_used advanced"""
    same = (s["alive"] != 0) & (s2["alive"] != 0) & (s["rng_key_lo"] == s2["rng_key_lo"]) & \
        (s["rng_key_hi"] == s2["rng_key_hi"])
    return set(cls[same & (s2["time_used"] > s["time_used"])].tolist())


def test_handed_in_totals_equal_oracle(golden):
    """Updates whose totals are handed in (avgpu_set_global_totals: the path of
    avgpu_update_run, k_block_counts mode 2) against the oracle's: a full
    60x60 world of evolved organisms plus three long random genomes, so that
    the list classes 1..3 run inside class 0's launch; before each of 25
    updates both backends get the totals of two such worlds -- twice the
    oracle world's organisms and summed merit, not this world's own, which
    mode 0 would also reproduce.  Every update's counters equal, then every
    cell, field and digest; at least 100 births and a slice run in each list
    class (the oracle alone: 4907 births, classes 0..3)."""
    iset, env, cfg, genomes, merits = handed_in_world(golden)
    n = len(genomes)
    orc = ol.Backend("oracle", cfg, iset, env, ncells=n)
    gpu = ol.Backend("gpu", cfg, iset, env, ncells=n)
    for b in (orc, gpu):
        b.set_orgs(0, genomes, merits, deterministic=False)
    births, classes = 0, set()
    s, cls = handed_in_view(orc, n)
    for upd in range(25):
        alive = s["alive"] != 0
        merit, orgs = 2.0 * float(s["merit"][alive].sum()), 2 * int(alive.sum())
        for b in (orc, gpu):
            b._call("set_global_totals", b.h, merit, orgs)
        so = orc.run_update()
        sg = gpu.run_update()
        for f in ("num_organisms", "insts_executed", "births", "deaths", "divides", "births_dropped",
                  "births_overwritten", "births_cancelled", "cum_insts_executed", "cum_births"):
            assert getattr(so, f) == getattr(sg, f), (upd, f, getattr(so, f), getattr(sg, f))
        assert list(so.task_orgs) == list(sg.task_orgs), upd
        births += so.births
        s2, cls2 = handed_in_view(orc, n)
        classes |= handed_in_ran(s, cls, s2)
        s, cls = s2, cls2
    a, oa, fa = orc.states(0, n, CAP)
    b, ob, fb = gpu.states(0, n, CAP)
    bad = pu.diff_states(a, b, oa, ob, fa, fb, CAP)
    assert not bad, f"{len(bad)} mismatches: {bad[:5]}"
    nbad, cells = pu.compare_digests(orc.digests(0, n), gpu.digests(0, n))
    assert nbad == 0, f"{nbad} cell digests differ, first {cells}"
    assert births >= 100 and classes >= {1, 2, 3}, (births, classes)
    assert gpu.counters(cumulative=1)[capi.CNT_BAD_RECORD] == 0


STATS_INT_FIELDS = ("update", "num_organisms", "insts_executed", "births", "births_dropped", "deaths", "divides",
                    "cum_insts_executed", "cum_births", "slices", "births_overwritten", "births_cancelled", "seed",
                    "sched_pred", "sched_pred_n", "sub_steps", "sched_carry", "insts_wasted", "sched_pred_cnt")
STATS_SUM_FIELDS = ("sum_merit", "sum_fitness", "sum_gestation", "sum_genome_length", "sum_mem_size",
                    "ave_generation")


def test_every_stats_field_equals_oracle(golden):
    """Every field of avgpu_update_stats of a batch-world update, GPU against
    oracle: the statistics vector's slots (device.h ST_*) one by one, so that
    a swapped or shifted slot fails here and not only where it bends a later
    trajectory.  handed_in_world on its own totals, adaptive batch steps
    (sub_updates = 0): 20 updates, avgpu_set_clock on both backends with their
    own last statistics (every slot it writes: the running sums, the pick
    carry, the predictor's shard words and organisms), 20 more.  Integer
    fields and max_fitness equal; the double sums and ave_generation within
    1e-12 relative (sums added in different orders: test_serial_gpu's bound);
    lane_steps, which the oracle does not produce, positive.  On the oracle's
    own values: every compared field but births_dropped non-zero in some
    update, an update of more than one batch step, a pick carry of each
    sign."""
    import ctypes as C
    iset, env, cfg, genomes, merits = handed_in_world(golden)
    cfg.sub_updates = 0
    n = len(genomes)
    orc = ol.Backend("oracle", cfg, iset, env, ncells=n)
    gpu = ol.Backend("gpu", cfg, iset, env, ncells=n)
    for b in (orc, gpu):
        b.set_orgs(0, genomes, merits, deterministic=False)
    ntask = 9                              # the logic-9 tasks
    seen = {f: False for f in STATS_INT_FIELDS + STATS_SUM_FIELDS + ("max_fitness",)}
    seen.update({("task_orgs", t): False for t in range(ntask)})
    seen.update({("sched_pred_bins", q): False for q in range(4)})
    steps, carries = [], []
    for upd in range(40):
        if upd == 20:
            for b, st in ((orc, so), (gpu, sg)):
                b._call("set_clock", b.h, C.byref(st))
        so = orc.run_update()
        sg = gpu.run_update()
        for f in STATS_INT_FIELDS:
            assert getattr(so, f) == getattr(sg, f), (upd, f, getattr(so, f), getattr(sg, f))
        assert list(so.task_orgs) == list(sg.task_orgs), (upd, list(so.task_orgs), list(sg.task_orgs))
        assert list(so.sched_pred_bins) == list(sg.sched_pred_bins), (upd, list(so.sched_pred_bins),
                                                                      list(sg.sched_pred_bins))
        assert so.max_fitness == sg.max_fitness, (upd, so.max_fitness, sg.max_fitness)
        for f in STATS_SUM_FIELDS:
            a, b = getattr(so, f), getattr(sg, f)
            assert abs(a - b) <= 1e-12 * abs(a), (upd, f, a, b)
        assert sg.lane_steps > 0, upd
        for f in STATS_INT_FIELDS + STATS_SUM_FIELDS + ("max_fitness",):
            seen[f] |= getattr(so, f) != 0
        for t in range(ntask):
            seen[("task_orgs", t)] |= so.task_orgs[t] != 0
        for q in range(4):
            seen[("sched_pred_bins", q)] |= so.sched_pred_bins[q] != 0
        steps.append(so.sub_steps)
        carries.append(so.sched_carry)
    never = [f for f, s in seen.items() if not s and f != "births_dropped"]
    assert not never, f"always zero in the oracle: {never}"
    assert max(steps) > 1, steps
    assert min(carries) < 0 < max(carries), carries


def test_update_totals_stays_within_its_buffer(golden):
    """avgpu_update_totals writes the two doubles its header documents --
    the sum of scheduler weights and the living organisms -- and nothing past
    them: of an 8-double device buffer of sentinels, doubles 2..7 keep their
    bits.  handed_in_world as loaded: no organism is a fresh newborn, so its
    weight is its merit."""
    import ctypes as C
    import numpy as np
    import torch
    iset, env, cfg, genomes, merits = handed_in_world(golden)
    n = len(genomes)
    gpu = ol.Backend("gpu", cfg, iset, env, ncells=n)
    gpu.set_orgs(0, genomes, merits, deterministic=False)
    sentinel = 0x7FF4C0DE5E1271E1          # a NaN no sum produces
    buf = torch.full((8,), sentinel, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu._call("update_totals", gpu.h, C.c_void_p(buf.data_ptr()))
    gpu.lib.avgpu_sync(gpu.h)
    got = buf.cpu().numpy()
    assert got[2:].tolist() == [sentinel] * 6, [hex(v) for v in got.tolist()]
    weight, orgs = got[:2].view(np.float64).tolist()
    s, _ = handed_in_view(gpu, n)
    alive = s["alive"] != 0
    assert orgs == int(alive.sum()) > 0, (orgs, int(alive.sum()))
    want = float(s["merit"][alive].sum())
    assert want > 0 and abs(weight - want) <= 1e-12 * want, (weight, want)


def test_lazy_statistics_equal_eager(golden):
    """An update run with out == NULL skips the statistics reduction (the bench
    regime); the counts still reach the running sums (folded in by the next
    update's counter reset) and avgpu_get_stats reduces on demand: the same
    world run lazily equals the world run with statistics every update --
    stats, per-update and cumulative counters, every cell."""
    import ctypes as C
    iset, env, cfg = pu.load_env(golden, seed=101)
    n = cfg.world_x * cfg.world_y
    eager = ol.Backend("gpu", cfg, iset, env, ncells=n)
    lazy = ol.Backend("gpu", cfg, iset, env, ncells=n)
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    for b in (eager, lazy):
        b.set_orgs(n // 2 + 30, [anc], deterministic=False)
    fields = [f for f, _ in capi.AvgpuUpdateStats._fields_]

    def vals(st):
        return [list(v) if hasattr(v, "__len__") else v for v in (getattr(st, f) for f in fields)]

    for upd in range(120):
        se = eager.run_update()
        lazy._call("run_update", lazy.h, None)
        if upd % 7 == 6 or upd > 110:
            sl = capi.AvgpuUpdateStats()
            lazy._call("get_stats", lazy.h, C.byref(sl))
            assert vals(se) == vals(sl), upd
            assert eager.counters(1) == lazy.counters(1), upd
            assert eager.counters(0) == lazy.counters(0), upd
        elif upd % 5 == 0:
            assert eager.counters(1) == lazy.counters(1), upd      # shards still pending
    assert se.num_organisms > 100 and se.cum_births > 100
    assert (eager.digests() == lazy.digests()).all()


@pytest.mark.parametrize("T,geometry", [(2, 2), (4, 2), (2, 1)])
def test_gpu_strip_tiles_equal_single_world(golden, T, geometry):
    """Multi-GPU row on one GPU: T strips of one 64x64 world run
    through the halo protocol (avida_amd/tiles.py, in-process loopback
    transport) equal the untiled oracle world, every cell, every field."""
    import torch
    from avida_amd import tiles
    import tile_util as tu
    X, Y, U = 64, 64, 40
    ref, rstats = tu.single("oracle", golden, X, Y, U, geometry=geometry)
    pairs = [tu.make_tile("gpu", golden, X, Y, T, k, geometry=geometry, device="cuda")
             for k in range(T)]
    world = tiles.StripWorld([t for _, t in pairs], tiles.LoopbackTransport())
    sent = 0
    for u in range(U):
        world.update()
        torch.cuda.synchronize()
        sent += sum(tu.records_sent(t) for _, t in pairs)
        tot = [tu.tile_stats(b) for b, _ in pairs]
        for f in ("num_organisms", "insts_executed", "births", "deaths", "divides", "births_dropped",
                  "births_overwritten"):
            assert sum(getattr(s, f) for s in tot) == getattr(rstats[u], f), (u, f)
    a, oa, fa = ref.states(0, X * Y, CAP)
    per = X * Y // T
    for k, (b, _) in enumerate(pairs):
        s, o, f = b.states(0, per, CAP)
        lo = k * per
        bad = pu.diff_states(a[lo:lo + per], s, oa[lo * CAP:(lo + per) * CAP], o,
                             fa[lo * CAP:(lo + per) * CAP], f, CAP)
        assert not bad, f"tile {k}: {len(bad)} mismatches, first {bad[:3]}"
    assert sent > 0


def _resource_env(golden, variant):
    """spatial_res_100u's environment (variant "flow": diffusion and gravity on,
    a torus ResA and a grid ResB, so FlowAll runs) or resources_9r's nine
    consumed global pools"""
    import copy
    if variant == "bench":
        import bench
        return files.parse_environment(bench.resource_env_text(48, 40)), \
            files.read_instset(os.path.join(golden, "resources_9r", "instset-heads.cfg")).parse_sequence(
                "rucavcqgfcqapqeccthzscpcccpqcxaqnccxxbcgdutycasvab")
    if variant == "9r":
        d = os.path.join(golden, "resources_9r")
        return files.read_environment(os.path.join(d, "environment.9resource")), \
            files.read_org(os.path.join(d, "9task.org"),
                           files.read_instset(os.path.join(d, "instset-heads.cfg")))
    env = files.read_environment(os.path.join(golden, "spatial_res_100u", "environment.cfg"))
    if variant in ("flow", "diffuse"):
        env = copy.deepcopy(env)
        a, b = env.resources[0], env.resources[1]
        a.geometry, a.xdiffuse, a.ydiffuse, a.xgravity, a.ygravity = 2, 1.0, 0.5, 0.2, -0.1
        a.inflow_x1, a.inflow_x2, a.inflow_y1, a.inflow_y2 = 40, 50, 45, 52    # box wraps the torus
        b.xdiffuse, b.ydiffuse, b.xgravity, b.ygravity = 0.3, 1.0, -0.4, 0.25
        if variant == "diffuse":     # zero gravity (one axis of ResB only)
            a.xgravity = a.ygravity = 0.0
            b.xgravity = 0.0
            # the global pool first (resource index != spatial slot), drawn on by AND
            order = [2, 0, 1]
            env.resources[:] = [env.resources[i] for i in order]
            for r in env:
                if r.resource:
                    r.resource = 1 + order.index(r.resource - 1)
            for c in env.cells:
                c.resource = order.index(c.resource)
            env[2].resource, env[2].max_fraction, env[2].max_number = 1, 0.01, 5.0
    iset = files.read_instset(os.path.join(golden, "resources_9r", "instset-heads.cfg"))
    return env, iset.parse_sequence("rucavcqgfcqapqeccthzscpcccpqcxaqnccxxbcgdutycasvab")


@pytest.mark.parametrize("variant", ["spatial", "flow", "diffuse", "9r", "bench"])
def test_world_updates_resources_bit_exact(golden, variant):
    """Updates with environment resources (the environment around the
    path): spatial grids, CELL lists, diffusion/gravity flows and consumed
    global pools; GPU world == oracle world, every cell, every field, and every
    resource level and per-cell amount bit for bit."""
    env, anc = _resource_env(golden, variant)
    iset = files.read_instset(os.path.join(golden, "resources_9r", "instset-heads.cfg"))
    cfg = capi.cfg_from_avida(files.read_avida_cfg(None, {"WORLD_X": 48, "WORLD_Y": 40}), seed=23)
    n = cfg.world_x * cfg.world_y
    orc = ol.Backend("oracle", cfg, iset, env, ncells=n)
    gpu = ol.Backend("gpu", cfg, iset, env, ncells=n)
    for b in (orc, gpu):
        b.set_orgs(0, [anc] * 200, [100.0] * 200, deterministic=False)
    for upd in range(60):
        so = orc.run_update()
        sg = gpu.run_update()
        for f in ("num_organisms", "insts_executed", "births", "deaths", "divides"):
            assert getattr(so, f) == getattr(sg, f), (upd, f, getattr(so, f), getattr(sg, f))
        lo, go = orc.resources(spatial=True)
        lg, gg = gpu.resources(spatial=True)
        assert bits(lo) == bits(lg), (upd, lo, lg)          # bit patterns: -0.0 is not 0.0
        assert [bits(g) for g in go] == [bits(g) for g in gg], upd
    a, oa, fa = orc.states(0, n, CAP)
    b, ob, fb = gpu.states(0, n, CAP)
    bad = pu.diff_states(a, b, oa, ob, fa, fb, CAP)
    assert not bad, f"{len(bad)} mismatches: {bad[:5]}"
    assert so.num_organisms > 200


@pytest.mark.parametrize("shape", [(130, 37), (5, 7), (63, 18), (2, 33), (124, 16)])
def test_resource_step_world_shapes(golden, shape):
    """k_res_step's windows (62 written columns x 8 rows a wave, the rim lanes
    wrapping mod WORLD_X): worlds narrower than a window, a last window that
    wraps, row counts off the band size, a torus and a grid resource with
    diffusion and gravity -- every level and per-cell amount == the oracle's
    after every update."""
    env, anc = _resource_env(golden, "flow")
    iset = files.read_instset(os.path.join(golden, "resources_9r", "instset-heads.cfg"))
    X, Y = shape
    cfg = capi.cfg_from_avida(files.read_avida_cfg(None, {"WORLD_X": X, "WORLD_Y": Y}), seed=29)
    n = X * Y
    orc = ol.Backend("oracle", cfg, iset, env, ncells=n)
    gpu = ol.Backend("gpu", cfg, iset, env, ncells=n)
    k = min(60, n // 2)
    for b in (orc, gpu):
        b.set_orgs(0, [anc] * k, [100.0] * k, deterministic=False)
    for upd in range(25):
        so, sg = orc.run_update(), gpu.run_update()
        assert (so.num_organisms, so.insts_executed, so.births) == (sg.num_organisms, sg.insts_executed, sg.births)
        lo, go = orc.resources(spatial=True)
        lg, gg = gpu.resources(spatial=True)
        assert bits(lo) == bits(lg), (upd, lo, lg)          # bit patterns: -0.0 is not 0.0
        assert [bits(g) for g in go] == [bits(g) for g in gg], upd
    assert (orc.digests() == gpu.digests()).all()


@pytest.mark.parametrize("variant", ["logic9", "9r"])
def test_world_subupdates_bit_exact(golden, variant):
    """sub_updates = 3 (DESIGN.md 5 "Sub-updates": an update's picks in three
    batch steps, the scheduler weights re-read before each, resources stepped
    once per update, global consumption settled after each step): GPU world ==
    oracle world, every update's counters (summed over the steps), every
    resource level, then every cell, field and digest."""
    if variant == "logic9":
        iset, env, cfg = pu.load_env(golden, seed=31)
        anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
        orgs, merits, updates = [anc], None, 400
    else:
        env, anc = _resource_env(golden, variant)
        iset = files.read_instset(os.path.join(golden, "resources_9r", "instset-heads.cfg"))
        cfg = capi.cfg_from_avida(files.read_avida_cfg(None, {"WORLD_X": 48, "WORLD_Y": 40}), seed=23)
        orgs, merits, updates = [anc] * 200, [100.0] * 200, 60
    cfg.sub_updates = 3
    n = cfg.world_x * cfg.world_y
    orc = ol.Backend("oracle", cfg, iset, env, ncells=n)
    gpu = ol.Backend("gpu", cfg, iset, env, ncells=n)
    for b in (orc, gpu):
        b.set_orgs(0 if merits else n // 2 + cfg.world_x // 2, orgs, merits, deterministic=False)
    for upd in range(updates):
        so = orc.run_update()
        sg = gpu.run_update()
        for f in ("num_organisms", "insts_executed", "births", "deaths", "divides", "births_dropped",
                  "births_overwritten", "births_cancelled", "cum_insts_executed", "cum_births", "slices"):
            assert getattr(so, f) == getattr(sg, f), (upd, f, getattr(so, f), getattr(sg, f))
        assert list(so.task_orgs) == list(sg.task_orgs), upd
        if variant != "logic9":
            assert orc.resources(spatial=True) == gpu.resources(spatial=True), upd
    # the update's picks are UD = AVE_TIME_SLICE x N split over the steps
    assert so.num_organisms > 100
    a, oa, fa = orc.states(0, n, CAP)
    b, ob, fb = gpu.states(0, n, CAP)
    bad = pu.diff_states(a, b, oa, ob, fa, fb, CAP)
    assert not bad, f"{len(bad)} mismatches: {bad[:5]}"
    nbad, cells = pu.compare_digests(orc.digests(0, n), gpu.digests(0, n))
    assert nbad == 0, f"{nbad} cell digests differ, first {cells}"
    assert gpu.counters(cumulative=1)[capi.CNT_BAD_RECORD] == 0


@pytest.mark.parametrize("T,geometry,env_kind", [(2, 2, "tile"), (4, 1, "tile"), (4, 2, "bench")])
def test_gpu_strip_tiles_with_resources(golden, T, geometry, env_kind):
    """Config 5's path on one GPU: T strips with spatial resources (flows,
    inflow box and CELL list across strip edges, edge rows exchanged) and a
    consumed global pool (consumption all-reduced) == the untiled oracle world:
    organisms, per-cell amounts and pool levels bit for bit, every update."""
    import torch
    from avida_amd import tiles
    import tile_util as tu
    from test_tiles import resource_grids_match
    X, Y, U = 64, 64, 30
    if env_kind == "bench":          # configs[4]'s environment (bench.py --env resources)
        import bench
        env = files.parse_environment(bench.resource_env_text(X, Y))
    else:
        env = tu.resource_env(golden)
    per_update = []
    ref, rstats = tu.single("oracle", golden, X, Y, U, geometry=geometry, env=env,
                            on_update=lambda u, b: per_update.append(b.resources(spatial=True)))
    pairs = [tu.make_tile("gpu", golden, X, Y, T, k, geometry=geometry, device="cuda", env=env)
             for k in range(T)]
    world = tiles.StripWorld([t for _, t in pairs], tiles.LoopbackTransport())
    for u in range(U):
        world.update()
        torch.cuda.synchronize()
        tot = [tu.tile_stats(b) for b, _ in pairs]
        for f in ("num_organisms", "insts_executed", "births", "deaths", "divides"):
            assert sum(getattr(s, f) for s in tot) == getattr(rstats[u], f), (u, f)
        resource_grids_match(per_update[u], [b for b, _ in pairs], T, X, Y)
    a, oa, fa = ref.states(0, X * Y, CAP)
    per = X * Y // T
    for k, (b, _) in enumerate(pairs):
        s, o, f = b.states(0, per, CAP)
        lo = k * per
        bad = pu.diff_states(a[lo:lo + per], s, oa[lo * CAP:(lo + per) * CAP], o,
                             fa[lo * CAP:(lo + per) * CAP], f, CAP)
        assert not bad, f"tile {k}: {len(bad)} mismatches, first {bad[:3]}"


@pytest.mark.parametrize("kinds", [("gpu", "gpu"), ("gpu", "oracle"), ("oracle", "gpu")])
@pytest.mark.parametrize("env_kind", ["logic9", "resources"])
def test_checkpoint_resume_across_backends(golden, tmp_path, kinds, env_kind):
    """A checkpoint written by one backend and restored into the other (or the
    same) continues bit for bit like the world that never stopped."""
    from test_checkpoint import resume_case
    resume_case(kinds[0], kinds[1], golden, env_kind, tmp_path)


def test_driver_gpu_equals_oracle(golden, tmp_path):
    """avida_amd/driver.py on the GPU (ProductWorld) and on the oracle over the
    spatial_res_100u config: the data files agree (count with its genotype
    columns, tasks, resource, dominant exactly: the census is equal; averages to print precision -- their sums reduce in another order)."""
    from avida_amd import driver
    cfgdir = os.path.join(golden, "spatial_res_100u", "config")
    g, o = tmp_path / "gpu", tmp_path / "oracle"
    dg = driver.Driver(cfgdir, str(g))
    assert dg.run() == 100
    dg.world.close()
    driver.Driver(cfgdir, str(o), make_world=lambda cfg, iset, env: ol.Backend("oracle", cfg, iset, env)).run()

    def rows(p):
        return [l.split() for l in open(p) if l.strip() and not l.startswith("#")]
    for name in ("count.dat", "tasks.dat", "resource.dat", "dominant.dat"):
        assert rows(g / name) == rows(o / name), name
    for name in ("average.dat", "time.dat"):
        for a, b in zip(rows(g / name), rows(o / name)):
            assert [float(x) for x in a] == pytest.approx([float(x) for x in b], rel=1e-5), name


def test_trace_every_instruction(golden):
    """Per-instruction traces (avida_amd/trace.py, the reference tracer's
    PrintStatus at cpu/cHardwareCPU.cc:956): 192 organisms -- ancestor mutants
    and evolved detail-50000 genotypes -- single-stepped 600 times with copy
    and divide mutations on; GPU state == oracle state before every one of the
    600 instructions (no divergence can hide between chunk boundaries), and the
    PrintStatus texts agree."""
    from avida_amd import trace
    iset, env, cfg = pu.load_env(golden, overrides={"COPY_MUT_PROB": 0.02, "DIVIDE_MUT_PROB": 0.05,
                                                    "DEATH_METHOD": 0})
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    iset_c = files.read_instset(os.path.join(golden, "instset-classic.cfg"))
    pop = [bytes(iset.op_of_name(iset_c.names[o]) for o in g) for g in pu.pop_genomes(golden, iset_c)[::40][:96]]
    g = pu.mutants_of(anc, iset, 96, rate=0.02, seed=4) + pop
    n = len(g)
    orc, gpu = (ol.Backend(k, cfg, iset, env, ncells=n) for k in ("oracle", "gpu"))
    for b in (orc, gpu):
        b.set_orgs(0, g, deterministic=False)
    for step in range(600):
        a, oa, fa = orc.states(0, n, 512)
        s, os_, fs = gpu.states(0, n, 512)
        nbad, rep = pu.diff_states_np(a, s, oa, os_, fa, fs, 512)
        assert nbad == 0, f"before instruction {step + 1}: {nbad} organisms differ {rep[:3]}"
        if step % 150 == 0:
            for i in range(0, n, 17):
                assert trace.status_text(a[i], oa[i * 512:(i + 1) * 512], iset) == \
                    trace.status_text(s[i], os_[i * 512:(i + 1) * 512], iset)
        orc.step(0, n, uniform=1, mode=capi.MODE_FROZEN)
        gpu.step(0, n, uniform=1, mode=capi.MODE_FROZEN)
    assert sum(a[i].num_divides for i in range(n)) > 0


@pytest.mark.parametrize("allow_parent", [0, 1])
def test_birth_method3_full_grid(golden, allow_parent):
    """BIRTH_METHOD 3 (an empty neighbour, else the parent's cell without a
    draw; cPopulation::PositionOffspring, main/cPopulation.cc:5407) on a full
    grid: with ALLOW_PARENT 0 the offspring is never placed and the parent
    lives (ActivateOffspring :706-713, BS_NO_CELL, counted as dropped); with
    ALLOW_PARENT 1 it replaces its parent.  Every update's counters equal,
    then every cell and digest, GPU world == oracle world."""
    ov = {"WORLD_X": 32, "WORLD_Y": 32, "BIRTH_METHOD": 3, "ALLOW_PARENT": allow_parent}
    iset, env, cfg = pu.load_env(golden, overrides=ov, seed=29)
    n = cfg.world_x * cfg.world_y
    orc = ol.Backend("oracle", cfg, iset, env, ncells=n)
    gpu = ol.Backend("gpu", cfg, iset, env, ncells=n)
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    for b in (orc, gpu):
        b.set_orgs(0, [anc] * n, deterministic=False)
    dropped = births = 0
    for upd in range(40):
        so, sg = orc.run_update(), gpu.run_update()
        for f in ("num_organisms", "insts_executed", "births", "deaths", "divides", "births_dropped",
                  "births_overwritten", "births_cancelled"):
            assert getattr(so, f) == getattr(sg, f), (upd, f, getattr(so, f), getattr(sg, f))
        dropped += so.births_dropped
        births += so.births
    if allow_parent:
        assert births > 0 and dropped == 0
    else:
        assert dropped > 0 and births == 0   # the grid stays full of the ancestors
    a, oa, fa = orc.states(0, n, CAP)
    b, ob, fb = gpu.states(0, n, CAP)
    bad = pu.diff_states(a, b, oa, ob, fa, fb, CAP)
    assert not bad, f"{len(bad)} mismatches: {bad[:5]}"
    assert gpu.counters(cumulative=1)[capi.CNT_BAD_RECORD] == 0
