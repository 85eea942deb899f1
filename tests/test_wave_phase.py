"""The interpreter's wave phase (avida_amd/csrc/interp_core.h interpret_chunk,
after its slow switch): h-alloc's fill, which every requesting lane writes into
its own tape at once (tape_fill), beside the divides and label searches, which
the wave serves one requesting lane after the other.

Worlds of hand-written organisms of one or two waves, constant slicing (a slice
is exactly AVE_TIME_SLICE instructions, so the lanes of a wave reach their first
instruction in the same iteration), GPU against the oracle after every update or
step: every cell's state record, its tape and flags, its digest, the update's
statistics, AVGPU_CNT_SPILLS where a world spills (the helpers of
test_stack_shift.py and test_size_classes.py).  What a world is built to show is
asserted from the oracle's states alone, in the unmarked tests as well, so that
a GPU test cannot pass vacuously."""
import os

import numpy as np
import pytest

from avida_amd import capi, files
import oracle_lib as ol
import parity_util as pu
import test_size_classes as tsc
import test_stack_shift as tss

CAP = capi.MAX_GENOME
ENVS = tss.ENVS                 # the class-0 kernel families: plain, REC, RES, !SIMPLE


def heads(golden):
    return files.read_instset(os.path.join(golden, "instset-heads.cfg"))


def alloc_genome(iset, length):
    """h-alloc, then nop-C"""
    return bytes([iset.op_of_name("h-alloc")]) + bytes([iset.op_of_name("nop-C")]) * (length - 1)


class TapeWorld(tss.World):
    """tss.World with construction-1 records (parity_util) put over its organisms"""

    records = ()

    def backend(self, kind):
        b = super().backend(kind)
        pu.put_records(b, self.records)
        return b


def tapes(backend, n):
    """(states, ops, flags) with the ops and flags as n x CAP arrays"""
    st, ops, fl = backend.states(0, n, CAP)
    return st, np.frombuffer(ops, dtype=np.uint8).reshape(n, CAP), np.frombuffer(fl, dtype=np.uint8).reshape(n, CAP)


# ---- fill alignment ----------------------------------------------------------

FILL_LENS = [20 + c % 32 for c in range(64)] + [37] * 64      # a = len, b = 3 len: every residue of both mod 16
FILL_LISTS = {70: 150, 90: 300, 110: 600}                    # cells of the second wave: classes 1 / 2 / 3


def fill_world(golden, env="def", lists=False):
    iset = heads(golden)
    lens = list(FILL_LENS)
    if lists:
        for c, length in FILL_LISTS.items():
            lens[c] = length
    w = TapeWorld(golden, 16, 8, [alloc_genome(iset, length) for length in lens], 3,
                  instset="instset-heads.cfg", env=env)
    w.lens = lens
    return w


def check_fill(world, ends):
    lens = np.array(world.lens)
    assert {(a % 16, 3 * a % 16) for a in lens[:64]} >= {(r, 3 * r % 16) for r in range(16)}
    assert {3 * a % 16 for a in lens[:64]} == set(range(16))
    first = ends[1]
    assert (ends[0]["mem_size"] == lens).all() and (first["mem_size"] == 3 * lens).all()
    assert (first["errors"] == 0).all() and (first["alive"] != 0).all() and (first["reg"][:, 0] == lens).all()
    # the new sites on the oracle: op 0 without a flag, behind the genome as it was
    orc = world.backend("oracle")
    _, ops0, _ = tapes(orc, world.n)
    orc.run_update()
    _, ops1, fl1 = tapes(orc, world.n)
    orc.close()
    for c, a in enumerate(lens):
        assert not ops1[c, a:3 * a].any() and not fl1[c, a:3 * a].any(), c
        assert (ops1[c, :a] == ops0[c, :a]).all() and ops1[c, 0] != 0, c


def test_fill_design_on_oracle(golden):
    world = fill_world(golden, lists=True)
    check_fill(world, tss.run(world, 2, with_gpu=False)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS)
def test_fill_alignment(golden, env):
    """64 lanes fill in the same iteration, from every a mod 16 to every b mod
    16; a second wave of equal lengths with one
    organism of each list class among them; in each class-0 kernel family"""
    world = fill_world(golden, env=env, lists=True)
    ends, _, _ = tss.run(world, 3, with_gpu=True, first_compare=True)
    check_fill(world, ends)


@pytest.mark.gpu
def test_fill_over_the_whole_tape(golden):
    """the tapes as avgpu_get_states returns them with the full capacity,
    after every update: the device's equal the oracle's over the whole slot"""
    world = fill_world(golden, lists=True)
    orc, gpu = world.backend("oracle"), world.backend("gpu")
    for u in range(3):
        for b in (orc, gpu):
            b.run_update()
        _, oo, of = tapes(orc, world.n)
        _, go, gf = tapes(gpu, world.n)
        assert (go == oo).all() and (gf == of).all(), u
    orc.close()
    gpu.close()


# ---- class bounds --------------------------------------------------------------

def bound_scenario(golden, route):
    """the parents of test_size_classes' B, all its sizes in one world of 64:
    106 (318 sites, class 0) beside 107 (321, a spill its wave continues) and
    the same at the list classes' bounds"""
    sizes = [(tsc.B_CASES[c % len(tsc.B_CASES)][0],) * 2 for c in range(64)]
    calls = [("update", 0)] if route == "update" else [(route, 3)]
    scn = tsc.Scenario(golden, 8, calls, cells=range(64), first_mem={c: tsc.grown(P) for c, (P, _) in enumerate(sizes)},
                       ov=tsc.NO_DIVIDE_MUT, records=(range(64), sizes), divided=range(64))
    k = 1 if route == "update" else 2
    scn.want_hops = [tsc.B_CASES[c % len(tsc.B_CASES)][k] for c in range(64)]
    return scn


def check_bounds(scn, out):
    first = out[0]
    assert list(first.hops) == scn.want_hops
    assert all(first.after["mem_size"][c] == m for c, m in scn.first_mem.items())
    assert (first.after["errors"] == 0).all() and (first.after["num_divides"] == 1).all()


@pytest.mark.parametrize("route", ["update", "step_frozen"])
def test_bounds_design_on_oracle(golden, route):
    scn = bound_scenario(golden, route)
    check_bounds(scn, tsc.run(scn, with_gpu=False))


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["update", "step_frozen"])
def test_class_bounds(golden, route):
    """divide, then h-alloc to exactly a slot's capacity and to three sites
    more, in one wave: the mixed launch's slots (update) and the rows'"""
    scn = bound_scenario(golden, route)
    check_bounds(scn, tsc.run(scn, with_gpu=True))


# ---- failing allocations -------------------------------------------------------

def failing_world(golden, k):
    """wave 0: the k scattered lanes allocate, the others were handed in as
    allocated (REQUIRE_ALLOCATE 1: their h-alloc faults and writes nothing);
    wave 1: every second lane allocates"""
    iset = heads(golden)
    asks = set(pu.scattered(64, k)) | set(range(64, 128, 2))
    w = TapeWorld(golden, 16, 8, [alloc_genome(iset, length) for length in FILL_LENS], 3,
                  instset="instset-heads.cfg", patch={"mal_active": {c: 1 for c in range(128) if c not in asks}})
    w.asks, w.lens = sorted(asks), FILL_LENS
    return w


def check_failing(world, ends):
    lens, first = np.array(world.lens), ends[1]
    asks = np.zeros(world.n, dtype=bool)
    asks[world.asks] = True
    assert (first["mem_size"][asks] == 3 * lens[asks]).all() and (first["errors"][asks] == 0).all()
    assert (first["mem_size"][~asks] == lens[~asks]).all() and (first["errors"][~asks] == 1).all()
    assert (first["alive"] != 0).all()


@pytest.mark.parametrize("k", [1, 2, 64])
def test_failing_design_on_oracle(golden, k):
    world = failing_world(golden, k)
    check_failing(world, tss.run(world, 1, with_gpu=False)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 64])
def test_failing_allocations(golden, k):
    """one, two and 64 lanes of a wave fill, beside lanes whose h-alloc faults"""
    world = failing_world(golden, k)
    check_failing(world, tss.run(world, 3, with_gpu=True, first_compare=True)[0])


# ---- mixed kinds in one slow phase ------------------------------------------------

LABEL_LENS = (1, 2, 10)                                      # 10 = AVGPU_MAX_LABEL
PLACES = ("near", "far", "none", "behind")
MIXED_LEN = 100
DIVIDERS = [c for c in range(64) if c % 16 >= 14]


def search_genome(iset, length, place):
    """(genome, the site of its h-search, the site its search finds or None).
    The label after h-search is nop-A nop-B nop-C ... and its complement is
    written once: in the first 64 sites, past them, nowhere, or before the
    h-search (the instruction pointer is handed in on the h-search); every
    other site is `inc`, so no other run of nops can hold the label."""
    op = iset.op_of_name
    nops = [op("nop-A"), op("nop-B"), op("nop-C")]
    g = [op("inc")] * MIXED_LEN
    at = 40 if place == "behind" else 0
    g[at] = op("h-search")
    for i in range(length):
        g[at + 1 + i] = nops[i % 3]
    target = {"near": 20, "far": 70, "none": None, "behind": 5}[place]
    if target is not None:
        for i in range(length):
            g[target + i] = nops[(i + 1) % 3]
    return bytes(g), at, target


def mixed_world(golden, env="def"):
    """per lane by c % 16: 0..11 an h-search (3 label lengths x 4 places), 12
    and 13 an h-alloc, 14 and 15 a viable divide (construction 1); all of them
    the lane's first instruction"""
    iset = heads(golden)
    genomes, ips, plan = [], {}, {}
    for c in range(64):
        k = c % 16
        if k < 12:
            length, place = LABEL_LENS[k // 4], PLACES[k % 4]
            g, at, target = search_genome(iset, length, place)
            genomes.append(g)
            ips[c] = (at, 0, 0, 0)
            plan[c] = (length, at, target)
        elif k < 14:
            genomes.append(alloc_genome(iset, 21 + c % 30))
        else:
            genomes.append(None)
    w = TapeWorld(golden, 8, 8, genomes, 2, instset="instset-heads.cfg", env=env,
                  ov=dict(tsc.NO_DIVIDE_MUT), patch={"head": ips})
    scratch = ol.Backend("oracle", w.cfg, w.iset, w.env, ncells=w.n)
    w.records = pu.predivide_records(scratch, iset, tsc.ancestor(golden)[1], DIVIDERS, [(106, 106)] * len(DIVIDERS))
    scratch.close()
    w.plan = plan
    return w


def check_mixed(world, ends, stats):
    """after the first update (two instructions): h-search's BX = the distance
    from the label's end to the found label's last site, or 0, CX = the label's
    length, the flow head behind the found label; the allocations; the divides"""
    first = ends[1]
    # (a divider's offspring may have replaced a neighbour: the cells that kept their key)
    kept = (ends[0]["rng_key_lo"] == first["rng_key_lo"]) & (ends[0]["rng_key_hi"] == first["rng_key_hi"])
    seen = set()
    for c, (length, at, target) in world.plan.items():
        if not kept[c]:
            continue
        found = at + length if target is None else target + length - 1
        # (the second instruction is the `inc` behind the label: BX + 1)
        assert first["reg"][c][1] == found - (at + length) + 1 and first["reg"][c][2] == length, (c, first["reg"][c])
        assert first["head"][c][0] == at + length + 2, c
        assert first["head"][c][3] == (found + 1) % MIXED_LEN, c
        seen.add((length, PLACES[c % 4]))
    assert seen == {(n, p) for n in LABEL_LENS for p in PLACES}
    allocs = [c for c in range(64) if c % 16 in (12, 13) and kept[c]]
    assert len(allocs) >= 4 and all(first["mem_size"][c] == 3 * (21 + c % 30) for c in allocs)
    assert stats[0].divides == len(DIVIDERS) and stats[0].births >= 2
    assert (first["errors"][kept] == 0).all()


def test_mixed_design_on_oracle(golden):
    world = mixed_world(golden)
    ends, stats, _ = tss.run(world, 1, with_gpu=False)
    check_mixed(world, ends, stats)


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS)
def test_mixed_kinds_in_one_slow_phase(golden, env):
    """h-alloc, h-search (labels of 1, 2 and 10 nops; found in the first window
    of 64 sites, past it, before the instruction, and not found) and viable
    divides, all in the first iteration of one wave"""
    world = mixed_world(golden, env=env)
    ends, stats, _ = tss.run(world, 4, with_gpu=True, first_compare=True)
    check_mixed(world, ends, stats)


# ---- divide reset ---------------------------------------------------------------

RESET_PARENTS = [y * 16 + x for y in range(8) for x in range(16) if (x + y) % 2 == 0]


def reset_world(golden, env="def"):
    """construction-1 parents of 100 .. 131 sites (every residue of the divide
    point, and of the fill that follows it over the offspring's copy) with both
    stacks full; three IO stand before their h-divide, where the instruction
    pointer is handed in, so that their task checks are queued when the divide
    comes.  After it the parent starts over: h-alloc."""
    iset, anc = tsc.ancestor(golden)
    w = TapeWorld(golden, 16, 8, [None] * 128, 6, instset="instset-heads.cfg", env=env, ov=dict(tsc.NO_DIVIDE_MUT))
    sizes = [(100 + i % 32,) * 2 for i in range(len(RESET_PARENTS))]
    scratch = ol.Backend("oracle", w.cfg, w.iset, w.env, ncells=w.n)
    records = pu.predivide_records(scratch, iset, anc, RESET_PARENTS, sizes)
    scratch.close()
    io = iset.op_of_name("IO")
    w.records = []
    for i, ((cell, st, ops, flags), (P, _)) in enumerate(zip(records, sizes)):
        assert iset.names[ops[P - 4]] == "h-divide"
        ops = ops[:P - 7] + bytes([io]) * 3 + ops[P - 4:]
        st[0].head[0] = P - 7
        tss.put(st[0], "stack", [[100 * (k + 1) + i + j + 1 for j in range(tss.STK)] for k in range(2)])
        tss.put(st[0], "stack_ptr", (i % tss.STK, (7 * i + 3) % tss.STK))
        st[0].cur_stack = i & 1
        tss.put(st[0], "reg", tss.regs_of(i))
        w.records.append((cell, st, ops, flags))
    w.sizes = sizes
    return w


def check_reset(world, ends, stats):
    before, first = ends[0], ends[1]
    assert (before["stack"][RESET_PARENTS] != 0).all()
    assert stats[0].divides == len(RESET_PARENTS) and stats[0].births > 32
    kept = [i for i, c in enumerate(RESET_PARENTS) if (before["rng_key_lo"][c], before["rng_key_hi"][c]) ==
            (first["rng_key_lo"][c], first["rng_key_hi"][c])]
    assert len(kept) > 40
    cells = [RESET_PARENTS[i] for i in kept]
    # three IO, the divide, h-alloc, one more: the stacks cleared, the memory grown again
    assert (first["num_divides"][cells] == 1).all() and not first["stack"][cells].any()
    assert (first["output_total"][cells] == 3).all() and (first["time_used"][cells] == 6).all()
    assert all(first["mem_size"][RESET_PARENTS[i]] == 3 * world.sizes[i][0] for i in kept)
    assert {world.sizes[i][0] % 16 for i in kept} == set(range(16))


def test_reset_design_on_oracle(golden):
    world = reset_world(golden)
    ends, stats, _ = tss.run(world, 1, with_gpu=False)
    check_reset(world, ends, stats)


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS)
def test_divide_reset_then_alloc(golden, env):
    world = reset_world(golden, env=env)
    ends, stats, _ = tss.run(world, 3, with_gpu=True, first_compare=True)
    check_reset(world, ends, stats)


# ---- newborn pass ------------------------------------------------------------------

def newborn_world(golden, env):
    """64 ancestors, slices of 100: they divide in their fourth update, and a
    newborn runs its h-alloc in the newborn pass of that update"""
    iset, anc = tsc.ancestor(golden)
    w = tss.World(golden, 8, 8, [anc] * 64, 100, instset="instset-heads.cfg", env=env, ov={"COPY_MUT_PROB": 0.0075})
    return w


def check_newborns(ends, stats):
    born = [u for u, s in enumerate(stats) if s.births > 0]
    assert born and born[0] + 2 < len(stats), born
    u = born[0]
    before, after, later = ends[u], ends[u + 1], ends[u + 2]
    nb = (before["rng_key_lo"] != after["rng_key_lo"]) | (before["rng_key_hi"] != after["rng_key_hi"])
    ran = nb & (after["time_used"] > 0) & (after["mem_size"] == 3 * after["birth_length"]) & (after["mal_active"] != 0)
    assert ran.sum() >= 16, (nb.sum(), ran.sum())
    same = (after["rng_key_lo"] == later["rng_key_lo"]) & (after["rng_key_hi"] == later["rng_key_hi"])
    assert (later["time_used"][ran & same] > after["time_used"][ran & same]).all() and (ran & same).sum() > 0


def test_newborn_design_on_oracle(golden):
    ends, stats, _ = tss.run(newborn_world(golden, "def"), 7, with_gpu=False)
    check_newborns(ends, stats)


@pytest.mark.gpu
@pytest.mark.parametrize("env", ["def", "rec"])
def test_newborn_pass(golden, env):
    """a wave of newborns that all allocate in their first iteration, with
    counter streams and with recorded ones; the next update runs them on"""
    ends, stats, _ = tss.run(newborn_world(golden, env), 7, with_gpu=True)
    check_newborns(ends, stats)


# ---- the list classes' rows, the serial world -----------------------------------------

def rows_scenario(golden):
    """avgpu_step runs the list classes in their own kernels: unallocated
    organisms of 150 / 300 / 600 sites (classes 1 / 2 / 3) beside class 0's"""
    iset = heads(golden)
    lens = [(150, 300, 600, 37 + c % 16)[c % 4] for c in range(64)]
    return tsc.Scenario(golden, 8, [("step_frozen", 3), ("step_world", 3)], cells=range(64),
                        first_mem={c: 3 * length for c, length in enumerate(lens)},
                        orgs=[(0, [alloc_genome(iset, length) for length in lens], [100.0] * 64)])


def test_rows_design_on_oracle(golden):
    scn = rows_scenario(golden)
    tsc.check_design(scn, tsc.run(scn, with_gpu=False))


@pytest.mark.gpu
def test_list_rows(golden):
    scn = rows_scenario(golden)
    tsc.check_design(scn, tsc.run(scn, with_gpu=True))


@pytest.mark.gpu
def test_serial_world(golden):
    """avgpu_run_serial_updates: single steps of lane 0 through h-alloc,
    h-search and divides, three updates of 64 ancestors"""
    iset, env, cfg = pu.load_env(golden, seed=11, overrides={"WORLD_X": 8, "WORLD_Y": 8})
    anc = tsc.ancestor(golden)[1]
    orc, gpu = (ol.Backend(k, cfg, iset, env, ncells=64) for k in ("oracle", "gpu"))
    for b in (orc, gpu):
        b.set_orgs(0, [anc] * 64, deterministic=False)
    for u in range(16):
        so, sg = orc.run_serial_update(), gpu.run_serial_update()
        for f in ("num_organisms", "insts_executed", "births", "deaths", "divides"):
            assert getattr(so, f) == getattr(sg, f), (u, f, getattr(so, f), getattr(sg, f))
        tss.compare(orc, gpu, 64, f"serial update {u}")
    assert sum(s.num_divides for s in orc.states(0, 64, CAP)[0]) > 0
    orc.close()
    gpu.close()
