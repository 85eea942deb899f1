"""Directed parity tests for the interpreter's LDS size classes and spills
(avida_amd/csrc/interp_launch.h k_interpret, interp_core.h interpret_chunk;
device.h need_of / class_of).  The oracle has no size classes, so every world
here is built to outgrow its slots on demand (parity_util: construction 1 a handed-in organism
about to divide and then allocate, construction 2 a chain of h-allocs at
REQUIRE_ALLOCATE 0, construction 3 copy insertions from constant recorded
streams), and the spills a call must make are read off the oracle's own states
before and after it (parity_util.class_view / expected_spills).

Every scenario runs twice: on the oracle alone (unmarked: the designed cells
are exactly the cells the class view expects to spill, they got a budget, they
divided, they made no error), and GPU against oracle (every field, tape, flag
and digest after every call, AVGPU_CNT_SPILLS == the expected spills).

Two capacity sets are pinned (parity_util.SLOT_CHAINS): a world update runs
the list classes in class 0's launch, 960 / 1600 / 2048 sites per organism,
avgpu_step runs them in their rows, 768 / 1536 / 2048; class 0 holds 320, and
its spills are continued by their own wave (world mode, groups of 21) or in
row 4.

A spill inside the newborn pass needs copy insertions (a fresh class-0
newborn cannot otherwise grow) and a pass long enough to reach the copy loop,
about 100 instructions: F-newborn-spill runs it at AVE_TIME_SLICE 200."""
import collections
import os

import numpy as np
import pytest

from avida_amd import capi, files
import oracle_lib as ol
import parity_util as pu

CAP = capi.MAX_GENOME
STAT_FIELDS = ("num_organisms", "insts_executed", "births", "deaths", "divides", "births_dropped",
               "births_overwritten", "births_cancelled", "cum_insts_executed", "cum_births", "slices")
NO_DIVIDE_MUT = {"DIVIDE_INS_PROB": 0.0, "DIVIDE_DEL_PROB": 0.0}
STEP_MODE = {"step_world": capi.MODE_WORLD, "step_frozen": capi.MODE_FROZEN}


class Scenario:
    """One world and the calls made on it.
    calls: (route, uniform budget) -- route "update", "step_world" or
    "step_frozen"; orgs: (first cell, genomes, merits) for set_orgs;
    records: (cells, (P, C) per cell) of construction 1, put over orgs;
    rec: "random", or (stream, offsets).
    The design's claims, all checked on the oracle:
    cells: the designed cells, each of which spills `spills` times over all
    calls (0: the case pins that a size still fits) and no other cell spills;
    first_mem: {cell: mem_size after the first call's slices} -- what shows
    that a cell ran its h-alloc and reached the size the case is about;
    every cell of `cells` and `first_mem` gets min_budget from the scheduler
    of an update, makes no error and stays alive;
    divided: cells that divide in the first call; lists: the lengths of the
    class 1 / 2 / 3 lists of the seeded world; newborn_classes: {offspring
    length: class}, each of which must run in the newborn pass; rows: the
    spill rows of avgpu_step hold more entries than their grids;
    newborn_spill: newborns outgrow their slots inside their pass (the cells
    they land in are the placement's choice: `cells` are the parents, which
    spill in the main pass)."""

    def __init__(self, golden, side, calls, cells=(), spills=0, first_mem=None, ov=None, env="def", orgs=(),
                 records=None, rec=None, min_budget=2, divided=(), lists=None, newborn_classes=None, rows=False,
                 newborn_spill=False, seed=7):
        ov = dict(ov or {}, WORLD_X=side, WORLD_Y=side)
        self.iset, self.env, self.cfg = pu.load_env(golden, overrides=ov, seed=seed)
        self.cfg.sub_updates = 1                 # one batch step per update: one allotment, one newborn pass
        if env == "res":                         # the bench's resource environment: IP_DEF_RES
            import bench
            self.env = files.parse_environment(bench.resource_env_text(side, side))
        elif env == "generic":
            # IP_GENERIC: a twice-only requisite is outside the simple form (capi.hip avgpu_load_env's `simple` loop:
            # of the requisites only max_count 1, the once mask, and INT32_MAX keep `simple`;
            # interp.hip interp_of then chooses the generic kernel)
            for r in self.env:
                r.has_requisite, r.min_count, r.max_count = 1, 0, 2
        self.n = side * side
        self.calls, self.min_budget = calls, min_budget
        self.cells, self.spills, self.first_mem = sorted(cells), spills, dict(first_mem or {})
        self.orgs, self.rec, self.divided = orgs, rec, list(divided)
        self.lists, self.newborn_classes, self.rows = lists, newborn_classes, rows
        self.newborn_spill = newborn_spill
        assert all(r != "update" for r, _ in calls[1:]), "the main-pass twin follows one update, the first call"
        self.records = []
        if records:
            scratch = self.backend("oracle", populate=False)
            self.records = pu.predivide_records(scratch, self.iset, ancestor(golden)[1], records[0], records[1])
            scratch.close()

    def backend(self, kind, populate=True):
        b = ol.Backend(kind, self.cfg, self.iset, self.env, ncells=self.n)
        if populate:
            for first, genomes, merits in self.orgs:
                b.set_orgs(first, genomes, merits, deterministic=False)
            pu.put_records(b, self.records)
            if self.rec == "random":             # every cell its own segment of one recorded stream
                per = 4000
                b.set_rng_mode(capi.RNG_RECORDED, np.random.default_rng(5).random(self.n * per),
                               np.arange(self.n, dtype=np.int64) * per)
            elif self.rec is not None:
                b.set_rng_mode(capi.RNG_RECORDED, *self.rec)
        return b


def ancestor(golden):
    """(the heads instruction set, default-heads.org)"""
    iset = files.read_instset(os.path.join(golden, "instset-heads.cfg"))
    return iset, files.read_org(os.path.join(golden, "default-heads.org"), iset)


# What one call of a scenario showed.  before / after: the oracle's states
# before the call and after its slices (an update: before any placement);
# hops: the expected spills per cell, newborn_hops the newborn pass's share of
# them; newborn_classes: {offspring length: class} of the newborns that ran;
# stats: the oracle's update statistics; cnt_spills: the GPU's AVGPU_CNT_SPILLS
Call = collections.namedtuple("Call", "route before after budgets hops newborn_hops newborn_classes stats cnt_spills")


def compare(orc, gpu, n, what):
    a, oa, fa = orc.states(0, n, CAP)
    b, ob, fb = gpu.states(0, n, CAP)
    if n <= 1024:
        bad = pu.diff_states(a, b, oa, ob, fa, fb, CAP)
        assert not bad, f"{what}: {len(bad)} mismatches: {bad[:5]}"
    else:
        nbad, report = pu.diff_states_np(a, b, oa, ob, fa, fb, CAP)
        assert nbad == 0, f"{what}: {nbad} cells differ: {report[:5]}"
    nbad, cells = pu.compare_digests(orc.digests(0, n), gpu.digests(0, n))
    assert nbad == 0, f"{what}: {nbad} cell digests differ, first {cells}"


def run(scn, with_gpu):
    """Runs the scenario's calls on the oracle (and the GPU, compared after
    every call); returns a Call per call.  An update's main pass is read from
    a twin oracle that steps the same states by the update's own budgets
    without placing the births."""
    n = scn.n
    orc = scn.backend("oracle")
    twin = scn.backend("oracle") if scn.calls[0][0] == "update" else None
    gpu = scn.backend("gpu") if with_gpu else None
    out = []
    for k, (route, budget) in enumerate(scn.calls):
        before = pu.state_array(orc)
        ran_nb, so, nb_hops = {}, None, np.zeros(n, dtype=np.int64)
        if route == "update":
            so = orc.run_update()
            bud = pu.last_budgets(orc)
            twin.step(0, n, budget=[int(x) for x in bud], mode=capi.MODE_WORLD)
            after, full = pu.state_array(twin), pu.state_array(orc)
            hops = pu.expected_spills(before, after, route)
            # the survivors of the placement are the twin's organisms
            same = (full["rng_key_lo"] == after["rng_key_lo"]) & (full["rng_key_hi"] == after["rng_key_hi"]) & \
                (after["alive"] != 0)
            assert (full["mem_size"][same] == after["mem_size"][same]).all()
            # the newborns: activated with their genome, nothing allocated
            nb = (full["alive"] != 0) & ~same
            fresh = full.copy()
            fresh["mem_size"], fresh["mal_active"] = full["birth_length"], 0
            fresh["alive"] = nb
            nb_hops = pu.expected_spills(fresh, full, route)
            hops += nb_hops
            _, ncls, _ = pu.class_view(fresh, route)
            for c in np.nonzero(nb & (full["time_used"] > 0))[0]:
                ran_nb[int(full["birth_length"][c])] = int(ncls[c])
        else:
            orc.step(0, n, uniform=budget, mode=STEP_MODE[route])
            after = pu.state_array(orc)
            bud = np.full(n, budget)
            hops = pu.expected_spills(before, after, route)
        spills = None
        if gpu:
            if route == "update":
                sg = gpu.run_update()
                for f in STAT_FIELDS:
                    assert getattr(so, f) == getattr(sg, f), (k, f, getattr(so, f), getattr(sg, f))
                assert list(so.task_orgs) == list(sg.task_orgs), k
                assert sg.births_dropped == 0
            else:
                gpu.step(0, n, uniform=budget, mode=STEP_MODE[route])
            compare(orc, gpu, n, f"call {k} ({route})")
            c = gpu.counters()
            spills = c[capi.CNT_SPILLS]
            print(f"call {k} {route}: expected spills {int(hops.sum())}, CNT_SPILLS {spills}")
            assert spills == hops.sum(), (k, route, spills, int(hops.sum()))
            assert c[capi.CNT_BAD_RECORD] == 0 and c[capi.CNT_REC_EXHAUSTED] == 0
        out.append(Call(route, before, after, bud, hops, nb_hops, ran_nb, so, spills))
    if scn.rec is not None:
        assert orc.lib.orc_rec_exhausted() == 0
    for b in (orc, twin, gpu):
        if b:
            b.close()
    return out


def check_design(scn, out):
    """the oracle alone: the scenario is what its design says"""
    first, last = out[0], out[-1]
    total = sum(call.hops for call in out)
    if scn.newborn_spill:
        assert first.newborn_hops.sum() > 0
        total = total - first.newborn_hops
    got = {int(c): int(total[c]) for c in np.nonzero(total)[0]}
    want = {c: scn.spills for c in scn.cells if scn.spills}
    assert got == want, (sorted(set(got) ^ set(want)), got)
    # every designed cell, spilling or not, ran what the case is about
    checked = sorted(set(scn.cells) | set(scn.first_mem))
    assert checked, "a scenario names the cells it is about"
    if first.route == "update":
        short = [c for c in checked if first.budgets[c] < scn.min_budget]
        assert not short, f"designed cells without a budget of {scn.min_budget}: {short} (pick another seed)"
        assert first.stats.births_dropped == 0
    for call in (first, last):
        assert (call.after["errors"][checked] == 0).all() and (call.after["alive"][checked] != 0).all()
    wrong = {c: int(first.after["mem_size"][c]) for c, m in scn.first_mem.items() if first.after["mem_size"][c] != m}
    assert not wrong, f"cells that did not reach their designed size: {wrong}"
    assert (first.after["num_divides"][scn.divided] == first.before["num_divides"][scn.divided] + 1).all()
    if scn.lists:
        _, cls, _ = pu.class_view(first.before, first.route)
        alive = first.before["alive"] != 0
        assert tuple(int(((cls == c) & alive).sum()) for c in (1, 2, 3)) == scn.lists
        assert ((cls == 0) & alive).sum() > 0
    if scn.newborn_classes:
        # every offspring was placed (two that chose one empty cell: the later one stays)
        so = first.stats
        assert so.births + so.births_overwritten == so.divides == len(scn.divided) and so.births_cancelled == 0
        assert first.newborn_classes == scn.newborn_classes, first.newborn_classes
    if scn.rows:
        # row 4 holds class 0's spills, rows 5 + 6 every other spill: each
        # more entries than the 16 one-lane blocks of its launch
        _, cls, _ = pu.class_view(first.before, first.route)
        row4 = int(((cls == 0) & (first.hops > 0)).sum())
        assert row4 > 16 and int(first.hops.sum()) - row4 > 16, (row4, int(first.hops.sum()))


# ---- the scenarios ---------------------------------------------------------

def grown(P):
    """what h-alloc grows P sites to (OFFSPRING_SIZE_RANGE 2, the 2048-site cap)"""
    return min(3 * P, capi.MAX_GENOME)


def case_a(golden, k, variant, rec):
    """A. Continuation groups: 64 living cells, one class-0 wave; k scattered
    cells spill (150 -> 450 sites), the others stay (106 -> 318)."""
    des = pu.scattered(64, k)
    sizes = [(150, 150) if c in des else (106, 106) for c in range(64)]
    calls = [("step_world", 30)] if variant == "step_world" else [("update", 0)]
    return Scenario(golden, 8, calls, cells=des, spills=1, first_mem={c: grown(sizes[c][0]) for c in range(64)},
                    ov=NO_DIVIDE_MUT, env=variant if variant != "step_world" else "def",
                    records=(range(64), sizes), rec="random" if rec else None, divided=range(64))


# B. Slot bounds: (P, spills in a world update, spills in avgpu_step FROZEN);
# the parent of P sites with a copy of P sites starts in the class of 2 P and
# allocates to min(3 P, 2048): update capacities 320 / 960 / 1600, row
# capacities 320 / 768 / 1536 (parity_util.SLOT_CHAINS)
B_CASES = [(106, 0, 0), (107, 1, 1),                              # 318 | 321 around class 0's 320
           (256, 0, 0), (257, 0, 1), (320, 0, 1), (321, 1, 1),    # 768 | 771 (row), 960 | 963 (mixed)
           (512, 0, 0), (513, 0, 1), (533, 0, 1), (534, 1, 1),    # 1536 | 1539 (row), 1599 | 1602 (mixed)
           (682, 1, 1), (683, 1, 1)]                              # 2046, and 2049 capped at 2048


def case_b(golden, P, hops, route):
    """32 scattered cells of (P, P), the others (106, 106): every cell must
    show its allocated size on the oracle -- a case that expects no spill pins
    the capacity only if its cells reached min(3 P, 2048) sites"""
    des = pu.scattered(64, 32, seed=P)
    sizes = [(P, P) if c in des else (106, 106) for c in range(64)]
    calls = [("update", 0)] if route == "update" else [(route, 3)]
    return Scenario(golden, 8, calls, cells=des, spills=hops, first_mem={c: grown(sizes[c][0]) for c in range(64)},
                    ov=NO_DIVIDE_MUT, records=(range(64), sizes), divided=range(64))


def case_c(golden, route):
    """C. Chains: 12 scattered cells run h-alloc three times (100 -> 300 -> 900
    -> 2048 sites, two spills in one call), the others are the ancestor."""
    iset, anc = ancestor(golden)
    des = pu.scattered(64, 12, seed=2)
    chain = pu.chain_genome(iset)
    return Scenario(golden, 8, [("update", 0)] if route == "update" else [(route, 7)], cells=des, spills=2,
                    first_mem={c: 2048 if c in des else 300 for c in range(64)},
                    ov=dict(NO_DIVIDE_MUT, REQUIRE_ALLOCATE=0), min_budget=5,
                    orgs=[(0, [chain if c in des else anc for c in range(64)], [100.0] * 64)])


def case_d(golden, k, route, slip):
    """D. Copy-spill rewind: the ancestor padded to 106 sites allocates to 318;
    with COPY_INS_PROB 0.5 the k cells whose recorded stream is 0.25 throughout
    insert a site at every h-copy, the others (0.75) never do.  90
    instructions reach the copy loop, then budgets of 5 walk through the
    crossing of 320 sites (slip: SLIP_COPY_MODE 1 and COPY_SLIP_PROB 0.5, the
    first copy's memory slip crosses)."""
    iset, anc = ancestor(golden)
    ov = {"COPY_INS_PROB": 0.5}
    if slip:
        ov.update({"SLIP_COPY_MODE": 1, "COPY_SLIP_PROB": 0.5})
    des = pu.scattered(64, k, seed=4)
    return Scenario(golden, 8, [(route, 90)] + [(route, 5)] * 10, cells=des, spills=1,
                    first_mem={c: 318 for c in range(64)}, ov=ov,
                    orgs=[(0, [pu.padded_ancestor(anc, 106, iset)] * 64, [100.0] * 64)],
                    rec=pu.constant_streams(64, des))


def e_lengths():
    """E. list lengths around a chunk and around a whole grid of chunks, per
    mixed class (organisms per chunk, blocks): 1, per - 1, per, per + 1,
    nb x per, nb x per + 1"""
    cols = [[1, per - 1, per, per + 1, nb * per, nb * per + 1] for per, nb in pu.MIX_GRIDS]
    return list(zip(*cols))


def case_e(golden, lists):
    """Unallocated nop-padded ancestors of 150 / 300 / 600 sites need 450 /
    900 / 1800: classes 1 / 2 / 3; the other cells hold the ancestor, class 0.
    Every list cell shows its allocated size on the oracle."""
    iset, anc = ancestor(golden)
    side = 16 if sum(lists) <= 128 else 128
    n = side * side
    cells = pu.scattered(n, sum(lists), seed=6)
    lengths = [150] * lists[0] + [300] * lists[1] + [600] * lists[2]
    genomes = [anc] * n
    for c, length in zip(cells, lengths):
        genomes[c] = pu.padded_ancestor(anc, length, iset)
    return Scenario(golden, side, [("update", 0)], cells=cells, spills=0,
                    first_mem={c: grown(length) for c, length in zip(cells, lengths)},
                    orgs=[(0, genomes, [100.0] * n)], lists=tuple(lists))


def case_e_rows(golden):
    """The rows of avgpu_step: 1024 cells, frozen, budget 3; 40 class-0 spills
    (row 4: 16 blocks), 20 spills from class 1 and 20 from class 2 (rows 5 + 6:
    16 blocks), one lane per wave, so every block strides.  The other cells
    hold the ancestor."""
    n = 1024
    cells = pu.scattered(n, 80, seed=8)
    sizes = [(150, 150)] * 40 + [(257, 257)] * 20 + [(513, 513)] * 20
    return Scenario(golden, 32, [("step_frozen", 3)], cells=cells, spills=1,
                    first_mem={c: grown(P) for c, (P, _) in zip(cells, sizes)}, ov=NO_DIVIDE_MUT,
                    orgs=[(0, [ancestor(golden)[1]] * n, [100.0] * n)], records=(cells, sizes), divided=cells,
                    rows=True)


# F. the offspring's length C, its parent's P, the class of its need 3 C
F_CASES = [(106, 106, 0), (107, 106, 1), (256, 150, 1), (257, 150, 2), (512, 300, 2), (513, 300, 3)]
F_PARENTS = [y * 16 + x for y in range(16) for x in range(16) if (x + y) % 2 == 0]


def case_f(golden):
    """F. Newborn pass: 16 x 16, parents on the even diagonals, so that every
    offspring finds an empty neighbour; the offspring of C sites needs 3 C and
    runs in the newborn list (class 0) or the newborn launch's class 1 / 2 / 3
    blocks.  The parents allocate to 3 P without a spill."""
    sizes = [(F_CASES[i % 6][1], F_CASES[i % 6][0]) for i in range(len(F_PARENTS))]
    return Scenario(golden, 16, [("update", 0)], cells=F_PARENTS, spills=0,
                    first_mem={c: grown(P) for c, (P, _) in zip(F_PARENTS, sizes)}, ov=NO_DIVIDE_MUT,
                    records=(F_PARENTS, sizes), divided=F_PARENTS,
                    newborn_classes={C: cls for C, _, cls in F_CASES})


def case_f_spill(golden):
    """A spill inside the newborn pass: the parents of F with offspring of 106
    sites, COPY_INS_PROB 0.5 and AVE_TIME_SLICE 200 -- a newborn's pass is long
    enough to allocate (318 sites) and to copy past 320; the parents cross it
    too, in the main pass, and none finishes a second copy."""
    return Scenario(golden, 16, [("update", 0)], cells=F_PARENTS, spills=1,
                    ov=dict(NO_DIVIDE_MUT, COPY_INS_PROB=0.5, AVE_TIME_SLICE=200),
                    records=(F_PARENTS, [(106, 106)] * len(F_PARENTS)), divided=F_PARENTS, newborn_spill=True)


A_K = [1, 21, 22, 42, 43, 63, 64]
A_VARIANTS = [(v, r) for v in ("def", "res", "generic", "step_world") for r in (False, True)]
SCENARIOS = {}
for _k in A_K:
    for _v, _r in A_VARIANTS:
        SCENARIOS[f"A-{_v}{'-rec' if _r else ''}-k{_k}"] = (case_a, (_k, _v, _r))
for _P, _hu, _hs in B_CASES:
    SCENARIOS[f"B-update-P{_P}"] = (case_b, (_P, _hu, "update"))
    SCENARIOS[f"B-step_frozen-P{_P}"] = (case_b, (_P, _hs, "step_frozen"))
for _route in ("step_world", "step_frozen", "update"):
    SCENARIOS[f"C-{_route}"] = (case_c, (_route,))
for _k in (1, 22, 64):
    for _route in ("step_frozen", "step_world"):
        SCENARIOS[f"D-{_route}-k{_k}"] = (case_d, (_k, _route, False))
for _route in ("step_frozen", "step_world"):
    SCENARIOS[f"D-{_route}-slip-k22"] = (case_d, (22, _route, True))
for _lists in e_lengths():
    SCENARIOS["E-lists-" + "-".join(str(x) for x in _lists)] = (case_e, (_lists,))
SCENARIOS["E-rows"] = (case_e_rows, ())
SCENARIOS["F-newborns"] = (case_f, ())
SCENARIOS["F-newborn-spill"] = (case_f_spill, ())


def _make(golden, name):
    fn, args = SCENARIOS[name]
    return fn(golden, *args)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_design_on_oracle(golden, name):
    """The oracle alone decides that a scenario is valid: the class view's
    expected spill set is exactly the designed cells (none where the case pins
    a size that still fits), every designed cell got its budget (none left
    out: another seed otherwise), made no error and reached its designed
    size, and the divides, list lengths and newborn classes are the designed
    ones."""
    scn = _make(golden, name)
    check_design(scn, run(scn, with_gpu=False))


@pytest.mark.parametrize("slip", [False, True])
def test_copy_spill_both_sides_of_the_crossing(golden, slip):
    """D on the oracle: the crossing of 320 sites happens inside the budgets of
    5 -- calls before it and after it are compared as well.  Five instructions
    hold at most two h-copies: insertions alone grow a cell by at most two
    sites per call, so in the slip case a jump of more than five sites in the
    crossing call is the memory slip's."""
    scn = _make(golden, "D-step_frozen-slip-k22" if slip else "D-step_frozen-k22")
    out = run(scn, with_gpu=False)
    crossing = [k for k, call in enumerate(out) if call.hops.sum() > 0]
    assert len(crossing) == 1 and 1 <= crossing[0] < len(out) - 1, crossing
    call = out[crossing[0]]
    jump = call.after["mem_size"][scn.cells] - call.before["mem_size"][scn.cells]
    assert (call.before["mem_size"][scn.cells] <= 320).all() and (call.after["mem_size"][scn.cells] > 320).all()
    assert (jump > 5).all() if slip else (jump <= 2).all(), jump


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_gpu_equals_oracle(golden, name):
    """GPU == oracle after every call of the scenario -- every state field,
    the tape and its flags up to mem_size, the digests, an update's statistics
    -- and AVGPU_CNT_SPILLS of each call == the spills the class view reads
    from the oracle's states; no bad record, no dropped birth, no exhausted
    stream."""
    scn = _make(golden, name)
    check_design(scn, run(scn, with_gpu=True))
