"""Directed tests for the scheduler (avida_amd/csrc/sched.hip: k_merit_partial,
k_block_counts, k_tree_up, k_tree_down, k_allot; the oracle's block_levels /
top_tree / block_split / allot_interpret) against tests/sched_spec.py, a plain
numpy restatement.

How a budget is observed: every organism here is 50 sites of nop-C, which
never divides, under DEATH_METHOD 0 and one batch step per update
(cfg.sub_updates = 1), so a living cell's time_used grows by exactly its
budget in one run_update.  Merits and head starts that set_orgs would not
take (0, NaN, inf, negative; head_start) are written with get_states /
set_states on both backends.

Unmarked tests run the oracle alone against the spec; the tests marked gpu run
the same worlds on both backends: the device's time_used deltas equal the
oracle's orc_last_budgets and the spec, credit, head_start and every cell's
digest are equal after every update.

Left out on purpose: INTEGRATED's clamp of lambda at 1e8.  A case that reaches
it runs 1e8 instructions in one lane.

Measured on an MI355X: each GPU test under 0.3 s, the 1024 x 1026 world's
first test 1.1 s (it also computes the oracle's and the untiled world's
updates, which the others share); the timeouts, 30 s and 60 s, leave room for
a cold device and a busy host, no more."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from avida_amd import capi, files
import oracle_lib as ol
import parity_util as pu
import sched_spec as ss

CONSTANT, PROBABILISTIC, INTEGRATED = 0, 1, 2
NOP_LEN = 50
AVE = ss.AVE_TIME_SLICE
# the stats fields tests/test_parity_full.py compares
STAT_FIELDS = ("num_organisms", "insts_executed", "births", "deaths", "divides", "births_dropped",
               "births_overwritten")
# one cell per corner of k_allot's layout (lane l holds cells l, l + 64, l + 128, l + 192 of a
# block): lanes 0 and 63 in each of the four slots, then block 1 of a 17 x 17 world (33 cells)
LANE_SLOT_CELLS = (0, 63, 64, 127, 128, 191, 192, 255, 256, 288)


class NopWorld:
    """A world of nop-C organisms.  orgs: (first cell, merits) runs for
    set_orgs; patch: {field: {cell: value}} written over them by set_states.
    backend(kind, ncells) makes an empty strip of ncells cells of this world
    instead, which the caller seeds."""

    def __init__(self, golden, X, Y, slicing, orgs=(), patch=None, sub=1, seed=7):
        ov = {"WORLD_X": X, "WORLD_Y": Y, "SLICING_METHOD": slicing, "DEATH_METHOD": 0}
        self.iset, self.env, self.cfg = pu.load_env(golden, overrides=ov, seed=seed)
        self.cfg.sub_updates = sub
        self.X, self.Y, self.n = X, Y, X * Y
        self.orgs, self.patch = list(orgs), patch or {}
        self.nop = bytes([self.iset.op_of_name("nop-C")]) * NOP_LEN

    def seed(self, b, first, merits):
        merits = np.asarray(merits, dtype=np.float64)
        b.set_orgs_np(first, self.nop * len(merits), np.full(len(merits), NOP_LEN), merits)

    def backend(self, kind, ncells=None):
        b = ol.Backend(kind, self.cfg, self.iset, self.env, ncells=ncells or self.n)
        if ncells is None:
            for first, merits in self.orgs:
                self.seed(b, first, merits)
            put_fields(b, self.n, self.patch)
        return b


def put_fields(b, n, patch, cap=64):
    """write {field: {cell: value}} into the records of cells [0, n)"""
    if not patch:
        return
    st, ops, fl = b.states(0, n, cap)
    for field, values in patch.items():
        for cell, v in values.items():
            setattr(st[cell], field, v)
    b._call("set_states", b.h, 0, n, st, (C.c_uint8 * len(ops)).from_buffer_copy(ops),
            (C.c_uint8 * len(fl)).from_buffer_copy(fl), cap)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_spec(slicing, before, after, what):
    """One update of one backend against sched_spec, from its records before
    and after: returns the budgets (the time_used deltas)."""
    alive = before["alive"] != 0
    assert np.array_equal(after["alive"] != 0, alive), what          # nobody dies or is born here
    bud = after["time_used"].astype(np.int64) - before["time_used"]
    assert not bud[~alive].any(), what
    assert not after["head_start"][alive].any(), f"{what}: a head start outlived its allotment"
    w = np.where(alive, ss.weights(before["merit"], before["head_start"]), 0.0)
    ud = AVE * int(alive.sum())
    if slicing == CONSTANT or not ss.tree_total(w) > 0.0:
        want, credit = ss.constant_budgets(alive), before["credit"]
    elif slicing == INTEGRATED:
        want, credit = ss.integrated_budgets(w, np.where(alive, before["credit"], 0.0), ud)
    else:
        assert not bud[w == 0.0].any(), f"{what}: a weight-0 organism was scheduled"
        assert int(bud.sum()) == ud, (what, int(bud.sum()), ud)
        return bud
    bad = np.nonzero(bud != want)[0]
    assert len(bad) == 0, f"{what}: budgets differ from the spec at {bad[:5].tolist()}: " \
                          f"{bud[bad[:5]].tolist()} / {want[bad[:5]].tolist()}"
    bad = np.nonzero((bits(after["credit"]) != bits(credit)) & alive)[0]
    assert len(bad) == 0, f"{what}: credit differs from the spec at {bad[:5].tolist()}"
    return bud


def step(world, backends, what):
    """One run_update on every backend (the oracle first), each checked
    against the spec; the oracle's deltas equal orc_last_budgets, every other
    backend equals the oracle in budgets, credit, head_start and digests.
    Returns the budgets."""
    slicing = world.cfg.slicing_method
    before = [pu.state_array(b, world.n) for b in backends]
    for b in backends:
        b.run_update()
    after = [pu.state_array(b, world.n) for b in backends]
    orc = backends[0]
    assert orc.kind == "oracle"
    last = pu.last_budgets(orc).astype(np.int64)
    alive = before[0]["alive"] != 0
    dig = orc.digests()
    for b, s0, s1 in zip(backends, before, after):
        bud = check_spec(slicing, s0, s1, f"{what} ({b.kind})")
        bad = np.nonzero((bud != last) & alive)[0]
        assert len(bad) == 0, f"{what} ({b.kind}): time_used deltas differ from orc_last_budgets at " \
                              f"{bad[:5].tolist()}: {bud[bad[:5]].tolist()} / {last[bad[:5]].tolist()}"
        if b is not orc:
            assert np.array_equal(bits(s1["credit"]), bits(after[0]["credit"])), what
            assert np.array_equal(s1["head_start"], after[0]["head_start"]), what
            nbad, cells = pu.compare_digests(dig, b.digests())
            assert nbad == 0, f"{what}: {nbad} cells' digests differ, first {cells}"
    return np.where(alive, last, 0)


def run(world, kinds, updates, each=None, start=None):
    """`updates` checked updates of the world on the backends `kinds`;
    start(backends) before the first, each(u, budgets, backends) after every
    update"""
    bs = [world.backend(k) for k in kinds]
    try:
        if start:
            start(bs)
        for u in range(updates):
            bud = step(world, bs, f"update {u}")
            if each:
                each(u, bud, bs)
    finally:
        for b in bs:
            b.close()


ORACLE, BOTH = ("oracle",), ("oracle", "gpu")


# ---------------------------------------------------------------------------
# the scenarios (run on the oracle alone, and on both backends)

def constant_world(golden):
    merits = np.random.default_rng(1).uniform(0.5, 300.0, 289)
    return NopWorld(golden, 17, 17, CONSTANT, [(0, merits)])


def scenario_constant(golden, kinds):
    def each(u, bud, bs):
        assert (bud == AVE).all()
    run(constant_world(golden), kinds, 6, each)


INTEGRATED_SETS = ("dyadic", "uniform", "giant")


def integrated_merits(name):
    rng = np.random.default_rng(2)
    if name == "dyadic":                          # sums exact in any order
        return 2.0 ** rng.integers(0, 10, 289)
    if name == "uniform":                         # the total depends on the tree's order
        return rng.uniform(0.5, 300.0, 289)
    m = np.full(289, 8.0)                         # one large budget, far below the 1e8 clamp
    m[137] = 2.0 ** 20
    return m


def scenario_integrated(golden, kinds, name):
    merits = integrated_merits(name)
    world = NopWorld(golden, 17, 17, INTEGRATED, [(0, merits)])
    seen = []

    def each(u, bud, bs):
        seen.append(bud)
        if name == "giant":
            assert 8000 < bud[137] <= AVE * 289 and bud[137] < 1e6
    run(world, kinds, 6, each)
    # the carry is live: some organism's budget changes from update to update
    assert any((seen[0] != b).any() for b in seen[1:])
    # and not trivially 0: the first update already leaves fractions behind
    assert ss.integrated_budgets(merits, np.zeros(289), AVE * 289)[1].any()


HS_CELLS = {5: 0x8000, 260: 0xFFFF}


def scenario_head_start(golden, kinds):
    world = NopWorld(golden, 17, 17, INTEGRATED, [(0, np.full(289, 8.0))], {"head_start": HS_CELLS})
    plain = ss.integrated_budgets(np.full(289, 8.0), np.zeros(289), AVE * 289)[0]

    def each(u, bud, bs):
        if u == 0:      # the head starts weigh in: 1.5 and (nearly) 2 merits, the others below their 30
            assert bud[5] > plain[5] and bud[260] > bud[5] and bud[0] <= plain[0]
            for b in bs:
                assert not pu.state_array(b, world.n)["head_start"].any()

    def start(bs):
        for b in bs:
            hs = pu.state_array(b, world.n)["head_start"]
            assert {int(c): int(hs[c]) for c in np.nonzero(hs)[0]} == HS_CELLS
    run(world, kinds, 3, each, start)


ZERO_WEIGHT = {0: 0.0, 256: 0.0, 63: float("nan"), 288: float("nan"), 64: float("inf"), 255: -1.0}
BAD_MERITS = 4                                   # of those: NaN, NaN, inf, -1 (0.0 is a valid weight)


# "capped": cell 100 holds 1.5e308, a weight capped at 2^990 that takes (nearly) every pick;
# "plain": without it, so that the weight-0 organisms sit among organisms that do get picks
ZERO_WEIGHT_CASES = (("capped", PROBABILISTIC), ("plain", PROBABILISTIC), ("plain", INTEGRATED))


def scenario_zero_weights(golden, kinds, case, slicing, each_extra=None):
    merit = {**ZERO_WEIGHT, 100: 1.5e308} if case == "capped" else ZERO_WEIGHT
    world = NopWorld(golden, 17, 17, slicing, [(0, np.full(289, 8.0))], {"merit": merit})
    rest = np.setdiff1d(np.arange(289), list(ZERO_WEIGHT))

    def each(u, bud, bs):
        assert not bud[list(ZERO_WEIGHT)].any()
        if slicing == PROBABILISTIC:
            assert int(bud.sum()) == AVE * 289
        if case == "capped":
            assert bud[100] > AVE * 280           # the capped weight is scheduled
        else:
            assert (bud[rest] > 0).sum() > 270 and int(bud[rest].sum()) >= AVE * 289 - 289
        if each_extra:
            each_extra(u, bud, bs)
    run(world, kinds, 2, each)


def scenario_all_zero(golden, kinds, slicing):
    world = NopWorld(golden, 17, 17, slicing, [(0, np.full(289, 8.0))],
                     {"merit": {c: 0.0 for c in range(289)}})

    def each(u, bud, bs):
        assert (bud == AVE).all()
    run(world, kinds, 2, each)


SINGLE_WORLDS = {
    # X, Y: the cells the organism takes in turn
    "17x17": (17, 17, LANE_SLOT_CELLS),                       # nb = 2: one top-tree level
    "16x16": (16, 16, LANE_SLOT_CELLS[:8]),                   # nb = 1: L = 0, no top-tree level
    "40x33": (40, 33, LANE_SLOT_CELLS + (1279, 1280, 1319)),  # nb = 6: two zero leaves, a 40-cell last block
}


def scenario_single(golden, kinds, name):
    X, Y, cells = SINGLE_WORLDS[name]
    world = NopWorld(golden, X, Y, PROBABILISTIC)
    bs = [world.backend(k) for k in kinds]
    try:
        for c in cells:
            for b in bs:
                world.seed(b, c, [8.0])
            bud = step(world, bs, f"{name}, cell {c}")
            assert bud[c] == AVE and int(bud.sum()) == AVE, (c, bud[c], int(bud.sum()))
            for b in bs:
                b.kill(c)
    finally:
        for b in bs:
            b.close()


# ---------------------------------------------------------------------------
# A. the oracle against the spec

def test_constant_oracle(golden):
    """SLICING_METHOD 0 (allot_interpret's `consts` branch): AVE_TIME_SLICE
    for every organism, whatever its merit, 6 updates"""
    scenario_constant(golden, ORACLE)


@pytest.mark.parametrize("name", INTEGRATED_SETS)
def test_integrated_oracle(golden, name):
    """SLICING_METHOD 2 (allot_interpret's lam / credit carry): budgets and
    the credit carry equal sched_spec.integrated_budgets bit for bit over 6
    updates -- dyadic merits (any summation order), uniform(0.5, 300) (the
    tree's order), one merit 2^20 among 8s (a budget of ~8650, far below the
    clamp)"""
    scenario_integrated(golden, ORACLE, name)


def test_head_start_oracle(golden):
    """sched_weight's head start under INTEGRATED: cells 5 (0x8000) and 260
    (0xFFFF) weigh m (1 + hs / 65536) in update 0, every head_start reads 0
    afterwards and updates 1..2 follow the plain merits"""
    scenario_head_start(golden, ORACLE)


@pytest.mark.parametrize("case,slicing", ZERO_WEIGHT_CASES)
def test_zero_weights_oracle(golden, case, slicing):
    """weight-0 organisms (merit 0, NaN, inf, negative), with and without one
    capped weight (1.5e308): block_split gives the six budget 0 and the update
    still hands out exactly 30 x 289 picks; under INTEGRATED they take no part
    in the total either (the spec's budgets and credit, bit for bit)"""
    scenario_zero_weights(golden, ORACLE, case, slicing)


@pytest.mark.parametrize("slicing", (PROBABILISTIC, INTEGRATED))
def test_all_weights_zero_oracle(golden, slicing):
    """every merit 0: the total-0 fallback (`consts` without CONSTANT) gives
    every organism AVE_TIME_SLICE"""
    scenario_all_zero(golden, ORACLE, slicing)


@pytest.mark.parametrize("name", SINGLE_WORLDS)
def test_single_organism_oracle(golden, name):
    """one living organism in an empty world, at each lane / slot corner of
    the block tree, in block 0 and in a partial last block: it takes all 30
    picks (block_split down one path; top_tree with L = 0, 1 and 3)"""
    scenario_single(golden, ORACLE, name)


def test_binomial_tree_distribution_oracle(golden):
    """binom_draw (inversion below a mean of 6, the skew-corrected normal
    above) through the whole tree: over 400 updates of a 24 x 24 world with
    weights from {1, 2, 4, 64} and every 7th cell at 0.001, each update's
    budgets sum to UD = 17280, and against Multinomial(UD, w / sum w)
    (a) the Pearson chi-square of the per-cell totals (dof 575) has an
    upper-tail probability >= 1e-4, (b) per weight class with a mean budget
    >= 1, the mean over its cells of sample variance / (UD p (1 - p)) lies in
    [0.95, 1.05] -- about 140 cells x 400 updates per class put that ratio's
    sampling error near 0.006; the band is eight times that, from the
    binomial, not from the code.
    Measured (numpy seed 1, world seed 7): chi-square 641.3 (upper tail
    0.028), ratios 0.997, 1.013, 1.016, 1.006 for weights 1, 2, 4, 64; seven
    other pairs of seeds gave chi-squares of 521 .. 613."""
    rng = np.random.default_rng(1)
    n, updates = 576, 400
    w = rng.choice([1.0, 2.0, 4.0, 64.0], n)
    w[::7] = 0.001
    world = NopWorld(golden, 24, 24, PROBABILISTIC, [(0, w)])
    orc = world.backend("oracle")
    ud = AVE * n
    buds = np.zeros((updates, n), dtype=np.int64)
    for u in range(updates):
        orc.run_update()
        buds[u] = pu.last_budgets(orc)
        assert int(buds[u].sum()) == ud, u
    s = pu.state_array(orc, n)
    assert np.array_equal(s["time_used"], buds.sum(axis=0))
    orc.close()
    p = ss.multinomial_p(w)
    expect = updates * ud * p
    chi2 = float((((buds.sum(axis=0) - expect) ** 2) / expect).sum())
    tail = ss.chi2_sf(chi2, n - 1)
    print(f"chi-square {chi2:.1f} (dof {n - 1}), upper tail {tail:.3g}")
    ratios = {}
    for cls in (0.001, 1.0, 2.0, 4.0, 64.0):
        sel = w == cls
        if ud * p[sel][0] < 1.0:
            continue
        ratios[cls] = float((buds[:, sel].var(axis=0, ddof=1) / (ud * p[sel] * (1.0 - p[sel]))).mean())
    print("variance ratios", {k: round(v, 4) for k, v in ratios.items()})
    assert sorted(ratios) == [1.0, 2.0, 4.0, 64.0]           # inversion (means 2..8) and the normal branch
    assert tail >= 1e-4, (chi2, tail)
    for cls, r in ratios.items():
        assert 0.95 <= r <= 1.05, (cls, r)


# ---------------------------------------------------------------------------
# B. the device against the oracle and the spec

@pytest.mark.gpu
@pytest.mark.timeout(30)
def test_constant_gpu(golden):
    """k_allot's `consts` branch under SLICING_METHOD 0"""
    scenario_constant(golden, BOTH)


@pytest.mark.gpu
@pytest.mark.timeout(30)
@pytest.mark.parametrize("name", INTEGRATED_SETS)
def test_integrated_gpu(golden, name):
    """k_allot's INTEGRATED branch: lam = UD w / total from k_block_counts'
    TOT_DIV / TOT_UD, the credit carry in W.credit"""
    scenario_integrated(golden, BOTH, name)


@pytest.mark.gpu
@pytest.mark.timeout(30)
def test_head_start_gpu(golden):
    """sched_weight's CTL_HS head start in k_merit_partial and k_allot, and
    k_allot clearing it (`ctl & ~CTL_HS_MASK`)"""
    scenario_head_start(golden, BOTH)


@pytest.mark.gpu
@pytest.mark.timeout(30)
@pytest.mark.parametrize("case,slicing", ZERO_WEIGHT_CASES)
def test_zero_weights_gpu(golden, case, slicing):
    """sched_weight / merit_ok in k_merit_partial and k_allot, both branches:
    weight-0 organisms in lanes 0 and 63, slots 0, 1 and 3, and in the partial
    last block; AVGPU_CNT_BAD_RECORD counts the living organisms whose merit
    is NaN, inf or negative (4; merit 0.0 is a valid weight)"""
    def each(u, bud, bs):
        assert bs[1].counters()[capi.CNT_BAD_RECORD] == BAD_MERITS
    scenario_zero_weights(golden, BOTH, case, slicing, each)


@pytest.mark.gpu
@pytest.mark.timeout(30)
@pytest.mark.parametrize("slicing", (PROBABILISTIC, INTEGRATED))
def test_all_weights_zero_gpu(golden, slicing):
    """k_allot's `!(total > 0.0)` fallback to AVE_TIME_SLICE"""
    scenario_all_zero(golden, BOTH, slicing)


@pytest.mark.gpu
@pytest.mark.timeout(30)
@pytest.mark.parametrize("name", SINGLE_WORLDS)
def test_single_organism_gpu(golden, name):
    """k_allot's shuffle tree down to one cell in each lane / slot corner;
    k_block_counts with L = 0 (16 x 16), L = 1 and a zero-padded leaf level
    (40 x 33: 6 blocks in 8 leaves)"""
    scenario_single(golden, BOTH, name)


def sequential_sum(w):
    t = 0.0
    for v in w.tolist():
        t += v
    return t


def update_totals(gpu):
    """avgpu_update_totals into an 8-double device buffer of sentinels:
    (total weight, organisms); nothing is written past the two"""
    import torch
    sentinel = 0x7FF4C0DE5E1271E1          # a NaN no sum produces
    buf = torch.full((8,), sentinel, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu._call("update_totals", gpu.h, C.c_void_p(buf.data_ptr()))
    gpu.lib.avgpu_sync(gpu.h)
    got = buf.cpu().numpy()
    assert got[2:].tolist() == [sentinel] * 6, [hex(v) for v in got.tolist()]
    return got[:2].view(np.float64).tolist()


@pytest.mark.gpu
@pytest.mark.timeout(30)
@pytest.mark.parametrize("head_starts", (False, True))
def test_deterministic_total_gpu(golden, head_starts):
    """k_merit_partial's fixed pairwise order and k_block_counts' heap tree
    (BC_TOTALS_ONLY, 6 blocks in 8 leaves): avgpu_update_totals' first double
    equals sched_spec.tree_total bit for bit on merits whose sum depends on
    the order (asserted), its second the organism count, and nothing is
    written past them; once more with head starts on some cells"""
    rng = np.random.default_rng(4)
    n = 40 * 33
    merits = rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(0, 41, n)
    hs = np.zeros(n, dtype=np.int64)
    patch = {}
    if head_starts:
        cells = rng.choice(n, 200, replace=False)
        hs[cells] = rng.integers(1, 0x10000, 200)
        patch = {"head_start": {int(c): int(hs[c]) for c in cells}}
    world = NopWorld(golden, 40, 33, PROBABILISTIC, [(0, merits)], patch)
    w = ss.weights(merits, hs)
    want = ss.tree_total(w)
    assert want != sequential_sum(w), "these merits do not tell the tree's order from a plain sum"
    assert head_starts == (want != ss.tree_total(merits))
    gpu = world.backend("gpu")
    total, orgs = update_totals(gpu)
    gpu.close()
    assert orgs == n
    assert total == want, (total.hex(), want.hex())


def other_orders(w):
    """the sum of w in three other plausible orders: a block's cells in
    adjacent pairs; a lane's four cells as (0 + 1) + (2 + 3); the block
    partials left to right"""
    nb = (len(w) + 255) // 256
    s = np.zeros(nb * 256)
    s[:len(w)] = w
    s = s.reshape(nb, 256)

    def heap(part):
        t = np.zeros(1 << max(0, int(len(part) - 1).bit_length()))
        t[:len(part)] = part
        while len(t) > 1:
            t = t[0::2] + t[1::2]
        return float(t[0])
    adj = s
    while adj.shape[1] > 1:
        adj = adj[:, 0::2] + adj[:, 1::2]
    lane = (s[:, 0:64] + s[:, 64:128]) + (s[:, 128:192] + s[:, 192:256])
    stride = 32
    while stride >= 1:
        lane = lane[:, :stride] + lane[:, stride:2 * stride]
        stride //= 2
    return heap(adj[:, 0]), heap(lane[:, 0]), sequential_sum(ss.block_partials(w))


@pytest.mark.gpu
@pytest.mark.timeout(30)
def test_deterministic_total_absorbing_gpu(golden):
    """The same total on weights built to expose its order.  A pairwise sum is
    accurate, so two orders usually round to the same double (of eight random
    merit sets, a swapped lane order changed one total).  Here one organism
    weighs 2^60 among integers below 256: whatever joins its path through
    k_merit_partial's lane sums, shuffles and k_block_counts' tree is rounded
    to a multiple of 256 as it joins, so the total records which cells were
    summed before they met it.  The heavy organism takes each lane / slot
    corner of block 0 and cells of blocks 1, 2, 4 and 5 in turn; every total
    equals sched_spec.tree_total bit for bit, and each of three other orders
    (other_orders) would have been told apart at three positions or more
    (asserted)"""
    rng = np.random.default_rng(6)
    n = 40 * 33
    world = NopWorld(golden, 40, 33, PROBABILISTIC)
    gpu = world.backend("gpu")
    told = np.zeros(4, dtype=int)
    try:
        for cell in LANE_SLOT_CELLS[:9] + (700, 1279, 1280, 1319):
            w = rng.integers(1, 256, n).astype(np.float64)
            w[cell] = 2.0 ** 60
            want = ss.tree_total(w)
            told += [want != t for t in other_orders(w) + (sequential_sum(w),)]
            world.seed(gpu, 0, w)
            total, orgs = update_totals(gpu)
            assert orgs == n
            assert total == want, (cell, total.hex(), want.hex())
    finally:
        gpu.close()
    assert (told >= 3).all(), told


@pytest.mark.gpu
@pytest.mark.timeout(30)
@pytest.mark.parametrize("slicing", (CONSTANT, INTEGRATED))
def test_replicating_world_gpu(golden, slicing):
    """Replicators under SLICING_METHOD 0 and 2 (k_allot's branches with
    births.h's newborn budgets, carry and credit resets): a 24 x 24 world of
    ancestor point mutants, default mutation rates, DEATH_METHOD 2, adaptive
    steps (always 1 here), 40 updates -- the statistics and every digest equal
    the oracle's after every update; more than 500 births, and deaths under
    INTEGRATED"""
    ov = {"WORLD_X": 24, "WORLD_Y": 24, "SLICING_METHOD": slicing, "DEATH_METHOD": 2}
    iset, env, cfg = pu.load_env(golden, overrides=ov)
    cfg.sub_updates = 0
    n = 576
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    genomes = pu.mutants_of(anc, iset, n, rate=0.01)
    merits = (2.0 ** np.random.default_rng(5).integers(0, 6, n)).tolist()
    orc, gpu = (ol.Backend(k, cfg, iset, env, ncells=n) for k in BOTH)
    for b in (orc, gpu):
        b.set_orgs(0, genomes, merits, deterministic=False)
    births = deaths = 0
    for u in range(40):
        so, sg = orc.run_update(), gpu.run_update()
        for f in STAT_FIELDS:
            assert getattr(so, f) == getattr(sg, f), (u, f, getattr(so, f), getattr(sg, f))
        nbad, cells = pu.compare_digests(orc.digests(), gpu.digests())
        assert nbad == 0, f"update {u}: {nbad} cells differ, first {cells}"
        births += sg.births
        deaths += sg.deaths
    orc.close()
    gpu.close()
    assert births > 500, births
    assert slicing != INTEGRATED or deaths >= 1, deaths


# ---- the chunked top tree: more than 4096 blocks ----
BIG_X, BIG_Y = 1024, 1026                         # 4104 blocks: chunk 0 full, chunk 1 holds 8
BIG_BLOCKS = (0, 2051, 2052, 4095, 4096, 4103)    # both ends of both strips and of both chunks
BIG_UPDATES = 3


@functools.lru_cache(maxsize=None)
def big_seed():
    """(cells, merits, runs): every cell of BIG_BLOCKS plus 3000 random cells,
    merits 2^[0, 8]; runs = the cells as (first, count) ranges, none of which
    crosses the strip edge at block 2052"""
    rng = np.random.default_rng(11)
    n = BIG_X * BIG_Y
    cells = set(int(c) for c in rng.choice(n, 3000, replace=False))
    for b in BIG_BLOCKS:
        cells.update(range(b * 256, b * 256 + 256))
    cells = np.array(sorted(cells), dtype=np.int64)
    merits = 2.0 ** rng.integers(0, 9, len(cells))
    edge = (BIG_Y // 2) * BIG_X
    cut = np.nonzero((np.diff(cells) != 1) | (cells[1:] == edge))[0] + 1
    runs = [(int(r[0]), len(r)) for r in np.split(cells, cut)]
    return cells, merits, runs


def big_world(golden, sub):
    return NopWorld(golden, BIG_X, BIG_Y, PROBABILISTIC, sub=sub)


def big_fill(world, b, lo=0, hi=None):
    """seed the cells of [lo, hi) into backend b at local indices"""
    cells, merits, runs = big_seed()
    hi = world.n if hi is None else hi
    at = 0
    for first, count in runs:
        if lo <= first < hi:
            world.seed(b, first - lo, merits[at:at + count])
        at += count


def big_time_used(b, runs, lo=0):
    """time_used of the cells of `runs`, read range by range (the whole
    world's records are 512 MB)"""
    out = []
    for first, count in runs:
        st = (capi.AvgpuCpuState * count)()
        b._call("get_states", b.h, first - lo, count, st, None, None, 0)
        out.append(np.frombuffer(st, dtype=np.dtype(capi.AvgpuCpuState))["time_used"].astype(np.int64))
    return np.concatenate(out)


BLOCK_RUNS = [(b * 256, 256) for b in BIG_BLOCKS]


@functools.lru_cache(maxsize=None)
def big_reference(golden, sub):
    """the oracle's 3 updates of the big world: per update the digests, the
    budgets of the seeded cells (one batch step) and insts_executed"""
    cells, merits, runs = big_seed()
    world = big_world(golden, sub)
    orc = world.backend("oracle")
    big_fill(world, orc)
    out = []
    for u in range(BIG_UPDATES):
        st = orc.run_update()
        bud = pu.last_budgets(orc).astype(np.int64)
        if sub == 1:
            assert int(bud.sum()) == int(bud[cells].sum()) == AVE * len(cells), u
        out.append((orc.digests(), bud[cells], st.insts_executed))
    orc.close()
    return out


@functools.lru_cache(maxsize=None)
def big_untiled(golden, sub):
    """the untiled GPU world's 3 updates: per update the digests, the
    time_used of the seeded cells (sub = 1) or of BIG_BLOCKS' cells, and
    insts_executed"""
    cells, merits, runs = big_seed()
    world = big_world(golden, sub)
    gpu = world.backend("gpu")
    big_fill(world, gpu)
    out = []
    for u in range(BIG_UPDATES):
        st = gpu.run_update()
        out.append((gpu.digests(), big_time_used(gpu, runs if sub == 1 else BLOCK_RUNS), st.insts_executed))
    gpu.close()
    return out


@pytest.mark.gpu
@pytest.mark.timeout(60)
@pytest.mark.parametrize("sub", (1, 2))
def test_chunked_tree_untiled_gpu(golden, sub):
    """k_tree_up, k_block_counts(chunked = 1) and k_tree_down on a world of
    4104 blocks (BC_OWN): chunk 1 is partly filled (tree_leaf returns 0 past
    nbt; k_tree_down's hi = 7 there), the weight sits at both ends of both
    chunks.  Every digest equals the oracle's over 3 updates; with one batch
    step the seeded cells' time_used deltas equal orc_last_budgets and every
    update hands out 30 x (seeded cells) picks; blocks 4095 and 4096, on
    either side of the chunk edge, both get picks in every update"""
    cells, merits, runs = big_seed()
    assert (BIG_X * BIG_Y + 255) // 256 == 4104 > 4096
    ref, got = big_reference(golden, sub), big_untiled(golden, sub)
    is_block = {b: (cells // 256) == b for b in BIG_BLOCKS}
    prev = None
    for u in range(BIG_UPDATES):
        (dref, bud, insts_ref), (dgot, tu, insts) = ref[u], got[u]
        nbad, where = pu.compare_digests(dref, dgot)
        assert nbad == 0, f"update {u}: {nbad} cells differ, first {where}"
        assert insts == insts_ref == AVE * len(cells), (u, insts, insts_ref)
        delta = tu - (prev if prev is not None else 0)
        prev = tu
        if sub == 1:
            bad = np.nonzero(delta != bud)[0]
            assert len(bad) == 0, f"update {u}: budgets differ at cells {cells[bad[:5]].tolist()}"
            assert int(delta.sum()) == AVE * len(cells)
            share = {b: int(delta[is_block[b]].sum()) for b in BIG_BLOCKS}
        else:
            share = {b: int(delta[256 * i:256 * (i + 1)].sum()) for i, b in enumerate(BIG_BLOCKS)}
        assert share[4095] > 0 and share[4096] > 0, (u, share)


@pytest.mark.gpu
@pytest.mark.timeout(60)
@pytest.mark.parametrize("sub", (1, 2))
def test_chunked_tree_strips_gpu(golden, sub):
    """The same world as 2 loopback strips of 513 rows (BC_GATHERED, 2052
    blocks each): strip 1 starts at block 2052, not a multiple of 4096, and
    its blocks lie in chunks 0 and 1 (asserted), so k_tree_down runs two
    workgroups for it with lo = 2052 in chunk 0 and hi = 7 in chunk 1, and
    k_block_counts(chunked = 1) splits over both chunk roots.  The strips'
    digests equal the untiled GPU world's and the oracle's over 3 updates,
    their insts_executed sum to the untiled world's"""
    import torch
    from avida_amd import tiles
    T, rows = 2, BIG_Y // 2
    world = big_world(golden, sub)
    nloc = rows * BIG_X // 256
    assert rows * BIG_X % 256 == 0 and nloc == 2052
    b0 = 1 * nloc                                  # strip 1's first block
    assert b0 % 4096 != 0 and b0 >> 12 == 0 and (b0 + nloc - 1) >> 12 == 1
    ref, full = big_reference(golden, sub), big_untiled(golden, sub)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    strips = []
    for k in range(T):
        b = world.backend("gpu", ncells=rows * BIG_X)
        b.lib.avgpu_set_stream(b.h, stream)
        t = tiles.Tile(b.lib, b.p, b.h, k * rows, T, "cuda")
        big_fill(world, b, k * rows * BIG_X, (k + 1) * rows * BIG_X)
        strips.append((b, t))
    sw = tiles.StripWorld([t for _, t in strips], tiles.LoopbackTransport())
    try:
        for u in range(BIG_UPDATES):
            sw.update()
            torch.cuda.synchronize()
            assert sw.steps == sub
            insts = 0
            for b, _ in strips:
                s = capi.AvgpuUpdateStats()
                b._call("get_stats", b.h, s)
                insts += s.insts_executed
            assert insts == full[u][2], (u, insts, full[u][2])
            dig = np.concatenate([b.digests() for b, _ in strips])
            for what, want in (("the untiled GPU world", full[u][0]), ("the oracle", ref[u][0])):
                nbad, where = pu.compare_digests(want, dig)
                assert nbad == 0, f"update {u}: {nbad} cells differ from {what}, first {where}"
    finally:
        for b, _ in strips:
            b.close()
