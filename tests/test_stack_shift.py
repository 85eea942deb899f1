"""Class 0's register stacks in depth order (avida_amd/csrc/stack_rot.h;
interp_core.h VSTK): the class-0 kernels rotate the record's stack rings to
depth order at stage-in and back at write-back, and run pop and push as shifts
in the branch-free part of the iteration, without parking.  The record, the
pointers and everything outside those kernels keep the ring.

Worlds of hand-written organisms, one wave (8 x 8) or two (16 x 8), constant
slicing (a slice is exactly AVE_TIME_SLICE instructions), GPU against the
oracle: every cell's state record (stack, stack_ptr and cur_stack among its
fields), its tape and flags, its digest and the update's statistics after every
update.  What a world is built to show is asserted from the oracle's states
alone in the unmarked tests, so that a GPU test cannot pass vacuously."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from avida_amd import build, capi, files
import oracle_lib as ol
import parity_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = capi.MAX_GENOME
STK = 10                     # AVGPU_STACK_SIZE
STAT_FIELDS = ("num_organisms", "insts_executed", "births", "deaths", "divides", "births_dropped",
               "births_overwritten", "births_cancelled", "cum_insts_executed", "cum_births", "slices")
ENVS = ("def", "rec", "res", "generic")     # the class-0 kernel families: plain, REC, RES, !SIMPLE


# ---- the rotations themselves, on the host ---------------------------------

def test_rotations_on_the_host(tmp_path):
    """stack_rot.h compiled for the host: both rotations at all 10 x 10 pointer
    pairs, and shifted pushes / pops against the ring through more than a full
    turn (tests/host/stack_rot_check.cc)"""
    exe = str(tmp_path / "stack_rot_check")
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or \
        os.path.join(os.path.dirname(os.path.realpath(build.HIPCC)), "..", "lib", "llvm", "bin", "clang++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "avida_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "stack_rot_check.cc")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


# ---- worlds -----------------------------------------------------------------

class World:
    """genomes: one per cell from cell 0 (None: the cell stays empty); patch:
    {field: {cell: value}} written over the injected records by set_states on
    either backend (registers, stacks, pointers: an injected organism has none)."""

    def __init__(self, golden, X, Y, genomes, slice_len, env="def", instset="instset-classic.cfg", ov=None,
                 patch=None, seed=7):
        ov = dict({"WORLD_X": X, "WORLD_Y": Y, "SLICING_METHOD": 0, "AVE_TIME_SLICE": slice_len,
                   "COPY_MUT_PROB": 0.0}, **(ov or {}))
        self.iset, self.env, self.cfg = pu.load_env(golden, instset=instset, overrides=ov, seed=seed)
        self.cfg.sub_updates = 1               # one batch step per update: one slice per organism and update
        if env == "res":                       # the bench's resource environment
            import bench
            self.env = files.parse_environment(bench.resource_env_text(X, Y))
        elif env == "generic":                 # a twice-only requisite is outside the simple form
            for r in self.env:
                r.has_requisite, r.min_count, r.max_count = 1, 0, 2
        self.rec = env == "rec"
        self.n = X * Y
        self.genomes, self.patch = list(genomes), patch or {}

    def backend(self, kind):
        b = ol.Backend(kind, self.cfg, self.iset, self.env, ncells=self.n)
        for c, g in enumerate(self.genomes):
            if g is not None:
                b.set_orgs(c, [g], [100.0], deterministic=False)
        if self.patch:
            st, ops, fl = b.states(0, self.n, CAP)
            for field, values in self.patch.items():
                for cell, v in values.items():
                    put(st[cell], field, v)
            b._call("set_states", b.h, 0, self.n, st, (C.c_uint8 * len(ops)).from_buffer_copy(ops),
                    (C.c_uint8 * len(fl)).from_buffer_copy(fl), CAP)
        if self.rec:                           # every cell its own segment of one recorded stream
            per = 2000
            b.set_rng_mode(capi.RNG_RECORDED, np.random.default_rng(5).random(self.n * per),
                           np.arange(self.n, dtype=np.int64) * per)
        return b


def put(rec, field, v):
    if field == "stack":
        for k in range(2):
            for j in range(STK):
                rec.stack[k][j] = v[k][j]
    elif isinstance(v, (tuple, list)):
        for j, x in enumerate(v):
            getattr(rec, field)[j] = x
    else:
        setattr(rec, field, v)


def compare(orc, gpu, n, what):
    a, oa, fa = orc.states(0, n, CAP)
    b, ob, fb = gpu.states(0, n, CAP)
    bad = pu.diff_states(a, b, oa, ob, fa, fb, CAP)
    assert not bad, f"{what}: {len(bad)} mismatches: {bad[:5]}"
    nbad, cells = pu.compare_digests(orc.digests(0, n), gpu.digests(0, n))
    assert nbad == 0, f"{what}: {nbad} cell digests differ, first {cells}"


def run(world, updates, with_gpu, first_compare=False):
    """The oracle's state arrays after every update (index 0: before the
    first), its statistics per update, and the GPU's counters per update; with
    a GPU every update is compared."""
    orc = world.backend("oracle")
    gpu = world.backend("gpu") if with_gpu else None
    ends, stats, counters = [pu.state_array(orc)], [], []
    if gpu and first_compare:
        compare(orc, gpu, world.n, "as handed in")
    for upd in range(updates):
        so = orc.run_update()
        if gpu:
            sg = gpu.run_update()
            for f in STAT_FIELDS:
                assert getattr(so, f) == getattr(sg, f), (upd, f, getattr(so, f), getattr(sg, f))
            assert list(so.task_orgs) == list(sg.task_orgs), upd
            compare(orc, gpu, world.n, f"update {upd}")
            c = gpu.counters()
            assert c[capi.CNT_BAD_RECORD] == 0 and c[capi.CNT_REC_EXHAUSTED] == 0
            counters.append(c)
        ends.append(pu.state_array(orc))
        stats.append(so)
    if world.rec:
        assert orc.lib.orc_rec_exhausted() == 0
    orc.close()
    if gpu:
        gpu.close()
    return ends, stats, counters


def regs_of(lane):
    """three distinct non-zero register values per lane"""
    return (7 * lane + 1, -(lane + 3), 0x1000 + lane)


# ---- ring positions and wrap ------------------------------------------------

def ring_genome(iset, lane):
    """A straight line: k = lane % 13 pushes (11 and 12 overwrite the ring's
    oldest entries), then k + 2 pops (the last two from an empty stack), each
    with a nop modifier A / B / C in turn or none; by lane // 13 a swap-stk
    leads, and one sits in the middle of the pushes and of the pops, so that
    both stacks hold data and the current stack differs from lane to lane."""
    op = iset.op_of_name
    k, v = lane % 13, lane // 13
    nops = [op("nop-A"), op("nop-B"), op("nop-C"), None]

    def stack_ops(name, count, phase, swap_at):
        out = []
        for j in range(count):
            if j == swap_at:
                out.append(op("swap-stk"))
            out.append(op(name))
            m = nops[(j + phase) % 4]
            if m is not None:
                out.append(m)
        return out

    g = [op("swap-stk")] if v & 1 else []
    g += stack_ops("push", k, lane, k // 2 if v >= 2 else -1)
    g += [op("inc"), op("nop-A")]
    g += stack_ops("pop", k + 2, lane + 1, (k + 2) // 2 if v >= 2 else -1)
    g += [op("swap-stk"), op("inc"), op("nop-C")]
    while len(g) < 12:                          # (AVGPU_MIN_GENOME is 8)
        g.append(op("nop-C"))
    return bytes(g)


def ring_world(golden, slice_len, env="def"):
    iset = files.read_instset(os.path.join(golden, "instset-classic.cfg"))
    genomes = [ring_genome(iset, lane) for lane in range(64)]
    return World(golden, 8, 8, genomes, slice_len, env=env, patch={"reg": {c: regs_of(c) for c in range(64)}})


def walk(iset, genome, steps):
    """The first `steps` instructions of one of the straight-line genomes above
    (push, pop, inc, swap-stk and nops only; the pointer wraps at the end):
    (stack pointers, current stack, the largest pushes - pops reached per stack)"""
    names = [iset.names[c] for c in genome]
    assert set(names) <= {"push", "pop", "inc", "swap-stk", "nop-A", "nop-B", "nop-C"}
    ip, cur, sp, net, peak = 0, 0, [0, 0], [0, 0], [0, 0]
    for _ in range(steps):
        name = names[ip]
        if name == "push":
            sp[cur] = (sp[cur] - 1) % STK
            net[cur] += 1
            peak[cur] = max(peak[cur], net[cur])
        elif name == "pop":
            sp[cur] = (sp[cur] + 1) % STK
            net[cur] -= 1
        elif name == "swap-stk":
            cur ^= 1
        if name in ("push", "pop", "inc") and ip + 1 < len(names) and names[ip + 1].startswith("nop-"):
            ip += 1
        ip = (ip + 1) % len(names)
    return sp, cur, peak


def check_ring_design(world, ends, slice_len):
    """from the oracle's states alone: the update ends show every pointer value
    on stack 0 and at least 5 on stack 1, lanes of the one wave that differ in
    their current stack, and an organism more than 10 pushes deep -- read from
    its genome and the instructions the oracle says it ran, a walk the oracle's
    own pointers confirm at every update end"""
    sp0, sp1, deep, mixed = set(), set(), 0, 0
    for u, s in enumerate(ends[1:], 1):
        assert (s["alive"] != 0).all() and (s["time_used"] == u * slice_len).all(), u
        for c in range(world.n):
            sp, cur, peak = walk(world.iset, world.genomes[c], int(s["time_used"][c]))
            assert (list(s["stack_ptr"][c]), int(s["cur_stack"][c])) == (sp, cur), (u, c)
            deep += max(peak) > STK
        sp0 |= set(int(x) for x in s["stack_ptr"][:, 0])
        sp1 |= set(int(x) for x in s["stack_ptr"][:, 1])
        mixed += len(set(int(x) for x in s["cur_stack"])) == 2
        assert (s["stack"] != 0).any()
    assert sp0 == set(range(STK)) and len(sp1) >= 5 and deep > 0 and mixed > 0, (sp0, sp1, deep, mixed)


RING_UPDATES = 12
RING_CASES = [(e, s) for e in ENVS for s in (1, 3, 7)]


@pytest.mark.parametrize("slice_len", [1, 3, 7])
def test_ring_design_on_oracle(golden, slice_len):
    world = ring_world(golden, slice_len)
    ends, _, _ = run(world, RING_UPDATES, with_gpu=False)
    check_ring_design(world, ends, slice_len)


@pytest.mark.gpu
@pytest.mark.parametrize("env,slice_len", RING_CASES)
def test_ring_positions_and_wrap(golden, env, slice_len):
    """slices of 1, 3 and 7 instructions end between any two stack ops, so the
    rotations run at every pointer value; again from recorded streams, in the
    resource environment and in a generic one -- each its own kernel"""
    world = ring_world(golden, slice_len, env=env)
    ends, _, _ = run(world, RING_UPDATES, with_gpu=True)
    check_ring_design(world, ends, slice_len)


# ---- state handed in ----------------------------------------------------------

def handed_in_world(golden):
    world = ring_world(golden, 7)
    world.patch.update({
        "stack": {c: [[1000 * (k + 1) + 10 * c + j + 1 for j in range(STK)] for k in range(2)] for c in range(64)},
        "stack_ptr": {c: (c % STK, (3 * c + c // STK + 1) % STK) for c in range(64)},
        "cur_stack": {c: (c >> 1) & 1 for c in range(64)},
    })
    return world


def check_handed_in(ends):
    s = ends[0]
    assert (s["stack"] != 0).all()
    both = (s["stack_ptr"][:, 0] != 0) & (s["stack_ptr"][:, 1] != 0)
    assert both.sum() > 32 and len(set(map(tuple, s["stack_ptr"]))) > 20
    assert (ends[1]["stack"] != s["stack"]).any()        # the update's stack ops changed the rings


def test_handed_in_design_on_oracle(golden):
    check_handed_in(run(handed_in_world(golden), 1, with_gpu=False)[0])


@pytest.mark.gpu
def test_state_handed_in(golden):
    """avgpu_set_states with full rings and pointers other than 0 on both
    stacks: read back untouched, then after each of three updates"""
    ends, _, _ = run(handed_in_world(golden), 3, with_gpu=True, first_compare=True)
    check_handed_in(ends)


# ---- neighbours in the same iteration ----------------------------------------

SNIPPETS = (("push", "nop-A"), ("push",), ("push", "nop-C"), ("pop", "nop-A"), ("pop",), ("pop", "nop-C"),
            ("h-copy",), ("if-label", "nop-A"), ("if-label", "nop-B", "nop-C"), ("IO", "nop-A"), ("IO",),
            ("nand",), ("nand", "nop-A"), ("swap-stk",), ("inc", "nop-C"), ("add",))
BESIDE = ("h-copy", "if-label", "IO", "nand")


def neighbour_genomes(iset, n):
    """per lane its own sequence of 16 snippets, stack ops beside h-copy,
    if-label, IO and nand: the lanes of a wave are at different ops in every
    iteration, so the inline blocks run under partial masks"""
    out, heads = [], []
    for lane in range(n):
        rnd = random.Random(1000 + lane)
        seq = [SNIPPETS[rnd.randrange(len(SNIPPETS))] for _ in range(16)]
        heads.append([s[0] for s in seq])
        out.append(bytes(iset.op_of_name(x) for s in seq for x in s))
    return out, heads


def neighbour_world(golden):
    iset = files.read_instset(os.path.join(golden, "instset-classic.cfg"))
    genomes, heads = neighbour_genomes(iset, 128)
    world = World(golden, 16, 8, genomes, 5, ov={"COPY_MUT_PROB": 0.0075},
                  patch={"reg": {c: regs_of(c) for c in range(128)}})
    return world, heads


def check_neighbours(heads, ends):
    pairs = set()
    for h in heads:
        for a, b in zip(h, h[1:]):
            if a in ("push", "pop") and b in BESIDE:
                pairs.add((a, b))
            if b in ("push", "pop") and a in BESIDE:
                pairs.add((b, a))
    assert pairs == {(s, o) for s in ("push", "pop") for o in BESIDE}
    # at every step of the first slice some lanes are at a stack op and others are not
    for step in range(5):
        at = [h[step] in ("push", "pop") for h in heads[:64]]
        assert 4 < sum(at) < 60, (step, sum(at))
    last = ends[-1]
    assert (last["stack"] != 0).any() and (last["output_total"] > 0).any() and (last["alive"] != 0).all()


def test_neighbours_design_on_oracle(golden):
    world, heads = neighbour_world(golden)
    check_neighbours(heads, run(world, 8, with_gpu=False)[0])


@pytest.mark.gpu
def test_neighbours_in_the_same_iteration(golden):
    world, heads = neighbour_world(golden)
    check_neighbours(heads, run(world, 8, with_gpu=True)[0])


# ---- divide and newborn pass ---------------------------------------------------

PARENTS = [y * 16 + x for y in range(8) for x in range(16) if (x + y) % 2 == 0]
CHILD_HEADS = (("inc", "push", "inc", "push", "nop-B", "swap-stk", "inc", "nop-A", "push", "nop-A", "pop", "nop-C"),
               ("inc", "nop-C", "push", "nop-C", "push", "nop-C", "pop", "swap-stk", "push", "nop-C"),
               ("pop", "inc", "push", "push", "push", "swap-stk", "inc", "push"))


def divide_world(golden):
    """The parents of test_size_classes' construction 1 (their first
    instruction divides) on the even diagonals of 16 x 8, handed in with full
    stacks and pointers that differ by lane; each offspring is the ancestor
    behind a head of pushes and pops, which it runs in the update of its birth
    (the newborn pass, 30 instructions)."""
    iset = files.read_instset(os.path.join(golden, "instset-heads.cfg"))
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    P = Cn = 106
    world = World(golden, 16, 8, [None] * 128, 30, instset="instset-heads.cfg",
                  ov={"DIVIDE_INS_PROB": 0.0, "DIVIDE_DEL_PROB": 0.0})
    scratch = ol.Backend("oracle", world.cfg, world.iset, world.env, ncells=world.n)
    records = pu.predivide_records(scratch, iset, anc, PARENTS, [(P, Cn)] * len(PARENTS))
    scratch.close()
    world.records = []
    for i, (cell, st, ops, flags) in enumerate(records):
        head = bytes(iset.op_of_name(x) for x in CHILD_HEADS[i % 3])
        # the ancestor with a shorter run of nop-C, so that the offspring stays class 0 (3 x 106 sites)
        assert iset.names[anc[4]] == "mov-head" and iset.names[anc[-9]] == "h-search"
        child = head + anc[:5] + bytes([iset.op_of_name("nop-C")]) * (Cn - len(head) - 14) + anc[-9:]
        ops = ops[:P] + child + ops[P + Cn:]
        put(st[0], "stack", [[100 * (k + 1) + i + j + 1 for j in range(STK)] for k in range(2)])
        put(st[0], "stack_ptr", (i % STK, (7 * i + 3) % STK))
        st[0].cur_stack = i & 1
        world.records.append((cell, st, ops, flags))
    return world


class DivideWorld:
    """World's interface over the records of divide_world"""

    def __init__(self, golden):
        self.w = divide_world(golden)
        self.n, self.rec = self.w.n, False

    def backend(self, kind):
        b = self.w.backend(kind)
        pu.put_records(b, self.w.records)
        return b


def check_divide(ends, stats):
    before, first = ends[0], ends[1]
    assert (before["stack"][PARENTS] != 0).all() and stats[0].divides == len(PARENTS) and stats[0].births > 32
    # the parents' stacks were cleared: 29 instructions of the ancestor's start hold no stack op
    # (a parent may have been replaced by a neighbour's offspring: those that kept their key)
    kept = [c for c in PARENTS if (before["rng_key_lo"][c], before["rng_key_hi"][c]) ==
            (first["rng_key_lo"][c], first["rng_key_hi"][c])]
    assert len(kept) > 48 and (first["num_divides"][kept] == 1).all()
    assert not first["stack"][kept].any() and not first["stack_ptr"][kept].any()
    # newborns with stack entries at the end of the update of their birth
    nb = (before["alive"] == 0) & (first["alive"] != 0)
    assert (nb & (first["time_used"] > 0) & (first["stack"] != 0).any(axis=(1, 2))).sum() > 32
    assert len(set(map(tuple, first["stack_ptr"][nb]))) >= 3


def test_divide_design_on_oracle(golden):
    ends, stats, _ = run(DivideWorld(golden), 2, with_gpu=False)
    check_divide(ends, stats)


@pytest.mark.gpu
def test_divide_and_newborn_pass(golden):
    ends, stats, _ = run(DivideWorld(golden), 5, with_gpu=True)
    check_divide(ends, stats)


# ---- spill continuation ----------------------------------------------------------

SPILL_HEAD = ("inc", "push", "inc", "nop-A", "push", "nop-A", "swap-stk", "inc", "nop-C", "push", "nop-C", "push",
              "h-alloc", "pop", "nop-C", "swap-stk", "pop", "push", "nop-C", "inc", "push", "nop-A", "inc")


def spill_world(golden):
    """REQUIRE_ALLOCATE 0.  Even lanes: 110 sites handed in as allocated --
    class 0 (device.h need_of) -- push on both stacks, h-alloc to 330 sites in
    mid-slice, past class 0's 320, and pop as class 1, continued by their wave.
    Odd lanes: the same genome not yet allocated needs 330 sites from the
    start, a list class with its stacks in LDS, and spills nowhere."""
    iset = files.read_instset(os.path.join(golden, "instset-heads.cfg"))
    nc = iset.op_of_name("nop-C")
    head = bytes(iset.op_of_name(x) for x in SPILL_HEAD)
    n = 64
    genomes = []
    for lane in range(n):
        pre = bytes([nc]) * (lane % 5)           # the lanes reach their ops in different iterations
        genomes.append(pre + head + bytes([nc]) * (110 - len(pre) - len(head)))
    return World(golden, 8, 8, genomes, 30, instset="instset-heads.cfg", ov={"REQUIRE_ALLOCATE": 0},
                 patch={"mal_active": {c: 1 for c in range(0, n, 2)}, "reg": {c: regs_of(c) for c in range(n)}})


def check_spill(ends, counters):
    before, first = ends[0], ends[1]
    _, cls, _ = pu.class_view(before, "update")
    even, odd = np.arange(0, 64, 2), np.arange(1, 64, 2)
    assert (cls[even] == 0).all() and (cls[odd] == 1).all()
    assert (first["mem_size"] == 330).all() and (first["errors"] == 0).all() and (first["alive"] != 0).all()
    assert (first["stack"][:, 0] != 0).any(axis=1).all() and (first["stack_ptr"] != 0).any(axis=1).all()
    for u in range(len(ends) - 1):
        hops = pu.expected_spills(ends[u], ends[u + 1], "update")
        want = 32 if u == 0 else 0
        assert hops.sum() == want and (u > 0 or (hops[even] == 1).all())
        if counters:
            assert counters[u][capi.CNT_SPILLS] == want, (u, counters[u][capi.CNT_SPILLS])


def test_spill_design_on_oracle(golden):
    ends, _, counters = run(spill_world(golden), 3, with_gpu=False)
    check_spill(ends, counters)


@pytest.mark.gpu
def test_spill_continuation(golden):
    ends, _, counters = run(spill_world(golden), 3, with_gpu=True)
    check_spill(ends, counters)
