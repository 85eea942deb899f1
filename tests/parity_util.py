"""Helpers shared by the parity tests: build matched oracle/GPU backends and
compare organism state tuples field by field."""
from __future__ import annotations

import os
import random

from avida_amd import capi, files
import oracle_lib as ol

STATE_FIELDS = [n for n, _ in capi.AvgpuCpuState._fields_ if not n.startswith("pad")]


def state_tuple(s):
    out = {}
    for n in STATE_FIELDS:
        v = getattr(s, n)
        if hasattr(v, "__len__"):
            v = [list(x) if hasattr(x, "__len__") else x for x in v]
        out[n] = v
    return out


def diff_states(a, b, ops_a, ops_b, fl_a, fl_b, cap):
    """Return a list of (index, field, a, b) mismatches; memory compared up to mem_size."""
    bad = []
    for i in range(len(a)):
        if a[i].birth_length == 0 and b[i].birth_length == 0:
            continue   # never-occupied cell: no organism, nothing to compare
        ta, tb = state_tuple(a[i]), state_tuple(b[i])
        for k in STATE_FIELDS:
            if ta[k] != tb[k]:
                bad.append((i, k, ta[k], tb[k]))
        m = a[i].mem_size
        if m == b[i].mem_size:
            o = i * cap
            if ops_a[o:o + m] != ops_b[o:o + m]:
                bad.append((i, "mem_ops", None, None))
            if fl_a[o:o + m] != fl_b[o:o + m]:
                bad.append((i, "mem_flags", None, None))
    return bad


def load_env(golden, instset="instset-heads.cfg", overrides=None, seed=7):
    iset = files.read_instset(os.path.join(golden, instset))
    env = files.read_environment(os.path.join(golden, "environment-logic9.cfg"))
    cfg = capi.cfg_from_avida(files.read_avida_cfg(None, overrides or {}), seed=seed)
    return iset, env, cfg


def pop_genomes(golden, iset_classic):
    """BASELINE config 2: the 3599 organisms of heads_midrun_30u/config/detail-50000.pop
    (genotypes expanded by num_cpus, classic legacy instset) + the ancestor."""
    gs = files.read_pop(os.path.join(golden, "detail-50000.pop"))
    out = []
    for g in gs:
        seq = iset_classic.parse_sequence(g.sequence)
        out.extend([seq] * g.num_cpus)
    return out


def random_genomes(iset, n, lo=8, hi=400, seed=1):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        L = rnd.randint(lo, hi)
        out.append(bytes(rnd.randrange(len(iset.names)) for _ in range(L)))
    return out


def mutants_of(seq, iset, n, rate=0.03, seed=2):
    """Point mutants of a viable genome: exercises copy loops, divides, labels."""
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        g = bytearray(seq)
        for i in range(len(g)):
            if rnd.random() < rate:
                g[i] = rnd.randrange(len(iset.names))
        out.append(bytes(g))
    return out


def diff_states_np(a, b, ops_a, ops_b, fl_a, fl_b, cap, first=0, limit=20):
    """diff_states for large worlds: raw struct bytes and memory images are
    compared with numpy, the field-by-field report only for mismatching cells
    (at most `limit`).  Returns (number of mismatching cells, report)."""
    import ctypes as C
    import numpy as np
    n = len(a)
    sz = C.sizeof(capi.AvgpuCpuState)
    ra = np.frombuffer(a, dtype=np.uint8).reshape(n, sz)
    rb = np.frombuffer(b, dtype=np.uint8).reshape(n, sz)
    bad = np.any(ra != rb, axis=1)
    msz = np.frombuffer(a, dtype=np.uint8).reshape(n, sz)[:, capi.AvgpuCpuState.mem_size.offset:
                                                            capi.AvgpuCpuState.mem_size.offset + 4]
    m = np.ascontiguousarray(msz).view(np.int32).reshape(n)
    keep = np.arange(cap)[None, :] < np.minimum(m, cap)[:, None]
    oa = np.frombuffer(ops_a, dtype=np.uint8).reshape(n, cap)
    ob = np.frombuffer(ops_b, dtype=np.uint8).reshape(n, cap)
    fa = np.frombuffer(fl_a, dtype=np.uint8).reshape(n, cap)
    fb = np.frombuffer(fl_b, dtype=np.uint8).reshape(n, cap)
    bad |= np.any((oa != ob) & keep, axis=1) | np.any((fa != fb) & keep, axis=1)
    idx = np.nonzero(bad)[0]
    report = []
    for i in idx[:limit]:
        i = int(i)
        ta, tb = state_tuple(a[i]), state_tuple(b[i])
        diffs = [k for k in STATE_FIELDS if ta[k] != tb[k]]
        report.append((first + i, diffs or ["memory"]))
    return len(idx), report


M64 = (1 << 64) - 1


def _mix(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def digest_of(state, ops, flags, handlers):
    """Python restatement of the per-cell state digest (avida_amd/csrc/state.hip
    k_state_digest, oracle orc_state_digests) from one avgpu_get_states record
    and its memory (op codes, flags bit0 copied / bit2 executed)."""
    import ctypes as C
    import struct
    if state.birth_length == 0:
        return 0
    raw = bytes(C.string_at(C.addressof(state), C.sizeof(state)))
    h = 0x9E3779B97F4A7C15
    for k, (w,) in enumerate(struct.iter_unpack("<I", raw)):
        h = _mix(h ^ ((k << 32) | w))
    m = state.mem_size
    for k in range((m + 3) // 4):
        v = 0
        for j in range(4):
            q = 4 * k + j
            if q < m:
                b = (handlers[ops[q]] & 0x3F) | (0x40 if flags[q] & 1 else 0) | (0x80 if flags[q] & 4 else 0)
                v |= b << (8 * j)
        h = _mix(h ^ (((0x10000 + k) << 32) | v))
    return h


def compare_digests(da, db, first=0, limit=10):
    """(number of differing cells, first `limit` differing global cell ids)"""
    import numpy as np
    idx = np.nonzero(da != db)[0]
    return len(idx), [int(first + i) for i in idx[:limit]]


# ---------------------------------------------------------------------------
# LDS size classes of the interpreter (tests/test_size_classes.py): a class
# view over state arrays, and worlds whose organisms outgrow their slots on
# demand.

# device.h CLASS0_SIZE .. CLASS3_SIZE (and class_of)
CLASS_SIZES = (320, 768, 1536, 2048)
# The capacities a slice passes through, by route and by the class k_allot gave
# it; an organism whose memory outgrows one capacity spills into the next.
#  "update" (run_update, main and newborn pass): the list classes run in the
#    class-0 launch's mixed blocks, interp_core.h interpret_chunk's Scap =
#    min(S * kslot, 2048) with k_interpret's kslot 3 / 5 / 7 (interp_launch.h)
#    = 960 / 1600 / 2048; a class-0 spill is continued by its own wave in a
#    960-site slot (k_interpret's run_chunk); every later spill goes to rows
#    5 + 6, which run in class 3's slots (interp.hip launch_classes)
#  "step_world" (avgpu_step, MODE_WORLD): class 0 continues in-wave as above,
#    the list classes run their rows, Scap = S (launch_classes' rows 1..3)
#  "step_frozen" (avgpu_step, other modes): class 0's spills run row 4 in
#    class 1's slots (launch_classes' row 4)
SLOT_CHAINS = {
    "update": ((320, 960, 2048), (960, 2048), (1600, 2048), (2048,)),
    "step_world": ((320, 960, 2048), (768, 2048), (1536, 2048), (2048,)),
    "step_frozen": ((320, 768, 2048), (768, 2048), (1536, 2048), (2048,)),
}
# organisms per chunk and blocks of the mixed launch's list classes 1 / 2 / 3
# (interp_launch.h MIX_B1 / MIX_B2 / MIX_B3, k_interpret's per = 64 / kslot)
MIX_GRIDS = ((21, 512), (12, 16), (9, 8))
PER3 = 21                      # k_interpret's PER3: continued spills per group


def state_array(backend, n=None):
    """the backend's state records as a numpy structured array (a copy)"""
    import numpy as np
    n = n or backend.ncells
    st = (capi.AvgpuCpuState * n)()
    backend._call("get_states", backend.h, 0, n, st, None, None, 0)
    return np.frombuffer(st, dtype=np.dtype(capi.AvgpuCpuState)).copy()


def class_view(s, route, size_range=2):
    """Per cell of a state array: (need, class, capacity) -- device.h need_of
    (:900-904: the memory, or what h-alloc would grow it to while the organism
    has not allocated) and class_of, and the capacity of the slot the cell's
    slice starts in on `route` (SLOT_CHAINS)."""
    import numpy as np
    m = s["mem_size"].astype(np.int64)
    grown = m + np.minimum(size_range * m, capi.MAX_GENOME - m)
    need = np.where(s["mal_active"] != 0, m, np.maximum(grown, m))
    cls = np.searchsorted(CLASS_SIZES[:3], need, side="left")
    cap = np.array([SLOT_CHAINS[route][c][0] for c in range(4)])[cls]
    return need, cls, cap


def expected_spills(before, after, route):
    """Per cell, the spills of one call on `route`, from the oracle's states
    before the call and after its slices (before any placement): an organism
    alive before it spills once for every capacity of its class's chain that
    its memory afterwards exceeds.  (Every construction here grows at most
    once past each capacity per call, and never shrinks after growing.)"""
    import numpy as np
    _, cls, _ = class_view(before, route)
    m = after["mem_size"].astype(np.int64)
    hops = np.zeros(len(before), dtype=np.int64)
    for c in range(4):
        sel = (cls == c) & (before["alive"] != 0)
        for cap in SLOT_CHAINS[route][c]:
            hops[sel & (m > cap)] += 1
    return hops


def last_budgets(orc):
    """the oracle's budgets of its last allotment (orc_last_budgets)"""
    import ctypes as C
    import numpy as np
    out = np.zeros(orc.ncells, dtype=np.int32)
    got = orc.lib.orc_last_budgets(C.c_void_p(orc.h), out.ctypes.data_as(C.c_void_p))
    assert got == orc.ncells
    return out


def padded_ancestor(anc, length, iset):
    """default-heads.org with nop-C added to its run of nop-C up to `length`
    sites: the same replicator (h-alloc, h-search, copy loop, h-divide)"""
    assert length >= len(anc)
    nopc = iset.op_of_name("nop-C")
    assert anc[10] == nopc
    return anc[:10] + bytes([nopc]) * (length - len(anc)) + anc[10:]


def predivide_records(orc, iset, anc, cells, sizes, merit=100.0):
    """Construction 1: for each of `cells` a record of an organism about to
    divide -- a parent of P sites (the padded ancestor, every site flagged
    executed) followed by its copy of C sites (the ancestor padded to C,
    flagged copied), memory allocated, the instruction pointer on the
    parent's h-divide, read head at P, write head at 0, birth and genome
    length max(P, C) -- so that its first instruction divides (the parent
    keeps P sites, the pointer returns to 0) and its second, h-alloc, grows
    it to min(3 P, 2048) sites.  sizes: one (P, C) per cell.  The records
    start from what the oracle `orc` holds after an ordinary injection, which
    gives them valid inputs and keys; returns (records, ops, flags) for
    set_states with cap MAX_GENOME, one cell at a time."""
    cap = capi.MAX_GENOME
    out = []
    for cell, (P, C) in zip(cells, sizes):
        orc.set_orgs(cell, [padded_ancestor(anc, max(P, C), iset)], [merit], deterministic=False)
        st, _, _ = orc.states(cell, 1, cap)
        s = st[0]
        tape = padded_ancestor(anc, P, iset) + padded_ancestor(anc, C, iset)
        assert len(tape) <= cap and iset.names[tape[P - 4]] == "h-divide" and iset.names[tape[0]] == "h-alloc"
        s.mem_size, s.mal_active = P + C, 1
        s.head[0], s.head[1], s.head[2], s.head[3] = P - 4, P, 0, P - 8
        s.birth_length = s.genome_length = max(P, C)
        ops = tape + bytes(cap - len(tape))
        flags = bytes([4]) * P + bytes([1]) * C + bytes(cap - len(tape))
        out.append((cell, st, ops, flags))
    return out


def put_records(backend, records):
    """hand construction-1 records to a backend (set_states)"""
    import ctypes as C
    cap = capi.MAX_GENOME
    for cell, st, ops, flags in records:
        backend._call("set_states", backend.h, cell, 1, st,
                      (C.c_uint8 * cap).from_buffer_copy(ops), (C.c_uint8 * cap).from_buffer_copy(flags), cap)


def chain_genome(iset, length=100):
    """Construction 2 (REQUIRE_ALLOCATE 0): h-alloc nop-C three times, then
    nop-C -- 100 -> 300 -> 900 -> 2048 sites in five instructions"""
    ha, nc = iset.op_of_name("h-alloc"), iset.op_of_name("nop-C")
    return bytes([ha, nc] * 3) + bytes([nc]) * (length - 6)


def constant_streams(n, hit_cells, per=4096, hit=0.25, miss=0.75):
    """Construction 3: a recorded stream of two constant segments and per-cell
    offsets -- the cells of hit_cells draw `hit` for ever, the others `miss`"""
    import numpy as np
    stream = np.concatenate([np.full(per, hit), np.full(per, miss)])
    off = np.full(n, per, dtype=np.int64)
    off[list(hit_cells)] = 0
    return stream, off


def scattered(n, k, seed=3):
    """k of n lanes, scattered (no prefix), ascending"""
    return sorted(random.Random(seed * 1000 + k).sample(range(n), k))
