"""Parent derivation for the ancestry tests, from organism states alone.

An offspring's RNG key is derive_key(parent's key, the parent's divide number,
0x1B873593) (avida_amd/csrc/device.h derive_key, oracle/oracle.cc), and every
organism's key is unique.  So the states of a world before and after an update
name every newcomer's parent with no help from the code that records
ancestry: a newcomer is a living cell whose key changed; its parent is the
organism -- living before the update, or itself a newcomer of it -- one of
whose next divide numbers derives the newcomer's key.  The expected parent key
of a newcomer is then the genotype key (census) of that parent organism.

derive_key / lowbias32 are restated here in numpy.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from avida_amd import capi, files
import oracle_lib as ol
import parity_util as pu

CAP = 512
OFFSPRING_SALT = 0x1B873593
MAX_DIVIDES = 8      # divides of one organism in one update the search covers


def lowbias32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def derive_key(a_lo, a_hi, x, y):
    """(lo, hi) of derive_key(a_lo, a_hi, x, y), elementwise over uint32 arrays"""
    a_lo, a_hi = np.asarray(a_lo, dtype=np.uint32), np.asarray(a_hi, dtype=np.uint32)
    x = np.asarray(x, dtype=np.uint32)
    y = np.uint32(y)
    with np.errstate(over="ignore"):
        lo = lowbias32(lowbias32(x ^ a_lo) + y)
        hi = lowbias32(lowbias32(y ^ a_hi) + x + np.uint32(0x632BE5AB))
    return lo, hi


def _field(st, name, dtype):
    """one scalar field of an array of AvgpuCpuState as a numpy array"""
    n, sz = len(st), C.sizeof(capi.AvgpuCpuState)
    raw = np.frombuffer(st, dtype=np.uint8).reshape(n, sz)
    off = getattr(capi.AvgpuCpuState, name).offset
    w = np.dtype(dtype).itemsize
    return np.ascontiguousarray(raw[:, off:off + w]).view(dtype).reshape(n).copy()


class Snapshot:
    """what the derivation reads of a world: per cell alive, RNG key (one
    uint64), divides so far, genotype key"""

    def __init__(self, backend, first=0, count=None):
        n = backend.ncells - first if count is None else count
        st, _, _ = backend.states(first, n, CAP)
        self.alive = _field(st, "alive", np.int32) != 0
        lo, hi = _field(st, "rng_key_lo", np.uint32), _field(st, "rng_key_hi", np.uint32)
        self.lo, self.hi = lo, hi
        self.key = lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32))
        self.ndiv = _field(st, "num_divides", np.int32)
        self.gkey = backend.census(first, n)["genotype_key"].copy()
        self.gkey[~self.alive] = 0

    @staticmethod
    def join(parts):
        s = object.__new__(Snapshot)
        for f in ("alive", "lo", "hi", "key", "ndiv", "gkey"):
            setattr(s, f, np.concatenate([getattr(p, f) for p in parts]))
        return s


def derive_parents(before, after):
    """(newcomers, parent_gkey, unresolved, ambiguous, parent_cell): the cells
    of `after` that hold an organism `before` did not (ascending), the
    genotype key of each one's parent organism (0 where none was found), how
    many found no parent / more than one, and the parent's cell (in `before`,
    or -2 - its cell in `after` when the parent is itself a newcomer; -1 none)."""
    new = np.flatnonzero(after.alive & (~before.alive | (after.key != before.key)))
    want = {int(after.key[c]): int(c) for c in new}
    assert len(want) == len(new), "two newcomers share an RNG key"
    found = {}           # newcomer cell -> [(parent gkey, parent cell)]
    # candidate parents: (lo, hi, divides before the update, genotype key, cell code)
    live = np.flatnonzero(before.alive)
    cand = [(before.lo[live], before.hi[live], before.ndiv[live], before.gkey[live], live)]
    while cand:
        lo, hi, nd0, gk, cell = cand.pop()
        hit = []
        for k in range(1, MAX_DIVIDES + 1):
            clo, chi = derive_key(lo, hi, (nd0 + k).astype(np.uint32), OFFSPRING_SALT)
            ck = clo.astype(np.uint64) | (chi.astype(np.uint64) << np.uint64(32))
            for j in np.flatnonzero(np.isin(ck, after.key[new])):
                c = want[int(ck[j])]
                if c not in found:
                    hit.append(c)
                found.setdefault(c, []).append((int(gk[j]), int(cell[j])))
        if hit:          # the closure: a newcomer may be the parent of another
            h = np.array(sorted(set(hit)), dtype=np.int64)
            cand.append((after.lo[h], after.hi[h], np.zeros(len(h), dtype=np.int32), after.gkey[h], -2 - h))
    pk = np.array([found[int(c)][0][0] if int(c) in found else 0 for c in new], dtype=np.uint64)
    pcell = np.array([found[int(c)][0][1] if int(c) in found else -1 for c in new], dtype=np.int64)
    unresolved = sum(1 for c in new if int(c) not in found)
    ambiguous = sum(1 for v in found.values() if len(v) > 1)
    return new, pk, unresolved, ambiguous, pcell


def expected_parent_keys(prev_expected, before, after):
    """the parent-key row after an update from the one before it: newcomers
    take their derived parent's genotype key, survivors keep theirs, dead
    cells report 0.  Returns (row, newcomers, unresolved, ambiguous, parent cells)."""
    new, pk, unresolved, ambiguous, pcell = derive_parents(before, after)
    row = np.where(after.alive, prev_expected, np.uint64(0)).astype(np.uint64)
    row[new] = pk
    return row, new, unresolved, ambiguous, pcell


# ---- the worlds the parent-key tests run (CPU: the derivation resolves every
# newcomer on the oracle; GPU: pkey == the derivation) ----
# name -> (X, Y, geometry, overrides, sub_updates, serial, updates)
HOT = {"COPY_MUT_PROB": 0.02}     # most births found a genotype
WORLDS = {
    "torus16_bm0": (16, 16, 2, dict(HOT, BIRTH_METHOD=0, ALLOW_PARENT=0), 1, False, 45),
    "torus16_bm4": (16, 16, 2, dict(HOT, BIRTH_METHOD=4), 1, False, 45),
    "torus16_allow_parent": (16, 16, 2, dict(HOT, BIRTH_METHOD=0, ALLOW_PARENT=1, PREFER_EMPTY=0), 1, False, 45),
    "torus16_sub3": (16, 16, 2, dict(HOT, BIRTH_METHOD=0), 3, False, 45),
    "grid9x7_bm0": (9, 7, 1, dict(HOT, BIRTH_METHOD=0, ALLOW_PARENT=0), 1, False, 130),
    "grid9x7_bm4_sub3": (9, 7, 1, dict(HOT, BIRTH_METHOD=4, ALLOW_PARENT=1), 3, False, 130),
    "serial8_bm0": (8, 8, 2, dict(HOT, BIRTH_METHOD=0), 0, True, 130),
    "serial8_bm5": (8, 8, 2, dict(HOT, BIRTH_METHOD=5), 0, True, 130),
}
SEED = 11


def ancestor(golden, iset):
    return files.read_org(os.path.join(golden, "default-heads.org"), iset)


def make_world(kind, golden, name):
    """a full world of the ancestor under WORLDS[name]: (backend, step, updates)"""
    X, Y, geometry, ov, sub, serial, updates = WORLDS[name]
    ov = dict(ov, WORLD_X=X, WORLD_Y=Y, WORLD_GEOMETRY=geometry)
    iset, env, cfg = pu.load_env(golden, overrides=ov, seed=SEED)
    cfg.sub_updates = sub
    anc = ancestor(golden, iset)
    b = ol.Backend(kind, cfg, iset, env, ncells=X * Y)
    b.set_orgs(0, [anc] * (X * Y), deterministic=False)
    return b, (b.run_serial_update if serial else b.run_update), updates


def parent_keys(b, first=0, count=None):
    """avgpu_get_parent_keys of a product backend"""
    n = b.ncells - first if count is None else count
    out = np.zeros(n, dtype=np.uint64)
    b._call("get_parent_keys", b.h, first, n, out.ctypes.data_as(C.c_void_p))
    return out


def set_parent_keys(b, keys, first=0):
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    b._call("set_parent_keys", b.h, first, len(k), k.ctypes.data_as(C.c_void_p))
