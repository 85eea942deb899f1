"""Test-infrastructure loader for the CPU oracle (oracle/liboracle.so).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg use this.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from avida_amd import capi, files
from avida_amd.world import World

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_SO = os.path.join(ORACLE_DIR, "liboracle.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")

_lib = None

# what only the oracle has, or has with a signature of its own
ORACLE_ONLY = {
    "create": (C.c_void_p, [C.POINTER(capi.AvgpuCfg), C.c_int64]),
    "destroy": (None, [C.c_void_p]),
    "rec_exhausted": (C.c_int64, []),
    "last_budgets": (C.c_int, [C.c_void_p, C.c_void_p]),
    "op_hist": (C.c_int, [C.POINTER(C.c_int64), C.c_int]),
}


def load_oracle():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(ORACLE_SO):
        subprocess.run(["make", "-s", "-C", ORACLE_DIR], check=True)
    lib = capi.bind_common(C.CDLL(ORACLE_SO), "orc_")
    _lib = capi.bind(lib, "orc_", ORACLE_ONLY)
    return _lib


class Backend(World):
    """World over the oracle (kind "oracle", prefix orc_) or the product (any
    other kind, avgpu_), plus what only the tests need."""

    def __init__(self, kind, cfg: capi.AvgpuCfg, instset: files.InstSet, reactions, ncells=0,
                 device=0):
        self.kind, self.instset = kind, instset
        super().__init__(cfg, instset, reactions, ncells, device, oracle=load_oracle() if kind == "oracle" else None)

    def set_orgs(self, first, genomes, merits=None, inputs=None, deterministic=True):
        super().set_orgs(first, genomes, merits, inputs, deterministic)

    def set_orgs_np(self, first, blob, lens, merits=None, deterministic=False):
        """set_orgs for large worlds: genomes packed in `blob` (bytes), lens /
        merits numpy arrays"""
        import numpy as np
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        buf, _ = capi.pack_genomes([blob])
        m = None
        if merits is not None:
            merits = np.ascontiguousarray(merits, dtype=np.float64)
            m = merits.ctypes.data_as(C.POINTER(C.c_double))
        self._call("set_orgs", self.h, first, len(lens), buf, lens.ctypes.data_as(C.POINTER(C.c_int32)), m, None,
                   1 if deterministic else 0)

    def step(self, first, count, budget=None, uniform=0, mode=capi.MODE_FROZEN):
        b = None
        if budget is not None:
            b = (C.c_int32 * count)(*budget)
        self._call("step", self.h, first, count, b, uniform, mode)
        if self.kind != "oracle":
            self.lib.avgpu_sync(self.h)

    def digests(self, first=0, count=None):
        """per-cell state digests (numpy uint64) of a cell range:
        avgpu_state_digests / orc_state_digests"""
        import numpy as np
        if count is None:
            count = self.ncells - first
        out = np.zeros(count, dtype=np.uint64)
        self._call("state_digests", self.h, first, count, out.ctypes.data_as(C.c_void_p))
        return out

    def set_rng_mode(self, mode, stream=None, offsets=None):
        """avgpu_set_rng_mode / orc_set_rng_mode: stream = numpy float64
        array (RECORDED), offsets = numpy int64 per cell or None"""
        import numpy as np
        sp, n, op = None, 0, None
        if stream is not None:
            self._rec = np.ascontiguousarray(stream, dtype=np.float64)
            sp, n = self._rec.ctypes.data_as(C.c_void_p), len(self._rec)
        if offsets is not None:
            self._off = np.ascontiguousarray(offsets, dtype=np.int64)
            op = self._off.ctypes.data_as(C.c_void_p)
        self._call("set_rng_mode", self.h, mode, sp, n, op)

    def counters(self, cumulative=0):
        """avgpu_counters of the last update, or summed over every update
        (cumulative=1) (product only)"""
        out = (C.c_int64 * capi.NUM_COUNTERS)()
        self._call("counters", self.h, cumulative, out, capi.NUM_COUNTERS)
        return list(out)

    def run_serial_update(self):
        """one update of the serial world (reference schedule, births at once)"""
        return World.run_update(self, serial=True)     # (not a subclass's run_update, which may call this)


def recalculate(backend: Backend, genomes, generations=3):
    """cTestCPU::TestGenome viability recursion (cpu/cTestCPU.cc:233-326) over a batch.

    Returns per genome (result_at_depth0, exec_flags, viable)."""
    first = backend.test_genomes(genomes)
    viable = [False] * len(genomes)
    # chains: genome index -> list of ancestors' genomes for case 3
    pending = []
    for i, (r, f, child) in enumerate(first):
        if not r.divided:
            continue
        if r.copy_true:
            viable[i] = True
        else:
            pending.append((i, [genomes[i]], child))
    depth = 1
    while pending and depth < generations:
        nxt = []
        res = backend.test_genomes([c for (_, _, c) in pending])
        for (i, anc, child), (r, f, grandchild) in zip(pending, res):
            if not r.divided:
                continue
            if r.copy_true:
                viable[i] = True
                continue
            anc2 = anc + [child]
            if any(grandchild == a for a in anc2):
                viable[i] = True
                continue
            nxt.append((i, anc2, grandchild))
        # case 3 at depth>0 checks the offspring of depth d against ancestors < d
        pending = nxt
        depth += 1
    return [(r, f, viable[i]) for i, (r, f, _) in enumerate(first)]


AVGPU_FLAGS_CAP = 2049
