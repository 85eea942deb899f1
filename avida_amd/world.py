"""One world behind the C-ABI: the calls the product (libavida_gpu.so, prefix
avgpu_) and the CPU oracle (prefix orc_) share.  driver.ProductWorld adds what
only the product has, the tests' oracle_lib.Backend what only the tests need."""
from __future__ import annotations

import ctypes as C

from . import capi, checkpoint


class World:
    def __init__(self, cfg, iset, env, ncells=0, device=0, oracle=None):
        """`oracle`: the loaded oracle library, or None for the product"""
        if oracle is None:
            self.lib, self.p = capi.load_product(), "avgpu_"
            self.h = self.lib.avgpu_create(C.byref(cfg), device, ncells)
        else:
            self.lib, self.p = oracle, "orc_"
            self.h = self.lib.orc_create(C.byref(cfg), ncells)
        if not self.h:
            capi.check(self.lib, -1, self.p, "create")     # (a NULL handle: no code of its own)
        self.cfg = cfg
        self.ncells = ncells or cfg.world_x * cfg.world_y
        hid = (C.c_uint8 * len(iset.names))(*iset.handlers)
        red = (C.c_int32 * len(iset.names))(*iset.redundancy)
        self._call("load_instset", self.h, len(iset.names), hid, red)
        self.nres = 0
        if getattr(env, "resources", None):      # resources first: reactions name them
            self.load_resources(env)
        self._call("load_env", self.h, len(env), capi.reactions_array(env))

    def _call(self, name, *args):
        return capi.call(self.lib, self.p, name, *args)

    def close(self):
        if self.h:
            getattr(self.lib, self.p + "destroy")(self.h)
            self.h = None

    def load_resources(self, env):
        self.nres = len(env.resources)
        ra, ca = capi.resources_arrays(env.resources, env.cells)
        self._call("load_resources", self.h, self.nres, ra, len(env.cells), ca)

    def set_orgs(self, first, genomes, merits=None, inputs=None, deterministic=False):
        n = len(genomes)
        buf, lens = capi.pack_genomes(genomes)
        m = (C.c_double * n)(*(merits or [0.0] * n))
        inp = None
        if inputs is not None:
            flat = [v for t in inputs for v in t]
            inp = (C.c_int32 * len(flat))(*flat)
        self._call("set_orgs", self.h, first, n, buf, lens, m, inp, 1 if deterministic else 0)

    def kill(self, cell):
        self._call("kill", self.h, cell)

    def states(self, first, count, cap=capi.MAX_GENOME):
        st = (capi.AvgpuCpuState * count)()
        ops = (C.c_uint8 * (count * cap))()
        fl = (C.c_uint8 * (count * cap))()
        self._call("get_states", self.h, first, count, st, ops, fl, cap)
        return st, bytes(ops), bytes(fl)

    def census(self, first=0, count=None):
        """avgpu_census rows (numpy, capi.CENSUS_DTYPE) of a cell range"""
        return capi.get_census(self.lib, self.p, self.h, first, self.ncells - first if count is None else count)

    def test_genomes(self, genomes, flags_cap=2049, offspring=True):
        """[(result, executed flags, offspring genome)] of the test CPU;
        offspring=False asks for no offspring: [(result, None, None)]"""
        n = len(genomes)
        buf, lens = capi.pack_genomes(genomes)
        res = (capi.AvgpuTestResult * n)()
        flags = C.create_string_buffer(n * flags_cap)
        off = (C.c_uint8 * (n * capi.MAX_GENOME))() if offspring else None
        self._call("test_genomes", self.h, n, buf, lens, res, flags, flags_cap, off)
        if not offspring:
            return [(res[i], None, None) for i in range(n)]
        raw, offb = flags.raw, bytes(off)
        return [(res[i], raw[i * flags_cap:(i + 1) * flags_cap].split(b"\0", 1)[0].decode(),
                 offb[i * capi.MAX_GENOME:i * capi.MAX_GENOME + res[i].offspring_len]) for i in range(n)]

    def resources(self, spatial=False):
        """(levels, per-cell grids or None): avgpu_get_resources"""
        nres, n = self.nres, self.ncells
        lv = (C.c_double * max(1, nres))()
        sp = (C.c_double * max(1, nres * n))() if spatial else None
        self._call("get_resources", self.h, lv, sp)
        grids = [list(sp[r * n:(r + 1) * n]) for r in range(nres)] if spatial else None
        return list(lv[:nres]), grids

    def checkpoint(self, path):
        checkpoint.save(self.lib, self.p, self.h, self.ncells, self.nres, path)

    def restore(self, path):
        return checkpoint.load(self.lib, self.p, self.h, path)

    def run_update(self, serial=False):
        """one update; serial=True: under the reference's own schedule
        (avgpu_run_serial_updates: per-step merit-weighted picks, births at
        once) instead of the batch update"""
        st = capi.AvgpuUpdateStats()
        if serial:
            self._call("run_serial_updates", self.h, 1, C.byref(st))
        else:
            self._call("run_update", self.h, C.byref(st))
        return st
