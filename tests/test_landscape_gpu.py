"""avgpu_landscapes on the device against the specification
(avida_amd.landscape.spec over the CPU oracle) and the reference's golden
landscape files (tests/golden/landscape/, see test_landscape_spec.py).

Bound on the double sums: every term is >= 0, so any summation order of N
terms is within N * 2^-53 relative of the exact sum, and the specification's
math.fsum is the exact sum rounded once: N * 2^-52 covers both.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from avida_amd import capi, files, landscape
import oracle_lib as ol
import parity_util as pu
from test_landscape_spec import SEQ, exact_of, lineage_rows

pytestmark = pytest.mark.gpu

INT_FIELDS = ("total_count", "dead_count", "neg_count", "neut_count", "pos_count", "peak_rank",
              "base_gestation", "distance", "genome_length", "num_insts", "gestations", "site_count")
EXACT_DOUBLES = ("base_fitness", "base_merit", "peak_fitness")


def _land(golden, name):
    return os.path.join(golden, "landscape", name)


@pytest.fixture(scope="module")
def setup(golden):
    iset = files.read_instset(os.path.join(golden, "instset-classic.cfg"))
    env = files.read_environment(os.path.join(golden, "environment-logic9.cfg"))
    cfg = capi.cfg_from_avida(files.read_avida_cfg(None))
    orc = ol.Backend("oracle", cfg, iset, env, ncells=1)
    gpu = ol.Backend("gpu", cfg, iset, env, ncells=256)
    yield orc, gpu, iset
    orc.close()
    gpu.close()


@pytest.fixture(scope="module")
def spec1(setup):
    orc, _, iset = setup
    return landscape.spec(orc.test_genomes, iset.parse_sequence(SEQ), len(iset.names), 1)


def check_row(got, exp):
    """a device landscape against the specification's"""
    for f in INT_FIELDS:
        assert getattr(got, f) == getattr(exp, f), f
    for f in EXACT_DOUBLES:                       # one organism's value each
        assert getattr(got, f) == getattr(exp, f), f
    check_sums(got, {f: getattr(exp, f) for f in landscape.Landscape.SUM_FIELDS})
    # the entropy is a function of site_count alone
    assert (got.total_entropy, got.complexity) == landscape.entropy(exp.site_count, exp.num_insts)


def check_sums(got, exp):
    bound = got.total_count * 2.0 ** -52
    for f, e in exp.items():
        g = getattr(got, f)
        print(f"{f}: device {g!r} ({g.hex()}) specification {e!r} rel {abs(g - e) / e if e else 0.0:.3g} bound {bound:.3g}")
        assert abs(g - e) <= bound * abs(e), f


def raw(out, sc, ch):
    return out.tobytes(), sc.tobytes(), None if ch is None else ch.tobytes()


def test_one_step_golden(golden, setup, spec1, tmp_path):
    """1225 mutants: 19 full waves and 9 lanes"""
    _, gpu, iset = setup
    genome = iset.parse_sequence(SEQ)
    got, = landscape.full(gpu, [genome], 1)
    check_row(got, spec1)
    assert got.gestations == [1225, 115, 1]
    assert got.chart == spec1.chart               # bit-exact: each entry is one organism's fitness
    landscape.write_stats(got, tmp_path / "land.dat")
    assert landscape.data_tokens(tmp_path / "land.dat") == landscape.data_tokens(_land(golden, "land-1step.dat"))
    landscape.write_stats(got, tmp_path / "dump.dat", dump=True)
    assert landscape.data_tokens(tmp_path / "dump.dat") == landscape.data_tokens(_land(golden, "land-dump.dat"))
    landscape.write_dump(got, genome, tmp_path / "org.land")
    assert landscape.data_tokens(tmp_path / "org.land") == landscape.data_tokens(_land(golden, "org-Seq1.land"))
    ms, mutants, runs = landscape.last_timing(gpu)
    assert (mutants, runs) == (1225, 1225 + 115 + 1) and ms > 0


def test_chunk_independence(setup):
    """chunk 256: the 1225 mutants cross five chunks, each with survivors"""
    _, gpu, iset = setup
    genome = iset.parse_sequence(SEQ)
    landscape.set_chunk(gpu, 256)
    try:
        small = raw(*landscape.call(gpu, [genome], 1))
    finally:
        landscape.set_chunk(gpu, 65536)
    assert raw(*landscape.call(gpu, [genome], 1)) == small


def test_batch_lineage(golden, setup):
    """the 90 lineage genomes (lengths 46-56, two bases of fitness 0) in one call"""
    orc, gpu, iset = setup
    rows = lineage_rows(golden)
    genomes = [iset.parse_sequence(r[20]) for r in rows]
    out, sc, ch = landscape.call(gpu, genomes, 1)
    batch = landscape.full(gpu, genomes, 1)
    off = 0
    for i, (row, g, got) in enumerate(zip(rows, genomes, batch)):
        check_row(got, landscape.spec(orc.test_genomes, g, len(iset.names), 1))
        assert landscape.lineage_columns(got) == row[15:20], row[0]
        o1, s1, c1 = landscape.call(gpu, [g], 1)             # the same genome alone
        ni = len(iset.names)
        assert raw(o1, s1, c1) == raw(out[i:i + 1], sc[off:off + len(g)], ch[off * ni:(off + len(g)) * ni]), row[0]
        off += len(g)
    assert sum(1 for b in batch if b.base_fitness == 0) == 2


def test_two_step_golden(golden, setup, tmp_path):
    """735 000 mutants against land-2step.dat and the specification's exact record"""
    _, gpu, iset = setup
    genome = iset.parse_sequence(SEQ)
    first = landscape.call(gpu, [genome], 2)
    got = landscape.from_row(first[0][0], first[1])
    with open(_land(golden, "land-2step-exact.json")) as f:
        exp = json.load(f)
    assert got.gestations == [735000, 98545, 983]
    have = exact_of(got)
    for f in ("total_count", "dead_count", "neg_count", "neut_count", "pos_count", "peak_rank",
              "base_gestation", "gestations", "site_count") + EXACT_DOUBLES:
        assert have[f] == exp[f], f
    check_sums(got, {f: float.fromhex(exp[f]) for f in landscape.Landscape.SUM_FIELDS})
    landscape.write_stats(got, tmp_path / "land.dat")
    assert landscape.data_tokens(tmp_path / "land.dat") == landscape.data_tokens(_land(golden, "land-2step.dat"))
    assert raw(*landscape.call(gpu, [genome], 2)) == raw(*first)


def test_world_untouched(golden, setup, spec1):
    """a landscape call between queued updates leaves the world as it was"""
    _, fresh, iset = setup
    ov = {"WORLD_X": 16, "WORLD_Y": 16}
    _, env, cfg = pu.load_env(golden, "instset-classic.cfg", ov, seed=17)
    genome = iset.parse_sequence(SEQ)
    a = ol.Backend("gpu", cfg, iset, env, ncells=256)
    b = ol.Backend("gpu", cfg, iset, env, ncells=256)
    try:
        for w in (a, b):
            w.set_orgs(0, [genome] * 256, deterministic=False)
            for _ in range(3):
                w._call("run_update", w.h, None)              # queued: no statistics, no sync
        d0 = a.digests()
        mine = raw(*landscape.call(a, [genome], 1))
        assert (a.digests() == d0).all()
        for w in (a, b):
            for _ in range(2):
                w._call("run_update", w.h, None)
        again = raw(*landscape.call(a, [genome], 1))           # behind the two queued updates
        sa, sb = a.run_update(), b.run_update()
        assert bytes(sa) == bytes(sb)
        assert (a.digests() == b.digests()).all()
        assert mine == again == raw(*landscape.call(fresh, [genome], 1))
        assert landscape.from_row(np.frombuffer(mine[0], dtype=capi.LANDSCAPE_DTYPE)[0],
                                  np.frombuffer(mine[1], dtype=np.int32)).site_count == spec1.site_count
    finally:
        a.close()
        b.close()


def test_refusals(setup):
    """every refusal is AVGPU_EINVAL and leaves `out` untouched"""
    _, gpu, iset = setup
    lib, h = gpu.lib, gpu.h
    ni = len(iset.names)
    genome = iset.parse_sequence(SEQ)

    def refused(genomes, lens, n, distance, chart=False):
        blob = b"".join(genomes)
        buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(blob or b"\0")
        la = (C.c_int32 * max(1, len(lens)))(*lens)
        out = np.full(4, 0xAB, dtype=np.uint8).repeat(capi.LANDSCAPE_DTYPE.itemsize)
        keep = out.copy()
        sc = np.zeros(4096, dtype=np.int32)
        ch = np.zeros(4096 * capi.MAX_INST, dtype=np.float64) if chart else None
        rc = lib.avgpu_landscapes(h, n, buf, la, distance, out.ctypes.data_as(C.c_void_p),
                                  sc.ctypes.data_as(C.POINTER(C.c_int32)),
                                  ch.ctypes.data_as(C.POINTER(C.c_double)) if chart else None)
        assert rc == -1 and lib.avgpu_last_error(), (n, distance, chart)
        assert (out == keep).all() and not sc.any()

    for d in (0, 3, -1):
        refused([genome], [49], 1, d)
    refused([genome], [49], 1, 2, chart=True)
    for n in (0, -1):
        refused([genome], [49], n, 1)
    refused([genome], [0], 1, 1)
    refused([genome + genome * 41], [capi.MAX_GENOME + 1], 1, 1)
    refused([genome, genome], [49, -3], 2, 1)
    refused([genome[:20] + bytes([ni]) + genome[21:]], [49], 1, 1)
    refused([genome[:20] + bytes([255]) + genome[21:]], [49], 1, 2)
    for cells in (0, -256, 100, 300, 65536 + 64):
        assert lib.avgpu_set_landscape_chunk(h, cells) == -1
    # the chunk is as it was: the default still answers
    got, = landscape.full(gpu, [genome], 1)
    assert got.total_count == 1225
