"""avgpu_landscapes_indel and avgpu_landscape_pairs on the device against the
specification (avida_amd.landscape.spec_indel / spec_pairs over the CPU
oracle; the all-pairs record is tests/golden/landscape/land-pairs-exact.json,
see test_landscape_indel_spec.py).

Integer fields, peak_rank, base_*, peak_fitness, chart entries and site_count
are exact.  Bound on the double sums: every term is >= 0, so any summation
order of N terms is within N * 2^-53 relative of the exact sum, and the
specification's math.fsum is the exact sum rounded once: N * 2^-52 covers
both, N the number of terms of the sum's class (the mutants of the landscape,
or the pairs of one epistasis class).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from avida_amd import capi, files, landscape
import oracle_lib as ol
import parity_util as pu
from test_landscape_spec import SEQ, lineage_rows

pytestmark = pytest.mark.gpu

INSERT, DELETE = landscape.INSERT, landscape.DELETE
INT_FIELDS = ("total_count", "dead_count", "neg_count", "neut_count", "pos_count", "peak_rank",
              "base_gestation", "distance", "genome_length", "num_insts", "gestations", "site_count")
EXACT_DOUBLES = ("base_fitness", "base_merit", "peak_fitness")


def _land(golden, name):
    return os.path.join(golden, "landscape", name)


def _setup(golden, instset):
    iset = files.read_instset(os.path.join(golden, instset))
    env = files.read_environment(os.path.join(golden, "environment-logic9.cfg"))
    cfg = capi.cfg_from_avida(files.read_avida_cfg(None))
    return ol.Backend("oracle", cfg, iset, env, ncells=1), ol.Backend("gpu", cfg, iset, env, ncells=256), iset


@pytest.fixture(scope="module")
def setup(golden):
    orc, gpu, iset = _setup(golden, "instset-classic.cfg")
    yield orc, gpu, iset
    orc.close()
    gpu.close()


@pytest.fixture(scope="module")
def heads(golden):
    orc, gpu, iset = _setup(golden, "instset-heads.cfg")
    yield orc, gpu, iset
    orc.close()
    gpu.close()


@pytest.fixture(scope="module")
def golden_pairs(setup):
    """avgpu_landscape_pairs of the golden genome, once: (rows, epi, chart)"""
    _, gpu, iset = setup
    return landscape.call_pairs(gpu, [iset.parse_sequence(SEQ)])


def check_sum(name, got, exp, count):
    bound = count * 2.0 ** -52
    print(f"{name}: device {got!r} ({got.hex()}) specification {exp!r} "
          f"rel {abs(got - exp) / exp if exp else 0.0:.3g} bound {bound:.3g}")
    assert abs(got - exp) <= bound * abs(exp), name


def check_row(got, exp):
    """a device indel landscape against the specification's"""
    for f in INT_FIELDS + EXACT_DOUBLES:
        assert getattr(got, f) == getattr(exp, f), f
    for f in landscape.Landscape.SUM_FIELDS:
        check_sum(f, getattr(got, f), getattr(exp, f), got.total_count)
    assert (got.total_entropy, got.complexity) == (0.0, 0.0)


def raw(*arrays):
    return tuple(None if a is None else a.tobytes() for a in arrays)


def check_batch(orc, gpu, iset, genomes, kind):
    batch = landscape.full_indel(gpu, genomes, kind)
    for g, got in zip(genomes, batch):
        check_row(got, landscape.spec_indel(orc.test_genomes, g, len(iset.names), kind))
    return batch


def test_golden_indel(setup):
    """1300 insertion mutants of 50 sites, 49 deletion mutants of 48"""
    orc, gpu, iset = setup
    genome = iset.parse_sequence(SEQ)
    ins, = check_batch(orc, gpu, iset, [genome], INSERT)
    assert len(ins.site_count) == 50 and ins.gestations == [1300, 1017, 4]
    assert (ins.distance, ins.peak_rank, ins.peak_fitness) == (1, 1062, 3317.4214876033056)
    ms, mutants, runs = landscape.last_timing(gpu)
    assert (mutants, runs) == (1300, 1300 + 1017 + 4) and ms > 0
    dele, = check_batch(orc, gpu, iset, [genome], DELETE)
    assert len(dele.site_count) == 49 and dele.gestations == [49, 7, 0]
    assert (dele.distance, dele.peak_rank) == (1, -1)
    ms, mutants, runs = landscape.last_timing(gpu)
    assert (mutants, runs) == (49, 49 + 7) and ms > 0


def test_group_boundaries_and_batch(golden, setup):
    """every lineage genome of 47, 48 and 49 sites: mutants of 47 -> 48, 48 -> 49,
    49 -> 48 and 48 -> 47 sites cross the 16-B comparison group and a word; a
    48-site base fills its last group.  One of them alone: the batch's bytes."""
    orc, gpu, iset = setup
    genomes = [iset.parse_sequence(r[20]) for r in lineage_rows(golden) if int(r[2]) in (47, 48, 49)]
    assert sorted((L, sum(1 for g in genomes if len(g) == L)) for L in (47, 48, 49)) == [(47, 8), (48, 17), (49, 26)]
    for kind in (INSERT, DELETE):
        check_batch(orc, gpu, iset, genomes, kind)
        out, sc = landscape.call_indel(gpu, genomes, kind)
        i = next(k for k, g in enumerate(genomes) if len(g) == 48 and k > 0)
        off = sum(len(g) + (kind == INSERT) for g in genomes[:i])
        ln = len(genomes[i]) + (kind == INSERT)
        assert raw(*landscape.call_indel(gpu, [genomes[i]], kind)) == raw(out[i:i + 1], sc[off:off + ln])


def test_chunk_independence(setup):
    """chunk 256: the 1300 insertion mutants cross six chunks, each with survivors"""
    _, gpu, iset = setup
    genome = iset.parse_sequence(SEQ)
    landscape.set_chunk(gpu, 256)
    try:
        small = raw(*landscape.call_indel(gpu, [genome], INSERT))
    finally:
        landscape.set_chunk(gpu, 65536)
    assert raw(*landscape.call_indel(gpu, [genome], INSERT)) == small


def test_class_boundary(golden, heads):
    """insertion mutants of a 320-site genome have 321 sites and leave the
    interpreter's first size class; the deletion mutants of a 321-site genome
    enter it"""
    orc, gpu, iset = heads
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    nop_c = bytes([iset.op_of_name("nop-C")])
    g320 = anc[:50] + nop_c * 220 + anc[50:]
    g321 = anc[:50] + nop_c * 221 + anc[50:]
    assert (len(anc), len(g320), len(g321)) == (100, 320, 321)
    ins, = check_batch(orc, gpu, iset, [g320], INSERT)
    assert ins.total_count == 321 * len(iset.names) == 8346 and ins.base_fitness > 0
    assert min(ins.dead_count, ins.neg_count, ins.neut_count, ins.pos_count) > 0
    assert ins.gestations[2] == 306
    dele, = check_batch(orc, gpu, iset, [g321], DELETE)
    assert dele.total_count == 321 and len(dele.site_count) == 321


def test_pairs_golden(golden, setup, golden_pairs):
    """735 000 pairs against the specification's exact record"""
    _, gpu, iset = setup
    genome = iset.parse_sequence(SEQ)
    rows, epi, chart = golden_pairs
    with open(_land(golden, "land-pairs-exact.json")) as f:
        exp = json.load(f)
    ep = landscape.epistasis_from_row(epi[0])
    for f in landscape.Epistasis.INT_FIELDS:
        assert getattr(ep, f) == exp[f], f
    assert ep.total_epi_count == 735000 and ep.gestations == exp["epi_gestations"]
    for f, n in (("neg_epi_size", ep.neg_epi_count), ("pos_epi_size", ep.pos_epi_count),
                 ("no_epi_size", ep.no_epi_count)):
        check_sum(f, getattr(ep, f), float.fromhex(exp[f]), n)
    ls = landscape.from_row(rows[0], [], chart)
    for f in ("total_count", "dead_count", "neg_count", "neut_count", "pos_count", "peak_rank",
              "base_gestation", "gestations"):
        assert getattr(ls, f) == exp[f], f
    for f in EXACT_DOUBLES:
        assert getattr(ls, f) == float.fromhex(exp[f]), f
    for f in landscape.Landscape.SUM_FIELDS:
        check_sum(f, getattr(ls, f), float.fromhex(exp[f]), ls.total_count)
    assert ls.chart == [[float.fromhex(x) for x in row] for row in exp["chart"]]
    # the one-step half is avgpu_landscapes' distance-1 answer
    o1, _sc, c1 = landscape.call(gpu, [genome], 1)
    assert chart.tobytes() == c1.tobytes()
    for f in capi.LANDSCAPE_DTYPE.names:
        if f not in ("distance", "total_entropy", "complexity"):
            assert rows[0][f].tobytes() == o1[0][f].tobytes(), f
    assert (int(rows[0]["distance"]), float(rows[0]["total_entropy"]), float(rows[0]["complexity"])) == (0, 0.0, 0.0)
    exp_line, = landscape.data_tokens(_land(golden, "land-dump.dat"))
    assert landscape.stats_tokens(ls, dump=True) == exp_line
    ms, mutants, runs = landscape.last_timing(gpu)       # (of the avgpu_landscapes call just made)
    assert (mutants, runs) == (1225, 1225 + 115 + 1)
    assert raw(*landscape.call_pairs(gpu, [genome])) == raw(*golden_pairs)
    ms, mutants, runs = landscape.last_timing(gpu)
    assert mutants == 1225 + 735000 and runs == 1225 + 115 + 1 + sum(ep.gestations) and ms > 0


def test_pairs_zero_base(golden, setup, golden_pairs):
    """a base of fitness 0 stops at ProcessBase: no mutants, an all-zero epi
    row, and the golden genome beside it answers as alone"""
    orc, gpu, iset = setup
    genome = iset.parse_sequence(SEQ)
    ni = len(iset.names)
    dead = next(g for g in (iset.parse_sequence(r[20]) for r in lineage_rows(golden))
                if landscape.colony(orc.test_genomes, [g])[0][0] == 0)
    rows, epi, chart = landscape.call_pairs(gpu, [genome, dead])
    assert raw(rows[:1], epi[:1], chart[:49 * ni]) == raw(*golden_pairs)
    assert epi[1:].tobytes() == bytes(capi.EPISTASIS_DTYPE.itemsize)
    assert not chart[49 * ni:].any()
    ls = landscape.from_row(rows[1], [])
    exp, _ = landscape.spec_pairs(orc.test_genomes, dead, ni)
    for f in INT_FIELDS + EXACT_DOUBLES + landscape.Landscape.SUM_FIELDS + ("total_entropy", "complexity"):
        assert getattr(ls, f) == getattr(exp, f), f
    assert (ls.total_count, ls.gestations, ls.base_fitness, ls.genome_length, ls.num_insts) == \
        (0, [0, 0, 0], 0.0, len(dead), ni)


def test_world_untouched(golden, setup, golden_pairs):
    """an indel call and a pairs call between queued updates leave the world as it was"""
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
        mine = raw(*landscape.call_indel(a, [genome], INSERT))
        assert (a.digests() == d0).all()
        for w in (a, b):
            for _ in range(2):
                w._call("run_update", w.h, None)
        pairs = raw(*landscape.call_pairs(a, [genome]))        # behind the two queued updates
        again = raw(*landscape.call_indel(a, [genome], INSERT))
        sa, sb = a.run_update(), b.run_update()
        assert bytes(sa) == bytes(sb)
        assert (a.digests() == b.digests()).all()
        assert mine == again == raw(*landscape.call_indel(fresh, [genome], INSERT))
        assert pairs == raw(*golden_pairs)
    finally:
        a.close()
        b.close()


def test_refusals(setup):
    """every refusal is AVGPU_EINVAL and leaves the outputs untouched"""
    _, gpu, iset = setup
    lib, h = gpu.lib, gpu.h
    ni = len(iset.names)
    genome = iset.parse_sequence(SEQ)
    long = (genome * 42)[:capi.MAX_GENOME]

    def refused(genomes, lens, n, kind=None):
        """kind None: avgpu_landscape_pairs"""
        blob = b"".join(genomes)
        buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(blob or b"\0")
        la = (C.c_int32 * max(1, len(lens)))(*lens)
        out = np.full(4, 0xAB, dtype=np.uint8).repeat(capi.LANDSCAPE_DTYPE.itemsize)
        epi = np.full(4, 0xCD, dtype=np.uint8).repeat(capi.EPISTASIS_DTYPE.itemsize)
        keep_out, keep_epi = out.copy(), epi.copy()
        sc = np.zeros(8192, dtype=np.int32)
        ch = np.zeros(4096 * capi.MAX_INST, dtype=np.float64)
        lp = la if lens else None
        if kind is None:
            rc = lib.avgpu_landscape_pairs(h, n, buf, lp, out.ctypes.data_as(C.c_void_p),
                                           epi.ctypes.data_as(C.c_void_p), ch.ctypes.data_as(C.POINTER(C.c_double)))
        else:
            rc = lib.avgpu_landscapes_indel(h, n, buf, lp, kind, out.ctypes.data_as(C.c_void_p),
                                            sc.ctypes.data_as(C.POINTER(C.c_int32)))
        assert rc == -1 and lib.avgpu_last_error(), (n, lens, kind)
        assert (out == keep_out).all() and (epi == keep_epi).all() and not sc.any() and not ch.any()

    for kind in (0, 3, -1):
        refused([genome], [49], 1, kind)
    for kind in (INSERT, DELETE, None):
        # what avgpu_landscapes refuses
        for n in (0, -1):
            refused([genome], [49], n, kind)
        refused([genome], [0], 1, kind)
        refused([long + genome[:1]], [capi.MAX_GENOME + 1], 1, kind)
        refused([genome, genome], [49, -3], 2, kind)
        refused([genome[:20] + bytes([ni]) + genome[21:]], [49], 1, kind)
        refused([genome[:20] + bytes([255]) + genome[21:]], [49], 1, kind)
    refused([genome, long], [49, capi.MAX_GENOME], 2, INSERT)      # the mutants would have 2049 sites
    refused([genome, genome[:1]], [49, 1], 2, DELETE)              # no site would be left
    refused([genome, genome[:1]], [49, 1], 2, None)                # no pair of sites
    # the next valid calls still answer
    got, = landscape.full_indel(gpu, [genome], DELETE)
    assert got.total_count == 49
    one, = landscape.full_indel(gpu, [genome[:1]], INSERT)         # a one-site genome has insertion mutants
    assert (one.total_count, one.genome_length, len(one.site_count)) == (2 * ni, 1, 2)
