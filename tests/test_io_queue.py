"""The interpreter's queued IO task checks (interp_core.h, IOQ): in the simple
environment without finite resources an IO does at once only what the organism
sees and queues its task check, up to QUEUE_DEPTH per lane; the wave evaluates
the queues together when a lane's is full, before a divide of a lane that has
events, and at the slice's end.  Worlds whose slices hold more IOs than a
queue, whose divides follow IOs of the same slice and in which the order of
the events matters, GPU against the oracle:
every cell's state record, tape and the update's statistics, after every
update."""
import os

import numpy as np
import pytest

from avida_amd import capi, files
import oracle_lib as ol
import parity_util as pu

CAP = capi.MAX_GENOME
QUEUE_DEPTH = 3            # interp_core.h: IOQ_FULL
STAT_FIELDS = ("num_organisms", "insts_executed", "births", "deaths", "divides", "births_dropped",
               "births_overwritten", "births_cancelled", "cum_insts_executed", "cum_births", "slices")


def _seeded(golden, side):
    """the bench's seeding: the detail-50000.pop genotypes with their recorded
    merits, dealt to the cells by a fixed hash of the cell id"""
    iset = files.read_instset(os.path.join(golden, "instset-classic.cfg"))
    pool = []
    for g in files.read_pop(os.path.join(golden, "detail-50000.pop")):
        pool.extend([(iset.parse_sequence(g.sequence), g.merit)] * g.num_cpus)
    n = side * side
    picks = [pool[(c * 2654435761) % len(pool)] for c in range(n)]
    return iset, [g for g, _ in picks], [m for _, m in picks]


def make_world(golden, kind, side, seed, slice_len=None, requisites=None, sub_updates=0, rec_per=0):
    iset, genomes, merits = _seeded(golden, side)
    env = files.read_environment(os.path.join(golden, "environment-logic9.cfg"))
    for r in env:
        if requisites == "once":   # requisite:max_count=1 on every reaction
            r.has_requisite, r.min_count, r.max_count = 1, 0, 1
        elif requisites == "none":
            r.has_requisite, r.min_count, r.max_count = 0, 0, files.INT32_MAX
    ov = {"WORLD_X": side, "WORLD_Y": side}
    if slice_len:
        ov["AVE_TIME_SLICE"] = slice_len
    cfg = capi.cfg_from_avida(files.read_avida_cfg(None, ov), seed=seed)
    cfg.sub_updates = sub_updates
    n = side * side
    b = ol.Backend(kind, cfg, iset, env, ncells=n)
    b.set_orgs(0, genomes, merits, deterministic=False)
    if rec_per:                    # every seeded organism draws from its own recorded segment
        stream = np.random.default_rng(seed).random(n * rec_per)
        b.set_rng_mode(capi.RNG_RECORDED, stream, np.arange(n, dtype=np.int64) * rec_per)
    return b


def queue_evidence(prev, now):
    """From two consecutive ends of updates of one world run in one batch step
    per update (an organism that lives through the update runs one slice):
    (organisms that did more than QUEUE_DEPTH IOs in the slice, organisms that
    divided in it after a rewarded IO of the same slice -- the task counts the
    divide filed as the last gestation's exceed those at the slice's start).
    The second shows a divide that followed IOs of its slice, not that their
    events were still queued when it came."""
    deep = after_io = 0
    for p, q in zip(prev, now):
        if p.birth_length == 0 or not p.alive or not q.alive:
            continue
        if (p.rng_key_lo, p.rng_key_hi) != (q.rng_key_lo, q.rng_key_hi):
            continue               # replaced by a newborn
        if q.output_total - p.output_total > QUEUE_DEPTH:
            deep += 1
        if q.num_divides > p.num_divides and any(
                q.last_task_count[t] > p.cur_task_count[t] for t in range(9)):
            after_io += 1
    return deep, after_io


def path_evidence(prev, now):
    """From two consecutive ends of updates of the oracle's world: (organisms
    that ran from a list class -- more than 320 sites at the update's start --
    and did an IO, newborns that did an IO in the update of their birth, i.e.
    in the newborn pass)"""
    listed = nb_io = 0
    for p, q in zip(prev, now):
        same = (p.rng_key_lo, p.rng_key_hi) == (q.rng_key_lo, q.rng_key_hi)
        if same and p.alive:
            listed += p.mem_size > 320 and q.output_total > p.output_total
        elif not same and q.alive and q.output_total > 0:
            nb_io += 1
    return listed, nb_io


def run_pair(golden, side, seed, updates, evidence=False, **kw):
    """runs oracle and GPU side by side; returns the oracle's evidence sums
    (evidence: "queue" or "paths") and the GPU's cumulative counters"""
    orc = make_world(golden, "oracle", side, seed, **kw)
    gpu = make_world(golden, "gpu", side, seed, **kw)
    n = side * side
    ev = [0, 0, 0]
    births = 0
    prev = orc.states(0, n, CAP)[0] if evidence else None
    for upd in range(updates):
        so, sg = orc.run_update(), gpu.run_update()
        for f in STAT_FIELDS:
            assert getattr(so, f) == getattr(sg, f), (upd, f, getattr(so, f), getattr(sg, f))
        assert list(so.task_orgs) == list(sg.task_orgs), upd
        a, oa, fa = orc.states(0, n, CAP)
        b, ob, fb = gpu.states(0, n, CAP)
        nbad, report = pu.diff_states_np(a, b, oa, ob, fa, fb, CAP)
        assert nbad == 0, (upd, nbad, report[:5])
        births += so.births
        if evidence:
            got = queue_evidence(prev, a) if evidence == "queue" else path_evidence(prev, a)
            ev = [x + y for x, y in zip(ev, got)] + ev[len(got):]
            prev = a
    c = gpu.counters(cumulative=1)
    assert c[capi.CNT_BAD_RECORD] == 0
    if kw.get("rec_per"):
        assert c[capi.CNT_REC_EXHAUSTED] == 0 and orc.lib.orc_rec_exhausted() == 0
    orc.close()
    gpu.close()
    return ev, births, c


LONG = dict(side=16, seed=41, updates=20, slice_len=400, sub_updates=1)


@pytest.mark.gpu
def test_long_slices_fill_the_queues(golden):
    """16 x 16, AVE_TIME_SLICE about a gestation, one batch step per update:
    slices hold more IOs than the queue does and divides follow rewarded IOs
    of their own slice (whether events were still queued at the divide depends
    on the wave's other lanes) -- shown from the oracle's own states."""
    (deep, after_io, _), births, _ = run_pair(golden, evidence="queue", **LONG)
    assert deep > 0 and after_io > 0 and births > 0, (deep, after_io, births)


@pytest.mark.gpu
def test_once_only_requisites(golden):
    """a like world with requisite:max_count=1 set on every reaction (the once
    mask of the simple environment): a task pays once per gestation, so the
    order in which queued events are evaluated decides the bonus"""
    kw = dict(LONG, seed=47, slice_len=600, requisites="once")
    (deep, after_io, _), births, _ = run_pair(golden, evidence="queue", **kw)
    assert deep > 0 and after_io > 0 and births > 0, (deep, after_io, births)
    # the requisites bite in this world: without them it ends elsewhere
    kw.pop("updates")
    ends = []
    for req in ("once", "none"):
        w = make_world(golden, "oracle", **dict(kw, requisites=req))
        for _ in range(LONG["updates"]):
            w.run_update()
        ends.append(w.digests())
        w.close()
    assert (ends[0] != ends[1]).any()


@pytest.mark.gpu
def test_default_slices(golden):
    """32 x 32 at the default AVE_TIME_SLICE and adaptive batch steps: the
    newborn pass and the list classes with queues in play -- both shown to
    occur from the oracle's states.  (Spills are rare in this population; the
    spill continuation of these kernels runs, with CNT_SPILLS asserted, in
    test_rng_modes.py::test_copy_mutations_world_gpu.)"""
    (listed, nb_io, _), births, _ = run_pair(golden, side=32, seed=43, updates=60, evidence="paths")
    assert births > 100 and listed > 0 and nb_io > 0, (births, listed, nb_io)


@pytest.mark.gpu
def test_long_slices_recorded_streams(golden):
    """the long-slice world with every seeded organism on a recorded stream
    (the interpreter's REC instantiation)"""
    (deep, after_io, _), births, _ = run_pair(golden, evidence="queue", rec_per=4000, **LONG)
    assert deep > 0 and after_io > 0 and births > 0, (deep, after_io, births)
