"""ctypes mirror of include/avida_gpu.h (structures + the product library loader).

The product library is ``avida_amd/libavida_gpu.so`` (built in-tree by
``__graft_entry__.build()`` / ``avida_amd/build.py``).  There is no fallback:
if the library or a GPU is missing, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

MAX_REACTIONS = 16
MAX_GENOME = 2048
STACK_SIZE = 10
MAX_LABEL = 10

MODE_WORLD, MODE_TEST, MODE_FROZEN = 0, 1, 2
# enum avgpu_counter (tests/test_capi.py holds the two lists together)
CNT_CB0, CNT_CASE0 = 32, 38
(CNT_INSTS, CNT_DEATHS, CNT_DIVIDES, CNT_BIRTHS, CNT_DROPPED, CNT_SPILLS, CNT_SLICES,
 CNT_LANESTEPS, CNT_C0_SLICES, CNT_C0_SITES, CNT_CLK_STAGE, CNT_CLK_LOOP, CNT_CLK_WB,
 CNT_ITERS, CNT_IT_FAST, CNT_IT_COPY, CNT_IT_SLOW, CNT_WAVES, CNT_HALO_SENT,
 CNT_HALO_LOST, CNT_REC_EXHAUSTED, CNT_OVERSIZE, CNT_SUB_OVERFLOW, CNT_MEM_CAP,
 CNT_OVERWRITTEN, CNT_CANCELLED, CNT_BAD_RECORD, CNT_WASTED, CNT_STEPS) = range(29)
RNG_COUNTER, RNG_RECORDED = 0, 1
NUM_COUNTERS = 48

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libavida_gpu.so")


class AvgpuCfg(C.Structure):
    _fields_ = [
        ("world_x", C.c_int32), ("world_y", C.c_int32), ("world_geometry", C.c_int32),
        ("ave_time_slice", C.c_int32), ("slicing_method", C.c_int32),
        ("base_merit_method", C.c_int32), ("base_const_merit", C.c_int32),
        ("default_bonus", C.c_double),
        ("copy_mut_prob", C.c_double), ("copy_ins_prob", C.c_double), ("copy_del_prob", C.c_double),
        ("divide_mut_prob", C.c_double), ("divide_ins_prob", C.c_double),
        ("divide_del_prob", C.c_double),
        ("offspring_size_range", C.c_double), ("min_copied_lines", C.c_double),
        ("min_exe_lines", C.c_double),
        ("require_allocate", C.c_int32), ("death_method", C.c_int32), ("age_limit", C.c_int32),
        ("alloc_method", C.c_int32), ("divide_method", C.c_int32),
        ("max_label_exe_size", C.c_int32), ("birth_method", C.c_int32),
        ("prefer_empty", C.c_int32), ("allow_parent", C.c_int32),
        ("test_cpu_time_mod", C.c_int32), ("min_genome_size", C.c_int32),
        ("max_genome_size", C.c_int32), ("inherit_merit", C.c_int32),
        ("merit_default_bonus", C.c_double), ("required_bonus", C.c_double),
        ("seed", C.c_uint64),
        ("divide_slip_prob", C.c_double), ("divide_uniform_prob", C.c_double),
        ("slip_fill_mode", C.c_int32), ("sub_updates", C.c_int32),
        ("div_mut_prob", C.c_double), ("parent_mut_prob", C.c_double),
        ("divide_poisson_slip_mean", C.c_double), ("divide_poisson_mut_mean", C.c_double),
        ("divide_poisson_ins_mean", C.c_double), ("divide_poisson_del_mean", C.c_double),
        ("div_ins_prob", C.c_double), ("div_del_prob", C.c_double),
        ("div_uniform_prob", C.c_double), ("div_slip_prob", C.c_double),
        ("divide_trans_prob", C.c_double), ("divide_poisson_trans_mean", C.c_double),
        ("div_trans_prob", C.c_double),
        ("copy_uniform_prob", C.c_double), ("copy_slip_prob", C.c_double),
        ("slip_copy_mode", C.c_int32), ("trans_fill_mode", C.c_int32),
        ("parent_ins_prob", C.c_double), ("parent_del_prob", C.c_double),
        # knobs the library refuses away from their defaults (avgpu_create)
        ("point_mut_prob", C.c_double), ("point_ins_prob", C.c_double),
        ("point_del_prob", C.c_double), ("inst_point_mut_prob", C.c_double),
        ("div_lgt_prob", C.c_double), ("divide_lgt_prob", C.c_double),
        ("divide_poisson_lgt_mean", C.c_double),
        ("inject_mut_prob", C.c_double), ("inject_ins_prob", C.c_double),
        ("inject_del_prob", C.c_double),
        ("meta_copy_mut", C.c_double), ("meta_std_dev", C.c_double), ("death_prob", C.c_double),
        ("age_deviation", C.c_int32), ("divide_failure_resets", C.c_int32),
        ("special_mut_line", C.c_int32), ("population_cap", C.c_int32),
        ("generation_inc_method", C.c_int32), ("reset_inputs_on_divide", C.c_int32),
        ("epigenetic_method", C.c_int32), ("min_cycles", C.c_int32),
        ("required_task", C.c_int32), ("immunity_task", C.c_int32),
        ("required_reaction", C.c_int32), ("immunity_reaction", C.c_int32),
        ("require_single_reaction", C.c_int32), ("max_unique_task_count", C.c_int32),
        ("require_exact_copy", C.c_int32), ("fitness_method", C.c_int32),
        ("juv_period", C.c_int32), ("no_mut_insts_len", C.c_int32),
        ("test_fitness_measures", C.c_int32), ("pad_cfg2", C.c_int32),
        ("no_mut_insts", C.c_char * 64),
    ]


class AvgpuReaction(C.Structure):
    _fields_ = [
        ("task", C.c_int32), ("type", C.c_int32), ("value", C.c_double),
        ("max_number", C.c_double), ("min_count", C.c_int32), ("max_count", C.c_int32),
        ("has_requisite", C.c_int32), ("resource", C.c_int32),
        ("min_number", C.c_double), ("max_fraction", C.c_double),
        ("depletable", C.c_int32), ("pad", C.c_int32),
    ]


class AvgpuResource(C.Structure):
    _fields_ = [
        ("geometry", C.c_int32), ("pad", C.c_int32),
        ("initial", C.c_double), ("inflow", C.c_double), ("outflow", C.c_double),
        ("inflow_x1", C.c_int32), ("inflow_x2", C.c_int32), ("inflow_y1", C.c_int32),
        ("inflow_y2", C.c_int32), ("outflow_x1", C.c_int32), ("outflow_x2", C.c_int32),
        ("outflow_y1", C.c_int32), ("outflow_y2", C.c_int32),
        ("xdiffuse", C.c_double), ("ydiffuse", C.c_double), ("xgravity", C.c_double),
        ("ygravity", C.c_double),
    ]


class AvgpuCellResource(C.Structure):
    _fields_ = [("resource", C.c_int32), ("cell", C.c_int32), ("initial", C.c_double),
                ("inflow", C.c_double), ("outflow", C.c_double)]


class AvgpuCpuState(C.Structure):
    _fields_ = [
        ("reg", C.c_int32 * 3), ("head", C.c_int32 * 4),
        ("stack", (C.c_int32 * STACK_SIZE) * 2), ("stack_ptr", C.c_int32 * 2),
        ("cur_stack", C.c_int32), ("read_label_len", C.c_int32),
        ("read_label", C.c_int8 * MAX_LABEL), ("pad0", C.c_int16),
        ("mal_active", C.c_int32), ("mem_size", C.c_int32),
        ("cpu_cycles_used", C.c_int32), ("time_used", C.c_int32),
        ("gestation_start", C.c_int32), ("gestation_time", C.c_int32),
        ("num_divides", C.c_int32), ("generation", C.c_int32), ("alive", C.c_int32),
        ("genome_length", C.c_int32), ("copied_size", C.c_int32),
        ("child_copied_size", C.c_int32), ("executed_size", C.c_int32),
        ("max_executed", C.c_int32), ("birth_length", C.c_int32), ("input_ptr", C.c_int32),
        ("input_buf", C.c_int32 * 3), ("input_total", C.c_int32),
        ("output_buf", C.c_int32), ("output_total", C.c_int32), ("inputs", C.c_int32 * 3),
        ("cur_task_count", C.c_int32 * MAX_REACTIONS),
        ("last_task_count", C.c_int32 * MAX_REACTIONS),
        ("cur_reaction_count", C.c_int32 * MAX_REACTIONS),
        ("rng_counter", C.c_uint32), ("rng_key_lo", C.c_uint32), ("rng_key_hi", C.c_uint32),
        ("errors", C.c_int32), ("head_start", C.c_uint32), ("age", C.c_int32), ("pad1", C.c_int32),
        ("cur_bonus", C.c_double), ("merit", C.c_double), ("fitness", C.c_double),
        ("credit", C.c_double),
    ]


class AvgpuTestResult(C.Structure):
    _fields_ = [
        ("divided", C.c_int32), ("copy_true", C.c_int32), ("copied_size", C.c_int32),
        ("executed_size", C.c_int32), ("gestation_time", C.c_int32),
        ("offspring_len", C.c_int32), ("genome_length", C.c_int32), ("time_used", C.c_int32),
        ("merit", C.c_double), ("fitness", C.c_double),
        ("task_count", C.c_int32 * MAX_REACTIONS),
    ]


class AvgpuSerialState(C.Structure):
    """avgpu_serial_state (include/avida_gpu.h): the serial world's stream
    positions, reaper queue length and whether it has started"""
    _fields_ = [("sched_pos", C.c_int64), ("ctx_pos", C.c_int64), ("reaper_len", C.c_int64),
                ("started", C.c_int32), ("pad_", C.c_int32)]


class AvgpuUpdateStats(C.Structure):
    _fields_ = [
        ("update", C.c_int64), ("num_organisms", C.c_int64), ("insts_executed", C.c_int64),
        ("births", C.c_int64), ("births_dropped", C.c_int64), ("deaths", C.c_int64),
        ("divides", C.c_int64), ("task_orgs", C.c_int64 * MAX_REACTIONS),
        ("sum_merit", C.c_double), ("sum_fitness", C.c_double), ("sum_gestation", C.c_double),
        ("sum_genome_length", C.c_double), ("max_fitness", C.c_double),
        ("ave_generation", C.c_double), ("sum_mem_size", C.c_double),
        ("cum_insts_executed", C.c_int64), ("cum_births", C.c_int64), ("slices", C.c_int64),
        ("lane_steps", C.c_int64), ("births_overwritten", C.c_int64), ("births_cancelled", C.c_int64),
        ("seed", C.c_uint64), ("sched_pred", C.c_int64), ("sched_pred_n", C.c_int64), ("sub_steps", C.c_int64),
        ("sched_carry", C.c_int64), ("insts_wasted", C.c_int64), ("sched_pred_cnt", C.c_int64),
        ("sched_pred_bins", C.c_int64 * 4),
    ]


# avgpu_census (include/avida_gpu.h), read straight into numpy
CENSUS_DTYPE = np.dtype([("genotype_key", "<u8"), ("merit", "<f8"), ("fitness", "<f8"),
                         ("genome_length", "<i4"), ("gestation_time", "<i4"), ("copied_size", "<i4"),
                         ("executed_size", "<i4"), ("generation", "<i4"), ("num_divides", "<i4")])
assert CENSUS_DTYPE.itemsize == 48


def get_census(lib, prefix, handle, first, count):
    """Census rows (CENSUS_DTYPE) of cells first .. first+count-1 through
    {prefix}get_census (avgpu_ = the product, orc_ = the oracle)."""
    out = np.zeros(count, dtype=CENSUS_DTYPE)
    call(lib, prefix, "get_census", handle, first, count, out.ctypes.data_as(C.c_void_p))
    return out


# avgpu_genotype (include/avida_gpu.h): one row per genotype, keys ascending
GENOTYPE_DTYPE = np.dtype([("genotype_key", "<u8"), ("first_cell", "<i8"), ("num_units", "<i4"),
                           ("genome_length", "<i4"), ("num_gestated", "<i4"), ("reserved", "<i4"),
                           ("sum_merit", "<f8"), ("sum_fitness", "<f8"), ("sum_repro_rate", "<f8"),
                           ("max_fitness", "<f8"), ("sum_gestation", "<i8"), ("sum_copied", "<i8")])
assert GENOTYPE_DTYPE.itemsize == 80


class GENOTYPE_TOTALS(C.Structure):
    """avgpu_genotype_totals"""
    _fields_ = [("num_organisms", C.c_int64), ("num_genotypes", C.c_int64),
                ("sum_copied_size", C.c_int64), ("sum_executed_size", C.c_int64)]


def get_genotypes(lib, handle):
    """(table, totals) of a product world through avgpu_get_genotypes: the
    table (GENOTYPE_DTYPE, keys ascending) sized to the world's genotypes.
    The buffer starts at 1024 rows and keeps the largest size seen per
    library; a table that has outgrown it costs one more grouping."""
    totals = GENOTYPE_TOTALS()
    cap = getattr(lib, "_genotype_cap", 1024)
    while True:
        out = np.empty(cap, dtype=GENOTYPE_DTYPE)
        rc = lib.avgpu_get_genotypes(handle, out.ctypes.data_as(C.c_void_p), cap, C.byref(totals))
        if rc >= 0:
            return out[:rc], totals
        if rc != -1 or totals.num_genotypes <= cap:      # not the "cap too small" refusal
            check(lib, rc, name="get_genotypes")
        cap = lib._genotype_cap = int(totals.num_genotypes) + int(totals.num_genotypes) // 4 + 16


# avgpu_arbiter_row (include/avida_gpu.h): one row per active genotype, keys
# ascending; row j describes row j of the genotype table
ARBITER_ROW_DTYPE = np.dtype([("genotype_key", "<u8"), ("id", "<i8"), ("update_born", "<i8"),
                              ("total_units", "<i8"), ("num_units", "<i4"), ("genome_length", "<i4"),
                              ("name_no", "<i4"), ("threshold", "<i4")])
assert ARBITER_ROW_DTYPE.itemsize == 48
# avgpu_arbiter_summary: what one classification returns
ARBITER_SUMMARY_DTYPE = np.dtype([("update", "<i8"), ("num_organisms", "<i8"), ("num_genotypes", "<i8"),
                                  ("num_threshold", "<i8"), ("tot_genotypes", "<i8"), ("tot_threshold", "<i8"),
                                  ("next_id", "<i8"), ("num_new", "<i8"), ("num_gone", "<i8"),
                                  ("num_crossed", "<i8"), ("sum_copied_size", "<i8"),
                                  ("sum_executed_size", "<i8"), ("dominant_row", "<i8"),
                                  ("dominant_state", ARBITER_ROW_DTYPE), ("dominant", GENOTYPE_DTYPE)])
assert ARBITER_SUMMARY_DTYPE.itemsize == 232


# one genotype of the lineage store (the ancestry
# Systematics::Genotype keeps, systematics/Genotype.cc:139-176): rows ascending
# by id, parent_id 0 = injected, -1 = orphan; seq_off the birth genome's offset
# in the store's arena (16-B aligned canonical codes), -1 = not captured;
# update_deactivated -1 while the genotype is active
LINEAGE_ROW_DTYPE = np.dtype([("genotype_key", "<u8"), ("id", "<i8"), ("parent_id", "<i8"), ("seq_off", "<i8"),
                              ("update_born", "<i8"), ("update_deactivated", "<i8"), ("depth", "<i4"),
                              ("genome_length", "<i4"), ("gen_born", "<i4"), ("reserved", "<i4")])
assert LINEAGE_ROW_DTYPE.itemsize == 64
LINEAGE_SUMMARY_DTYPE = np.dtype([("rows", "<i8"), ("active_rows", "<i8"), ("arena_bytes", "<i8"),
                                  ("num_orphans", "<i8"), ("num_unsequenced", "<i8"), ("max_depth", "<i8"),
                                  ("dropped_last_prune", "<i8"), ("reserved", "<i8")])
assert LINEAGE_SUMMARY_DTYPE.itemsize == 64


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def enable_lineage(lib, handle, on=True, rows_hint=0, arena_hint=0):
    """avgpu_enable_lineage: the lineage store beside the device arbiter"""
    call(lib, "avgpu_", "enable_lineage", handle, int(bool(on)), int(rows_hint), int(arena_hint))


def get_lineage(lib, handle, summary_only=False):
    """(rows, arena bytes, summary) of the store through avgpu_get_lineage"""
    s = np.zeros(1, dtype=LINEAGE_SUMMARY_DTYPE)
    call(lib, "avgpu_", "get_lineage", handle, None, 0, None, 0, _vp(s))
    if summary_only:
        return None, None, s[0]
    rows = np.zeros(int(s[0]["rows"]), dtype=LINEAGE_ROW_DTYPE)
    arena = np.zeros(max(1, int(s[0]["arena_bytes"])), dtype=np.uint8)
    call(lib, "avgpu_", "get_lineage", handle, _vp(rows), len(rows), _vp(arena), len(arena), None)
    return rows, arena[:int(s[0]["arena_bytes"])], s[0]


def set_lineage(lib, handle, rows, arena, summary):
    rows = np.ascontiguousarray(rows, dtype=LINEAGE_ROW_DTYPE)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    s = np.array([summary], dtype=LINEAGE_SUMMARY_DTYPE)
    call(lib, "avgpu_", "set_lineage", handle, len(rows), _vp(rows) if len(rows) else None,
         _vp(arena) if len(arena) else None, len(arena), _vp(s))


def prune_lineage(lib, handle):
    s = np.zeros(1, dtype=LINEAGE_SUMMARY_DTYPE)
    call(lib, "avgpu_", "prune_lineage", handle, _vp(s))
    return s[0]


def classify_genotypes(lib, handle, update, threshold):
    """One classification on the device (avgpu_classify_genotypes): its
    summary, one ARBITER_SUMMARY_DTYPE record"""
    out = np.zeros(1, dtype=ARBITER_SUMMARY_DTYPE)
    call(lib, "avgpu_", "classify_genotypes", handle, int(update), int(threshold), _vp(out))
    return out[0]


def get_arbiter(lib, handle, rows_hint=0):
    """(rows, table, summary, sz_count) of the last classification through
    avgpu_get_arbiter: ARBITER_ROW_DTYPE and GENOTYPE_DTYPE rows, keys
    ascending, the summary record and the AVGPU_MAX_GENOME + 1 name counters"""
    summary = np.zeros(1, dtype=ARBITER_SUMMARY_DTYPE)
    sz = np.zeros(MAX_GENOME + 1, dtype=np.int64)
    call(lib, "avgpu_", "get_arbiter", handle, None, None, 0, _vp(summary), _vp(sz))
    m = int(summary[0]["num_genotypes"])
    rows = np.zeros(m, dtype=ARBITER_ROW_DTYPE)
    table = np.zeros(m, dtype=GENOTYPE_DTYPE)
    if m:
        rc = call(lib, "avgpu_", "get_arbiter", handle, _vp(rows), _vp(table), m, None, None)
        assert rc == m
    return rows, table, summary[0], sz


def set_arbiter(lib, handle, rows, summary, sz_count):
    """Install an arbiter state (avgpu_set_arbiter): resume or hand-over"""
    rows = np.ascontiguousarray(rows, dtype=ARBITER_ROW_DTYPE)
    summary = np.ascontiguousarray(np.asarray(summary, dtype=ARBITER_SUMMARY_DTYPE).reshape(1))
    sz = None if sz_count is None else np.ascontiguousarray(sz_count, dtype=np.int64)
    if sz is not None and len(sz) != MAX_GENOME + 1:
        raise ValueError("sz_count holds AVGPU_MAX_GENOME + 1 counters")
    call(lib, "avgpu_", "set_arbiter", handle, len(rows), _vp(rows), _vp(summary), _vp(sz))


def live_objects(lib):
    """Device buffers, pinned buffers, events and streams the library owns now (avgpu_live_objects)"""
    return int(lib.avgpu_live_objects())


# avgpu_landscape (include/avida_gpu.h): one row per base genome
MAX_INST = 64
LANDSCAPE_DTYPE = np.dtype([("total_count", "<i8"), ("dead_count", "<i8"), ("neg_count", "<i8"),
                            ("neut_count", "<i8"), ("pos_count", "<i8"), ("gestations", "<i8", (3,)),
                            ("peak_rank", "<i8"), ("base_fitness", "<f8"), ("base_merit", "<f8"),
                            ("peak_fitness", "<f8"), ("total_fitness", "<f8"), ("total_sqr_fitness", "<f8"),
                            ("pos_size", "<f8"), ("neg_size", "<f8"), ("total_entropy", "<f8"),
                            ("complexity", "<f8"), ("base_gestation", "<i4"), ("distance", "<i4"),
                            ("genome_length", "<i4"), ("num_insts", "<i4")])
assert LANDSCAPE_DTYPE.itemsize == 160
# avgpu_indel_kind, avgpu_epistasis (cLandscape::TestAllPairs' accumulators)
LAND_INSERT, LAND_DELETE = 1, 2
EPISTASIS_DTYPE = np.dtype([("total_epi_count", "<i8"), ("dead_epi_count", "<i8"), ("neg_epi_count", "<i8"),
                            ("pos_epi_count", "<i8"), ("no_epi_count", "<i8"), ("gestations", "<i8", (3,)),
                            ("neg_epi_size", "<f8"), ("pos_epi_size", "<f8"), ("no_epi_size", "<f8")])
assert EPISTASIS_DTYPE.itemsize == 88


# avida.cfg knobs outside avgpu_cfg's implemented set travel in its refused
# block (include/avida_gpu.h): the library itself refuses any of them set away
# from the reference default (avgpu_create -> AVGPU_EUNSUPPORTED), so the
# Python driver and a C++ caller are refused alike.  (cfg key, field, default,
# kind) -- main/cAvidaConfig.h:309-420, :525-537, :546-559.
REFUSED_KNOBS = [
    ("POINT_MUT_PROB", "point_mut_prob", 0.0, float), ("POINT_INS_PROB", "point_ins_prob", 0.0, float),
    ("POINT_DEL_PROB", "point_del_prob", 0.0, float),
    ("INST_POINT_MUT_PROB", "inst_point_mut_prob", 0.0, float),
    ("DIV_LGT_PROB", "div_lgt_prob", 0.0, float), ("DIVIDE_LGT_PROB", "divide_lgt_prob", 0.0, float),
    ("DIVIDE_POISSON_LGT_MEAN", "divide_poisson_lgt_mean", 0.0, float),
    ("INJECT_MUT_PROB", "inject_mut_prob", 0.0, float), ("INJECT_INS_PROB", "inject_ins_prob", 0.0, float),
    ("INJECT_DEL_PROB", "inject_del_prob", 0.0, float),
    ("META_COPY_MUT", "meta_copy_mut", 0.0, float), ("META_STD_DEV", "meta_std_dev", 0.0, float),
    ("DEATH_PROB", "death_prob", 0.0, float),
    ("AGE_DEVIATION", "age_deviation", 0, int), ("DIVIDE_FAILURE_RESETS", "divide_failure_resets", 0, int),
    ("SPECIAL_MUT_LINE", "special_mut_line", -1, int), ("POPULATION_CAP", "population_cap", 0, int),
    ("GENERATION_INC_METHOD", "generation_inc_method", 1, int),
    ("RESET_INPUTS_ON_DIVIDE", "reset_inputs_on_divide", 0, int),
    ("EPIGENETIC_METHOD", "epigenetic_method", 0, int), ("MIN_CYCLES", "min_cycles", 0, int),
    ("REQUIRED_TASK", "required_task", -1, int), ("IMMUNITY_TASK", "immunity_task", -1, int),
    ("REQUIRED_REACTION", "required_reaction", -1, int), ("IMMUNITY_REACTION", "immunity_reaction", -1, int),
    ("REQUIRE_SINGLE_REACTION", "require_single_reaction", 0, int),
    ("MAX_UNIQUE_TASK_COUNT", "max_unique_task_count", -1, int),
    ("REQUIRE_EXACT_COPY", "require_exact_copy", 0, int), ("FITNESS_METHOD", "fitness_method", 0, int),
    ("JUV_PERIOD", "juv_period", 0, int),
]
# Divide_TestFitnessMeasures1 (cpu/cHardwareBase.cc:978-1085) runs a test CPU
# on every offspring when any of these is set: avgpu_cfg.test_fitness_measures
TEST_FITNESS_KNOBS = ["REVERT_FATAL", "REVERT_DETRIMENTAL", "REVERT_NEUTRAL", "REVERT_BENEFICIAL",
                      "REVERT_TASKLOSS", "REVERT_EQUALS", "STERILIZE_FATAL", "STERILIZE_DETRIMENTAL",
                      "STERILIZE_NEUTRAL", "STERILIZE_BENEFICIAL", "STERILIZE_TASKLOSS",
                      "STERILIZE_UNSTABLE", "FAIL_IMPLICIT"]
# Knobs accepted without effect, with the reason.  SPECULATIVE only decides
# whether the reference's serial ProcessStep pre-executes up to 32 more
# instructions of the picked organism (main/cPopulation.cc:5740-5788); the
# batched update has no serial interleaving to speculate on.
IGNORED = {"SPECULATIVE": "batched update: no serial schedule to speculate on"}


def _num(v, kind, default):
    try:
        return kind(float(v))
    except (TypeError, ValueError):
        return default


def cfg_from_avida(cfg, seed=None) -> AvgpuCfg:
    """Fill an AvgpuCfg from a files.AvidaConfig.  Every knob of the path is a
    field; the library refuses (avgpu_create) what it does not implement."""
    g = cfg.get
    c = AvgpuCfg()
    c.world_x, c.world_y = g("WORLD_X"), g("WORLD_Y")
    c.world_geometry = g("WORLD_GEOMETRY")
    c.ave_time_slice = g("AVE_TIME_SLICE")
    c.slicing_method = g("SLICING_METHOD")
    c.base_merit_method = g("BASE_MERIT_METHOD")
    c.base_const_merit = g("BASE_CONST_MERIT")
    c.default_bonus = g("DEFAULT_BONUS")
    c.copy_mut_prob = g("COPY_MUT_PROB")
    c.copy_ins_prob = g("COPY_INS_PROB")
    c.copy_del_prob = g("COPY_DEL_PROB")
    c.divide_mut_prob = g("DIVIDE_MUT_PROB")
    c.divide_ins_prob = g("DIVIDE_INS_PROB")
    c.divide_del_prob = g("DIVIDE_DEL_PROB")
    c.offspring_size_range = g("OFFSPRING_SIZE_RANGE")
    c.min_copied_lines = g("MIN_COPIED_LINES")
    c.min_exe_lines = g("MIN_EXE_LINES")
    c.require_allocate = g("REQUIRE_ALLOCATE")
    c.death_method = g("DEATH_METHOD")
    c.age_limit = g("AGE_LIMIT")
    c.alloc_method = g("ALLOC_METHOD")
    c.divide_method = g("DIVIDE_METHOD")
    c.max_label_exe_size = g("MAX_LABEL_EXE_SIZE")
    c.birth_method = g("BIRTH_METHOD")
    c.prefer_empty = g("PREFER_EMPTY")
    c.allow_parent = g("ALLOW_PARENT")
    c.test_cpu_time_mod = g("TEST_CPU_TIME_MOD")
    c.min_genome_size = g("MIN_GENOME_SIZE")
    c.max_genome_size = g("MAX_GENOME_SIZE")
    c.inherit_merit = g("INHERIT_MERIT")
    c.merit_default_bonus = g("MERIT_DEFAULT_BONUS")
    c.required_bonus = g("REQUIRED_BONUS")
    s = g("RANDOM_SEED") if seed is None else seed
    c.seed = int(s) & 0xFFFFFFFFFFFFFFFF if int(s) >= 0 else 0x1234ABCD
    f = lambda k, d=0.0: _num(g(k, d), float, d)   # noqa: E731
    i = lambda k, d=0: _num(g(k, d), int, d)       # noqa: E731
    c.divide_slip_prob = f("DIVIDE_SLIP_PROB")
    c.divide_uniform_prob = f("DIVIDE_UNIFORM_PROB")
    c.slip_fill_mode = i("SLIP_FILL_MODE")
    c.div_mut_prob = f("DIV_MUT_PROB")
    c.parent_mut_prob = f("PARENT_MUT_PROB")
    c.divide_poisson_slip_mean = f("DIVIDE_POISSON_SLIP_MEAN")
    c.divide_poisson_mut_mean = f("DIVIDE_POISSON_MUT_MEAN")
    c.divide_poisson_ins_mean = f("DIVIDE_POISSON_INS_MEAN")
    c.divide_poisson_del_mean = f("DIVIDE_POISSON_DEL_MEAN")
    c.div_ins_prob = f("DIV_INS_PROB")
    c.div_del_prob = f("DIV_DEL_PROB")
    c.div_uniform_prob = f("DIV_UNIFORM_PROB")
    c.div_slip_prob = f("DIV_SLIP_PROB")
    c.divide_trans_prob = f("DIVIDE_TRANS_PROB")
    c.divide_poisson_trans_mean = f("DIVIDE_POISSON_TRANS_MEAN")
    c.div_trans_prob = f("DIV_TRANS_PROB")
    c.copy_uniform_prob = f("COPY_UNIFORM_PROB")
    c.copy_slip_prob = f("COPY_SLIP_PROB")
    c.slip_copy_mode = i("SLIP_COPY_MODE")
    c.trans_fill_mode = i("TRANS_FILL_MODE")
    c.parent_ins_prob = f("PARENT_INS_PROB")
    c.parent_del_prob = f("PARENT_DEL_PROB")
    for key, field, default, kind in REFUSED_KNOBS:
        setattr(c, field, _num(g(key, default), kind, default))
    nmi = g("NO_MUT_INSTS", "")
    nmi = str(nmi).strip() if nmi not in (None, 0) else ""
    c.no_mut_insts_len = len(nmi)
    c.no_mut_insts = nmi.encode()[:63]
    c.test_fitness_measures = int(any(_num(g(k, 0), float, 1.0) != 0.0 for k in TEST_FITNESS_KNOBS))
    return c


def reactions_array(reactions):
    arr = (AvgpuReaction * max(1, len(reactions)))()
    for i, r in enumerate(reactions):
        arr[i].task, arr[i].type, arr[i].value = r.task, r.proc_type, r.value
        arr[i].max_number, arr[i].min_count = r.max_number, r.min_count
        arr[i].max_count, arr[i].has_requisite = r.max_count, r.has_requisite
        arr[i].resource = getattr(r, "resource", 0)   # 1 + index, 0 = infinite
        arr[i].min_number = getattr(r, "min_number", 0.0)
        arr[i].max_fraction = getattr(r, "max_fraction", 1.0)
        arr[i].depletable = getattr(r, "depletable", 1)
    return arr


def resources_arrays(resources, cells):
    """files.Resource / files.CellResource lists -> ctypes arrays"""
    ra = (AvgpuResource * max(1, len(resources)))()
    for i, r in enumerate(resources):
        for f, _ in AvgpuResource._fields_:
            if f != "pad":
                setattr(ra[i], f, getattr(r, f))
    ca = (AvgpuCellResource * max(1, len(cells)))()
    for i, c in enumerate(cells):
        ca[i].resource, ca[i].cell = c.resource, c.cell
        ca[i].initial, ca[i].inflow, ca[i].outflow = c.initial, c.inflow, c.outflow
    return ra, ca


def pack_genomes(genomes):
    """(uint8 buffer, int32 lens): genomes (op-code byte strings) back to back
    as the C-ABI takes them; the buffer is never empty"""
    blob = b"".join(bytes(g) for g in genomes)
    return ((C.c_uint8 * max(1, len(blob))).from_buffer_copy(blob or b"\0"),
            (C.c_int32 * len(genomes))(*[len(g) for g in genomes]))


V, I, I32, I64, U64, D = C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_double
U8P, I32P, I64P, DP = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
CFGP, STATSP, SERIALP = C.POINTER(AvgpuCfg), C.POINTER(AvgpuUpdateStats), C.POINTER(AvgpuSerialState)
STATEP = C.POINTER(AvgpuCpuState)
# Every function of include/avida_gpu.h (tests/test_capi.py holds the two
# together): name without its prefix -> (restype, argtypes, does the oracle
# have it as orc_<name>?)
SIGNATURES = {
    "last_error": (C.c_char_p, [], True),
    "cfg_defaults": (None, [CFGP], False),
    "create": (V, [CFGP, I, I64], False),        # (orc_create takes no device: tests/oracle_lib.py)
    "check_cfg": (I, [CFGP], False),
    "destroy": (I, [V], True),
    "sync": (I, [V], False),
    "load_instset": (I, [V, I, U8P, I32P], True),
    "load_env": (I, [V, I, C.POINTER(AvgpuReaction)], True),
    "load_resources": (I, [V, I, C.POINTER(AvgpuResource), I, C.POINTER(AvgpuCellResource)], True),
    "set_resources": (I, [V, DP, DP], True),
    "get_resources": (I, [V, DP, DP], True),
    "set_org": (I, [V, I64, U8P, I, D, I32P], False),
    "set_orgs": (I, [V, I64, I64, U8P, I32P, DP, I32P, I], True),
    "kill": (I, [V, I64], True),
    "step": (I, [V, I64, I64, I32P, I32, I], True),
    "run_update": (I, [V, STATSP], True),
    "run_updates": (I, [V, I, STATSP], True),
    "run_serial_updates": (I, [V, I, STATSP], True),
    "set_serial_streams": (I, [V, V, I64, V, I64], True),
    "get_serial_state": (I, [V, SERIALP, V, V, V, V, I64], True),
    "set_serial_state": (I, [V, SERIALP, V, V, V, V], True),
    "update_totals": (I, [V, V], False),
    "update_run": (I, [V, V, STATSP], False),
    "set_stream": (I, [V, V], False),
    "set_rng_mode": (I, [V, I, V, I64, V], True),
    "get_states": (I, [V, I64, I64, STATEP, U8P, U8P, I], True),
    "set_states": (I, [V, I64, I64, STATEP, U8P, U8P, I], True),
    "set_clock": (I, [V, STATSP], True),
    "get_census": (I, [V, I64, I64, V], True),
    "set_genotype_keys": (I, [V, I64, I64, V], True),
    "state_digests": (I, [V, I64, I64, V], True),
    "test_genomes": (I, [V, I, U8P, I32P, C.POINTER(AvgpuTestResult), C.c_char_p, I, U8P], True),
    "get_stats": (I, [V, STATSP], True),
    "stats_vector": (I, [V, C.POINTER(V)], False),
    "set_global_totals": (I, [V, D, I64], True),
    "last_step_insts": (I, [V, I64P], True),
    "last_kernel_ms": (I, [V, DP, I64P], False),
    "kernel_times": (I, [V, DP, I64P], False),
    "set_timing": (I, [V, I], False),
    "counters": (I, [V, I, I64P, I], False),
    "live_objects": (I64, [], False),
    # strip tiles (include/avida_gpu.h "strip tiles")
    "set_tile": (I, [V, I64, I64], True),
    "tile_buffer_bytes": (I, [V, I64P, I64P, I64P], True),
    "set_tile_buffers": (I, [V] * 9, True),
    "tile_partials": (I, [V, V], True),
    "tile_begin": (I, [V, V, I], True),
    "tile_steps": (I, [V, V, I, C.POINTER(I)], True),
    "tile_begin_step": (I, [V, V, I, I, I], True),
    "tile_place": (I, [V, I, I], True),
    "tile_finish": (I, [V, STATSP], True),
    "tile_res_bytes": (I, [V, I64P], True),
    "set_tile_res_buffers": (I, [V] * 5, True),
    "tile_res_cons": (I, [V, V], True),
    "tile_res_settle": (I, [V, V], True),
    # the genotype table, the device-resident arbiter, ancestry and the lineage
    # store: the oracle has the census
    "get_genotypes": (I, [V, V, I64, C.POINTER(GENOTYPE_TOTALS)], False),
    "last_genotypes_ms": (I, [V, DP, I64P], False),
    "classify_genotypes": (I, [V, I64, I32, V], False),
    "get_arbiter": (I, [V, V, V, I64, V, V], False),
    "set_arbiter": (I, [V, I64, V, V, V], False),
    "reset_arbiter": (I, [V], False),
    "last_arbiter_ms": (I, [V, DP, I64P], False),
    "get_parent_keys": (I, [V, I64, I64, V], False),
    "set_parent_keys": (I, [V, I64, I64, V], False),
    "enable_lineage": (I, [V, I, I64, I64], False),
    "get_lineage": (I, [V, V, I64, V, I64, V], False),
    "set_lineage": (I, [V, I64, V, V, I64, V], False),
    "prune_lineage": (I, [V, V], False),
    "last_lineage_ms": (I, [V, DP, DP], False),
    # mutational landscapes, genetic distances, population events: the oracle
    # runs the specifications of landscape.py, distance.py and popevents.py
    "landscapes": (I, [V, I, U8P, I32P, I, V, I32P, DP], False),
    "landscapes_indel": (I, [V, I, U8P, I32P, I, V, I32P], False),
    "landscape_pairs": (I, [V, I, U8P, I32P, V, V, DP], False),
    "set_landscape_chunk": (I, [V, I64], False),
    "last_landscape_ms": (I, [V, DP, I64P, I64P], False),
    "genome_distances": (I, [V, I, U8P, I32P, I64, I32P, I32P, I32P, I32P], False),
    "cell_distances": (I, [V, I64, I64, U8P, I32, I32P, I32P], False),
    "site_histogram": (I, [V, I64, I64, I32P, I64P], False),
    "last_distance_ms": (I, [V, DP, I64P, I64P], False),
    "kill_cells": (I, [V, V, I64, I64P], False),
    "kill_prob": (I, [V, D, U64, I64P], False),
    "kill_rect": (I, [V, I, I, I, I, I64P], False),
    "kill_genotypes": (I, [V, V, I64, D, U64, I64P], False),
    "keep_sample": (I, [V, I64, U64, I64P], False),
    "last_event_ms": (I, [V, DP, I64P], False),
}
EXPORTED = ["avgpu_" + name for name in SIGNATURES]


def bind(lib, prefix, signatures, strict=False):
    """Declare restype and argtypes of {prefix}{name} for every entry of
    `signatures`.  A symbol the library lacks is an error when `strict`, else
    it is skipped (the oracle, an older diagnostic build)."""
    for name, (res, args, *_) in signatures.items():
        fn = getattr(lib, prefix + name) if strict else getattr(lib, prefix + name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def bind_common(lib, prefix):
    """Declare the functions shared by the product and the oracle."""
    return bind(lib, prefix, {n: s for n, s in SIGNATURES.items() if s[2]})


_lib = None


def lib_build_hash(path=None):
    """the first 16 hex digits of the SHA-256 of the library file: which
    build a measurement (profiles/pmc_k_interpret320.json) belongs to"""
    import hashlib
    with open(path or LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def load_product(path=None):
    """Load the in-tree HIP library; raise if it is missing (no fallback).
    `path` selects a diagnostic build (tools/phase_clocks.py); it is not
    cached, and like one named by AVGPU_DIAG_LIB it may be an earlier build
    without the newer functions (tools/gpu/ab_var.sh measures such builds)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    p = path or os.environ.get("AVGPU_DIAG_LIB") or LIB_PATH   # diagnostic builds (tools/)
    if not os.path.exists(p):
        raise RuntimeError(f"{p} missing: run __graft_entry__.build() first")
    lib = bind(C.CDLL(p), "avgpu_", SIGNATURES, strict=p == LIB_PATH)
    if path is None:
        _lib = lib
    return lib


def check(lib, rc, prefix="avgpu_", name="call failed"):
    """the one failure path: rc < 0 raises with the library's last_error"""
    if rc is not None and rc < 0:
        msg = getattr(lib, prefix + "last_error")()
        raise RuntimeError(f"{prefix}{name} ({rc}): {msg.decode() if msg else ''}")
    return rc


def call(lib, prefix, name, *args):
    """{prefix}{name}(*args) through check"""
    return check(lib, getattr(lib, prefix + name)(*args), prefix, name)
