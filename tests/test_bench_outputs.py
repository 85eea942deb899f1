"""bench.py --dump-outputs: the arrays it writes (bench.dump_outputs) and, on
the GPU, a plain run of the benchmark itself -- its line, its number of timed
steps and its outputs against the same world run in this process."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from avida_amd import capi, files
import oracle_lib as ol
import parity_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"stats": np.float64, "cells": np.float64, "merit": np.float64, "fitness": np.float64,
         "census": np.float32, "state_cells": np.float64, "states": np.float64,
         "tape_ops": np.float32, "tape_flags": np.float32}


def _load(d, suffix=""):
    assert sorted(os.listdir(d)) == sorted(f"{k}{suffix}.npy" for k in NAMES)
    out = {k: np.load(os.path.join(d, f"{k}{suffix}.npy")) for k in NAMES}
    for k, a in out.items():
        assert a.dtype == NAMES[k], (k, a.dtype)
    assert sum(a.nbytes for a in out.values()) <= 64e6
    return out


def test_dump_outputs_of_an_oracle_world(golden, tmp_path):
    iset, env, cfg = pu.load_env(golden, seed=101)
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    n = cfg.world_x * cfg.world_y
    b = ol.Backend("oracle", cfg, iset, env, ncells=n)
    b.set_orgs(n // 2, [anc], deterministic=False)
    for _ in range(30):
        st = b.run_update()
    assert st.num_organisms > 1
    for k in ("a", "b"):
        bench.dump_outputs(b.lib, capi, b.h, n, str(tmp_path / k), prefix="orc_")
    a, a2 = _load(tmp_path / "a"), _load(tmp_path / "b")
    for k in NAMES:                                   # the sample is fixed
        assert np.array_equal(a[k], a2[k]), k
    names = bench.STATS_INT_FIELDS + bench.STATS_F64_FIELDS
    assert a["stats"][names.index("update")] == st.update
    assert a["stats"][names.index("num_organisms")] == st.num_organisms
    assert a["stats"][names.index("cum_births")] == st.cum_births
    assert a["stats"][names.index("sum_merit")] == st.sum_merit
    assert np.array_equal(a["cells"], np.arange(n))
    census = capi.get_census(b.lib, "orc_", b.h, 0, n)
    assert np.array_equal(a["merit"], census["merit"])
    assert np.array_equal(a["fitness"], census["fitness"])
    assert a["census"].shape == (n, len(bench.CENSUS_INT_FIELDS))
    assert np.array_equal(a["census"][:, 0], census["genome_length"])
    assert int((a["census"][:, 0] > 0).sum()) == st.num_organisms
    # state records and tapes of whole runs of cells, as get_states returns them
    ids = a["state_cells"].astype(np.int64)
    assert len(ids) == bench.DUMP_BLOCKS * bench.DUMP_BLOCK_CELLS == len(set(ids.tolist()))
    assert a["tape_ops"].shape == a["tape_flags"].shape == (len(ids), capi.MAX_GENOME)
    s, ops, _ = b.states(int(ids[0]), bench.DUMP_BLOCK_CELLS)
    assert np.array_equal(a["states"][:bench.DUMP_BLOCK_CELLS],
                          np.array([bench._state_row(x) for x in s]))
    assert np.array_equal(a["tape_ops"][:bench.DUMP_BLOCK_CELLS].astype(np.uint8).tobytes(), ops)
    b.close()


def test_dump_outputs_samples_a_large_world(golden, tmp_path, monkeypatch):
    """more cells than DUMP_CELLS: a fixed seeded sample of that many"""
    monkeypatch.setattr(bench, "DUMP_CELLS", 500)
    iset, env, cfg = pu.load_env(golden, seed=101)
    anc = files.read_org(os.path.join(golden, "default-heads.org"), iset)
    n = cfg.world_x * cfg.world_y
    b = ol.Backend("oracle", cfg, iset, env, ncells=n)
    b.set_orgs(0, [anc] * n, deterministic=False)
    b.run_update()
    bench.dump_outputs(b.lib, capi, b.h, n, str(tmp_path), suffix=".rank1", prefix="orc_")
    a = _load(tmp_path, ".rank1")
    cells = a["cells"].astype(np.int64)
    assert len(cells) == 500 == len(a["merit"]) == len(a["census"])
    assert np.all(np.diff(cells) > 0) and cells[-1] < n
    assert np.array_equal(a["merit"], capi.get_census(b.lib, "orc_", b.h, 0, n)["merit"][cells])
    b.close()


SIDE, BURN, WARM, STEPS = 64, 20, 2, 3


@pytest.mark.gpu
def test_plain_bench_run_line_and_outputs(golden, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` in a process of
    its own: the line of a plain run, K timed steps, and outputs equal to the
    same world run burn-in + W + K updates here."""
    out = tmp_path / "run"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARM), "--side", str(SIDE), "--burn-in", str(BURN),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "organism-instructions/s"
    assert line["higher_is_better"] is True and line["dtype"] == "int32"
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (STEPS, WARM, 1)
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["value"] == pytest.approx(line["config"]["insts_per_update"] / (line["ms_per_step"] * 1e-3))
    assert line["full"] is False
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["config"]["long_run"] is None
    got = _load(out)

    lib = capi.load_product()
    h, cfg, n, _ = bench.build_world(lib, capi, files, golden, SIDE, 101, 0, 0, 1)
    for _ in range(BURN + WARM + STEPS):
        capi.check(lib, lib.avgpu_run_update(h, None))
    bench.dump_outputs(lib, capi, h, n, str(tmp_path / "here"))
    lib.avgpu_destroy(h)
    want = _load(tmp_path / "here")
    assert want["stats"][0] == BURN + WARM + STEPS - 1    # stats[0]: the last update's number, from 0
    for k in NAMES:
        assert np.array_equal(got[k], want[k]), k
