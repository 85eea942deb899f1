"""Directed tests of the spatial resource step on the device (resources.hip:
k_res_step's windows, row registers, ghost row and lane shifts, res_edge_sum's
sorting network, div_const's guard branches, the boxes, the CELL list, the
fused and the rates path in one update): the GPU world must equal the oracle
world in BITS -- levels and per-cell amounts, signed zeros and all -- after
every one of 5 updates (the double buffer swaps an odd and an even number of
times).

The worlds are EMPTY: no organisms, so nothing but the resource kernels
decides the outcome.  Parameter sets, environments A..D, shapes and the two
seeded grid kinds are res_util's; the oracle itself is held to an independent
specification over the same matrix in test_res_spec.py, which also asserts
that the inputs reach the paths they are there for (each of div_const's three
operand classes, +-0 flows, negative amounts, multiply covered cells).
"""
import os
import subprocess
import sys

import pytest

import res_util as ru

pytestmark = pytest.mark.gpu


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else f"T{v}"


@pytest.mark.parametrize("shape", ru.SHAPES, ids=ru.shape_id)
def test_res_step_equals_oracle(golden, shape):
    """Every environment x grid kind of one shape (why each shape is there:
    res_util.SHAPES)."""
    X, Y = shape
    for which in ru.ENVS:
        for gkind in ru.KINDS:
            want = ru.run_case("oracle", golden, which, gkind, X, Y)
            got = ru.run_case("gpu", golden, which, gkind, X, Y)
            d = ru.first_difference(want, got)
            assert d is None, f"env {which} {gkind}: (update, resource, cell, oracle, gpu) = {d}"


@pytest.mark.parametrize("shape,T", ru.STRIPS, ids=_ids)
def test_res_step_strips_equal_untiled_oracle(golden, shape, T):
    """T strips of 2 rows on one GPU (edge rows exchanged through torch
    buffers) == the untiled oracle, environments A and C, both grid kinds."""
    import torch
    X, Y = shape
    for which in ("A", "C"):
        for gkind in ru.KINDS:
            want = ru.run_case("oracle", golden, which, gkind, X, Y)
            got = ru.run_strips("gpu", golden, which, gkind, X, Y, T, device="cuda",
                                after_update=torch.cuda.synchronize)
            assert ru.strips_difference(ru.make_env(which, X, Y), want, got) is None, (which, gkind)


@pytest.mark.parametrize("shape,T", ru.REFUSED_STRIPS, ids=_ids)
def test_product_refuses_narrow_strips_like_the_oracle(golden, shape, T):
    """2-row strips narrower than 128 columns: refused on both sides."""
    eo = ru.strips_refused("oracle", golden, *shape, T)
    eg = ru.strips_refused("gpu", golden, *shape, T)
    assert eo is not None and eg is not None, (eo, eg)


@pytest.mark.parametrize("band", [1, 3])
def test_band_size_knob(golden, band):
    """AVGPU_RES_ROWS (rows a wave walks down; read once per process): one
    fresh child process -- it opens the GPU itself -- steps environment A with
    both grid kinds on (64, 11) and (3, 3) and prints every update's bits."""
    env = dict(os.environ, AVGPU_RES_ROWS=str(band))
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "res_util.py")],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l.split() for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == len(ru.BAND_SHAPES) * len(ru.KINDS)
    it = iter(lines)
    for X, Y in ru.BAND_SHAPES:
        for gkind in ru.KINDS:
            line = next(it)
            assert line[:3] == [str(X), str(Y), gkind]
            want = [w for lv, gr in ru.run_case("oracle", golden, "A", gkind, X, Y) for w in lv + [v for g in gr for v in g]]
            got = [int(w, 16) for w in line[3:]]
            assert len(got) == len(want)
            bad = [i for i in range(len(want)) if want[i] != got[i]]
            assert not bad, (X, Y, gkind, bad[:3], "%016x %016x" % (want[bad[0]], got[bad[0]]))


def test_tiny_amounts_take_the_full_division(golden):
    """Environment A on one shape with every amount at 2^-1074 .. 2^-1010:
    div_const's quotients below 2^-900, where only the full division rounds
    correctly, decide every cell of the gravity-only resource (what makes this
    case bite: test_res_spec.py::test_tiny_amounts_inputs)."""
    X, Y = ru.TINY_SHAPE
    d = ru.first_difference(ru.run_case("oracle", golden, "A", "tiny", X, Y),
                            ru.run_case("gpu", golden, "A", "tiny", X, Y))
    assert d is None, f"(update, resource, cell, oracle, gpu) = {d}"
