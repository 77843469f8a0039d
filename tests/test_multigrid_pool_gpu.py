"""The V-cycle pressure solve added to the claim of tests/test_pool_contents_gpu.py: no result depends on what pooled device memory held. The hierarchy's memory -- the
coarse grids' tables, the masks, the child / parent tables, every level's p and right-hand side -- comes from the pool; option arena_fill (tests/pool_cases.py) makes every
block arrive filled with 0x00, 0xFF or 0x7F. Under EACH fill the pressure must equal the numpy mirror (tests/mg_cases.py) in every word, before and after a regrid that
drops the hierarchy, and so the three fills give the same bytes."""
import functools

import numpy as np
import pytest

import diag_cases as dc
import hnanosolver_amd as H
import mg_cases as mg
import special_cases as sc
from frame_cases import make_sim
from pool_cases import under_every_fill

pytestmark = pytest.mark.gpu

F = np.float32
DX = mg.DX


@pytest.fixture(autouse=True)
def restore_options():
    yield
    for k in ("arena_fill", "sor_block_lb"):
        H.set_option(k, None)


@functools.lru_cache(maxsize=None)
def references(variant):
    """the mirror's results, computed once and shared by the three fills"""
    pre, post, max_levels = variant
    o = np.ascontiguousarray(mg.ragged_deep(), dtype=np.int32)
    div = mg.divergence_for(o)
    want = mg.Mirror(o, pre, post, 8, max_levels, 1.0).solve(div, DX, 2)
    st = {"vel": np.random.default_rng(6).standard_normal((len(o) * 512, 3)).astype(F)}
    return o, div, want, st


@pytest.mark.parametrize("variant", [(2, 2, 0), (0, 2, 0), (1, 1, 2)], ids=["V22", "V02", "V11_two_levels"])
def test_vcycle_does_not_depend_on_pooled_memory(variant):
    pre, post, max_levels = variant
    o, div, want, st = references(variant)
    after = {}

    def scenario():
        g, s = make_sim(o, [], st, None, DX)  # (sim, grid tables and hierarchy all drawn under the fill)
        s.solve_method(1, pre, post, 8, max_levels, 1.0)
        dc.set_divergence(s, div)
        s.pressure_solve(2, DX)
        p = dc.pressure_of(s)
        assert dc.words(p) == dc.words(want), f"before the regrid: {sc.describe(p, want)}"
        g2 = s.regrid(2)  # a new arena, new grid tables, and the next solve builds a new hierarchy into what the pool hands out
        o2 = g2.coords()[::512].copy()
        if "div" not in after:
            after["div"] = mg.divergence_for(o2, seed=9)
            after["want"] = mg.Mirror(o2, pre, post, 8, max_levels, 1.0).solve(after["div"], DX, 2)
        dc.set_divergence(s, after["div"])
        s.pressure_solve(2, DX)
        p2 = dc.pressure_of(s)
        assert dc.words(p2) == dc.words(after["want"]), f"after the regrid: {sc.describe(p2, after['want'])}"
        out = {"p": p, "p after regrid": p2, "levels": s.solve_levels(), "residual": s.residual(DX)}
        s.close()
        return out

    under_every_fill(scenario)
