"""Points rasterised into fields do not depend on what pooled device memory held: the accumulator of a radial sum and of an average, drawn fresh from a pool that hands
out 0x00, 0xFF (NaN words, -1 as an int64) or 0x7F (3.39e38) bytes, gives the same bytes -- the bytes of the host mirror. As tests/test_splat_gpu.py does for the sum."""
import numpy as np
import pytest

import rasterize_cases as rc
import splat_cases as sp
from pool_cases import assert_fills_agree, run_under_fills
from test_rasterize_gpu import rig

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ("ragged32", "dense32"))
def test_rasterised_bytes_do_not_depend_on_the_pool(name):
    R, (_, vel, phi, xyz, vals, vvals, _, radii) = rig(name), rc.case(name)
    half = len(xyz) // 2
    want_a = rc.mirror(R.grid, [phi[0]], xyz[:half], [vals[0][:half]], kernel="radial", mode="add", radius=1.0)[0]
    want_b = rc.mirror(R.grid, [want_a[0], phi[1], vel], xyz[half:], [vals[1][half:], vals[2][half:], vvals[half:]], kernel="radial", mode="average", radius=4.0, min_weight=0.25)[0]
    want_c = rc.mirror(R.grid, [want_b[0]], xyz, [vals[3]], kernel="trilinear", mode="average")[0]

    def scenario():
        """a fresh accumulator of one channel, grown to four by an average of five components (two passes), then used again by an average of one"""
        R.grid.release_cache()
        a, _, _ = R.splat([phi[0]], xyz[:half], [vals[0][:half]], kernel="radial", mode="add", radius=1.0)
        b, status, _ = R.splat([a[0], phi[1], vel], xyz[half:], [vals[1][half:], vals[2][half:], vvals[half:]], kernel="radial", mode="average", radius=4.0, min_weight=0.25)
        c, _, _ = R.splat([b[0]], xyz, [vals[3]], kernel="trilinear", mode="average")
        assert sp.same_bytes(a[0], want_a[0]) and all(sp.same_bytes(x, y) for x, y in zip(b, want_b)) and sp.same_bytes(c[0], want_c[0])
        return {"a": a[0], "b0": b[0], "b1": b[1], "b2": b[2], "c": c[0], "status": status}

    assert_fills_agree(run_under_fills(scenario, (0x00, 0xFF, 0x7F)))
    R.grid.release_cache()
