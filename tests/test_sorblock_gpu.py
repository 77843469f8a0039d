"""Temporally blocked red-black SOR (hnanosolver_amd/csrc/hns_sorblock.hip: K iterations per launch on a block of leaves with a
2K-voxel halo) against the oracle's restatement of redBlackGaussSeidelUpdate (reference src/Cuda/Kernel.cu:591-623, two launches
per iteration) and against the library's own two-launch form: bit for bit, on dense, ragged and scattered leaf sets with negative
coordinates, for even and odd iteration counts, warm-started and from zero."""
import numpy as np
import pytest
import torch

import hnanosolver_amd as H
from hnanosolver_amd import api, device as D, fields
from oracle_lib import OracleGrid
from sor_cases import range_sweep

pytestmark = pytest.mark.gpu

SHAPES = [1, 2]  # block edge in leaves: one-leaf blocks (k_rbgs_block<1, K>: four iterations per launch up to 300 leaves, two beyond) and 16^3 blocks (k_rbgs_block_xy), each forced on every leaf set


def leaf_sets():
    rng = np.random.default_rng(5)
    o = np.unique(rng.integers(-6, 6, size=(400, 3)).astype(np.int32) * 8, axis=0)
    scatter = np.ascontiguousarray(o[fields.nanovdb_order(o)])
    # straddles the 128^3 lower-node and 4096^3 upper-node borders at negative coordinates
    shifted = fields.dense_leaves(24).astype(np.int64) + np.array([-4104, -16, 120])
    shifted = shifted.astype(np.int32)
    shifted = np.ascontiguousarray(shifted[fields.nanovdb_order(shifted)])
    # 2 x 2 x 2 leaves in each corner region of the int32 coordinate range: a 16^3 block's neighbours lie outside it there
    lo, hi = -2**31, 2**31 - 16
    corner = np.array([[i, j, k] for i in (0, 8) for j in (0, 8) for k in (0, 8)], dtype=np.int64)
    edge = np.concatenate([corner + np.array(c) for c in ((lo, lo, lo), (hi, hi, hi), (lo, 0, hi), (hi, lo, 0))]).astype(np.int32)
    edge = np.ascontiguousarray(edge[fields.nanovdb_order(edge)])
    return {"dense32": fields.dense_leaves(32), "dense40": fields.dense_leaves(40), "plume": fields.plume_leaves(16, 1.5, 0.3), "scatter": scatter,
            "node_borders": shifted, "one_leaf": np.array([[8, -8, 0]], dtype=np.int32), "int32_edge": edge}


@pytest.fixture(autouse=True)
def restore_options():
    yield
    for k in ("rbgs", "sor_block_lb"):
        H.set_option(k, None)


def solve(grid, div, p0, iters, **opts):
    for k, v in opts.items():
        H.set_option(k, str(v))
    p_a = p0.clone()
    p_b = torch.full_like(p0, 7.0)  # stale content of the second buffer must not matter
    out = D.rbgs_iterate(grid, div, p_a, p_b, 0.013, 1.93, iters).clone()
    for k in opts:
        H.set_option(k, None)
    return out


@pytest.mark.parametrize("name", list(leaf_sets()))
def test_blocked_sor_matches_two_launch_form_and_oracle(name):
    origins = leaf_sets()[name]
    grid = api.create_grid_from_leaves(origins, 0.013)
    n = len(origins) * 512
    g = torch.Generator(device="cpu").manual_seed(3)
    div = torch.randn(n, generator=g).cuda()
    p0 = (torch.rand(n, generator=g) * 2 - 1).cuda()
    oracle = OracleGrid(origins)
    for iters in (1, 2, 3, 4, 7, 10):  # (odd counts: the one left over is one more launch of the same kernel with two colour sweeps instead of four)
        want = solve(grid, div, p0, iters, rbgs="color")
        if iters in (3, 4):
            ref = oracle.rbgs_iterations(div.cpu().numpy(), 0.013, 1.93, iters, p0.cpu().numpy())
            assert np.array_equal(want.cpu().numpy(), ref), (name, iters, "two-launch form vs oracle")
        for lb in SHAPES:
            got = solve(grid, div, p0, iters, sor_block_lb=lb)
            assert torch.equal(want, got), (name, iters, lb, float((want - got).abs().max()))


def test_default_form_by_size_is_bit_identical():
    """whatever `rbgs = auto` picks for a grid size (one-leaf blocks with four or two iterations per launch, 16^3 blocks) gives the two-launch bits"""
    for R in (16, 48, 96):
        origins = fields.dense_leaves(R)
        grid = api.create_grid_from_leaves(origins, 1.0 / R)
        n = len(origins) * 512
        g = torch.Generator(device="cpu").manual_seed(R)
        div = torch.randn(n, generator=g).cuda()
        p0 = torch.zeros(n, device="cuda")
        for iters in (5, 8):
            assert torch.equal(solve(grid, div, p0, iters, rbgs="color"), solve(grid, div, p0, iters)), (R, iters)


def test_blocked_sor_known_answer_harmonic_fixed_point():
    """a discrete-harmonic p with div = 0 is a fixed point of every sweep wherever all six neighbours exist (tests/kats.py):
    inside a dense box, away from the outside-is-zero rim, K iterations per launch must leave it untouched"""
    R = 32
    origins = fields.dense_leaves(R)
    grid = api.create_grid_from_leaves(origins, 1.0 / R)
    c = fields.leaves_to_coords(origins).astype(np.float32)
    p = (c[:, 0] - 2 * c[:, 1] + 3 * c[:, 2]).astype(np.float32)  # linear: harmonic, small integers, sums exact
    p0 = torch.from_numpy(p).cuda()
    div = torch.zeros_like(p0)
    inner = torch.from_numpy(((c >= 8) & (c < R - 8)).all(1)).cuda()
    for lb in SHAPES:
        got = solve(grid, div, p0, 4, sor_block_lb=lb)
        assert torch.equal(got[inner], p0[inner]), lb


def test_every_occupancy_pattern_of_a_block():
    """a 16^3 block exists as soon as one of its 2 x 2 x 2 leaves does: all 255 occupancy patterns of one block, each inside a random half-filled
    neighbourhood of leaves (so that the 4 x 4 x 4 leaves under the tile are present and absent in every combination a mask can meet)"""
    rng = np.random.default_rng(11)
    cells = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)], dtype=np.int32)
    around = np.array([[i, j, k] for i in range(-2, 4) for j in range(-2, 4) for k in range(-2, 4) if not (0 <= i < 2 and 0 <= j < 2 and 0 <= k < 2)], dtype=np.int32)
    for pattern in range(1, 256):
        own = cells[[(pattern >> c) & 1 == 1 for c in range(8)]]
        o = np.concatenate([own, around[rng.random(len(around)) < 0.5]]) * 8 + np.array([-16, 32, -48], dtype=np.int32)
        o = np.ascontiguousarray(o[fields.nanovdb_order(o)].astype(np.int32))
        grid = api.create_grid_from_leaves(o, 0.02)
        n = len(o) * 512
        g = torch.Generator(device="cpu").manual_seed(pattern)
        div = torch.randn(n, generator=g).cuda()
        p0 = (torch.rand(n, generator=g) * 2 - 1).cuda()
        for iters in (4, 3) if pattern % 16 == 5 else (4,):  # (every sixteenth pattern also with an odd count: the one-iteration launch of the 16^3 kernel)
            want = solve(grid, div, p0, iters, rbgs="color")
            for lb in SHAPES:
                got = solve(grid, div, p0, iters, sor_block_lb=lb)
                assert torch.equal(want, got), (pattern, iters, lb, float((want - got).abs().max()))


@pytest.mark.parametrize("leaves", [8, 512, 4096])
def test_result_buffer_is_the_one_result_in_b_names(leaves):
    """include/hns.h, hns_dev_rbgs_iterate: which of p_a / p_b holds the result depends on the form the library picks, not on
    the parity of `iterations` -- the documented contract is *result_in_b, for every iteration count, under
    rbgs=auto. Checked through the raw C ABI: the named buffer holds the two-launch result, and it follows the plan's
    launch count."""
    import ctypes as C

    lib = H.load_library()
    R = {8: 16, 512: 64, 4096: 128}[leaves]
    origins = fields.dense_leaves(R)
    grid = api.create_grid_from_leaves(origins, 1.0 / R)
    n = len(origins) * 512
    g = torch.Generator(device="cpu").manual_seed(leaves)
    div = torch.randn(n, generator=g).cuda()
    p0 = torch.randn(n, generator=g).cuda()
    for iters in (1, 2, 3, 4, 6):
        want = solve(grid, div, p0, iters, rbgs="color")
        p_a, p_b = p0.clone(), torch.full_like(p0, 7.0)
        in_b = C.c_int(-1)
        rc = lib.hns_dev_rbgs_iterate(grid.ptr, div.data_ptr(), p_a.data_ptr(), p_b.data_ptr(), C.c_float(0.013), C.c_float(1.93), iters, C.byref(in_b), D.current_stream())
        assert rc == 0 and in_b.value in (0, 1)
        torch.cuda.synchronize()
        assert torch.equal(p_b if in_b.value else p_a, want), f"iterations = {iters}: the buffer named by result_in_b does not hold the result"
        _, launches, _ = D.rbgs_plan(grid, iters)
        assert in_b.value == (launches & 1), f"iterations = {iters}: result_in_b = {in_b.value} but the plan says {launches} launches"


def schedule_steps(lb, k_max, iterations):
    """ping-pong steps of a solve, from the rule in include/hns.h (hns_dev_rbgs_iterate): blocked, launches of four iterations while four per launch is the form and at
    least four remain, then of two, then one for an odd iteration left over; the colour form, one step per iteration"""
    if lb == 0:
        return iterations
    steps, left = 0, iterations
    while k_max == 4 and left >= 4:
        steps, left = steps + 1, left - 4
    return steps + left // 2 + left % 2


# leaves -> edge of the dense box in voxels, and per option the form it selects there: (block edge in leaves, iterations per launch); (0, 1) = the colour form.
# The smallest grids on which each form is the default: four per launch up to 300 leaves, one-leaf blocks up to 600, 16^3 blocks beyond. Forcing the block edge
# leaves the iterations per launch by size.
PLAN_FORMS = {
    8: (16, {(): (1, 4), ("sor_block_lb", 1): (1, 4), ("sor_block_lb", 2): (2, 2), ("rbgs", "color"): (0, 1)}),
    343: (56, {(): (1, 2), ("sor_block_lb", 1): (1, 2), ("sor_block_lb", 2): (2, 2), ("rbgs", "color"): (0, 1)}),
    729: (72, {(): (2, 2), ("sor_block_lb", 1): (1, 2), ("sor_block_lb", 2): (2, 2), ("rbgs", "color"): (0, 1)}),
}


@pytest.mark.parametrize("leaves", list(PLAN_FORMS))
def test_plan_and_solve_agree_for_every_form(leaves):
    """hns_grid_rbgs_plan and hns_dev_rbgs_iterate read one schedule: for every form (by size, either block edge forced, the colour form) and 0 .. 9 iterations the buffer
    *result_in_b names holds the colour form's bits, result_in_b is the parity of the steps, and the plan reports those steps as launches (two per iteration for the
    colour form), the form's iterations per launch and its kernel. Through the raw C ABI."""
    import ctypes as C

    lib = H.load_library()
    R, forms = PLAN_FORMS[leaves]
    origins = fields.dense_leaves(R)
    assert len(origins) == leaves
    grid = api.create_grid_from_leaves(origins, 1.0 / R)
    n = leaves * 512
    g = torch.Generator(device="cpu").manual_seed(leaves)
    div = torch.randn(n, generator=g).cuda()
    p0 = torch.randn(n, generator=g).cuda()
    want = [solve(grid, div, p0, iters, rbgs="color") for iters in range(10)]
    assert torch.equal(want[0], p0)
    for option, (lb, k_max) in forms.items():
        if option:
            H.set_option(option[0], str(option[1]))
        for iters in range(10):
            p_a, p_b = p0.clone(), torch.full_like(p0, 7.0)
            in_b = C.c_int(-1)
            rc = lib.hns_dev_rbgs_iterate(grid.ptr, div.data_ptr(), p_a.data_ptr(), p_b.data_ptr(), C.c_float(0.013), C.c_float(1.93), iters, C.byref(in_b), D.current_stream())
            torch.cuda.synchronize()
            what = f"{leaves} leaves, {option}, {iters} iterations"
            steps = schedule_steps(lb, k_max, iters)
            assert rc == 0 and in_b.value == (steps & 1), f"{what}: result_in_b = {in_b.value}, {steps} steps"
            assert torch.equal(p_b if in_b.value else p_a, want[iters]), f"{what}: the buffer named by result_in_b does not hold the result"
            if iters == 0:
                assert in_b.value == 0 and torch.equal(p_a, p0), f"{what}: p_a touched"
            desc, launches, per = D.rbgs_plan(grid, iters)
            assert launches == (steps if lb else 2 * iters), f"{what}: the plan says {launches} launches"
            assert per == (k_max if lb and iters >= 2 else 1), f"{what}: the plan says {per} iterations per launch"
            kernel = {0: "k_rbgs_color", 1: "k_rbgs_block<1,", 2: "k_rbgs_block_xy<2,"}[lb if iters else 0]  # (a solve of no iteration names no blocked kernel)
            assert desc.startswith(kernel), f"{what}: {desc}"
        if option:
            H.set_option(option[0], None)


@pytest.mark.parametrize("name", ["dense40", "plume", "scatter", "node_borders"])
def test_blocked_sor_over_a_launch_range(name):
    """Round 4: the blocked form over a LAUNCH RANGE [first, first + count) of the grid's leaves (what a multi-GPU rank's
    boundary / interior ranges are): two iterations in one launch, every leaf of the grid a tile source, only the leaves of
    the range stored. Owned leaves must equal two iterations of the two-launch form on the whole grid bit for bit; the other
    leaves of the output buffer must not be touched."""
    origins = leaf_sets()[name]
    n_leaves = len(origins)
    n = n_leaves * 512
    g = torch.Generator(device="cpu").manual_seed(n_leaves)
    div = torch.randn(n, generator=g).cuda()
    p0 = torch.randn(n, generator=g).cuda()
    whole = api.create_grid_from_leaves(origins, 0.013)
    want = solve(whole, div, p0, 2, rbgs="color")
    for first, count in ((0, n_leaves // 3), (n_leaves // 3, n_leaves // 2), (n_leaves - 5, 5), (7, 1), (0, n_leaves)):
        count = max(1, min(count, n_leaves - first))
        part = api.create_grid_from_leaves(origins, 0.013)
        part.set_active_range(first, count)
        for lb in (0, 1, 2):  # by size, one-leaf blocks, 16^3 blocks
            H.set_option("sor_block_lb", str(lb))
            desc, launches, per = D.rbgs_plan(part, 2)
            assert launches == 1 and "k_rbgs_block" in desc, (desc, launches)
            out, p_a, p_b, sl = range_sweep(part, div, p0, 2, first, count, 0.013, 1.93, f"{name} range [{first}, +{count}) lb={lb}")
            assert out is p_b
            assert torch.equal(out[sl], want[sl]), f"{name} range [{first}, +{count}) lb={lb}: owned leaves differ"
            assert torch.equal(p_a, p0)
        H.set_option("sor_block_lb", None)


def special_inputs(n_leaves, seed):
    """div and p0 with zeros of both signs, subnormals and NaN / inf (tests/special_cases.py) planted into a third of the leaves each; the non-finite third gets a
    stated number of plantings (every iteration widens a NaN's reach by two voxels)"""
    import special_cases as sc

    rng = np.random.default_rng(seed)
    n = n_leaves * 512
    div, p0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    t = max(1, n_leaves // 3) * 512
    for a in (div, p0):
        a[:t] = sc.plant("zeros", a[:t], rng)
        a[t:2 * t] = sc.plant("subnormal", a[t:2 * t], rng)
    few = 1 if n < 65536 else 4
    p0[2 * t:] = sc.plant_few(p0[2 * t:], rng, few) if n > 2 * t else p0[2 * t:]
    div[2 * t:] = sc.plant_few(div[2 * t:], rng, few) if n > 2 * t else div[2 * t:]
    return torch.from_numpy(div).cuda(), torch.from_numpy(p0).cuda()


def same_words(a, b):
    """equal as raw 32-bit words (torch.equal on floats calls a NaN unequal to itself), except that a NaN may differ from the other form's NaN in its sign bit:
    special_cases.nan_sign_differences says why, and what was measured"""
    import special_cases as sc

    return sc.nan_sign_differences(a.cpu().numpy(), b.cpu().numpy())[0]


@pytest.mark.parametrize("name", ["scatter", "dense40", "int32_edge"])
def test_blocked_sor_on_special_values(name):
    """zeros of both signs, subnormals, NaN and inf in div and p0: the blocked forms against the two-launch form, raw 32-bit words. A NaN is the sharpest tracer of the
    halo's dependency cone: one that arrives an iteration early or late moves the edge of the NaN region."""
    origins = leaf_sets()[name]
    grid = api.create_grid_from_leaves(origins, 0.013)
    div, p0 = special_inputs(len(origins), 21)
    for iters in (1, 2, 3, 4, 7):
        want = solve(grid, div, p0, iters, rbgs="color")
        share = float(torch.isnan(want).float().mean())
        assert 0 < share <= 0.5, (name, iters, share)
        for lb in SHAPES:
            got = solve(grid, div, p0, iters, sor_block_lb=lb)
            assert same_words(want, got), (name, iters, lb, int((want.view(torch.int32) != got.view(torch.int32)).sum()))


@pytest.mark.parametrize("name", ["dense40", "plume", "scatter", "node_borders"])
def test_blocked_sor_over_a_launch_range_on_special_values(name):
    """test_blocked_sor_over_a_launch_range with the special values in div and p0"""
    origins = leaf_sets()[name]
    n_leaves = len(origins)
    n = n_leaves * 512
    div, p0 = special_inputs(n_leaves, n_leaves)
    whole = api.create_grid_from_leaves(origins, 0.013)
    want = solve(whole, div, p0, 2, rbgs="color")
    assert 0 < float(torch.isnan(want).float().mean()) <= 0.5
    for first, count in ((0, n_leaves // 3), (n_leaves // 3, n_leaves // 2), (n_leaves - 5, 5), (7, 1), (0, n_leaves)):
        count = max(1, min(count, n_leaves - first))
        part = api.create_grid_from_leaves(origins, 0.013)
        part.set_active_range(first, count)
        for lb in (0, 1, 2):
            H.set_option("sor_block_lb", str(lb))
            out, p_a, p_b, sl = range_sweep(part, div, p0, 2, first, count, 0.013, 1.93, f"{name} range [{first}, +{count}) lb={lb}")
            assert out is p_b
            assert same_words(out[sl], want[sl]), f"{name} range [{first}, +{count}) lb={lb}: owned leaves differ"
            assert same_words(p_a, p0)
        H.set_option("sor_block_lb", None)
