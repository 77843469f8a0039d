"""The 16^3-block SOR kernel (k_rbgs_block_xy, hnanosolver_amd/csrc/hns_sorblock.hip) sweeps the rows of its 24 x 24 tile shell by shell: a row
takes part in sweep S only while its lateral excess over the block is <= NS - S, the rows beside the block's corners that cannot reach it are neither
fetched, staged nor swept. Any update the block needs and a sweep skipped, and any LDS entry read that no thread staged, changes bits: everything
here is compared as 32-bit words against the two-launch form (rbgs = color), with 16^3 blocks forced (sor_block_lb = 2), on leaf sets in which every
shell meets every tile situation -- a whole tile present (the unmasked path), tiles on faces, edges and corners of the leaf set, holes under tiles."""
import numpy as np
import pytest
import torch

import hnanosolver_amd as H
from hnanosolver_amd import api, device as D, fields
from diag_cases import pressure_of, set_divergence, words

pytestmark = pytest.mark.gpu

VS, OMEGA = 0.013, 1.93
ITERS = (1, 2, 3, 4, 5)  # 1: the ZERO / NS = 2 launch alone; 3, 5: four-sweep launches and the NS = 2 one left over; 4, 5: the buffers alternate


def _cube(shift):
    o = np.array([[i, j, k] for i in range(4) for j in range(4) for k in range(4)], dtype=np.int32) * 8 + np.int32(shift)
    return np.ascontiguousarray(o[fields.nanovdb_order(o)])


def _leaf_sets():
    aligned = _cube(0)  # 2 x 2 x 2 blocks on the 16-voxel lattice: every tile has absent leaf cells (the masked path)
    shifted = _cube(8)  # 3 x 3 x 3 blocks: the one at 16 has its whole tile present, faces / edges / corners hold four / two / one leaf
    gone = {(16, 16, 16), (24, 16, 24), (8, 32, 16), (32, 8, 8), (16, 24, 32)}  # leaves from inside: holes under the tiles around them
    holes = np.ascontiguousarray(np.array([o for o in shifted.tolist() if tuple(o) not in gone], dtype=np.int32))
    return {"aligned": aligned, "shifted": shifted, "holes": holes}


LEAF_SETS = _leaf_sets()


@pytest.fixture(autouse=True)
def restore_options():
    yield
    for k in ("rbgs", "sor_block_lb"):
        H.set_option(k, None)


def _solve(grid, div, p0, iters, **opts):
    for k, v in opts.items():
        H.set_option(k, str(v))
    p_a = p0.clone()
    p_b = torch.full_like(p0, 7.0)  # (stale content of the second buffer must not matter)
    out = D.rbgs_iterate(grid, div, p_a, p_b, VS, OMEGA, iters).clone()
    for k in opts:
        H.set_option(k, None)
    return out


def _words(t):
    return t.view(torch.int32)


def _same_bits(want, got, what):
    differ = _words(want) != _words(got)
    assert not bool(differ.any()), (what, int(differ.sum()), int(differ.nonzero()[0]))


def _random_fields(n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n, generator=g).cuda(), (torch.rand(n, generator=g) * 2 - 1).cuda()


@pytest.mark.parametrize("name", list(LEAF_SETS))
def test_shell_sweeps_give_the_two_launch_bits(name):
    origins = LEAF_SETS[name]
    grid = api.create_grid_from_leaves(origins, VS)
    div, warm = _random_fields(len(origins) * 512, 17)
    for p0 in (torch.zeros_like(warm), warm):
        for iters in ITERS:
            want = _solve(grid, div, p0, iters, rbgs="color")
            got = _solve(grid, div, p0, iters, sor_block_lb=2)
            _same_bits(want, got, (name, iters, "warm" if p0 is warm else "zero"))


@pytest.mark.parametrize("name", list(LEAF_SETS))
def test_solve_from_zero_of_a_sim(name):
    """a sim's pressure solve starts from p = 0 without reading it: its first launch is the ZERO kernel (for one iteration the ZERO, NS = 2 one), over whatever
    the two pressure buffers held -- the previous solve's result here"""
    origins = LEAF_SETS[name]
    grid = api.create_grid_from_leaves(origins, VS)
    sim = D.Sim(grid, ["density"])
    div = _random_fields(len(origins) * 512, 19)[0].cpu().numpy()
    set_divergence(sim, div)
    for iters in ITERS:
        H.set_option("rbgs", "color")
        sim.pressure_solve(iters, VS)
        want = pressure_of(sim)
        H.set_option("rbgs", None)
        H.set_option("sor_block_lb", "2")
        sim.pressure_solve(iters, VS)
        got = pressure_of(sim)
        H.set_option("sor_block_lb", None)
        assert words(want) == words(got), (name, iters, int((want.view(np.uint32) != got.view(np.uint32)).sum()))


def _tile_masks(origins):
    """voxels of the block at 16 .. 31 of the shifted cube (the one whose whole tile is present), and of its 24^3 tile minus the block"""
    c = torch.from_numpy(fields.leaves_to_coords(origins).astype(np.int64))
    block = ((c >= 16) & (c < 32)).all(1)
    tile = ((c >= 12) & (c < 36)).all(1)
    return block.cuda(), (tile & ~block).cuda()


@pytest.mark.parametrize("where", ["halo", "block"])
def test_structured_fields_around_the_fully_present_block(where):
    """p non-zero only in the halo shell of the fully present block, with div = 0: every bit of the block's result then comes through the shell rows;
    and p and div non-zero only in that block: every bit the neighbouring blocks compute comes out of it through their own shells"""
    origins = LEAF_SETS["shifted"]
    grid = api.create_grid_from_leaves(origins, VS)
    div, p = _random_fields(len(origins) * 512, 23)
    block, halo = _tile_masks(origins)
    assert int(block.sum()) == 16**3 and int(halo.sum()) == 24**3 - 16**3
    if where == "halo":
        p0, d = torch.where(halo, p, torch.zeros_like(p)), torch.zeros_like(div)
    else:
        p0, d = torch.where(block, p, torch.zeros_like(p)), torch.where(block, div, torch.zeros_like(div))
    for iters in ITERS:
        want = _solve(grid, d, p0, iters, rbgs="color")
        got = _solve(grid, d, p0, iters, sor_block_lb=2)
        _same_bits(want, got, (where, iters))
        if where == "halo" and iters >= 2:
            assert bool((want[block] != 0).any())  # (the halo did reach the block: the case is not vacuous)


@pytest.mark.parametrize("name", list(LEAF_SETS))
def test_result_does_not_depend_on_what_lds_held(name):
    """a solve over the same grid with p and div all NaN leaves NaN in every LDS entry a workgroup staged; the real solve behind it must give the bits of
    the two-launch form and of a run without the NaN solve in front -- a sweep that read an entry no thread staged would pick the NaN up"""
    origins = LEAF_SETS[name]
    grid = api.create_grid_from_leaves(origins, VS)
    div, warm = _random_fields(len(origins) * 512, 29)
    nan = torch.full_like(warm, float("nan"))
    for iters in (1, 4, 5):
        want = _solve(grid, div, warm, iters, rbgs="color")
        clean = _solve(grid, div, warm, iters, sor_block_lb=2)
        _solve(grid, nan, nan, iters, sor_block_lb=2)  # (result discarded)
        after = _solve(grid, div, warm, iters, sor_block_lb=2)
        _same_bits(want, after, (name, iters, "vs colour form"))
        _same_bits(clean, after, (name, iters, "vs the run without the NaN solve"))
