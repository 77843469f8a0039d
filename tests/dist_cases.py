"""The partitioned substep's test cases on one device, shared by the multi-GPU and pool-content tests: the single-grid run, the locally connected ranks of a
decomposition, and the comparison of what the ranks own with the single grid bit for bit."""
import numpy as np

from hnanosolver_amd import dist as HD
from hnanosolver_amd import fields

SIM_NAMES = ["density", "temperature", "fuel", "waste", "flame", "collision_sdf"]


def single_grid(origins, R, names, iters, substeps, dt=1.0 / 24.0, f=None):
    """f: a dictionary of fields in place of fields.synthetic_fields (the special-value cases)"""
    from hnanosolver_amd import api, device as D

    f = f or fields.synthetic_fields(origins, R)
    grid = api.create_grid_from_leaves(origins, 1.0 / R)
    sim = D.Sim(grid, names)
    arrays = {"vel": f["vel"].copy(), **{n: f[n].copy() for n in names}}
    sim.upload(arrays)
    for _ in range(substeps):
        sim.core_substep(iters, dt, 1.0 / R, D.current_stream())
    sim.download(arrays)
    return f, arrays


def run_local(origins, R, world, k, names, iters, substeps, dt=1.0 / 24.0, f=None):
    import torch

    f = f or fields.synthetic_fields(origins, R)
    ranks = [HD.DistRank(origins, world, r, 1.0 / R, n_scalars=len(names), sweeps_per_exchange=k) for r in range(world)]
    HD.DistRank.connect_local(ranks)
    # (which leaves a rank owns is the rank's own knowledge: DistRank.owned_ids / owned_voxels)
    for r, d in enumerate(ranks):
        d.upload(d.owned_voxels(f["vel"]), [d.owned_voxels(f[n]) for n in names])
    stream = int(torch.cuda.current_stream().cuda_stream)
    for _ in range(substeps):
        HD.DistRank.local_core_substep(ranks, iters, dt, stream)
    for d in ranks:
        d.synchronize(stream)
    return ranks


def check(ranks, want, names):
    # the ghost voxels the next kernels read hold their owners' bits (velocity: whole leaves; p: reach 1), whatever the transport wrote them with
    n_pairs, bad = HD.DistRank.ghost_check_local(ranks)
    assert not bad and (n_pairs > 0 or len(ranks) == 1), (n_pairs, bad[:3])
    for r, d in enumerate(ranks):
        got = d.download()
        assert np.array_equal(got["vel"], d.owned_voxels(want["vel"])), f"rank {r} velocity"
        for n, a in zip(names, got["scalars"]):
            assert np.array_equal(a, d.owned_voxels(want[n])), f"rank {r} {n}"


def sim_fields(origins, R):
    f = fields.synthetic_fields(origins, R)
    f["collision_sdf"] = fields.sphere_sdf(origins, R)
    f["waste"] = (0.05 * f["density"]).astype(np.float32)  # burning state: every combustion branch is exercised (tests/kats.py has the table)
    f["flame"] = (0.3 * f["fuel"]).astype(np.float32)
    return f


def partitioned_sim_substeps_match_single_grid(origins, R, world, k, iters, substeps, params, coll, dt=1.0 / 24.0):
    """`substeps` whole Compute_Sim substeps on `world` locally connected ranks: what every rank owns equals hns_sim_substep's on the one grid bit for bit"""
    import torch
    from hnanosolver_amd import api, device as D

    f = sim_fields(origins, R)
    grid = api.create_grid_from_leaves(origins, 1.0 / R)
    sim = D.Sim(grid, SIM_NAMES)
    want = {"vel": f["vel"].copy(), **{n: f[n].copy() for n in SIM_NAMES}}
    sim.upload(want)
    for _ in range(substeps):
        sim.substep(iters, dt, 1.0 / R, params, coll, D.current_stream())
    sim.download(want)

    ranks = [HD.DistRank(origins, world, r, 1.0 / R, n_scalars=len(SIM_NAMES), sweeps_per_exchange=k) for r in range(world)]
    HD.DistRank.connect_local(ranks)
    for r, d in enumerate(ranks):
        d.upload(d.owned_voxels(f["vel"]), [d.owned_voxels(f[n]) for n in SIM_NAMES])
    stream = int(torch.cuda.current_stream().cuda_stream)
    for _ in range(substeps):
        HD.DistRank.local_sim_substep(ranks, SIM_NAMES, iters, dt, params, coll, stream)
    for d in ranks:
        d.synchronize(stream)
    check(ranks, want, SIM_NAMES)
    return ranks, want
