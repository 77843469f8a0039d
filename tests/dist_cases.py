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


# What a rank reports of its exchanges (hns_dist_info), per form of the substep. tests/golden/dist_exchange_counts.json holds these as the commit BEFORE the halo
# exchange was stated once reported them (recorded by profiles/micro/dist_exchange_counts.py); tests/test_dist_gpu.py compares for equality.
COUNTERS = ("exchanges", "messages_sent", "packed_exchanges", "bytes_sent", "chained")
# form: (transport, library options, case, world, sweeps_per_exchange, iterations)
EXCHANGE_FORMS = {
    "local_one_peer": ("local", {"dist_mirror": "0"}, "dense32", 2, 4, 7),            # no combined tables: pack / unpack per peer
    "local_seven_peers": ("local", {"dist_mirror": "0"}, "plume", 8, 2, 7),           # the combined tables: one pack / unpack launch per field
    "local_dense64_k2": ("local", {}, "dense64", 2, 2, 7),                           # option dist_mirror at its default; 256 leaves per rank: still exchanged
    "local_chained": ("local", {}, "dense88", 2, 2, 7),                              # 665 leaves per rank: every kernel delivers its own halo (the full substep exchanges)
    "loopback_split": ("loopback", {"dist_unsplit": "0"}, "dense64", 2, 2, 9),        # two streams, boundary / interior launches
    "loopback_in_line": ("loopback", {"dist_unsplit": "always"}, "dense64", 2, 2, 9),  # two-stream transport, the short phases in line
}


def case_leaves(name):
    return {"dense32": lambda: (fields.dense_leaves(32), 32), "dense64": lambda: (fields.dense_leaves(64), 64), "dense88": lambda: (fields.dense_leaves(88), 88),
            "plume": lambda: (fields.plume_leaves(8, 1.5, 0.35), 64)}[name]()


def exchange_counts(form):
    """{"core": [counters of every rank after ONE core substep], "full": [the same after one whole Compute_Sim substep with collision]}, fresh ranks for each"""
    import torch
    import hnanosolver_amd as H
    from hnanosolver_amd import api

    transport, options, case, world, k, iters = EXCHANGE_FORMS[form]
    origins, R = case_leaves(case)
    f = sim_fields(origins, R)
    params = api.CombustionParams(factorScale=1.0, vorticityScale=0.01, buoyancyStrength=0.05)
    stream = int(torch.cuda.current_stream().cuda_stream)
    out = {}
    for o, v in options.items():
        H.set_option(o, v)
    try:
        for which, names in (("core", SIM_NAMES[:2]), ("full", SIM_NAMES)):
            ranks = [HD.DistRank(origins, world, r, 1.0 / R, n_scalars=len(names), sweeps_per_exchange=k) for r in range(world if transport == "local" else 1)]
            if transport == "local":
                HD.DistRank.connect_local(ranks)
            else:
                ranks[0].connect_loopback()
            for d in ranks:
                d.upload(d.owned_voxels(f["vel"]), [d.owned_voxels(f[n]) for n in names])
            if transport == "local":
                if which == "core":
                    HD.DistRank.local_core_substep(ranks, iters, 1.0 / 24.0, stream)
                else:
                    HD.DistRank.local_sim_substep(ranks, names, iters, 1.0 / 24.0, params, True, stream)
            elif which == "core":
                ranks[0].core_substep(iters, 1.0 / 24.0, stream)
            else:
                ranks[0].sim_substep(names, iters, 1.0 / 24.0, params, True, stream)
            for d in ranks:
                d.synchronize(stream)
            out[which] = [{c: d.info()[c] for c in COUNTERS} for d in ranks]
            if transport == "loopback":
                ranks[0].close()
    finally:
        for o in options:
            H.set_option(o, None)
    return out


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
