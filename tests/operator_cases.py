"""The drop-in operators' test data, shared by the operator, kernel-variant and pool-content tests: a GridIndexedData filled the way the HNanoSolver SOP
fills it, and a copy of its value blocks."""
import numpy as np

from hnanosolver_amd import api, fields


def build_data(origins, R, with_sdf=False, amplitude=96.0, combustion=True):
    f = fields.synthetic_fields(origins, R, amplitude_voxels=amplitude)
    coords = fields.leaves_to_coords(origins)
    d = api.GridIndexedData()
    d.allocateCoords(len(coords))
    d.pCoords()[:] = coords
    # insertion order as the HNanoSolver SOP adds them: float grids first, then velocity (order of getBlocksOfType matters)
    order = ["density", "temperature", "fuel", "waste", "flame"]
    for name in order:
        d.addValueBlock(name, d.FLOAT)
        d.pValues(name)[:] = f[name] if (combustion or name in ("density", "temperature")) else 0.0
    if with_sdf:
        d.addValueBlock("collision_sdf", d.FLOAT)
        sdf = fields.sphere_sdf(origins, R, center=(0.5, 0.3, 0.5), radius=0.15)
        sdf[::11] = np.float32(0.04)
        d.pValues("collision_sdf")[:] = sdf
    d.addValueBlock("vel", d.VEC3F)
    d.pValues("vel")[:] = f["vel"]
    return d


def snapshot(d):
    return {n: d.pValues(n).copy() for n in d.getBlocksOfType(d.FLOAT) + d.getBlocksOfType(d.VEC3F)}


def field_data(origins, f, floats=()):
    """what the single-purpose operators take: the float blocks named in `floats` (values from the field dictionary `f`, zeros for a name it lacks) and f's velocity"""
    coords = fields.leaves_to_coords(origins)
    d = api.GridIndexedData()
    d.allocateCoords(len(coords))
    d.pCoords()[:] = coords
    for name in floats:
        d.addValueBlock(name, d.FLOAT)
        d.pValues(name)[:] = f.get(name, 0.0)
    d.addValueBlock("vel", d.VEC3F)
    d.pValues("vel")[:] = f["vel"]
    return d
