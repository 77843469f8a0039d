"""TEST HELPER: the OracleGrid call signatures (tests/oracle_lib.py) on top of the HIP kernels, through the C ABI
(hns_dev_* via hnanosolver_amd.device; the operators via hnanosolver_amd.api). Lets one test body run against the oracle and
against the product.

slab=True runs every kernel-level call guard-banded: outputs and in-place operands are carved from a patterned stream_cases.Slab (two leaves of pattern
around each) instead of allocated one by one, and after the call the guards must be intact and every input that is not documented as in-place must hold
the bytes it was given. The values returned are the same either way."""
import numpy as np


class HipKernels:
    def __init__(self, leaves, voxel_size=1.0 / 32.0, slab=False):
        import torch

        from hnanosolver_amd import api, device

        self.t, self.D, self.api = torch, device, api
        self.origins = np.ascontiguousarray(leaves, dtype=np.int32)
        self.grid = api.create_grid_from_leaves(self.origins, voxel_size)
        self.slab = slab
        self._slab, self._given = None, {}

    def _d(self, a):
        return None if a is None else self.t.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    def _h(self, t):
        return t.cpu().numpy()

    def _bufs(self, what, inplace=None, **shapes):
        """device buffers the call writes: `shapes` = {name: shape} of pure outputs, `inplace` = {name: array} of operands updated in place -> {name: tensor}"""
        inplace = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in (inplace or {}).items()}
        if not self.slab:
            out = {k: self.t.empty(s, device="cuda") for k, s in shapes.items()}
            out.update({k: self._d(v) for k, v in inplace.items()})
            return out
        from stream_cases import Slab, sentinel

        specs = {k: (tuple(np.atleast_1d(s)), np.float32) for k, s in shapes.items()}
        specs.update({k: (v.shape, np.float32) for k, v in inplace.items()})
        self._slab, self._what = Slab(self.t, specs, "cuda"), what
        for k in shapes:
            sentinel(self._slab.views[k])
        for k, v in inplace.items():
            self._slab.views[k].copy_(self.t.from_numpy(v))
        return dict(self._slab.views)

    def _ins(self, **arrays):
        """device copies of the arrays the call only reads (None stays None)"""
        self._given = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in arrays.items() if v is not None}
        self._read = {k: self._d(v) for k, v in self._given.items()}
        return [self._read.get(k) for k in arrays]

    def _checked(self):
        """after the call: guards intact, inputs unchanged"""
        if self.slab and self._slab is not None:
            from stream_cases import assert_inputs_unchanged

            self.t.cuda.synchronize()
            self._slab.check(self._what)
            assert_inputs_unchanged(self._read, self._given, what=self._what)
            self._slab = None

    def advect_vector(self, vel, dt, inv_dx, sdf=None, has_collision=False):
        u, s = self._ins(vel=vel, sdf=sdf)
        out = self._bufs("advect_vector", out=u.shape)["out"]
        self.D.advect_vector(self.grid, u, out, dt, inv_dx, s, has_collision)
        self._checked()
        return self._h(out)

    def advect_scalar(self, vel, phi, dt, inv_dx, sdf=None, has_collision=False):
        u, p, s = self._ins(vel=vel, phi=phi, sdf=sdf)
        out = self._bufs("advect_scalar", out=p.shape)["out"]
        self.D.advect_scalar(self.grid, u, p, out, dt, inv_dx, s, has_collision)
        self._checked()
        return self._h(out)

    def advect_scalars(self, vel, phis, dt, inv_dx, sdf=None, has_collision=False):
        ins = self._ins(vel=vel, sdf=sdf, **{f"phi{i}": p for i, p in enumerate(phis)})
        u, s, src = ins[0], ins[1], ins[2:]
        b = self._bufs("advect_scalars", **{f"out{i}": p.shape for i, p in enumerate(src)})
        dst = [b[f"out{i}"] for i in range(len(src))]
        self.D.advect_scalars(self.grid, u, src, dst, dt, inv_dx, s, has_collision)
        self._checked()
        return [self._h(d) for d in dst]

    def divergence(self, vel, inv_dx):
        (u,) = self._ins(vel=vel)
        out = self._bufs("divergence", out=(len(vel),))["out"]
        self.D.divergence(self.grid, u, out, inv_dx)
        self._checked()
        return self._h(out)

    def rbgs(self, div, p, dx, color, omega):
        (d,) = self._ins(div=div)
        q = self._bufs("rbgs_color", inplace={"p": p})["p"]
        self.D.rbgs_color(self.grid, d, q, dx, omega, color)
        self._checked()
        return self._h(q)

    def rbgs_iterations(self, div, dx, omega, iterations, p0=None):
        """the production path: fused (red, black) launches"""
        n = len(div)
        (d,) = self._ins(div=div)
        b = self._bufs("rbgs_iterate", inplace={"a": np.zeros(n, np.float32) if p0 is None else p0, "b": np.zeros(n, np.float32)})
        res = self.D.rbgs_iterate(self.grid, d, b["a"], b["b"], dx, omega, iterations)
        self._checked()
        return self._h(res)

    def subtract_pressure_gradient(self, vel, p, inv_dx, sdf=None, has_collision=False):
        u, q, s = self._ins(vel=vel, p=p, sdf=sdf)
        out = self._bufs("subtract_pressure_gradient", out=u.shape)["out"]
        self.D.subtract_pressure_gradient(self.grid, u, q, out, inv_dx, s, has_collision)
        self._checked()
        return self._h(out)

    def combustion_oxygen(self, fuel, waste, temperature, div, flame, temp_gain, expansion):
        f, w, t, fl = self._ins(fuel=fuel, waste=waste, temperature=temperature, flame=flame)
        n = (len(fuel),)
        b = self._bufs("combustion_oxygen", inplace={"div": div}, out0=n, out1=n, out2=n, out3=n)
        outs = [b[f"out{i}"] for i in range(4)]
        self.D.combustion_oxygen(f, w, t, b["div"], fl, *outs, temp_gain, expansion)
        self._checked()
        return tuple(self._h(o) for o in outs) + (self._h(b["div"]),)

    def temperature_buoyancy(self, vel, temp, dt, ambient, strength):
        u, t = self._ins(vel=vel, temp=temp)
        out = self._bufs("temperature_buoyancy", out=u.shape)["out"]
        self.D.temperature_buoyancy(u, t, out, dt, ambient, strength)
        self._checked()
        return self._h(out)

    def vorticity_confinement(self, vel, dt, inv_dx, scale, factor_scale):
        (u,) = self._ins(vel=vel)
        out = self._bufs("vorticity_confinement", out=u.shape)["out"]
        self.D.vorticity_confinement(self.grid, u, out, dt, inv_dx, scale, factor_scale)
        self._checked()
        return self._h(out)

    def enforce_collision_boundaries(self, vel, sdf, voxel_size):
        (s,) = self._ins(sdf=sdf)
        u = self._bufs("enforce_collision_boundaries", inplace={"vel": vel})["vel"]
        self.D.enforce_collision_boundaries(self.grid, u, s, voxel_size)
        self._checked()
        return self._h(u)

    # ---- host drivers through the drop-in operators (results in place, like the reference) ----
    def _data(self, vel, fields_: dict):
        from hnanosolver_amd import fields as F

        d = self.api.GridIndexedData()
        c = F.leaves_to_coords(self.origins)
        d.allocateCoords(len(c))
        d.pCoords()[:] = c
        for n, a in fields_.items():
            d.addValueBlock(n, d.FLOAT)
            d.pValues(n)[:] = a
        d.addValueBlock("vel", d.VEC3F)
        d.pValues("vel")[:] = vel
        return d

    def compute_sim(self, vel, fields_: dict, iterations, dt, voxel_size, params, has_collision):
        d = self._data(vel, fields_)
        h = self.api.IndexGridHandle()
        self.api.CreateIndexGrid(d, h, voxel_size)
        self.api.Compute_Sim(d, h, iterations, dt, voxel_size, params, has_collision)
        h.reset()
        for n in fields_:
            fields_[n][:] = d.pValues(n)
        vel[:] = d.pValues("vel")
        return 0

    def project_non_divergent(self, vel, iterations, voxel_size):
        d = self._data(vel, {})
        self.api.ProjectNonDivergent(d, iterations, voxel_size)
        vel[:] = d.pValues("vel")
        return 0
