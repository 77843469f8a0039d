"""Registers, LDS and spills of every kernel of the projection side -- divergence (all forms), combustion and buoyancy, the SOR sweeps, the gradient -- and of the
other kernels of the same three files, read from the metadata at the end of the device listings that csrc/Makefile's `%.s` rule writes (the flags of the build).

Bounds, as tests/test_kernel_resources.py sets them for the advection kernels: nothing spills, nothing uses scratch, a kernel's LDS does not grow, and its VGPR count
does not pass the allocation granule (8) it sat in when the projection's expressions were gathered into hns_device.hpp (the counts below are those of the commit before).
Two exceptions. The three fused divergence kernels are bounded at 128, the occupancy step that their amdgpu_waves_per_eu attributes hold them at (four waves per SIMD
need <= 128 registers, five would need <= 96): the order in which the shared epilogue forms its values moves them about below that. The three element-wise
kernels are memory-bound grid-stride loops and are bounded at 32, where they still run at full occupancy."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

FUSED, ELEMENTWISE = 128, 32

# file: {mangled name: (kernel, VGPRs before, LDS bytes before)}
KERNELS = {
    "hns_pressure.hip": {
        "_ZN3hns12k_divergenceENS_7GridDevEPKfPff": ("k_divergence", 16, 108),
        "_ZN3hns12k_rbgs_colorENS_7GridDevEPKfPfffi": ("k_rbgs_color", 13, 108),
        "_ZN3hns16k_divergence_rowINS_8NoMirrorELb1EEEvNS_7GridDevEPKfPffT_": ("k_divergence_row<NoMirror,true>", 60, 12544),
        "_ZN3hns16k_divergence_rowINS_8NoMirrorELb0EEEvNS_7GridDevEPKfPffT_": ("k_divergence_row<NoMirror,false>", 64, 6400),
        "_ZN3hns16k_divergence_rowINS_11PhaseMirrorELb0EEEvNS_7GridDevEPKfPffT_": ("k_divergence_row<PhaseMirror,false>", 64, 6400),
        "_ZN3hns18k_divergence_zpairILb1EEEvNS_7GridDevEPKfPff": ("k_divergence_zpair<true>", 60, 25600),
        "_ZN3hns29k_divergence_combust_buoyancyILb1EEEvNS_7GridDevEPKfPffNS_11CombustFuseE": ("k_divergence_combust_buoyancy<true>", FUSED, 12544),
        "_ZN3hns29k_divergence_combust_buoyancyILb0EEEvNS_7GridDevEPKfPffNS_11CombustFuseE": ("k_divergence_combust_buoyancy<false>", FUSED, 9216),
        "_ZN3hns35k_divergence_combust_buoyancy_zpairENS_7GridDevEPKfPffNS_11CombustFuseE": ("k_divergence_combust_buoyancy_zpair", FUSED, 25600),
        "_ZN3hns21k_subtract_gradient_sINS_8NoMirrorEEEvNS_7GridDevEPKfS4_PffT_": ("k_subtract_gradient_s<NoMirror>", 42, 3584),
        "_ZN3hns21k_subtract_gradient_sINS_11PhaseMirrorEEEvNS_7GridDevEPKfS4_PffT_": ("k_subtract_gradient_s<PhaseMirror>", 45, 3584),
        "_ZN3hns19k_subtract_gradientILb1EEEvNS_7GridDevEPKfS3_PfS3_f": ("k_subtract_gradient<true>", 31, 108),
        "_ZN3hns19k_subtract_gradientILb0EEEvNS_7GridDevEPKfS3_PfS3_f": ("k_subtract_gradient<false>", 13, 108),
    },
    "hns_sorblock.hip": {
        "_ZN3hns11k_sb_leaderENS_7GridDevEiiPi": ("k_sb_leader", 20, 0),
        "_ZN3hns12k_sb_compactEPKiiPiS2_i": ("k_sb_compact", 14, 4096),
        "_ZN3hns10k_sb_tableENS_7GridDevEPKiiiiiiiPi": ("k_sb_table", 22, 0),
        "_ZN3hns12k_rbgs_blockILi1ELi2ELb1ELi4EEEvPKiPKfS4_Pfjff": ("k_rbgs_block<1,2,true,4>", 74, 23296),
        "_ZN3hns12k_rbgs_blockILi1ELi2ELb0ELi4EEEvPKiPKfS4_Pfjff": ("k_rbgs_block<1,2,false,4>", 88, 23296),
        "_ZN3hns12k_rbgs_blockILi1ELi4ELb1ELi8EEEvPKiPKfS4_Pfjff": ("k_rbgs_block<1,4,true,8>", 91, 53248),
        "_ZN3hns12k_rbgs_blockILi1ELi4ELb0ELi8EEEvPKiPKfS4_Pfjff": ("k_rbgs_block<1,4,false,8>", 113, 53248),
        "_ZN3hns12k_rbgs_blockILi1ELi2ELb1ELi2EEEvPKiPKfS4_Pfjff": ("k_rbgs_block<1,2,true,2>", 56, 23296),
        "_ZN3hns12k_rbgs_blockILi1ELi2ELb0ELi2EEEvPKiPKfS4_Pfjff": ("k_rbgs_block<1,2,false,2>", 76, 23296),
    },
    "hns_pointwise.hip": {
        "_ZN3hns19k_combustion_oxygenEPKfS1_S1_PfS1_S2_S2_S2_S2_ffmi": ("k_combustion_oxygen", ELEMENTWISE, 0),
        "_ZN3hns16k_combustion_divEPKfS1_Pffm": ("k_combustion_div", ELEMENTWISE, 0),
        "_ZN3hns22k_temperature_buoyancyEPKfS1_Pffffm": ("k_temperature_buoyancy", ELEMENTWISE, 0),
        "_ZN3hns13k_pack_leavesEPKfPKiPfi": ("k_pack_leaves", 10, 0),
        "_ZN3hns15k_unpack_leavesEPKfPKiPfi": ("k_unpack_leaves", 10, 0),
        "_ZN3hns11k_vorticityENS_7GridDevEPKfPffffi": ("k_vorticity", 142, 108),
        "_ZN3hns19k_enforce_collisionENS_7GridDevEPfPKff": ("k_enforce_collision", 27, 108),
        "k_field_digest": ("k_field_digest", 16, 32),
    },
}
# k_rbgs_block_xy<ZERO, M, K>: all twelve at 64 (ZERO) / 67 registers and 51,136 B
for zero, vgprs in ((1, 64), (0, 67)):
    for mirror in ("8NoMirror", "10PackMirror", "11PhaseMirror"):
        for k in (2, 4):
            KERNELS["hns_sorblock.hip"][f"_ZN3hns15k_rbgs_block_xyILb{zero}ENS_{mirror}ELi{k}EEEvPKiS3_PKfS5_PfjffT0_"] = (
                f"k_rbgs_block_xy<{'true' if zero else 'false'},{mirror.lstrip('0123456789')},{k}>", vgprs, 51136)


@pytest.fixture(scope="module")
def listings():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listings cannot be produced here")
    targets = [f"../lib/obj/{f}.s" for f in KERNELS]
    r = subprocess.run(["make", "-C", CSRC, "-j3"] + targets, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = {}
    for f, t in zip(KERNELS, targets):
        with open(os.path.join(CSRC, t)) as fh:
            out[f] = kernel_metadata(fh.read())
    return out


@pytest.mark.parametrize("file", sorted(KERNELS))
def test_every_kernel_of_the_file_is_listed(listings, file):
    assert set(listings[file]) == set(KERNELS[file]), sorted(set(listings[file]) ^ set(KERNELS[file]))


@pytest.mark.parametrize("file,name", [(f, n) for f in sorted(KERNELS) for n in sorted(KERNELS[f])])
def test_projection_kernel_resources(listings, file, name):
    kernel, vgpr_before, lds_bound = KERNELS[file][name]
    vgpr_bound = (vgpr_before + 7) // 8 * 8
    m = listings[file][name]
    print(f"{kernel}: vgpr {m['vgpr_count']} (<= {vgpr_bound}), sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']} (<= {lds_bound})")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["vgpr_count"] <= vgpr_bound, f"{kernel}: {m['vgpr_count']} VGPRs, bound {vgpr_bound}"
    assert m["group_segment_fixed_size"] <= lds_bound, f"{kernel}: {m['group_segment_fixed_size']} B of LDS, bound {lds_bound}"
