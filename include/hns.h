/*
 * hns.h -- C ABI of libhns.so: the MI355X-native (HIP, gfx950) implementation of HNanoSolver's per-substep hot path.
 *
 * This is the drop-in boundary. Each entry point replaces one of the reference's `extern "C"` C++-typed functions
 * (paths relative to the reference checkout), keeping argument meaning, synchronous in-place semantics and refusal
 * conditions, but with plain pointers/sizes and int return codes instead of C++ types and exceptions:
 *
 *   hns_grid_create                 <- CreateIndexGrid          src/Cuda/HNanoSolver.cu:375-390   (decl. src/SOP/HNanoSolver/SOP_HNanoSolver.hpp:82)
 *   hns_compute_sim                 <- Compute_Sim              src/Cuda/HNanoSolver.cu:9-372,393-396 (decl. src/SOP/HNanoSolver/SOP_HNanoSolver.hpp:84-85)
 *   hns_advect_index_grid           <- AdvectIndexGrid          src/Cuda/Advection.cu:13-112,169-171  (decl. src/SOP/Advection/SOP_VDBAdvect.hpp:66)
 *   hns_advect_index_grid_velocity  <- AdvectIndexGridVelocity  src/Cuda/Advection.cu:114-166,173-175 (decl. src/SOP/VelocityAdvection/SOP_VDBAdvectVelocity.hpp:60)
 *   hns_project_non_divergent       <- ProjectNonDivergent      src/Cuda/PressureProjection.cu:9-78,132-135 (decl. src/SOP/ProjectNonDivergent/SOP_VDBProjectNonDivergent.hpp:69)
 *   hns_divergence                  <- Divergence               src/Cuda/PressureProjection.cu:81-129       (decl. src/SOP/ProjectNonDivergent/SOP_VDBProjectNonDivergent.hpp:70)
 *
 * The type crossing the boundary in the reference is HNS::GridIndexedData (src/Utils/GridData.hpp:16-166): a
 * coordinate array plus named float / Vec3f blocks in insertion order. Here it is `hns_field[]` (same order) and the
 * `hns_grid` handle built from the coordinate array. All host arrays are caller-owned and overwritten in place.
 *
 * Data layout (identical to the reference's): flat leaf-dense arrays, element = leaf*512 + (x<<6 | y<<3 | z) where
 * leaf l is the l-th block of 512 coordinates handed to hns_grid_create (src/Utils/GridBuilder.hpp:156-166);
 * Vec3f fields are AoS float[3] on the host. All arithmetic is float32.
 *
 * `stream` is a hipStream_t passed as void* (NULL = the default stream). Every host-pointer entry point is
 * synchronous: it returns after the stream has drained, like the reference's cudaStreamSynchronize at the end of
 * each driver (HNanoSolver.cu:371, PressureProjection.cu:72, Advection.cu:99-103,158).
 *
 * Threading: hns_last_error() is thread-local, and one grid may be used by several host threads at once (Houdini cooks verbs
 * concurrently): each operator call works on its own device buffers -- the set kept with the grid if it is free, a private one
 * otherwise. Process-wide state, unlike the reference's entry points (which have none): the options of hns_set_option (atomics,
 * read by every entry point when it is called -- switch them while no call is in flight) and the pool of idle device
 * allocations (hns_trim_memory; internally locked).
 *
 * Device operands: every DEVICE pointer a caller passes -- directly, or inside a `float* const*` list -- needs the alignment of its element type and no more: 4 bytes for
 * float / int32_t / uint32_t, 8 for hns_stats, int64_t and uint64_t, 1 for unsigned char (masks, status, hit, flags), and 4 for the `void*` rows of hns_point_order_gather /
 * _scatter and hns_point_population_compact whatever row_bytes is. So `xyz + 3` of an (n, 3) float array, `field + 1` and a status array sliced out of a larger one at any
 * byte are all legal operands, and RESULTS DO NOT DEPEND ON THE ALIGNMENT: a call gives the same bytes at a 4-, 8- or 12-byte start as at a 16-byte one (where a kernel has
 * a wider path for 16-byte aligned operands it picks it per pointer, from that pointer's own bits; tests/test_operand_layout_gpu.py). A pointer misaligned for its own
 * element type has no defined result. Unless a function says otherwise ("may alias", "in place"), no output may overlap an input or another output of the same call, in
 * whole or in part; where a function says "must not alias" the overlap is refused with HNS_ERR_INVALID_ARGUMENT before anything is launched, identical pointers and an
 * output that starts inside its input alike.
 *
 * There is no CPU fallback: without a usable HIP device every compute entry point fails with HNS_ERR_NO_DEVICE.
 */
#ifndef HNS_H
#define HNS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HNS_VERSION 100

/* Return codes. Negative = failure; hns_last_error() holds the message (thread-local). */
#define HNS_OK 0
#define HNS_ERR_INVALID_ARGUMENT (-1) /* the reference throws std::invalid_argument (HNanoSolver.cu:12-23) */
#define HNS_ERR_RUNTIME (-2)          /* the reference throws std::runtime_error  (HNanoSolver.cu:44,62,196; Advection.cu:20,28) */
#define HNS_ERR_HIP (-3)              /* a HIP runtime call failed (the reference's CUDA_CHECK, Utils.cuh:10-18) */
#define HNS_ERR_NO_DEVICE (-4)        /* no HIP device / host-only grid */
#define HNS_ERR_TOPOLOGY (-5)         /* coordinates are not leaf-dense 8^3 blocks, or a leaf appears twice */

const char* hns_last_error(void);
int hns_version(void);
int hns_device_count(void); /* 0 when no HIP device is visible; never initialises a device context */
/* Device memory of destroyed simulation state and grid tables is kept in a small process-wide pool (at most six idle
 * allocations; the device is idle when memory enters it) so that the next cook, typically on a slightly different
 * topology, does not pay hipMalloc/hipFree again; this returns it to the driver. */
int hns_trim_memory(void);
/* Alternative kernel forms and data-movement strategies, kept as cross-checks of the default ones and for A/B measurement (all of them produce the same bits:
 * tests/test_kernel_variants_gpu.py). Process-wide, read by every entry point when it is called. value = NULL restores the default. Fifteen names: the
 * twelve of round 6 below (the twenty-four of round 5 -- five more SOR forms among them -- are history: DESIGN_HISTORY.md, profiles/micro/exp/), "lookahead" (with
 * hns_sim_substep), "collide" and the test switch "arena_fill":
 *   "rbgs"          auto | color. auto: temporally blocked red-black SOR (hns_sorblock.hip: two iterations per launch on 16^3-voxel blocks, two or four on one-leaf
 *                   blocks for grids of up to 600 leaves). color: the reference's own decomposition, two launches per iteration in place -- the independent cross-check
 *   "sor_block_lb"  0 = by size | 1 | 2: block edge of the temporally blocked form in leaves, whatever the size of the grid (how the tests reach both kernels on every leaf set)
 *   "advect"        auto | generic (64-bit addressed advection kernels)
 *   "collide"       auto | generic. With a collision SDF, auto: advect_vector and advect_scalars run 32-bit addressed kernels that stage the SDF of the leaf and one
 *                   voxel around it in LDS, and hns_sim_substep / hns_compute_sim fuse as without one ("fuse"). generic: the 64-bit addressed kernels and the
 *                   reference's three launches -- the independent cross-check. hns_sim_substep_plan tells which a substep gets
 *   "stencil"       auto | block (512-thread divergence and gradient kernels)
 *   "divergence"    auto | row | coalesced | zpair: the divergence kernel fetches its own leaf row by row, or in memory order with a hand-over through LDS, or that with
 *                   two z-adjacent leaves per workgroup handing each other their common z face (auto: the last from 16,384 leaves, the first below)
 *   "schedule"      auto | linear (workgroup -> leaf order: one chunk of the leaf list per XCD, 128-leaf segments beyond 40,000 leaves | plain leaf order; takes
 *                   effect when a grid's launch tables are next built)
 *   "fuse"          1 | 0 (hns_sim_substep / hns_compute_sim: divergence + combustion_oxygen + temperature_buoyancy as ONE launch that leaves
 *                   {fuel, waste, temperature, flame} as one 16-byte element per voxel, which advect_scalars then gathers its taps from; 0 = the reference's three
 *                   launches over five float arrays)
 *   "cook_cache"    1 | 0 (operator calls keep their device buffers with the grid)
 *   "cook_pipeline" 1 | 0 (hns_compute_sim overlaps its transfers with the substep)
 *   "dist_mirror"   1 | 0 | guarded: over the ipc or local transport a rank whose owned range is swept in 16^3 blocks, created with sweeps_per_exchange = 2, runs the
 *                   CHAINED substep -- every kernel stores the voxels its peers read into their ghost voxels itself, no exchanges (read when the ranks connect; all
 *                   ranks must agree). 0 = the exchanged substep, which is what RCCL ranks run. guarded = one wave waits for the peers in front of every chained launch
 *                   instead of the boundary workgroups inside it (ranks sharing one GPU)
 *   "dist_unsplit"  1 | 0: a rank of the exchanged substep with up to 16,384 owned leaves runs the sweeps of its pressure loop, its divergence and its gradient subtraction
 *                   as ONE launch over all owned leaves with pack / transfer / unpack behind it on the compute stream; 0 = boundary leaves on a communication stream beside
 *                   the interior launch at every size (what larger ranks always do)
 *   "dist_wire_us"  N: the loopback transport of hns_dist holds every exchange N microseconds (emulated wire time)
 *   "arena_fill"    off | 0 .. 255 (a byte, in decimal): a TEST switch, no kernel form. Every block the pool of device memory (hns_trim_memory) hands out -- simulation states,
 *                   grid and SOR tables, regrid scratch, masks, the deactivation and diagnostics tables, the V-cycle's hierarchy; one taken from the pool or fresh from the driver -- is first filled
 *                   with that byte over its whole size. No result may depend on it: 255 makes the block NaN as floats, -1 as ints and all-set as masks; 127 makes it
 *                   3.39e38, for what lets a NaN lose (tests/test_pool_contents_gpu.py). The fill is a hipMemset followed by a wait for the WHOLE device on every draw:
 *                   never leave it on in production, and never have it on while a stream is capturing (the wait would break the capture). Default off: one atomic load
 *                   per draw. hns_get_option answers "off" or the byte in decimal */
int hns_set_option(const char* name, const char* value);
const char* hns_get_option(const char* name); /* current value as a word; NULL for an unknown name */

/* ------------------------------------------------------------------------------------------------------------ */
/* Index grid (topology)                                                                                         */
/* ------------------------------------------------------------------------------------------------------------ */

typedef struct hns_grid hns_grid;

#define HNS_GRID_DEFAULT 0u
#define HNS_GRID_HOST_ONLY 1u     /* build the host tables only (no device upload); compute calls then fail */
#define HNS_GRID_SKIP_VALIDATE 2u /* trust that coords are leaf-dense; only every 512th coordinate is read */

/* Replaces CreateIndexGrid. coords_xyz = n_voxels x 3 int32 (openvdb::Coord[n], GridData.hpp:95), leaf-dense: each
 * consecutive block of 512 is one 8^3 leaf in x<<6|y<<3|z order. The flat index of coords[i] is i by construction
 * (the reference relies on offset(coords[i]) == i+1, Kernel.cu:505 vs :511). */
hns_grid* hns_grid_create(const int32_t* coords_xyz, uint64_t n_voxels, float voxel_size, unsigned flags, int* err);
/* Same topology from the 8-aligned leaf origins alone (n_leaves x 3). */
hns_grid* hns_grid_create_from_leaves(const int32_t* leaf_origins_xyz, uint64_t n_leaves, float voxel_size, unsigned flags, int* err);
void hns_grid_destroy(hns_grid*);

uint64_t hns_grid_leaf_count(const hns_grid*);
uint64_t hns_grid_voxel_count(const hns_grid*);
float hns_grid_voxel_size(const hns_grid*);
/* Kernels update leaves [0, n_active) only; leaves [n_active, leaf_count) are ghosts that are read but never written
 * (multi-GPU halo leaves). Default n_active = leaf_count. */
int hns_grid_set_active_leaves(hns_grid*, uint64_t n_active);
/* The same for any contiguous range: kernels update leaves [first, first + count). The multi-GPU driver orders a rank's
 * leaves [boundary | interior | ghosts] and sweeps the boundary leaves first, so that their halo is on the wire while the
 * interior is being computed. */
int hns_grid_set_active_range(hns_grid*, uint64_t first, uint64_t count);
uint64_t hns_grid_active_leaves(const hns_grid*);
/* advect_scalars reads ELEMENT 0 of each array for taps outside the domain (reference Kernel.cu:133,192,225). On a
 * leaf-partitioned rank "element 0" of the global arrays lives at another local index (the ghost copy of global leaf 0):
 * this sets the flat element index those taps read. Default 0 = the reference's behaviour on an unpartitioned grid. */
int hns_grid_set_outside_element(hns_grid*, uint64_t element_index);
/* Host-side queries (work on HOST_ONLY grids): IndexOffsetSampler<0>::offset (Stencils.hpp:59-61): 1-based, 0 = outside. */
int hns_grid_offsets(const hns_grid*, const int32_t* ijk, uint64_t n, uint64_t* out);
/* 27-neighbour leaf table, n_leaves x 27 int32, entry (dx+1)*9+(dy+1)*3+(dz+1), -1 = absent. */
int hns_grid_neighbor_table(const hns_grid*, int32_t* out);
/* Writes the n_voxels x 3 coordinate array the grid represents (what the reference keeps as d_coords). */
int hns_grid_coords(const hns_grid*, int32_t* out_xyz);
/* 1 if `coords_xyz` lists exactly this grid's leaves in the same order (the grid, and the device state kept with it, can
 * serve the next cook), 0 if not, < 0 if the coordinates are not leaf-dense (same checks and flags as hns_grid_create). */
int hns_grid_matches(const hns_grid*, const int32_t* coords_xyz, uint64_t n_voxels, unsigned flags);
/* Operator calls (hns_compute_sim ... hns_divergence) keep their device buffers with the grid between calls, so a cook on
 * an unchanged topology allocates nothing; this frees them early (hns_grid_destroy does it too), and with them the accumulator
 * hns_dev_splat_points keeps with the grid. */
int hns_grid_release_cache(hns_grid*);
/* Serialises the grid as a NanoVDB NanoGrid<ValueOnIndex> buffer (32.7.0 layout), the format the reference keeps its index
 * grid in (create_index_grid, HNanoSolver.cu:375-384 -> nanovdb voxelsToGrid): same header, tree, node and leaf contents,
 * so NanoVDB accessors return offset(ijk) = hns_grid_offsets(ijk). *size_out receives the byte size; pass buffer = NULL
 * to query it. `buffer` must be 32-byte aligned host memory. Works on HOST_ONLY grids. */
int hns_grid_export_nanovdb(const hns_grid*, void* buffer, uint64_t capacity, uint64_t* size_out);
/* Copy of the device-built launch order (inspection / tests): sched = n_active leaf ids in workgroup order. */
int hns_grid_launch_tables(const hns_grid*, int32_t* sched);

/* ------------------------------------------------------------------------------------------------------------ */
/* Either side of the path, without OpenVDB (host code; PARITY UNPINNED: OpenVDB is absent from the build image).   */
/* What HNS::IndexGridBuilder (src/Utils/GridBuilder.hpp:87-216) and the domain dilation of the HNanoSolver SOP      */
/* (src/SOP/HNanoSolver/SOP_HNanoSolver.cpp:186-199) do to OpenVDB trees, over raw 8^3 leaf buffers: a leaf is its     */
/* 8-aligned origin, an optional 512-bit active mask (byte x*8+y, bit z) and 512 values in x<<6|y<<3|z order.          */
/* ------------------------------------------------------------------------------------------------------------ */

#define HNS_FILL_ZERO 0 /* float / Vec3f sources: a domain leaf the source lacks reads 0 (GridBuilder.hpp:125-129,147-151) */
#define HNS_FILL_SDF 1  /* SDF sources: filled with BYTES 0x01, i.e. 2.4e-38f, as memset(..., 1, ...) does (:108) */
/* IndexGridBuilder::build: out[i] = the source leaf at domain_origins[i] (512*ncomp floats), or the fill. Tiles of the
 * source are ignored, as in the reference (only leaves are probed). */
int hns_gather_leaves(const int32_t* domain_origins, uint64_t n_domain, const int32_t* src_origins, uint64_t n_src, const float* src_values, int ncomp, int fill,
                      float* out);
/* IndexGridBuilder::writeIndexGrid: every domain leaf receives all of its 512 values (:198-211). */
int hns_scatter_leaves(const float* flat, uint64_t n_domain, int ncomp, float* const* leaf_buffers);
/* dilateVoxels(padding, NN_FACE_EDGE_VERTEX, IGNORE_TILES) of a leaf set, as a leaf set in OpenVDB leaf order: every leaf
 * with an active voxel (active_masks: n x 64 bytes, NULL = all active) within `padding_voxels` of its box. out_origins may
 * be NULL to query *n_out. */
int hns_dilate_leaves(const int32_t* origins, uint64_t n, const unsigned char* active_masks, int padding_voxels, int32_t* out_origins, uint64_t capacity,
                      uint64_t* n_out);
/* hns_dilate_leaves plus the dilated ACTIVE MASKS (n_out x 64 bytes, same layout): what a host caller needs to chain frames, since frame n+1's
 * domain depends on them (with padding 1, seven frames in eight keep the same leaves only because the masks carry the partial ring). Every
 * leaf of the result holds the active voxels of the input dilated by the Chebyshev ball of radius padding_voxels (padding_voxels iterations of
 * 26-neighbour dilation, SOP_HNanoSolver.cpp:190-193), cropped to the leaf. Leaf set and order equal hns_dilate_leaves'. out_origins and
 * out_masks may be NULL to query *n_out. */
int hns_dilate_leaf_masks(const int32_t* origins, uint64_t n, const unsigned char* active_masks, int padding_voxels, int32_t* out_origins,
                          unsigned char* out_masks, uint64_t capacity, uint64_t* n_out);
/* topologyUnion of two leaf sets, in OpenVDB leaf order, duplicates removed. */
int hns_union_leaves(const int32_t* a, uint64_t na, const int32_t* b, uint64_t nb, int32_t* out_origins, uint64_t capacity, uint64_t* n_out);
/* openvdb::tools::compSum(a, b) over leaf sets (SOP_HNanoSolver.cpp:159-179): the union of the two leaf sets in OpenVDB leaf order (as
 * hns_union_leaves), masks ORed (NULL = all active), values fl(a + b) per component, where a side without the leaf contributes +0.0f -- so a -0.0f
 * on one side alone becomes +0.0f (compSum applies the sum to every voxel of both trees). ncomp 1 or 3. out_* may be NULL to query *n_out.
 * Unaligned or duplicated origins in either input: HNS_ERR_TOPOLOGY. */
int hns_add_leaves(const int32_t* a_origins, uint64_t na, const unsigned char* a_masks, const float* a_values, const int32_t* b_origins, uint64_t nb,
                   const unsigned char* b_masks, const float* b_values, int ncomp, int32_t* out_origins, unsigned char* out_masks, float* out_values,
                   uint64_t capacity, uint64_t* n_out);
/* One field whose values decide which voxels stay active (hns_sim_deactivate, hns_deactivate_leaf_masks). */
typedef struct {
	const char* name; /* a float field of the sim; with ncomp 3: the velocity (any name that is not a float field's) */
	int ncomp;        /* 1 or 3 */
	float tolerance;  /* >= 0, not NaN; +inf allowed */
} hns_activity_field;
/* Host mirror of hns_sim_deactivate over n_leaves leaves in the sim's (grid) order: masks_in n_leaves x 64 bytes or NULL = all active; values[i]
 * = 512 * fields[i].ncomp floats per leaf (Vec3f AoS for ncomp 3); masks_out n_leaves x 64 bytes (may be masks_in). A voxel stays active iff it
 * is active in masks_in and some component of some listed field has |x| > tolerance (NaN counts as above). counts (or NULL): {active voxels,
 * leaves holding one} of masks_out. Refusals as hns_sim_deactivate's that need no sim (HNS_ERR_INVALID_ARGUMENT, masks_out untouched); a float
 * entry needs a name, and two entries of one name are refused. */
int hns_deactivate_leaf_masks(uint64_t n_leaves, const unsigned char* masks_in, const hns_activity_field* fields, const float* const* values, int n_fields,
                              unsigned char* masks_out, uint64_t* counts);

/* ------------------------------------------------------------------------------------------------------------ */
/* Drop-in operators (host pointers in, results in place, synchronous)                                           */
/* ------------------------------------------------------------------------------------------------------------ */

typedef struct {
	const char* name; /* block name, e.g. "density", "vel", "collision_sdf" */
	int ncomp;        /* 1 = float block, 3 = Vec3f block (AoS) */
	float* host;      /* n_voxels * ncomp floats, caller-owned */
} hns_field;

typedef struct { /* CombustionParams, src/Cuda/Kernels.cuh:6-13 */
	float expansionRate, temperatureRelease, buoyancyStrength, ambientTemp, vorticityScale, factorScale;
} hns_combustion_params;

/* Compute_Sim: [collision] -> advect_vector -> vorticity -> divergence -> combustion -> buoyancy -> `iterations` x
 * (red, black) SOR sweeps -> gradient subtraction -> [collision] -> advect_scalars over every float block except
 * "collision_sdf". Requires exactly one ncomp==3 field, >=1 float field, and float fields named fuel, waste,
 * temperature, flame (HNanoSolver.cu:42-63,193-201). omega = 2/(1+sinf(3.14159f*voxel_size)) (:257). */
int hns_compute_sim(hns_grid*, hns_field* fields, int n_fields, int iterations, float dt, float voxel_size,
                    const hns_combustion_params* params, int has_collision, void* stream);
/* The same cook when the caller feeds the previous cook's output straight back in -- what the reference's SOP does with its first
 * input (src/SOP/HNanoSolver/SOP_HNanoSolver.cpp:106: the "feedback" VDBs of frame n are frame n+1's state). resident[i] != 0 says that
 * fields[i].host still holds, untouched, what the previous hns_compute_sim(_resident) on this grid handed back for the block of that name;
 * such a field is not uploaded again: the device buffer it was downloaded from still holds it (the cook cache keeps operator state with
 * the grid, "cook_cache"). Two strengths:
 *   resident[i] = 1  VOUCHED. The caller knows what it changed (the SOP adds its sources itself, SOP_HNanoSolver.cpp:159-179: a block it
 *                    sourced into must NOT be flagged). The library only trips on gross mistakes: a signature of the array (its size and
 *                    4,096 evenly spread elements) must match the one taken when it was handed back. A sparse edit that misses the samples
 *                    is NOT detected and that field would silently stay stale on the device.
 *   resident[i] = 2  CHECKED. A 64-bit digest of EVERY element must match as well: an edit is noticed and the field uploaded, except with probability ~2^-64 (a
 *                    digest, not a comparison: two different arrays can collide). The digest is
 *                    taken on the DEVICE when the field is handed back (of the buffer the array is downloaded from: the same bits, one pass at
 *                    memory speed beside the downloads) by a call that asked for it, and on the HOST, on up to 8 threads, when the array comes
 *                    in again (hns_digest.hpp: an order-independent sum over 16-byte pieces). Measured at 256^3: 14.8 ms per cook against 19.8
 *                    for the plain warm cook and 11.9 vouched (profiles/r05_final_cook256.json); the first cook that asks finds no digest to
 *                    compare with and uploads.
 * Either way the field is uploaded as usual when the check fails, when the topology changed, or when another operator used the state in
 * between. resident == NULL: hns_compute_sim. *uploads_skipped (may be NULL) receives the number of fields that stayed on the device.
 * Results are bit-identical to hns_compute_sim whenever the promise holds. */
int hns_compute_sim_resident(hns_grid*, hns_field* fields, int n_fields, const unsigned char* resident, int* uploads_skipped, int iterations, float dt,
                             float voxel_size, const hns_combustion_params* params, int has_collision, void* stream);
/* AdvectIndexGrid: every float field through the single-field BFECC arithmetic (advect_scalar), no collision; the fields share one back-trace
 * (hns_dev_advect_scalar_multi), bit-identical to one advect_scalar launch per field. */
int hns_advect_index_grid(hns_grid*, hns_field* fields, int n_fields, float dt, float voxel_size, void* stream);
/* AdvectIndexGridVelocity: BFECC self-advection of the one Vec3f field. */
int hns_advect_index_grid_velocity(hns_grid*, hns_field* fields, int n_fields, float dt, float voxel_size, void* stream);
/* ProjectNonDivergent: divergence -> iterations x (red, black) -> u -= grad p. omega uses double sin (PressureProjection.cu:53). */
int hns_project_non_divergent(hns_grid*, hns_field* fields, int n_fields, uint64_t iterations, float voxel_size, void* stream);
/* Divergence: writes the float field named "divergence" (PressureProjection.cu:91). */
int hns_divergence(hns_grid*, hns_field* fields, int n_fields, float voxel_size, void* stream);

/* ------------------------------------------------------------------------------------------------------------ */
/* Device-resident simulation state (upload once, many substeps; what bench.py and the multi-GPU driver use)      */
/* ------------------------------------------------------------------------------------------------------------ */

typedef struct hns_sim hns_sim;

/* Allocates velocity + the named float fields + scratch on the current device. Field order = insertion order. */
hns_sim* hns_sim_create(hns_grid*, const char* const* float_names, int n_float, int* err);
void hns_sim_destroy(hns_sim*);
int hns_sim_upload(hns_sim*, const hns_field* fields, int n_fields, void* stream);   /* matches fields by name; ncomp 3 = velocity */
int hns_sim_download(hns_sim*, hns_field* fields, int n_fields, void* stream);       /* synchronous */
/* One Compute_Sim substep entirely on the device (no H2D/D2H, no allocation, asynchronous on `stream`). */
int hns_sim_substep(hns_sim*, int iterations, float dt, float voxel_size, const hns_combustion_params*, int has_collision, void* stream);
/* The metric's core substep: advect_vector -> divergence -> iterations x RB-SOR -> gradient subtraction ->
 * advect_scalars over every float field (SURVEY.md 8d "core substep"); asynchronous on `stream`. */
int hns_sim_core_substep(hns_sim*, int iterations, float dt, float voxel_size, void* stream);
/* AdvectIndexGrid and AdvectIndexGridVelocity on the device (Advection.cu:76-91,148-155; no collision): the named float fields (n_names = -1: every
 * float field) through hns_dev_advect_scalar_multi with the sim's CURRENT velocity; then, with advect_velocity != 0, the velocity through
 * hns_dev_advect_vector -- so the fields see the velocity before its self-advection, the order in which the two operators chain. Bit-identical to
 * hns_advect_index_grid over those fields followed by hns_advect_index_grid_velocity. Asynchronous on `stream`, no device allocation. What a substep
 * looked ahead (below) is dropped, as by every call that rewrites a field. Refused before anything is launched (HNS_ERR_INVALID_ARGUMENT): a name the sim lacks, a name listed
 * twice, a null name or list, n_names < -1, a negative dt, a voxel size <= 0, a sim lent to a grid's cook cache. */
int hns_sim_advect(hns_sim*, const char* const* names, int n_names, int advect_velocity, float dt, float voxel_size, void* stream);
/* Sample the sim's own fields at n points and trace points through its velocity (hns_dev_sample_points / hns_dev_trace_points below, which state the positions, the
 * arithmetic and the refusals) without the fields leaving the device. names: float fields of the sim (n_names = -1: all of them, in insertion order; "collision_sdf"
 * counts as any float field), then, with with_velocity != 0, the velocity as the LAST output; out: HOST array of device pointers in that order, n floats each (3n for the
 * velocity). hns_sim_trace_points moves xyz in place through the sim's current velocity with inv_dx = 1.0f / voxel_size, as hns_sim_advect forms it. Both are
 * asynchronous on `stream`, allocate nothing and write no field: the look-ahead memo, the active masks, the feedback signatures of hns_compute_sim_resident and the
 * solve report stay as they are. Refused besides what the hns_dev_* calls refuse: n_names < -1, a name the sim lacks, a name listed twice, nothing to sample, a
 * voxel_size that is not a positive finite number, a sim lent to a grid's cook cache. Not mirrored in hns_dist_*: a partitioned sim has no point calls. */
int hns_sim_sample_points(hns_sim*, const char* const* names, int n_names, int with_velocity, const float* xyz, uint64_t n, float* const* out, void* stream);
int hns_sim_trace_points(hns_sim*, float* xyz, uint64_t n, float dt, float voxel_size, int order, int steps, unsigned char* status, void* stream);
/* Point values added into the sim's own fields (hns_dev_splat_points below, which states the positions, the arithmetic, status, d_rejected and the refusals) without
 * anything leaving the device: the point emitter as an alternative to the leaf sources of hns_sim_regrid_sourced. names: n_names >= 0 float fields of the sim, field
 * names[i] receives values[i] (HOST array of device pointers, n floats each); with velocity_values != NULL the velocity receives those 3n floats (Vec3f AoS). activate != 0 on
 * a sim that holds active masks sets (an integer atomic OR) the mask bit of every tap that landed with a weight w > 0, whether or not its terms were accepted; a sim with
 * NULL masks stays all-active; activate == 0 leaves the masks untouched. Asynchronous on `stream`. Writing the velocity drops the look-ahead memo, as every call that
 * rewrites the velocity does, and the feedback signatures of hns_compute_sim_resident of the written fields are cleared; the solve report and the pressure of the last solve
 * stay as they are. POINTS THAT LAND OUTSIDE THE DOMAIN CANNOT ADD LEAVES: their taps are dropped and `status` shows them (fewer than 8); a caller that wants them makes
 * room first: hns_sim_regrid_seeded is the device-side way (the points seed the next domain without leaving the device); their leaves as an empty velocity source of
 * hns_sim_regrid_sourced is the host-side one (it turns the velocity into a sum: every -0.0f becomes +0.0f). Refused before anything is launched (HNS_ERR_INVALID_ARGUMENT) besides what hns_dev_splat_points
 * refuses: n_names < 0, a name the sim lacks or one listed twice, collision_sdf as a target (it comes from the collision input), nothing to write (no names and
 * velocity_values NULL), a sim lent to a grid's cook cache. Not mirrored in hns_dist_*: a partitioned sim has no point calls. */
int hns_sim_splat_points(hns_sim*, const char* const* names, int n_names, const float* velocity_values, const float* xyz, const float* const* values, uint64_t n,
                         int log2_quantum, int activate, unsigned char* status, uint64_t* d_rejected, void* stream);
/* Only the pressure hot loop on the sim's divergence/pressure buffers (pressure zeroed first); asynchronous. */
int hns_sim_pressure_solve(hns_sim*, int iterations, float voxel_size, void* stream);
/* hipEvent timing of the pressure hot loop on its launch stream: after hns_sim_timing(sim, max_solves) every pressure
 * loop (up to max_solves) is bracketed by an event pair; hns_sim_pressure_time() returns the summed milliseconds and the
 * number of fused-iteration launches they contained. hns_sim_timing(sim, 0) switches it off. */
int hns_sim_timing(hns_sim*, int max_solves);
int hns_sim_pressure_time(hns_sim*, float* total_ms, long long* launches);
/* hns_sim_stage_timing(sim, n) brackets the five stages of the next n hns_sim_core_substep / hns_sim_substep calls (six events per substep;
 * a switch of its own because the events cost microseconds each on the launch stream); hns_sim_stage_times: ms5 receives the
 * summed milliseconds of {advect_vector, divergence, pressure loop, gradient subtraction, advect_scalars} over *substeps
 * (hns_sim_substep: {collision + advect_vector + vorticity, divergence + combustion + buoyancy, pressure loop, gradient + collision, advect_scalars}).
 * The brackets stay where they are under look-ahead (below): a substep that found its advect_vector done has a nearly empty first stage, and the last
 * stage of the substep before it carried both advections. Per-stage fractions of those two stages say nothing then; their sum does. */
int hns_sim_stage_timing(hns_sim*, int max_substeps);
int hns_sim_stage_times(hns_sim*, float* ms5, long long* substeps);
/* Look-ahead (option "lookahead" = auto | 0 | 1). advect_scalars of one substep and advect_vector of the next read the same velocity with the same dt
 * and make the same backtrace, so where a substep's advect_scalars is one launch of the 32-bit float-only form without a collision field, that launch
 * can compute the next substep's advect_vector as well (hns_dev_advect_scalars_ahead) and the next hns_sim_substep / hns_sim_core_substep called with the
 * same dt and voxel size on the same grid skips its own. Results are bit-identical to lookahead = 0. auto (default): only after a substep call with
 * the same dt and voxel size as the one before, so a lone substep or a changing dt pays nothing and a frame of K substeps wastes at most its last
 * look-ahead; 1: from the first substep; 0: never. What was looked ahead is dropped by everything else that writes the velocity: hns_sim_upload, the
 * regrids, hns_sim_deactivate, a collision substep. hns_sim_download and the timing calls keep it. A sim whose substep was captured into a graph, one
 * lent to the operator calls, and one whose hns_sim_velocity_ptr was taken never look ahead (again).
 * hns_sim_lookahead_counts: substeps of this sim that launched the look-ahead form / that skipped their advect_vector launch for it. */
int hns_sim_lookahead_counts(hns_sim*, long long* produced, long long* consumed);
/* Which kernel form each stage of the next hns_sim_substep (params NULL: hns_sim_core_substep) with these arguments would launch; launches nothing. The description is
 * space-separated `stage=kernel` words for the stages collision advect_vector vorticity divergence pressure gradient advect_scalars, a kernel by its source name with its
 * template flags (k_advect_scalars_n<q4,coll>; several launches of one stage joined by +). An absent stage reads `=-`, an advect_vector that the look-ahead has already
 * computed `=memo`. dt, voxel size and iteration count are taken to be those of the previous substep call on the sim (dt and voxel size decide the look-ahead, the count
 * what the pressure stage is planned for), the stream to be one that is not being captured. Decided by the code that launches; the query reads the sim and changes nothing in it. */
int hns_sim_substep_plan(hns_sim*, const hns_combustion_params* params /* NULL: core */, int has_collision, char* description, uint64_t description_bytes);
/* Raw device pointers of the sim's buffers (Vec3f AoS velocity, float fields, divergence, pressure). hns_sim_velocity_ptr hands out a WRITABLE pointer
 * the library cannot watch: calling it switches look-ahead off for this sim for good. */
float* hns_sim_velocity_ptr(hns_sim*);
float* hns_sim_field_ptr(hns_sim*, const char* name);
float* hns_sim_divergence_ptr(hns_sim*);
float* hns_sim_pressure_ptr(hns_sim*);

/* ------------------------------------------------------------------------------------------------------------ */
/* Regrid of a device-resident sim: the domain change between two cooks, on the device                         */
/* ------------------------------------------------------------------------------------------------------------ */

/* Each cook the reference rebuilds the domain (SOP_HNanoSolver.cpp:186-199): the velocity's active topology, dilateVoxels(padding,
 * NN_FACE_EDGE_VERTEX), united with the collision SDF's topology; padding has a hard minimum of 1 (:32-36) and the output grids keep the
 * dilated topology (GridBuilder.hpp:198-214 clones the domain's masks; the deactivate + pruneInactive after it, :213-214, is commented out), so
 * the domain grows by `padding` voxels a frame. hns_sim_deactivate is that step, turned on: it clears the mask bits of quiet voxels, so the
 * next regrid can drop the leaves no active voxel reaches.
 *
 * Active masks are sim state: leaf_count x 64 bytes, byte x*8+y, bit z (the hns_dilate_leaves layout). A new sim has every voxel active (NULL masks);
 * hns_sim_set_active_masks(sim, NULL, ...) returns to that. hns_sim_active_masks is synchronous. */
int hns_sim_set_active_masks(hns_sim*, const unsigned char* masks, void* stream);
int hns_sim_active_masks(hns_sim*, unsigned char* out, void* stream);
/* Moves the sim onto the next frame's domain D and returns it as a NEW grid the caller owns (same voxel size; device tables built by the usual
 * path). Synchronous. Only leaf origins and masks cross PCIe, plus the SDF source when one is given.
 *   D       = the leaves holding an active voxel of the masks dilated by the Chebyshev ball of radius padding_voxels (0..1024), united with the SDF
 *             source's leaves; OpenVDB leaf order. Equals hns_union_leaves(hns_dilate_leaves(L, M, p), S).
 *   masks   = the dilated masks, ORed with sdf_masks (NULL = all active) on the SDF's leaves: hns_dilate_leaf_masks, then the union.
 *   fields  = velocity and every float field: the old leaf's values where the leaf existed, zeros elsewhere (HNS_FILL_ZERO).
 *   collision_sdf  with a source (sdf_values != NULL: n_sdf leaves at sdf_origins, 512 floats each, host memory): gathered from it, bytes 0x01
 *             where it has no leaf (HNS_FILL_SDF); without one: carried like any other field, bytes 0x01 on new leaves. A source for a sim without
 *             that field is HNS_ERR_INVALID_ARGUMENT.
 * Afterwards the sim runs on the new grid; the old grid is untouched and still the caller's to destroy. Pointers from hns_sim_*_ptr are
 * invalidated, the divergence / pressure scratch holds no defined values and the feedback signatures of hns_compute_sim_resident are cleared.
 * Results are independent of atomic ordering: two runs, and the host chain, give the same bytes.
 * Refused, with the sim and its grid left exactly as they were: a sim lent to a grid's cook cache and a grid whose launch range is not the whole
 * grid (HNS_ERR_INVALID_ARGUMENT); SDF origins not 8-aligned or duplicated (HNS_ERR_TOPOLOGY); an empty result (HNS_ERR_RUNTIME, the SOP's "No
 * active voxels"). */
hns_grid* hns_sim_regrid(hns_sim*, int padding_voxels, const int32_t* sdf_origins, uint64_t n_sdf, const unsigned char* sdf_masks,
                         const float* sdf_values, void* stream, int* err);
/* hipEvent split of the sim's last regrid, milliseconds: {candidate leaves, origins to the host + sort + grid tables, masks, field copy}. */
int hns_sim_regrid_times(hns_sim*, float* ms4);
/* One source of hns_sim_regrid_sourced: the leaves a frame's emitter adds into a field (the SOP's second input). */
typedef struct {
	const char* name;            /* a float field of the sim; with ncomp 3: the velocity (any name that is not a float field's) */
	int ncomp;                   /* 1 or 3 */
	const int32_t* origins;      /* n_leaves x 3, 8-aligned, no duplicates, any order */
	uint64_t n_leaves;           /* at most 2^22 */
	const unsigned char* masks;  /* n_leaves x 64 bytes or NULL = all active; they enter the domain only for the velocity (as in the reference) */
	const float* values;         /* n_leaves x 512 x ncomp floats, host memory */
} hns_leaf_source;
/* hns_sim_regrid after adding this frame's sources into the sim's fields (SOP_HNanoSolver.cpp:159-179, then :186-199). The result is
 * byte-identical to this host chain:
 *   1. hns_sim_download and hns_sim_active_masks;
 *   2. per source, hns_add_leaves(sim field, source); for the velocity the masks are added too;
 *   3. hns_dilate_leaf_masks of the summed velocity's leaves and masks;
 *   4. the union with the SDF leaves and their masks, as hns_sim_regrid does;
 *   5. hns_gather_leaves of every field onto the new domain, fill 0 (HNS_FILL_SDF for collision_sdf).
 * So: a velocity source leaf outside the current domain is a dilation seed like an old leaf; a float source leaf outside the final domain is
 * dropped, as in the reference (the gather only visits domain leaves); a sourced field is a sum on every leaf (a -0.0f there becomes +0.0f, also
 * on leaves the source lacks); fields without a source are carried exactly as hns_sim_regrid carries them. With n_sources 0 this IS
 * hns_sim_regrid. Only the source leaves cross PCIe, never the sim's fields.
 * The reference pairs sources with feedback grids by POSITION (i-th float source into the i-th float feedback grid); a shim passes
 * feedback_float_grids[i]->getName() as the name of source i.
 * Refused, with the sim and its grid left exactly as they were (besides hns_sim_regrid's refusals): a name the sim lacks, collision_sdf as a
 * source (the SDF comes from the collision input, never from the feedback), a second velocity source or two sources of one name, ncomp other
 * than 1 or 3 or ncomp 3 under a float field's name, values (or origins) NULL with n_leaves > 0, more than 2^22 leaves (HNS_ERR_INVALID_ARGUMENT);
 * unaligned or duplicated origins in a source (HNS_ERR_TOPOLOGY). hns_sim_regrid_times counts the source work in the phase it runs in. */
hns_grid* hns_sim_regrid_sourced(hns_sim*, int padding_voxels, const hns_leaf_source* sources, int n_sources, const int32_t* sdf_origins, uint64_t n_sdf,
                                 const unsigned char* sdf_masks, const float* sdf_values, void* stream, int* err);
/* hns_sim_regrid_sourced that also makes room for a device-resident point set: before the dilation the velocity's topology -- the sim's leaves and active masks, united
 * with the velocity source's where one is given -- is united with the seed set S of the n_seeds points at d_seed_xyz (DEVICE memory, n x 3 floats, index space; S is
 * defined at hns_point_leaves below): leaves united, masks ORed. A sim with NULL masks counts as all-active on its own leaves only; on a leaf that S alone brings the
 * mask is S's. S ADDS NO VALUE TO ANY FIELD: every field holds what the unseeded call would have produced on its smaller domain (a subset of the seeded one, since
 * dilation distributes over the union), carried onto the larger one with the usual fills (zeros; bytes 0x01 for collision_sdf). In particular the velocity is a copy, not a
 * sum, when there is no velocity leaf source: its -0.0f stay. So the result equals the host chain of hns_sim_regrid_sourced with a zero-valued velocity source over S
 * merged in for the domain and the masks, and the fields of the unseeded chain gathered onto that domain. n_seeds == 0 IS hns_sim_regrid_sourced. Seeds are a dilation
 * source of their own: a sim whose masks are all cleared, with no SDF and no sources, restarts from points alone instead of refusing with "No active voxels".
 * Afterwards every tap of every seeding point lies inside the domain, so hns_sim_splat_points reports status 8 for it. S is built on the device (hns_seed.hip) and never
 * crosses PCIe; only its leaf count does. *seeds_skipped (host, or NULL) is SET to the number of points that do not seed. hns_sim_regrid_times counts the seed work
 * with the candidates.
 * Refused, with the sim and its grid left exactly as they were: everything hns_sim_regrid_sourced refuses; d_seed_xyz NULL with n_seeds > 0 and n_seeds above 2^31 - 1
 * (HNS_ERR_INVALID_ARGUMENT); more than 2^23 distinct seed leaves, and the 2^22-leaf limit of the new domain (HNS_ERR_TOPOLOGY). Not mirrored in hns_dist_*: a
 * partitioned sim has no point calls. */
hns_grid* hns_sim_regrid_seeded(hns_sim*, int padding_voxels, const hns_leaf_source* sources, int n_sources, const float* d_seed_xyz, uint64_t n_seeds,
                                uint64_t* seeds_skipped /* host or NULL */, const int32_t* sdf_origins, uint64_t n_sdf, const unsigned char* sdf_masks,
                                const float* sdf_values, void* stream, int* err);
/* The end of a frame, after its substeps and before the next regrid: clears the active-mask bit of every voxel whose listed fields are all
 * quiet. The reference has this step commented out (GridBuilder.hpp:213-214: deactivate(grid, 0, 0) + pruneInactive on each output grid).
 *   A voxel STAYS ACTIVE iff it is active now and at least one listed component is not within tolerance; x is within iff |x| <= tolerance.
 *   The velocity's three components are tested one by one. So bits are only ever cleared, field values are never touched, -0.0f is within any
 *   tolerance, NaN is never within (a blown-up voxel stays active), and +inf is a legal tolerance.
 * The velocity alone at tolerance 0 clears exactly the voxels whose three components are all +-0: as we read OpenVDB's Activate.h, a zero
 * tolerance compares value == zero, so this is the reference's commented-out deactivate(vel, 0, 0). That reading is UNVERIFIED (OpenVDB is absent
 * from the build image), and no match is claimed for tolerances above 0. The sim holds one mask, the velocity's topology, the only one that shapes
 * the domain (SOP_HNanoSolver.cpp:186-199); the reference's deactivate + prune of each float grid is not mirrored (there it would only turn the
 * -0.0f of all-zero float leaves into +0.0f).
 * Nothing else changes: substeps ignore the masks and the feedback signatures of hns_compute_sim_resident stay valid. The next hns_sim_regrid
 * (_sourced) dilates what is still active (plus the velocity source masks), so a leaf no active voxel reaches within `padding` is dropped with
 * ALL its values, listed fields or not, unless it is an SDF leaf: list every field whose values matter. With nothing active, no SDF leaf and no
 * velocity source, that regrid refuses (HNS_ERR_RUNTIME, "No active voxels") and the sim stays as it is; a later sourced regrid works from there.
 * A sim with NULL masks (all active) gets its masks from the pooled arena, as hns_sim_set_active_masks does.
 * counts NULL: asynchronous on stream. Else counts[0] = active voxels, counts[1] = leaves holding one, and the call is synchronous.
 * Refused, with the masks left exactly as they were (HNS_ERR_INVALID_ARGUMENT): n_fields < 1 or a NULL list, a name the sim lacks, collision_sdf
 * (its topology comes from the collision input), two entries for one field or two velocity entries, ncomp other than 1 or 3 or ncomp 3 under a
 * float field's name, a negative or NaN tolerance, a sim lent to a grid's cook cache. Host mirror: hns_deactivate_leaf_masks. */
int hns_sim_deactivate(hns_sim*, const hns_activity_field* fields, int n_fields, uint64_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------------------------ */
/* Diagnostics of a device-resident sim: field statistics, the pressure residual, a residual stop rule           */
/* (new: the reference computes no norm of anything). Nothing here writes a field value.                         */
/* ------------------------------------------------------------------------------------------------------------ */

/* One record per component of a field. NaN voxels are counted and take part in nothing else; +-inf are values like any other.
 * THE REDUCTION. sum and sum_sq are f64 sums of x and x*x (exact in f64 for an f32 x: only the additions round) in ONE fixed order, which is part
 * of the interface -- the device and the host mirror hns_leaf_stats give the same bytes, and so do two calls, whatever the launch geometry:
 *   inside a leaf  lane L (0..63) adds the terms of voxels 64k + L (voxel = x<<6|y<<3|z) for k = 0..7 ascending, ((t0 + t1) + t2) + ...; then the 64
 *                  lane sums go through the balanced tree over lane index (an xor butterfly over lanes 1, 2, 4, 8, 16, 32);
 *   over leaves    a balanced tree over leaf index padded with +0.0 up to the next power of two: at level s = 1, 2, 4, ... entry i + s is added
 *                  to entry i for every i that is a multiple of 2s (+0.0 where i + s is past the last leaf).
 * The term of an inactive voxel and of a NaN is +0.0. A sum that comes out NaN (+inf and -inf both present) is stored as 0x7FF8000000000000.
 * No float or double atomics anywhere: the order does not depend on how the kernels were scheduled. */
typedef struct {
	uint64_t count;      /* voxels looked at (the active ones, or all) */
	uint64_t nan_count;  /* of them NaN */
	float min, max;      /* over the rest, ordered -0 < +0; none left: +inf, -inf */
	float max_abs;       /* none left: +0 */
	uint32_t reserved;   /* 0 */
	double sum, sum_sq;  /* over the rest */
} hns_stats;
/* Host mirror, brute force and OpenVDB-free: n_leaves leaves of 512 x ncomp floats (Vec3f AoS for ncomp 3), masks n_leaves x 64 bytes (byte x*8+y,
 * bit z) or NULL = every voxel; out receives ncomp records. n_leaves 0 gives the record of nothing (count 0, min +inf, max -inf, sums +0).
 * HNS_ERR_INVALID_ARGUMENT, out untouched: ncomp other than 1 or 3, out NULL, values NULL with n_leaves > 0. */
int hns_leaf_stats(uint64_t n_leaves, const unsigned char* masks, const float* values, int ncomp, hns_stats* out);
/* One field of hns_sim_stats, addressed as in hns_activity_field. */
typedef struct {
	const char* name; /* a float field of the sim; with ncomp 3: the velocity (any name that is not a float field's) */
	int ncomp;        /* 1 or 3 */
} hns_stats_field;
/* Statistics of the listed fields of a sim as the device holds them now, one record per component in list order (the velocity gives three, so a
 * caller forms the back-trace length dt * max(max_abs) / dx itself). use_masks != 0: over the voxels of the sim's active masks (NULL masks = every
 * voxel); 0: over every voxel. Synchronous. Equal in every byte to hns_leaf_stats of the downloaded fields (and masks). One wave per leaf reads the
 * fields; its partial records go into a table from the arena pool (made on first use, kept with the sim) that a second small launch folds.
 * Field values, masks, the feedback signatures of hns_compute_sim_resident and the look-ahead memo are untouched.
 * Refused with out untouched (HNS_ERR_INVALID_ARGUMENT): n_fields < 1 or a NULL list, a name the sim lacks, two entries for one field or two
 * velocity entries, ncomp other than 1 or 3 or ncomp 3 under a float field's name, a sim lent to a grid's cook cache. */
int hns_sim_stats(hns_sim*, const hns_stats_field* names, int n_fields, int use_masks, hns_stats* out, void* stream);
/* The Gauss-Seidel correction of the last pressure solve on this sim, per voxel (see hns_dev_residual), as one record over the leaves of the grid's
 * launch range. voxel_size: the one the solve ran with. Synchronous. HNS_ERR_RUNTIME when no solve has run on this sim's grid since the sim was
 * created or regridded (the pressure buffer holds no defined values then); HNS_ERR_INVALID_ARGUMENT for a sim lent to a grid's cook cache. */
int hns_sim_residual(hns_sim*, float voxel_size, hns_stats* out, void* stream);
/* A stop rule for the pressure solve of hns_sim_pressure_solve, hns_sim_substep and hns_sim_core_substep: with a control set, their `iterations` is
 * the MAXIMUM. The residual (hns_dev_residual's record) is taken at p = 0 (`initial`), after every check_every iterations and at the maximum; the
 * loop ends at the FIRST check where nan_count == 0 and max_abs <= max(abs_tol, rel_tol * initial.max_abs) -- the first crossing, not the last: the
 * norm does not fall monotonically. A solve that carries NaN runs to the maximum and reports converged = 0. rel_tol = abs_tol = 0 only monitors:
 * the loop never stops early and converged stays 0. Whatever number of iterations ran, pressure and every field equal, bit for bit, the
 * uncontrolled call with that number.
 * check_every >= 1; even values fit the kernels, which do two (small grids: four) iterations per launch -- an odd value costs an extra launch per
 * check. The host waits once per check for a few bytes in pinned memory, so a controlled call is refused on a capturing stream
 * (HNS_ERR_INVALID_ARGUMENT, nothing launched). hns_sim_timing counts the iterations that ran; the residual launches fall inside its brackets.
 * NULL switches the control off (the default): bit for bit and launch for launch the calls above without one. The drop-in operators and the sims
 * of a grid's cook cache never use a control; hns_dist_* has none (its residual would need an all-reduce over the ranks).
 * HNS_ERR_INVALID_ARGUMENT: a negative or NaN tolerance, check_every < 1, a sim lent to a grid's cook cache. */
typedef struct {
	float rel_tol, abs_tol;
	int check_every;
} hns_solve_control;
int hns_sim_set_solve_control(hns_sim*, const hns_solve_control*);
/* What the last controlled solve of this sim did: iterations run, checks taken (the one at p = 0 not counted), converged, the residual at p = 0 and
 * at the end; history (or NULL) receives the first min(checks, capacity) records of the checks in order, *n_history (or NULL) = checks.
 * HNS_ERR_RUNTIME when no controlled solve has run on this sim. */
typedef struct {
	int iterations, checks, converged;
	hns_stats initial, final;
} hns_solve_report;
int hns_sim_solve_report(hns_sim*, hns_solve_report*, hns_stats* history, int capacity, int* n_history);

/* ------------------------------------------------------------------------------------------------------------ */
/* A second solve method: geometric multigrid V-cycles on the leaf-sparse grid (new: the reference has SOR only)  */
/* ------------------------------------------------------------------------------------------------------------ */

/* Selected per sim, off by default: a sim that never sets a method runs the SOR loop bit for bit and launch for launch as before (one more pointer test). With method 1 set,
 * the `iterations` argument of hns_sim_pressure_solve, hns_sim_substep and hns_sim_core_substep is the number of V-CYCLES; under a solve control it is their maximum,
 * check_every counts cycles and hns_solve_report.iterations reports cycles. hns_sim_timing counts cycles, hns_sim_residual works after a V-cycle solve, and
 * hns_sim_substep_plan words the pressure stage `vcycle<pre,post,coarse_iterations>/L<levels>:<fine kernel>+k_mg_restrict+k_mg_color+k_mg_prolong`. omega is explicit: the
 * reference's 2 / (1 + sin(pi * voxel_size)) means nothing on a level with a doubled voxel size. The setter does its device work (the hierarchy) on a private stream it waits
 * for; the solves stay asynchronous on their own streams and allocate nothing. NULL, or method 0 (its other members are not looked at): back to SOR.
 *
 * THE HIERARCHY, per grid topology; a regrid drops it and the next solve (or hns_sim_solve_levels) builds it again -- which is refused on a capturing stream
 * (HNS_ERR_INVALID_ARGUMENT, nothing launched), as a controlled solve is.
 *   Level 0       the sim's grid; every voxel of every leaf is an unknown, as in the SOR.
 *   Level l + 1   voxel size doubled; coarse voxel I = i >> 1 per axis on global coordinates (a floor: negative coordinates work). Its leaves are the distinct
 *                 floor(origin / 16) * 8 of the level below. A coarse voxel is an UNKNOWN iff at least one of its eight children is an unknown of the level below (exact
 *                 masks, 64 bytes per leaf, byte x*8+y, bit z); every other voxel of a coarse leaf holds +0 and is never updated. Without the masks the cycle diverges on
 *                 ragged leaf sets (DESIGN_HISTORY.md).
 *   Depth         levels end at one leaf, at max_levels, or where the next level would have no fewer leaves than this one (leaves either side of coordinate 0 never merge:
 *                 floor keeps origins -8 and 0 apart; isolated far tiles do not merge either). A hierarchy of one level is `coarse_iterations` plain sweeps per cycle.
 *
 * THE ARITHMETIC: single rounded f32 operations, unfused; dx of level l + 1 is 2.0f * dx of level l, dx2 = dx * dx.
 *   Sweep         the red-black update of Kernel.cu:621-622 with the method's omega, on unknowns only; level 0 through hns_dev_rbgs_iterate's kernels.
 *   Residual      c = hns_dev_residual's correction of the level's p against its right-hand side (level 0: the divergence); +0 at a voxel that is not an unknown.
 *   Restriction   rhs_c[I] = (((c000 + c001) + (c010 + c011)) + ((c100 + c101) + (c110 + c111))) * k, children indexed dx dy dz, a child in an absent leaf reads +0,
 *                 k = -0.75f / dx2 of the FINE level: the mean of the children's residual in divergence units, -6 c / dx^2.
 *   Coarse solve  from e = 0, the sweep above with rhs_c and the coarse dx2.
 *   Prolongation  cell-centred trilinear: per axis the second coarse voxel is I + ((i & 1) ? 1 : -1); v = 0.75f * a + 0.25f * b (two multiplies, then an add) with a the value
 *                 at I's side, nested z, then y, then x; a coarse voxel that is absent or masked reads 0. Then p[i] = p[i] + v on unknowns only.
 *   One cycle on level l: `pre` sweeps; residual and restriction; the cycle on level l + 1 -- on the coarsest level `coarse_iterations` sweeps instead of all this --;
 *                 prolongation and add; `post` sweeps. The first cycle of a solve starts from p = 0.
 * The drop-in operators and the sims of a grid's cook cache never use a method; hns_dist_* has none.
 * HNS_ERR_INVALID_ARGUMENT, sim unchanged: a method other than 0 or 1, pre or post < 0 or both 0, coarse_iterations < 1, max_levels < 0, an omega that is not a finite
 * number strictly between 0 and 2, a grid whose launch range is not the whole grid, a sim lent to a grid's cook cache. */
typedef struct {
	int method;            /* 0 = SOR (default), 1 = V-cycle */
	int pre, post;         /* red-black iterations before / after the coarse correction on every level, >= 0, pre + post >= 1 */
	int coarse_iterations; /* iterations on the coarsest level, >= 1 */
	int max_levels;        /* 0 = as deep as the rule above goes; else at most this many levels, level 0 included */
	float omega;           /* relaxation factor of every sweep, 0 < omega < 2 */
} hns_solve_method;
int hns_sim_set_solve_method(hns_sim*, const hns_solve_method*);
/* The hierarchy's depth and (leaves_per_level != NULL) the leaf count of its first min(capacity, *n_levels) levels, level 0 first. Builds the hierarchy when a regrid
 * dropped it (synchronous then). HNS_ERR_RUNTIME when no method is set. */
int hns_sim_solve_levels(hns_sim*, int* n_levels, uint64_t* leaves_per_level, int capacity);

/* ------------------------------------------------------------------------------------------------------------ */
/* Kernel-level entry points on caller-owned DEVICE memory (asynchronous on `stream`).                           */
/* Velocity fields are Vec3f AoS on the device too (3 floats per voxel, `vel3`), exactly the host/reference layout.  */
/* ------------------------------------------------------------------------------------------------------------ */

/* advect_vector (Kernel.cu:354-453); out3 must not alias vel3: any overlap of the two fields is refused (HNS_ERR_INVALID_ARGUMENT, nothing launched) */
int hns_dev_advect_vector(hns_grid*, const float* vel3, float* out3, const float* sdf, int has_collision, float dt, float inv_dx, void* stream);
/* advect_scalar (Kernel.cu:269-352) */
int hns_dev_advect_scalar(hns_grid*, const float* vel3, const float* in, float* out, const float* sdf, int has_collision, float dt, float inv_dx,
                          void* stream);
/* advect_scalars (Kernel.cu:118-266); in/out are HOST arrays of n device pointers */
int hns_dev_advect_scalars(hns_grid*, const float* vel3, const float* const* in, float* const* out, int n, const float* sdf, int has_collision,
                           float dt, float inv_dx, void* stream);
/* advect_scalar over n >= 0 fields with ONE back-trace (in/out: HOST arrays of n device pointers): output i is bit-identical to hns_dev_advect_scalar of
 * field i with these arguments, whatever the options. Where the 32-bit addressed kernels apply (no collision field, a Vec3f field below 4 GiB, option
 * "advect" = auto) eight fields share a launch and with it the own-velocity load, the neighbour tables, both sets of tap offsets and the velocity gathers;
 * elsewhere one advect_scalar launch per field. Refused before anything is launched (HNS_ERR_INVALID_ARGUMENT, the first offending field's index in the
 * message): a null pointer, an out[i] that overlaps any in[j] or vel3, two out fields that overlap. The same in listed twice is allowed. */
int hns_dev_advect_scalar_multi(hns_grid*, const float* vel3, const float* const* in, float* const* out, int n, const float* sdf, int has_collision,
                                float dt, float inv_dx, void* stream);
/* advect_scalars over n <= 8 fields without a collision field AND advect_vector(vel3) into adv_out3 (not aliasing vel3: any overlap of the two is refused with HNS_ERR_INVALID_ARGUMENT), one launch: every output is
 * bit-identical to hns_dev_advect_scalars followed by hns_dev_advect_vector with these arguments. Applies where the 32-bit addressed kernels do
 * (a Vec3f field below 4 GiB, option "advect" = auto); HNS_ERR_INVALID_ARGUMENT elsewhere. */
int hns_dev_advect_scalars_ahead(hns_grid*, const float* vel3, const float* const* in, float* const* out, int n, float* adv_out3, float dt, float inv_dx,
                                 void* stream);
/* Fields at points: the trilinear samplers of the advection kernels (IndexSampler<float,1> and, on its device branch, IndexSampler<Vec3f,1>: Stencils.hpp:96-173) at n
 * arbitrary positions. xyz: n x 3 floats (AoS, device) in INDEX space -- voxel (i, j, k) has its sample at position (i, j, k), as the reference's samplers and the
 * advection kernels' back-traced positions have it; a caller with world positions divides by the voxel size itself, so that positions round in one known place. The cell is
 * Floor(xyz) (Stencils.hpp:25-43) with the GPU's float -> int conversion (saturating, NaN -> 0), a tap whose leaf is absent reads 0, and every leaf of the grid is readable
 * whatever its launch range (ghost leaves included). fields[i]: device pointer, ncomp[i] 1 (float) or 3 (Vec3f AoS); out[i]: device, n x ncomp[i] floats; fields, ncomp and
 * out are HOST arrays of n_fields entries. Up to eight fields share a launch and with it the cell, the tap indices and the fractions; output i is bit-identical to a call with
 * field i alone, float results to the reference's sampler. Asynchronous on `stream`, no device allocation; n == 0 launches nothing and looks at no device pointer (an empty array's may be null). Refused before anything is launched
 * (HNS_ERR_INVALID_ARGUMENT, the call and the argument in the message), outputs untouched: n_fields < 1, a null list or entry, a null xyz, an ncomp other than 1 or 3, an
 * out[i] equal to another out[j], to xyz or to a field, n above 2^31 - 1. */
int hns_dev_sample_points(hns_grid*, const float* const* fields, const int* ncomp, int n_fields, const float* xyz, uint64_t n, float* const* out, void* stream);
/* Points through the velocity: `steps` steps of xyz (n x 3, index space, updated in place) in one launch, with U(x) the Vec3f sample above, s = dt * inv_dx, h = 0.5f * s,
 * s6 = s * 0.16666667f, every operation one rounded float32 operation per component and every a + c*b a multiply, then an add:
 *   order 1  x' = x + s*U(x)
 *   order 2  k1 = U(x); x' = x + s*U(x + h*k1)
 *   order 4  k1 = U(x); k2 = U(x + h*k1); k3 = U(x + h*k2); k4 = U(x + s*k3); x' = x + s6*(((k1 + 2.0f*k2) + 2.0f*k3) + k4)
 * dt may be negative (a back-trace). A point with no leaf under any tap samples U = 0 and stays where it is. status: NULL, or n bytes (device): 1 iff the final position
 * is finite in all three components and the leaf of its cell exists, else 0. Asynchronous on `stream`, no device allocation; n == 0 launches nothing. Refused before
 * anything is launched (HNS_ERR_INVALID_ARGUMENT), positions and status untouched: a null xyz or vel3, an order not in {1, 2, 4}, steps < 1, a NaN dt, an inv_dx that is
 * not a positive finite number, n above 2^31 - 1, xyz, status and vel3 not three different buffers. Neither call is mirrored in hns_dist_*. */
int hns_dev_trace_points(hns_grid*, const float* vel3, float* xyz, uint64_t n, float dt, float inv_dx, int order, int steps, unsigned char* status, void* stream);
/* Points through the velocity against a collision SDF: hns_dev_trace_points with the SDF tested after every step, inside the same launch. sdf: a float field of the grid
 * (device), only read. Every line below is one rounded float32 operation per component, none contracted.
 *   Samplers S(x) is the float sample of hns_dev_sample_points on sdf (IndexSampler<float,1>, the unfused lerp, an absent tap reads 0); U the Vec3f sample; RK(x) one step
 *            of hns_dev_trace_points at `order`, with exactly its operations. A position x is IN COLLISION iff S(x) < threshold (0.0f: the reference's
 *            isInCollision(.., 0.0f)); a NaN sample is no collision.
 *   Start    bit 3 (value 8) of hit is set iff S(x_start) < threshold.
 *   Step     for a point that is not dead: x0 = x; x1 = RK(x0); d = S(x1). If !(d < threshold), x = x1. Otherwise by mode:
 *   STOP     x = x0; hit |= 2 (the reference's rule for a back-trace that lands in the collider, Kernel.cu:144-147).
 *   KILL     x = x1; the point is dead and takes no further step; hit |= 4.
 *   PUSH     hit |= 1; then up to `iterations` times while d < threshold:
 *              nb = S(x1 -+ e_axis) in the order -x, +x, -y, +y, -z, +z, each position formed as x1.c - 1.0f or x1.c + 1.0f, each a full sample with its own Floor;
 *              n  = the normalised central difference of hns_dev_enforce_collision_boundaries: g.c = (0.5f * inv_dx) * (nb[+c] - nb[-c]),
 *                   len = sqrtf((g.x*g.x + g.y*g.y) + g.z*g.z), n.c = (1.0f / len) * g.c if len > 1e-6f, else n = 0;
 *              a  = (threshold - d) * inv_dx; a = a + skin;
 *              x1.c = x1.c + a * n.c (a multiply, then an add); d = S(x1).
 *            After the loop: if still d < threshold, x = x0 and hit |= 2; otherwise x = x1.
 *   Outputs  status: NULL, or n bytes: 1 iff the point is not dead, its final position is finite in all three components and the leaf of its cell exists (the rule of
 *            hns_dev_trace_points, a dead point counting as outside: hns_point_population_select with at_least = 1 drops it). hit: NULL, or n bytes: the OR of the bits
 *            above over all steps; 0 for a point that never touched anything.
 * skin is an index-space distance added to every push; iterations (1 .. 8) is read by PUSH only but must be in range in every mode. Caveat: a leaf that the source of an
 * SDF lacks holds 2.4e-38f in reference-style data, and a tap outside the domain reads 0, so only threshold <= 0 is meaningful there; a positive threshold is allowed and
 * flags such places. Asynchronous on `stream`, no device allocation; n == 0 launches nothing and looks at no device pointer (the numbers and the spec, a host struct, are checked whatever n); on a grid with no leaves status and hit are set to 0
 * and nothing moves. Refused before anything is launched (HNS_ERR_INVALID_ARGUMENT, the call and the argument in the message), positions, status and hit untouched:
 * everything hns_dev_trace_points refuses, a null spec, a mode outside 1 .. 3, a threshold that is NaN or infinite, a skin that is NaN, infinite or negative, iterations
 * outside 1 .. 8, a null sdf, any two of xyz, vel3, sdf, status and hit being the same buffer. Not mirrored in hns_dist_*. */
#define HNS_COLLIDE_STOP 1
#define HNS_COLLIDE_PUSH 2
#define HNS_COLLIDE_KILL 3
typedef struct hns_point_collision {
	int mode;        /* HNS_COLLIDE_*: 1 .. 3 */
	float threshold; /* finite; a position is in collision iff S(x) < threshold */
	float skin;      /* finite, >= 0; index-space distance added to every push */
	int iterations;  /* 1 .. 8 pushes per step (PUSH only; the other modes ignore it but it must still be in range) */
} hns_point_collision;
int hns_dev_trace_points_collide(hns_grid*, const float* vel3, const float* sdf, float* xyz, uint64_t n, float dt, float inv_dx, int order, int steps,
                                 const hns_point_collision*, unsigned char* status, unsigned char* hit, void* stream);
/* The same on a sim's own buffers: its current velocity and its float field "collision_sdf", with inv_dx = 1.0f / voxel_size as hns_sim_trace_points forms it. The sim is
 * only read: the look-ahead memo, the active masks, the feedback signatures and the solve report stay as they are. Refused besides the above: a sim without a float field
 * "collision_sdf", a voxel_size that is not a positive finite number, a sim lent to a grid's cook cache. Not mirrored in hns_dist_*. */
int hns_sim_trace_points_collide(hns_sim*, float* xyz, uint64_t n, float dt, float voxel_size, int order, int steps,
                                 const hns_point_collision*, unsigned char* status, unsigned char* hit, void* stream);
/* POINTS WITH A VELOCITY OF THEIR OWN: embers, sparks, soot, debris. Where the traces above move a massless tracer (x' = U(x)), a point here carries a velocity and an
 * age: it is dragged towards the gas, falls, moves with its own velocity, and a step that lands in the collider sticks, bounces or kills it. hns_point_motion is an
 * object that OWNS the per-point arrays and hands device pointers out, as hns_point_order_get does; it reads the fluid from a hns_sim. No call here takes a caller's
 * data pointer: the arrays are carved from the library's pool and have the pool's alignment.
 *   Object   create draws ONE block of the pool of device memory on the current HIP device and carves five disjoint arrays of `capacity` rows from it: xyz (12 bytes a
 *            row), vel (12), age (4), status (1), hit (1); destroy returns the block. The object is bound to no grid: step uses the grid the sim has at that call, so the
 *            object survives regrids. hns_point_motion_get fills the info with the DEVICE pointers; it waits for nothing, and the pointers are valid until destroy. The
 *            caller fills xyz, vel and age through them (hns_point_population_birth may write xyz directly, hns_point_order_sort may read it). Before the first step
 *            status and hit hold whatever the pool held; nothing reads them. step allocates nothing and is asynchronous on the object's stream: the null stream until
 *            hns_point_motion_set_stream binds another.
 *   Units    positions are in index space (as for hns_dev_sample_points); vel is in the units of the sim's velocity.
 * The arithmetic of hns_point_motion_step. Every line below is one rounded float32 operation per component, none contracted.
 *   Host constants, formed in float32 on the host once per call: inv_dx = 1.0f / voxel_size; s = dt * inv_dx; k = drag * dt; r = 1.0f / (1.0f + k);
 *            gd.c = dt * gravity.c; ft = 1.0f - friction.
 *   Samplers U is the Vec3f sample of the sim's current velocity and S the float sample of its float field "collision_sdf": exactly the samplers of
 *            hns_dev_trace_points_collide. S is not evaluated at all in mode FREE.
 *   Rows     only rows 0 .. n - 1 are read or written.
 *   Skip     a row with a non-finite component of xyz is not stepped: its xyz, vel and age keep every bit, its status is 0 and its hit is 0 (the convention of
 *            hns_point_population_birth for the rows beyond the live count).
 *   Start    bit 3 (value 8) of hit is set iff S(x_start) < threshold; it is never set in mode FREE.
 *   Step     `steps` times, for a row that is not dead:
 *              1. x0 = x; u = U(x0).
 *              2. drag, implicit Euler: t.c = k * u.c; t.c = v.c + t.c; v.c = t.c * r.
 *              3. gravity: v.c = v.c + gd.c.
 *              4. move: m.c = s * v.c; x1.c = x0.c + m.c.
 *              5. age = age + dt.
 *              6. in mode FREE, x = x1 and the step ends here.
 *              7. otherwise d = S(x1). If !(d < threshold), a NaN included, then x = x1. Else the mode decides:
 *   STICK    x = x0; v = +0.0f in every component; hit |= 2.
 *   KILL     x = x1; the row is dead and takes no further step; hit |= 4.
 *   BOUNCE   hit |= 1; then up to `iterations` times while d < threshold:
 *              nb and n exactly as PUSH of hns_dev_trace_points_collide takes them: six samples at x1 -+ e_axis in the order -x, +x, -y, +y, -z, +z, and the normalised
 *                   central difference of hns_dev_enforce_collision_boundaries; n = 0 when len <= 1e-6f;
 *              on the first iteration only, reflect the velocity: vn = (v.x*n.x + v.y*n.y) + v.z*n.z; if vn < 0: w.c = vn * n.c; vt.c = v.c - w.c; a = restitution * vn;
 *                   p.c = ft * vt.c; q.c = a * n.c; v.c = p.c - q.c; hit |= 16;
 *              then PUSH's move: a = (threshold - d) * inv_dx; a = a + skin; x1.c = x1.c + a * n.c (a multiply, then an add); d = S(x1).
 *            After the loop: if still d < threshold, x = x0 and hit |= 2 -- the reflected velocity stays --; otherwise x = x1.
 *   Outputs  status is 1 iff the row is not dead, x is finite in all three components, the leaf of its cell exists, and age < max_age (a NaN age gives 0); hit is the
 *            OR of the bits above over all steps. hns_point_population_select(status, at_least = 1) therefore drops the dead, the escaped and the expired. x, v and age
 *            are written once, after the last step.
 *   No leaves  on a grid with no leaves U = 0 and S = 0, and no leaf exists: rows still fall under gravity, and every status is 0.
 * Refused before anything is launched and with nothing touched (HNS_ERR_INVALID_ARGUMENT, the call and the argument in the message) -- the numbers and the spec, a host
 * struct, first and whatever n, then the objects --: a null spec, n above 2^31 - 1, steps < 1, a NaN dt, a voxel_size that is not a positive finite number, a mode
 * outside 0 .. 3, a non-finite gravity component, a drag that is NaN, infinite or negative, a restitution or friction outside [0, 1] or NaN, a max_age that is NaN or
 * <= 0 (+inf is allowed: no point expires), a threshold that is not finite, a skin that is NaN, infinite or negative, iterations outside 1 .. 8 (read by BOUNCE only but
 * checked in every mode); a null object, n > capacity, a null sim (HNS_ERR_NO_DEVICE where there is no device), a sim lent to a grid's cook cache, a mode other than
 * FREE on a sim without a float field "collision_sdf"; create: a capacity above 2^31 - 1, and HNS_ERR_NO_DEVICE without a HIP device; get: a null object or info.
 * n == 0 launches nothing. The sim is only read: the look-ahead memo, the active masks, the feedback signatures and the solve report stay as they are. Not mirrored in
 * hns_dist_*, and there is no host mirror: the Python tests restate the text above in numpy. */
typedef struct hns_point_motion hns_point_motion;
hns_point_motion* hns_point_motion_create(uint64_t capacity, int* err);
void hns_point_motion_destroy(hns_point_motion*);
int hns_point_motion_set_stream(hns_point_motion*, void* hip_stream);
typedef struct hns_point_motion_info {
	uint64_t capacity;
	float* xyz;            /* DEVICE pointers handed out: capacity x 3 floats */
	float* vel;            /* capacity x 3 floats */
	float* age;            /* capacity floats */
	unsigned char* status; /* capacity bytes */
	unsigned char* hit;    /* capacity bytes */
} hns_point_motion_info;
int hns_point_motion_get(hns_point_motion*, hns_point_motion_info*);
#define HNS_MOTION_FREE 0 /* no collider looked at; the sim needs no collision_sdf */
#define HNS_MOTION_STICK 1
#define HNS_MOTION_BOUNCE 2
#define HNS_MOTION_KILL 3
typedef struct hns_point_motion_spec {
	int mode;         /* HNS_MOTION_*: 0 .. 3 */
	float gravity[3]; /* finite; units of the sim's velocity per unit of time */
	float drag;       /* finite, >= 0; 1 / the time in which a point takes up the gas's velocity */
	float restitution; /* 0 .. 1: the share of the normal speed a bounce gives back */
	float friction;   /* 0 .. 1: the share of the tangential velocity a bounce takes */
	float max_age;    /* > 0, +inf allowed: status is 0 from this age on */
	float threshold;  /* finite; a position is in collision iff S(x) < threshold */
	float skin;       /* finite, >= 0; index-space distance added to every push */
	int iterations;   /* 1 .. 8 pushes per bounced step */
} hns_point_motion_spec;
int hns_point_motion_step(hns_point_motion*, hns_sim*, uint64_t n, float dt, float voxel_size, int steps, const hns_point_motion_spec*);
/* SHAPING A SIM: curl-noise turbulence and field decay, the two operators a device-resident sim needs to be shaped without leaving the GPU. Turbulence adds a
 * divergence-free force to the velocity -- the curl of a three-channel gradient-noise potential, summed over octaves, optionally weighted by a control field --, which the
 * projection does not remove; decay relaxes float fields implicitly towards a target (smoke thins out, temperature cools to ambient). Both run in ONE launch over the
 * sim's leaves, in place. hns_shaping is an object that only holds the stream the launch goes to; the sim is an argument. No call here takes a caller's data pointer.
 *   Object   create allocates no device memory (HNS_ERR_NO_DEVICE without a HIP device); the null stream until hns_shaping_set_stream binds another.
 *   apply    asynchronous on the object's stream; allocates nothing. It updates all 512 voxels of the leaves in the grid's launch range [first, first + n_active), as
 *            the substep's pointwise stages do, whatever the active masks say, and writes nothing else: no other leaf, no other field, not the advected velocity, the
 *            pressure or the divergence, not the masks. When the velocity is written the sim forgets what it knew of it (the look-ahead memo and the velocity's feedback
 *            signature are dropped, as by hns_sim_splat_points); of a decayed field its signature alone -- the memo is a function of the velocity and of collision_sdf, which
 *            is why that field may not be decayed, so a call that only decays leaves the memo in place. Nothing else about the sim changes. A call
 *            with no turbulence (NULL, or amplitude == 0) and n_decays == 0 launches nothing and forgets nothing; with amplitude == 0 the velocity is neither read nor
 *            written; a grid with no leaves launches nothing.
 * The arithmetic. Every line below is one rounded float32 operation, none contracted; integers are uint32 and wrap. H is the hash of BIRTH AND DEATH OF POINTS.
 *   Host constants, formed in float32 on the host once per call: f_0 = frequency, f_o = f_(o-1) * lacunarity; a_0 = 1.0f, a_o = a_(o-1) * gain; kA = amplitude * dt;
 *            inv = 1.0f / (control_hi - control_lo); s_o = H(H(seed ^ 0x9E3779B9u) + o); per decay r = 1.0f / (1.0f + rate * dt).
 *   Lattice  the voxel has global coordinates x = (i, j, k). Per octave o and component c: q.c = f_o * (float)x.c; q.c = q.c + offset.c. If any component of q is not
 *            finite or has |q.c| >= 4194304.0f the octave's curl is c_o = (+0, +0, +0): that far out the fraction has no bits left. Otherwise the cell is
 *            I.c = Floor(q.c) and the fraction t.c = q.c - (float)I.c (0 <= t.c <= 1; 1 where the subtraction rounds up).
 *   Corners  h(I + (a,b,e)) = H(H(H(s_o ^ (uint32)(I.x+a)) ^ (uint32)(I.y+b)) ^ (uint32)(I.z+e)) for a, b, e in {0, 1}: one hash per lattice corner and octave. Channel m
 *            in {0, 1, 2} reads nibble (h >> 4m) & 15, which selects a gradient g from the 16 of improved Perlin noise, in this order:
 *            (1,1,0), (-1,1,0), (1,-1,0), (-1,-1,0), (1,0,1), (-1,0,1), (1,0,-1), (-1,0,-1), (0,1,1), (0,-1,1), (0,1,-1), (0,-1,-1), (1,1,0), (-1,1,0), (0,-1,1), (0,-1,-1),
 *            its components the floats +0.0f, 1.0f and -1.0f.
 *   Value    p = (t.x - a, t.y - b, t.z - e), where a component with a, b or e = 0 is t's itself and the others are t.c - 1.0f;
 *            d_abe = (g.x * p.x + g.y * p.y) + g.z * p.z: three multiplies (a zero component gives a signed zero), then the two adds in this order.
 *   Fades    u(t) = (((((6.0f * t - 15.0f) * t + 10.0f) * t) * t) * t, seven operations from the left; u'(t): b = t - 2.0f; b = b * t; b = b + 1.0f; e = 30.0f * t;
 *            e = e * t; u' = e * b.
 *   Lerp     lerp(v0, v1, w): d = v1 - v0; d = w * d; v0 + d.
 *   Nests    L(v) over eight corner values v_abe: first along z, v_ab = lerp(v_ab0, v_ab1, u(t.z)); then along y, v_a = lerp(v_a0, v_a1, u(t.y)); then along x,
 *            lerp(v_0, v_1, u(t.x)). A nest over four values runs the same order with the missing axis left out.
 *   Partials dN_m/dx = u'(t.x) * L_yz(d_1be - d_0be) + L(g_abe.x): the four differences, their nest z then y, the multiply, the nest of the gradients' x components,
 *            the add. dN_m/dy likewise with d_a1e - d_a0e, the nest z then x, u'(t.y) and g_abe.y; dN_m/dz with d_ab1 - d_ab0, the nest y then x, u'(t.z) and g_abe.z.
 *            N itself is not formed. Derivatives are taken in lattice units.
 *   Curl     of the potential (N_0, N_1, N_2): c_o.x = dN_2/dy - dN_1/dz; c_o.y = dN_0/dz - dN_2/dx; c_o.z = dN_1/dx - dN_0/dy -- six of the nine partials. Each
 *            octave is divergence-free on its own, so the sum is. C.c = sum over o = 0 .. octaves - 1 in ascending order of a_o * c_o.c: C.c = +0; then per octave
 *            e = a_o * c_o.c; C.c = C.c + e. A component of one octave's c_o has a magnitude of 0.81 on average and 3.9 at the peak of 4,000 samples (tests/test_shaping_cases.py prints both): choose the amplitude by that.
 *   Control  without a control w is not formed and k = kA. With one, c is the control field's value at the voxel BEFORE this call's decay: w = c - control_lo;
 *            w = w * inv; w = fminf(fmaxf(w, 0.0f), 1.0f) with the GPU's min / max, which a NaN operand loses, formed as w = w > 0.0f ? w : +0.0f;
 *            w = w < 1.0f ? w : 1.0f -- so a NaN c gives w = 0, and so does -0 --; k = kA * w.
 *   Velocity e = k * C.c; v.c = v.c + e. NaN and inf in v pass through by the arithmetic.
 *   Decay    of each listed field, after the control was read: t = f - target; t = t * r; f = target + t.
 * hns_shaping_curl_host evaluates C of the voxel (i, j, k) -- before amplitude, control and dt -- ON THE HOST, from the header the kernel includes (hns_noise.hpp); it
 * ignores control, control_lo and control_hi, and needs no device. There is no host mirror over whole arrays (it would take data pointers): the Python tests restate the
 * text above in numpy and compare every byte.
 * Refused before anything is launched and with nothing touched (HNS_ERR_INVALID_ARGUMENT, the call and the argument in the message) -- the numbers and the specs, host
 * structs, first, then the objects --: a NaN, infinite or negative dt; an amplitude or offset component that is not finite, a frequency that is not finite and > 0,
 * octaves outside 1 .. 4, a lacunarity that is not finite and >= 1, a gain outside 0 .. 1 or NaN, with a control a control_lo or control_hi that is not finite or
 * control_lo >= control_hi; n_decays outside 0 .. 8, a null decays with n_decays > 0, a null decay name, a rate that is NaN, infinite or negative, a target that is not
 * finite; then a null object, a null sim (HNS_ERR_NO_DEVICE where there is no device), a sim lent to a grid's cook cache, a control or decay name that is not a float
 * field of the sim, "collision_sdf" as a decay name (it may be the control), a decay name given twice. curl_host: a null spec or out, and the spec's numbers as above.
 * Not mirrored in hns_dist_*. */
typedef struct hns_shaping hns_shaping;
hns_shaping* hns_shaping_create(int* err);
void hns_shaping_destroy(hns_shaping*);
int hns_shaping_set_stream(hns_shaping*, void* hip_stream);
typedef struct hns_turbulence_spec {
	float amplitude;     /* finite; velocity units per unit of time; 0 = read and write no velocity */
	float frequency;     /* finite, > 0; lattice cells per voxel of octave 0 */
	float offset[3];     /* finite; lattice units; the caller scrolls it to animate */
	int octaves;         /* 1 .. 4 */
	float lacunarity;    /* finite, >= 1 */
	float gain;          /* finite, 0 .. 1 */
	unsigned int seed;
	const char* control; /* NULL, or the name of a float field of the sim */
	float control_lo;    /* finite, control_lo < control_hi; read only with a control */
	float control_hi;
} hns_turbulence_spec;
typedef struct hns_decay_spec {
	const char* name; /* a float field of the sim, not "collision_sdf" */
	float rate;       /* finite, >= 0; in the limit of small dt the e-folding rate of the distance to the target */
	float target;     /* finite */
} hns_decay_spec;
int hns_shaping_apply(hns_shaping*, hns_sim*, float dt, const hns_turbulence_spec* turbulence, const hns_decay_spec* decays, int n_decays);
typedef struct hns_shaping_curl {
	float c[3];
} hns_shaping_curl;
int hns_shaping_curl_host(const hns_turbulence_spec*, int i, int j, int k, hns_shaping_curl* out);
/* DIFFUSING A SIM: implicit diffusion of float fields (heat conduction, smoke diffusion) and viscosity of the velocity, the operator that spreads a field of a
 * device-resident sim without leaving the GPU. For each listed field solve (I - a L) x = b: b is the field as it stands at the call,
 * a = coefficient * dt / voxel_size^2, L the 7-point Laplacian over the UNKNOWNS of the sim. It is implicit, so it is stable at any a; the solve is a fixed number of
 * Jacobi or Chebyshev-accelerated Jacobi iterations, one launch each over all listed fields. hns_diffusion is an object that holds the stream the launches go to and
 * the pooled scratch of its calls; the sim is an argument. No call here takes a caller's data pointer.
 *   Object   create allocates no device memory (HNS_ERR_NO_DEVICE without a HIP device); the null stream until hns_diffusion_set_stream binds another.
 *   apply    asynchronous on the object's stream. It updates only the unknowns of the listed fields, and of the velocity when viscosity gives a non-zero a, and writes
 *            nothing else the caller can observe: no other field, not the divergence, not the pressure, not the masks. Device pointers the sim has handed out stay valid,
 *            and the result lies behind them. When the velocity is written the sim forgets what it knew of it (the look-ahead memo and the velocity's feedback signature
 *            are dropped, as by hns_shaping_apply); of a written float field its signature alone. A call that leaves every term at a == 0, or a grid without leaves,
 *            launches nothing and forgets nothing. Otherwise: one launch that classifies the faces, `iterations` launches, and with iterations == 1 one copy.
 *   Scratch  each written field needs two iterates beside b. Of the velocity they are the sim's advected-velocity and vorticity buffers (the memo in the first goes
 *            with the forget); of a float field the sim's own next-value buffer of that field and one array from the pool. The object draws ONE block from the pool on the
 *            first apply that launches -- two code bytes per voxel and one float per voxel and written float field --, draws a larger one when a later call needs more
 *            (which waits for the device), keeps it between calls and gives it back in destroy. The iterations write every word of the scratch before they read it
 *            for a result: no result depends on what that memory held. The first iteration reads the field itself and the last writes into it (a thread of the last
 *            launch reads b and x^(k-2) of its own voxel only, its neighbours from the scratch), so there is no copy, except with iterations == 1.
 * The mathematics.
 *   Voxel classes  a voxel is SOLID iff collide != 0, its leaf exists and collision_sdf < threshold there (a NaN is not solid: the rule of the collision trace). A voxel
 *            is an UNKNOWN iff its leaf exists, its bit in the sim's active masks is set (no masks = every voxel) and it is not solid. Every voxel that is not an
 *            unknown keeps its bytes: it is never written.
 *   Faces    of an unknown, in the fixed order +x, -x, +y, -y, +z, -z. OPEN: the neighbour is an unknown. WALL: the neighbour is solid. Closed: everything else (an
 *            absent leaf, an inactive voxel). For a float field open faces exchange; wall and closed faces are zero-flux. For the velocity (all three components, the
 *            same faces) a wall face is a no-slip wall at rest: it counts in m and adds nothing to the sum. m = open faces for a float field; m = open + wall faces
 *            for the velocity.
 *   Host constants, in float32 on the host, one rounded operation per step, once per field and call: h2 = voxel_size * voxel_size; a = coefficient * dt; a = a / h2;
 *            for m = 0..6: e = a * (float)m; den = 1.0f + e; r_m = 1.0f / den; s = 6.0f * a; den = 1.0f + s; rho = s / den; q = rho * rho;
 *            w_1 = 1.0f; w_2 = 1.0f / (1.0f - q * 0.5f) as h = q * 0.5f; d = 1.0f - h; w_2 = 1.0f / d;
 *            w_(k+1) = 1.0f / (1.0f - (q * 0.25f) * w_k) as c = q * 0.25f; e = c * w_k; d = 1.0f - e; w_(k+1) = 1.0f / d. There is no division on the device.
 *   Iteration k = 1..iterations, per unknown and component, one rounded float32 operation per line, none contracted: x^0 = b; S = +0.0f;
 *            for each OPEN face in the order above: S = S + x^(k-1)[neighbour]; t = a * S; t = b + t; j = t * r_m.
 *            Jacobi (method 0): x^k = j. Chebyshev (method 1): x^1 = j; for k >= 2: d = j - x^(k-2); d = w_k * d; x^k = x^(k-2) + d.
 *            Chebyshev reads only its own voxel of x^(k-2), so x^k may be written over x^(k-2). NaN and inf pass through by the arithmetic.
 *   Result   a Jacobi sweep reads only the previous iterate: the result is unique, whatever order workgroups retire in. There are no atomics.
 *   Convergence, to choose the iteration count by: Jacobi contracts the max-norm error by rho per iteration and keeps every iterate of a float field inside
 *            [min b, max b]. Chebyshev reaches 2 sigma^k / (1 + sigma^(2k)) with sigma = rho / (1 + sqrt(1 - rho^2)); it loses that monotonicity and is worse for the first
 *            few iterations at large a. Measured on the numpy mirror (tests/test_diffusion_cases.py prints them): at a = 4 after 40 iterations the error is 3e-2 for Jacobi
 *            and 1e-4 for Chebyshev (max|b| = 8); at a = 0.05 both are converged to float32 in 8 iterations.
 *   Exact solution  of a float field conserves the sum of x over the unknowns. The velocity's does not: the wall takes momentum.
 *   Skipped  a term whose a is +0 (coefficient 0 or dt 0) is skipped: neither read nor written, and the sim forgets nothing of it. The same holds for viscosity.
 * hns_diffusion_schedule_host forms the host constants of one coefficient ON THE HOST, with no device: a, r[m] = r_m, rho, omega[k-1] = w_k for k = 1 .. iterations
 * (omega[0] = 1.0f) and +0.0f behind them. There is no host mirror over whole arrays (it would take data pointers): the Python tests restate the text above in numpy
 * and compare every byte.
 * Refused before anything is launched and with nothing touched (HNS_ERR_INVALID_ARGUMENT, the call and the argument in the message) -- the numbers and the host
 * structs first, then the objects --: a null spec; a NaN, infinite or negative dt; a voxel_size that is not finite and > 0; iterations outside 1 .. 256; method outside
 * 0 .. 1; a viscosity or a coefficient that is NaN, infinite or negative; any a or 6 a that is not finite; with collide a threshold that is not finite; n_terms outside
 * 0 .. 8; null terms with n_terms > 0; a null name; then a null object, a null sim (HNS_ERR_NO_DEVICE where there is no device), a sim lent to a grid's cook cache, a
 * name that is not a float field of the sim, "collision_sdf" as a term, a name listed twice, collide on a sim without a collision_sdf field; then, of a call that has
 * something to launch, a sim and an object on different devices and a grid whose launch range is not the whole grid (as the multigrid solve refuses it: a face of a
 * leaf outside the range would be neither open nor closed). schedule_host: a null out and the same numbers. Not mirrored in hns_dist_*. */
typedef struct hns_diffusion hns_diffusion;
hns_diffusion* hns_diffusion_create(int* err);
void hns_diffusion_destroy(hns_diffusion*);
int hns_diffusion_set_stream(hns_diffusion*, void* hip_stream);
typedef struct hns_diffusion_term {
	const char* name;  /* a float field of the sim, not "collision_sdf" */
	float coefficient; /* finite, >= 0; the diffusivity, in voxel_size^2 per unit of dt */
} hns_diffusion_term;
typedef struct hns_diffusion_spec {
	int iterations;  /* 1 .. 256 */
	int method;      /* 0 Jacobi, 1 Chebyshev */
	float viscosity; /* finite, >= 0; the velocity's coefficient, 0 = the velocity is neither read nor written */
	int collide;     /* 0: no voxel is solid; 1: the sim's collision_sdf decides */
	float threshold; /* finite; read only with collide */
} hns_diffusion_spec;
int hns_diffusion_apply(hns_diffusion*, hns_sim*, float dt, float voxel_size, const hns_diffusion_spec*, const hns_diffusion_term* terms, int n_terms);
typedef struct hns_diffusion_schedule {
	float a;
	float r[7];
	float rho;
	float omega[256]; /* omega[k-1] = w_k; omega[0] = 1.0f */
} hns_diffusion_schedule;
int hns_diffusion_schedule_host(float coefficient, float dt, float voxel_size, int iterations, hns_diffusion_schedule* out);
/* Point values into fields: the transpose of hns_dev_sample_points -- every point adds w * v to the eight voxels of its cell -- with an accumulation that does not depend on
 * the order the adds retire in. fields[i]: device pointer, ncomp[i] 1 (float) or 3 (Vec3f AoS), added into IN PLACE; values[i]: device, n x ncomp[i] floats, the value of
 * each point for field i; fields, ncomp and values are HOST arrays of n_fields (1 .. 8) entries; xyz as for hns_dev_sample_points.
 *   Cell     ijk = Floor(xyz) with the GPU's saturating float -> int conversion, f = xyz - float(ijk), taps = the eight corners of the trilinear sampler's stencil.
 *   Weights  wx[0] = 1.0f - fx, wx[1] = fx, likewise y and z; w(di,dj,dk) = (wx[di] * wy[dj]) * wz[dk]; the term of a component with point value v is t = w * v. Each of
 *            these is one rounded f32 operation, none contracted.
 *   Landing  a point with a non-finite position component lands nowhere; otherwise a tap lands iff its leaf exists (any leaf of the grid, ghost leaves included).
 *   Accepted a landed tap's term is accepted iff t is finite and |t| * 2^-Q < 2^62, Q = log2_quantum (-40 .. 0).
 *   Sum      an accepted term adds the int64 k = rint((double)t * 2^-Q), ties to even, to the voxel's 64-bit accumulator of that component, modulo 2^64 -- on the device
 *            an integer atomic add. Integer addition is associative: the result does not depend on scheduling. No float atomics.
 *   Finish   every voxel whose accumulator a is non-zero gets field = field + (float)((double)(int64)a * 2^Q), an f32 add; every other voxel keeps its bytes (-0.0f stays).
 * So a term is rounded once, to a multiple of 2^Q (the default of the Python layer, Q = -32, resolves 2.3e-10 and accepts |t| < 2^30), the sum of a voxel is exact, and the
 * field sees one rounded add. status: NULL, or n bytes (device): the number of taps of each point that landed, 0 .. 8 -- positions only. d_rejected: NULL, or one uint64_t
 * (device) the call ADDS the number of (point, component, tap) terms to that landed but were not accepted (NaN or inf values, terms beyond the bound). Up to eight fields
 * share a call and with it the cell and the weights; output i is bit-identical to a call with field i alone. The host mirror hns_grid_splat_points gives the same bytes.
 * The accumulator -- int64 channels over all voxels plus a touched word per leaf, sized for min(4, sum of ncomp) channels, 32 bytes a voxel at four -- is pooled device memory
 * kept with the grid (made on first use, enlarged when a later call needs more channels, returned by hns_grid_release_cache and hns_grid_destroy). A call with more
 * components runs several launches. It is all zero between calls: cleared when drawn from the pool, and zeroed again by the finish kernel, which visits only the leaves a
 * tap landed in. Calls on one grid must follow each other on one stream. Asynchronous on `stream`; n == 0 launches nothing and looks at no device pointer. Refused before
 * anything is launched (HNS_ERR_INVALID_ARGUMENT, the call and the argument in the message), everything untouched: a null list or entry, a null xyz, an ncomp other than 1
 * or 3, n_fields outside 1 .. 8, n above 2^31 - 1, log2_quantum outside -40 .. 0, two equal field pointers, a field equal to xyz, to a values array, to status or to
 * d_rejected. Not mirrored in hns_dist_*. */
int hns_dev_splat_points(hns_grid*, float* const* fields, const int* ncomp, int n_fields, const float* xyz, const float* const* values, uint64_t n, int log2_quantum,
                         unsigned char* status, uint64_t* d_rejected, void* stream);
/* Host mirror of hns_dev_splat_points and hns_sim_splat_points: the same arguments over HOST arrays, brute force over hns_grid_offsets-style lookups, the same integer
 * arithmetic (uint64 wrap-around) and the same conversions (saturating Floor); works on HNS_GRID_HOST_ONLY grids. masks: NULL, or leaf_count x 64 bytes (byte x*8+y, bit z)
 * in which, with activate != 0, the bit of every landed tap with w > 0 is set. *rejected (or NULL) is ADDED to, as d_rejected is. Refusals as hns_dev_splat_points'. */
int hns_grid_splat_points(const hns_grid*, float* const* fields, const int* ncomp, int n_fields, const float* xyz, const float* const* values, uint64_t n, int log2_quantum,
                          unsigned char* masks, int activate, unsigned char* status, uint64_t* rejected);
/* POINTS RASTERISED INTO FIELDS: a radius footprint in place of the cell, and a weighted average in place of the sum. A spec stored with a grid is read by every later
 * hns_dev_splat_points on that grid, one stored with a sim by every later hns_sim_splat_points (the sim keeps it across regrids); the calls themselves are unchanged, and
 * with the default spec {0, 0, ..} they give the bytes, the launches and the accumulator they gave before there was a spec. Everything not restated here -- positions,
 * landing, acceptance, the int64 sum, d_rejected, log2_quantum, the refusals -- is hns_dev_splat_points'. Every line below is one rounded f32 operation, none contracted;
 * the divisions are correctly rounded.
 *   Radial footprint (kernel 1) of a point x with radius r (r = d_radius[p] where d_radius is given, else spec.radius):
 *     Which points rasterise  a point rasterises iff each coordinate satisfies the seeds' condition (hns_point_leaves: "Which points seed") AND 0 < r && r <= spec.radius
 *                             (a NaN fails both). Any other point lands nowhere: status 0.
 *     Box      per axis lo = Floor(x - r) + 1 and E = (int)ceilf(2.0f * r) <= 8; the candidates are lo .. lo + E - 1: at most two leaves per axis lie under them.
 *     Weight   of candidate (i, j, k): dx = (float)i - x.x, likewise dy, dz; d2 = (dx*dx + dy*dy) + dz*dz; r2 = r*r; inv = 1.0f / r2; q = d2 * inv; the voxel is in the
 *              footprint iff q < 1.0f, and then a = 1.0f - q, w = a * a. THE BOX IS PART OF THE DEFINITION: a voxel outside it is not in the footprint whatever its q.
 *              Some 280 of the 512 candidates at r = 4; r = 1 at an integer position is that one voxel with w = 1.0f.
 *     status   (radial calls) 2 iff the footprint is non-empty and every voxel of it landed, 1 iff some but not all landed, else 0. The trilinear 0 .. 8 is unchanged.
 *     activate the mask bit of every landed footprint voxel with w > 0 is set, whether or not its terms were accepted (the trilinear rule).
 *   Average (mode 1), with either kernel: every pass carries one more channel W whose term is w itself (t = w * 1.0f), put through the same acceptance and sum; a pass
 *   holds up to three value channels and W, a call with more components runs more passes, each with its own W, so that output i still equals a call with field i alone.
 *     Finish   every voxel whose W accumulator a_w is non-zero: Wsum = (float)((double)(int64)a_w * 2^Q), Vsum likewise from a_v, den = fmaxf(Wsum, min_weight),
 *              field = Vsum / den, REPLACING the old value. A voxel with a_w == 0 keeps its bytes, even where an a_v is non-zero. All accumulators end zero either way.
 *   So point values all equal to 1.0f average to exactly 1.0f wherever Wsum >= min_weight (the two accumulators are the same integer), and doubling every point leaves an
 *   average unchanged bit for bit while no accumulator wraps (2 a_v / 2 a_w). The accumulator is sized for min(4, components + 1) channels in average mode.
 *   On the device the radial kernel (hns_rasterize.hip) gives a group of 1, 4, 16 or 64 lanes to each point -- the square of ceil(2 * spec.radius) rounded up to a power of
 *   two --, so that the adds of one wave instruction go to the contiguous accumulator pieces of z-runs; a spec.radius far above the radii in d_radius leaves lanes idle.
 * The setters do no device work and refuse (HNS_ERR_INVALID_ARGUMENT, the stored spec unchanged): a null grid or sim, kernel or mode outside {0, 1}, radial with a radius
 * that is NaN or outside (0, 4], d_radius with kernel 0, a min_weight that is negative or not finite. spec NULL stores the default. radius is ignored by
 * kernel 0, min_weight by mode 0. d_radius is read by every later splat call, asynchronously: the caller keeps it alive. Not mirrored in hns_dist_*. */
typedef struct hns_splat_spec {
    int kernel;             /* 0 trilinear (the cell of hns_dev_splat_points), 1 radial */
    int mode;               /* 0 add, 1 average */
    float radius;           /* radial: the radius in voxels (index space), 0 < radius <= 4.0f; with d_radius: the caller's upper bound of it */
    const float* d_radius;  /* radial: NULL, or n floats in device memory, one radius per point */
    float min_weight;       /* average: finite, >= 0 */
} hns_splat_spec;
int hns_grid_set_splat_spec(hns_grid*, const hns_splat_spec* spec);
int hns_sim_set_splat_spec(hns_sim*, const hns_splat_spec* spec);
int hns_grid_get_splat_spec(const hns_grid*, hns_splat_spec* spec);
int hns_sim_get_splat_spec(const hns_sim*, hns_splat_spec* spec);
/* Host mirror of both splat calls under a spec (NULL: the default, and then this is hns_grid_splat_points): the arguments of hns_grid_splat_points behind the spec, whose
 * d_radius is a HOST pointer here. The same integers, the same bytes. */
int hns_grid_splat_points_spec(const hns_grid*, const hns_splat_spec* spec, float* const* fields, const int* ncomp, int n_fields, const float* xyz,
                               const float* const* values, uint64_t n, int log2_quantum, unsigned char* masks, int activate, unsigned char* status, uint64_t* rejected);
/* THE SEEDS OF A POINT SET: the leaves a point set needs in the domain so that every tap of every point lands (what hns_sim_regrid_seeded unites into the velocity's
 * topology, and with hns_grid_create_from_leaves a fresh grid around a particle set). xyz: n x 3 floats, index space, as for hns_dev_sample_points.
 *   Which points seed  a point seeds iff each coordinate c satisfies -8388608.0f <= c && c < 8388607.0f (NaN and +-inf fail): beyond 2^23 a float32 has no fraction, and
 *                      inside the range a leaf coordinate fits 21 bits. Points that do not seed are counted in *skipped and seed nothing.
 *   Cell and taps      (i, j, k) = Floor(xyz), exact in this range; the taps are the eight voxels (i+di, j+dj, k+dk). ALL EIGHT are seeds whatever their trilinear
 *                      weights: a point at an integer position still finds its whole cell inside the domain (a later splat reports status 8).
 *   The seed set S     the leaves (origin = coordinate & ~7) holding at least one tap, each with a 64-byte mask (byte x*8+y, bit z, local coordinates) in which exactly
 *                      the tap bits are set; origins in OpenVDB leaf order. S depends on the SET of points only: not on their order or multiplicity.
 * hns_point_leaves is the host mirror, plain C++ (the two-call idiom of hns_dilate_leaf_masks): *n_leaves is always set; origins_out (cap x 3) and masks_out (cap x 64, or
 * NULL) are written only when origins_out is not NULL and *n_leaves <= cap; *skipped (or NULL) is set, not added to. HNS_ERR_INVALID_ARGUMENT: xyz NULL with n > 0,
 * n_leaves NULL, n above 2^31 - 1; HNS_ERR_TOPOLOGY: more than 2^23 distinct leaves. */
int hns_point_leaves(const float* xyz, uint64_t n, int32_t* origins_out, unsigned char* masks_out, uint64_t cap, uint64_t* n_leaves, uint64_t* skipped);
/* The same for points in DEVICE memory of HIP device `device`: arguments and results are the host mirror's, byte for byte; d_xyz is device memory, every output is host
 * memory. Synchronous; scratch comes from the pool of device memory. Two passes over the points, since the number of leaves is not known beforehand (hns_seed.hip): the
 * leaves as keys into a hash -- equal keys merged within a wave before memory is touched, a compare-and-swap only on a slot a load shows empty --, then the tap bits as
 * at most eight 64-bit integer ORs a point, each skipped when a load shows its bits set. The result does not depend on the order anything retires in. HNS_ERR_NO_DEVICE
 * where there is no HIP device (no CPU fallback: hns_point_leaves is the host's); HNS_ERR_TOPOLOGY: more than 2^23 distinct leaves (the candidate-hash bound of the
 * regrid). Not mirrored in hns_dist_*. */
int hns_dev_point_leaves(int device, const float* d_xyz, uint64_t n, int32_t* origins_out, unsigned char* masks_out, uint64_t cap, uint64_t* n_leaves, uint64_t* skipped,
                         void* stream);
/* THE LEAF ORDER OF A POINT SET: a stable sort of points by the voxel (or the leaf) of their cell, as a permutation with per-leaf ranges, and the moves that carry any
 * per-point attribute array through that permutation and back. The point kernels above run some five times faster on points in this order than on the same points
 * permuted. xyz: n x 3 floats, index space, as for hns_dev_sample_points; L is the grid's leaf count.
 *   Which points sort  a point sorts iff each coordinate satisfies the seeds' condition (hns_point_leaves: "Which points seed"); NaN and +-inf fail.
 *   Cell               (i, j, k) = Floor(xyz), exact in this range; off = the grid's 1-based offset of that voxel, 0 where its leaf is absent (what hns_grid_offsets
 *                      returns). Every leaf of the grid counts, whatever its launch range.
 *   Voxel key          a uint32: off - 1 for a point that sorts and whose leaf exists -- the flat field index of its cell's voxel, leaf * 512 + ((i&7)<<6 | (j&7)<<3 | (k&7));
 *                      512 * L for a point that sorts and whose leaf is absent ("outside"); 512 * (L + 1) for a point that does not sort.
 *   Level              level 1 sorts by the voxel key; level 0 by key >> 9: the leaf, then L, then L + 1.
 *   Order              perm[r] is the index in xyz of the point of rank r; keys are non-decreasing in r, and points of equal key keep ascending index: the sort is
 *                      stable. The result is therefore unique: it depends neither on the algorithm nor on the order anything retires in.
 *   Keys out           keys[r] is the key (at the call's level) of point perm[r].
 *   Ranges             leaf_start has L + 3 uint32 entries: leaf_start[q] = the number of points whose LEAF-level key is < q, q = 0 .. L + 2, at both levels. Leaf q owns the
 *                      ranks leaf_start[q] .. leaf_start[q + 1]; leaf_start[L] starts the outside points, leaf_start[L + 1] the points that do not sort, and
 *                      leaf_start[L + 2] = n. An empty leaf has an empty range. (CSR over the grid's leaves: what a binned splat reads.)
 * The sort needs scratch sized by the point count and leaves results that later calls read, so it is an object. create draws every buffer -- perm, keys, the (key, index)
 * ping-pong, leaf_start, the tile histograms -- from the pool of device memory, sized for `capacity` points (24 bytes a point, and one histogram row of 1 KiB per 2048
 * points); destroy returns them. sort, gather and scatter allocate nothing and are asynchronous on the object's stream: the null stream until hns_point_order_set_stream binds
 * another, and every later call of the object is ordered on that stream and on nothing else. The object refers to its grid, which must outlive it. A sort may follow a
 * sort, with a larger or a smaller n: nothing of the earlier one survives. n == 0 zeroes leaf_start on the stream and launches no kernel.
 * On the device (hns_pointorder.hip) the sort is a least-significant-digit radix sort of (key, index) pairs with 8-bit digits; the number of passes, 1 .. 4, is
 * ceil(bits of 512 * (L + 1), or of L + 1 at level 0, / 8): it depends on the grid and the level only, never on the data. No kernel waits on another workgroup.
 * hns_point_order_get fills the info with DEVICE pointers into the object's buffers (valid until the next sort or the destroy; no wait; before any sort n = 0 and
 * level = -1). gather: dst row r = src row perm[r]; scatter: dst row perm[r] = src row r, for rows 0 .. n - 1 of the last sort, rows of row_bytes bytes -- a multiple of 4
 * in 4 .. 64: one float up to a 16-float attribute row, xyz itself at 12; scatter(gather(x)) == x. Rows of dst beyond n - 1 keep their bytes.
 * Refused with HNS_ERR_INVALID_ARGUMENT (the call and the argument in the message), nothing touched: a null object, grid or xyz (with n > 0); a capacity or n above
 * 2^31 - 1; n > capacity; a level outside {0, 1}; a grid with (L + 2) * 512 > 2^32; an HNS_GRID_HOST_ONLY grid; a row_bytes outside the rule; a null d_src or d_dst
 * (with n > 0); d_src == d_dst; gather or scatter before any sort. HNS_ERR_NO_DEVICE where there is no HIP device. Not mirrored in hns_dist_*. */
typedef struct hns_point_order hns_point_order;
hns_point_order* hns_point_order_create(hns_grid*, uint64_t capacity, int* err);
void hns_point_order_destroy(hns_point_order*);
int hns_point_order_set_stream(hns_point_order*, void* hip_stream);
int hns_point_order_sort(hns_point_order*, const float* d_xyz, uint64_t n, int level);
typedef struct hns_point_order_info {
    const uint32_t* perm;        /* n entries */
    const uint32_t* keys;        /* n entries */
    const uint32_t* leaf_start;  /* n_leaves + 3 entries */
    uint64_t n, n_leaves, capacity;
    int level;
} hns_point_order_info;
int hns_point_order_get(const hns_point_order*, hns_point_order_info*);
int hns_point_order_gather(const hns_point_order*, const void* d_src, void* d_dst, int row_bytes);
int hns_point_order_scatter(const hns_point_order*, const void* d_src, void* d_dst, int row_bytes);
/* POINT VALUES INTO FIELDS THROUGH A LEAF ORDER: hns_dev_splat_points / hns_sim_splat_points for the n points of the object's last sort, with each leaf's voxels summed in
 * LDS by one workgroup and the fields written with plain stores, in place of one global atomic per term. The new path is selected by calling it: the plain calls are
 * unchanged. fields, ncomp, n_fields, values, log2_quantum, status and d_rejected are those of hns_dev_splat_points; names, n_names, velocity_values and activate those of
 * hns_sim_splat_points; n is the n of the last sort. The device form reads the spec stored with the object's grid, the sim form the sim's: the radial kernel and the
 * average mode run under the same specs. No stream argument: like sort, gather and scatter the calls run on the stream bound to the object.
 *   rows      how the per-point arrays -- d_xyz, every values[i], spec.d_radius, status -- are laid out. 0 (original): row perm[r] belongs to rank r; these are the arrays
 *             the sort saw. 1 (ranked): row r belongs to rank r; the caller has gathered them with hns_point_order_gather and keeps its attributes in sorted order.
 *   Contract  the positions are, bit for bit, those of the last sort (rows = 1: its gather). Then every field holds exactly the bytes hns_dev_splat_points
 *             (hns_sim_splat_points) leaves for the same points in their original order, with either kernel and either mode; the increment of *d_rejected is the same;
 *             status is the same under the row mapping; with activate the sim's masks are the same. With other positions WHICH terms are added is unspecified; every
 *             access still stays inside the caller's n rows and the grid's voxels.
 *   Tail      the ranks from leaf_start[L] on -- points whose cell's leaf is absent, points that do not sort -- can still land (a cell in an absent leaf next to an
 *             existing one; a finite trilinear point beyond 2^23). A per-point kernel adds their terms into the grid's accumulator with integer atomics, as the plain calls
 *             do, BEFORE the leaf kernel, which adds a touched leaf's piece of the accumulator into its sums: a voxel reached by a tail point and a binned point gets one
 *             sum and one rounded add. The host never waits for the length of the tail. status, where asked for, comes from the same kernel walking every rank.
 *   Leaves    one workgroup per leaf Q walks the ranks of the leaves whose points can reach Q (trilinear: the eight leaves Q - {0,1}^3; radial: all 27 neighbours, since
 *             with r <= 4 a box lies under its point's leaf and that leaf's neighbours), recomputes each point's candidates and keeps those inside Q. Every
 *             (point, tap, channel) term is evaluated by exactly one workgroup, rejected terms are counted there. Both sort levels give the same bytes.
 * Asynchronous on the object's stream. Allocates nothing beyond the grid's pooled splat accumulator (which the plain calls draw too) and leaves it and the touched words all
 * zero: plain and ordered calls may alternate on one grid, on one stream. n == 0 launches nothing. One workgroup per destination leaf: a point set concentrated in a few
 * leaves is summed by a few workgroups, and the plain calls are then the faster ones. Refused before anything is launched (HNS_ERR_INVALID_ARGUMENT, the call and the
 * argument in the message), everything untouched: whatever the corresponding plain call refuses; a null object; a call before any sort; rows outside {0, 1}; a sim whose grid
 * is not the object's grid. Not mirrored in hns_dist_*. */
int hns_point_order_splat(const hns_point_order*, float* const* fields, const int* ncomp, int n_fields, const float* d_xyz, const float* const* values, int rows,
                          int log2_quantum, unsigned char* status, uint64_t* d_rejected);
int hns_point_order_splat_sim(const hns_point_order*, hns_sim*, const char* const* names, int n_names, const float* velocity_values, const float* d_xyz,
                              const float* const* values, int rows, int log2_quantum, int activate, unsigned char* status, uint64_t* d_rejected);
/* Host mirror of hns_point_order_sort: xyz and the outputs are HOST arrays -- perm n entries, keys (or NULL) n entries, leaf_start (or NULL) L + 3 entries --, plain C++
 * around std::stable_sort over hns_grid_offsets-style lookups; works on HNS_GRID_HOST_ONLY grids. The same bytes as the device's. Refusals as above, and a null perm
 * with n > 0. */
int hns_grid_sort_points(const hns_grid*, const float* xyz, uint64_t n, int level, uint32_t* perm, uint32_t* keys, uint32_t* leaf_start);
/* POINT NEIGHBOURHOODS THROUGH A LEAF ORDER: what relates a point to other points -- for every point the number of points around it, a density and a push away from
 * them --, read off the order of a voxel-level sort. L is the grid's leaf count and inside = leaf_start[L]: the ranks below it are the points that sort and whose cell's
 * leaf exists.
 *   Cell table  cell_start has 512 * L + 1 uint32 entries: cell_start[v] = the number of ranks r < inside with keys[r] < v. Voxel v (a flat field index) owns the ranks
 *               cell_start[v] .. cell_start[v + 1]; cell_start[512 * L] = inside. Defined by the sort alone, so unique. It needs the sort at level 1: after a sort at level 0,
 *               or before any sort, hns_point_order_cells and hns_point_order_neighbours are refused. The table lives in the object: 4 * (512 * L + 1) bytes drawn from the
 *               pool of device memory by the first call that needs it (what hns_point_order_create draws is unchanged) and returned by destroy. It is rebuilt on the
 *               object's stream by the first call behind every sort that needs it, so a stale table is never read. hns_point_order_cells returns a DEVICE pointer, valid
 *               until the next sort or the destroy; no host wait. With n == 0 the table is all zero. hns_point_order_info keeps its layout.
 *   rows        as for hns_point_order_splat. 0 (original): row perm[r] of d_xyz and of every output belongs to rank r. 1 (ranked): row r belongs to rank r.
 *   Contract    the positions are, bit for bit, those of the last sort (rows = 1: its gather). With other positions WHICH pairs are found is unspecified; every access
 *               still stays inside the caller's n rows, the object's buffers and the grid's tables (leaves are looked up by coordinates, never taken from a key).
 *   Outputs     d_count n uint32, d_density n floats, d_push n x 3 floats; any may be NULL, not all three. Every row of a non-NULL output is written.
 *   Takes part  a point takes part iff its rank is < inside. Every other point gets count 0, density +0.0f and push (+0, +0, +0), and is no one's neighbour.
 *   Box         h = radius, 0 < h <= 2. Along axis c the box of point i is the cells lo_c = (int)floorf(x_i.c - h) .. hi_c = (int)floorf(x_i.c + h), the subtraction and
 *               the addition being f32 operations: at most 5 cells an axis (6 where x + h rounds up to an integer) under at most two leaves an axis.
 *   Pair        j is a neighbour of i iff j != i, j takes part, Floor(x_j) lies in i's box on all three axes, and with dx = x_i.x - x_j.x (f32), likewise dy, dz,
 *               the radial footprint's weight holds (hns_splat_spec: "Weight"): d2 = (dx*dx + dy*dy) + dz*dz; inv = 1.0f / (h*h); q = d2 * inv; q < 1.0f; and then
 *               a = 1.0f - q, w = a * a. THE BOX IS PART OF THE DEFINITION: a point whose cell is outside it is no neighbour whatever its q.
 *   Terms       count_i = the number of neighbours. density_i sums the int64 k = rint((double)w * 2^32), ties to even. push_i.c is taken from the pairs with d2 > 0 only:
 *               d = sqrtf(d2); s = w / d; t_c = d_c * s; the sum of rint((double)t_c * 2^32). Every line is one rounded f32 operation, none contracted; the division and
 *               the root are correctly rounded. A coincident pair (d2 == 0) counts, has w = 1.0f and adds nothing to the push. No term is refused: |t| is about 1 at
 *               most, and 2^31 - 1 of them fit an int64.
 *   Finish      each sum a becomes (float)((double)(int64)a * 2^-32): the sums are exact, so a result depends neither on the order the pairs are met in nor on how
 *               they are split over lanes. The push points away from the neighbours: x_i + c * push_i thins a clump.
 * On the device (hns_neighbours.hip) the table is one workgroup per leaf -- a histogram of the leaf's ranks in LDS, a scan on top of leaf_start[leaf] --, and the query
 * goes by rank, so that neighbouring lanes hold points of the same or of adjacent voxels: 4, 16 or 32 lanes share a point and split the (x, y) columns of its box; a
 * column's z-run is one contiguous range of ranks per leaf under it, read from two entries of the table; the lanes' int64 sums are added across lanes. No kernel waits on
 * another workgroup. The query is asynchronous on the object's stream (no stream argument, like sort, gather and the ordered splat) and allocates nothing beyond the table;
 * n == 0 launches nothing and looks at no pointer. Refused before anything is launched (HNS_ERR_INVALID_ARGUMENT, the call and the argument in the message), nothing
 * touched: a null object; no sort yet; a sort at level 0; rows outside {0, 1}; a radius that is NaN, <= 0 or > 2; a null d_xyz (with n > 0); a null d_cell_start; all three
 * outputs NULL; an output equal to d_xyz or to another output. Not mirrored in hns_dist_*. */
int hns_point_order_cells(hns_point_order*, const uint32_t** d_cell_start);
int hns_point_order_neighbours(hns_point_order*, const float* d_xyz, int rows, float radius, uint32_t* d_count, float* d_density, float* d_push);
/* Host mirror of hns_point_order_neighbours: xyz and the outputs are HOST arrays with rows in the ORIGINAL order (no sort is needed: the cells come from the positions), plain
 * C++ with a cell list over hns_grid_offsets-style lookups; works on HNS_GRID_HOST_ONLY grids. The same bytes as the device's. Refusals as above, a null grid, and an n
 * above 2^31 - 1. */
int hns_grid_point_neighbours(const hns_grid*, const float* xyz, uint64_t n, float radius, uint32_t* count, float* density, float* push);
/* BIRTH AND DEATH OF POINTS: a stream of items, each with a small count c, expanded into sum(c) rows in item order, with the counts kept on the device. Death is c in
 * {0, 1} per point (select, then compact of every attribute array); birth is c in {0 .. K} per voxel of a field. A frame loop -- trace, drop the dead, append the newborn,
 * splat -- then runs without a host wait: the host keeps calling every point kernel with n = capacity, and the rows beyond the live count hold NaN positions, which the
 * point calls above treat as nothing (they land nowhere, they do not sort, their status is 0).
 *   Object    hns_point_population is modelled on hns_point_order: create draws every buffer from the pool of device memory -- slot, `capacity` uint32 words; one count word
 *             per tile of 2048 items for max(capacity, voxels of the grid) items; the two uint64 counters {live, wanted} --, destroy returns them. It refers to its grid,
 *             which must outlive it. live = wanted = 0 after create. set_stream binds the stream (the null stream before); set_live, select, compact, birth and birth_sim are
 *             asynchronous on that stream and on nothing else, allocate nothing, and launch nothing whose length depends on data: the host never learns a count unless it
 *             asks. counts waits for the stream and returns the two counters (either pointer may be NULL). set_live(n) sets live = wanted = n on the stream, for a caller
 *             that already holds n rows. get fills the info with DEVICE pointers -- slot, and counters[0] = live, counters[1] = wanted -- and the n of the last select; no wait.
 *   Select    point i < n is kept iff d_flags[i] >= at_least, at_least in 1 .. 255 (the status bytes of hns_dev_trace_points and of the splat calls are such flags).
 *             slot[i] = the number of kept points below i, or 0xFFFFFFFF for a dropped point. live = wanted = the number kept. n == 0 sets both to 0 and launches no kernel.
 *   Compact   for the n and the slot of the last select: dst row slot[i] = src row i for every kept i, rows of row_bytes bytes, a multiple of 4 in 4 .. 64 as for
 *             hns_point_order_gather. The move is stable, so the result is unique. With fill_word != NULL every 32-bit word of rows live .. n - 1 of dst becomes *fill_word,
 *             which the host reads at the call; with fill_word == NULL those rows keep their bytes. Rows of dst from n on are never touched. d_src != d_dst. One select
 *             serves any number of compacts: one per attribute array.
 *   Birth     the device form visits every leaf of the object's grid, whatever its launch range. A voxel has the flat index e = leaf * 512 + (x<<6 | y<<3 | z) and the
 *             global coordinates (i, j, k) = origin + (x, y, z). d_field: one float per voxel; d_masks: NULL, or leaf_count x 64 bytes.
 *     Eligible  all of: d_masks == NULL or the voxel's bit is set (byte x*8+y, bit z: the layout of hns_sim_active_masks); v = field[e] satisfies v > threshold (a NaN
 *               fails); each coordinate c satisfies -8388608 <= c && c <= 8388606, so that every birth meets the seeds' condition of hns_point_leaves.
 *     Hash      H(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16, on uint32. h = H(H(H(H(seed ^ 0x9E3779B9) ^ (uint32)i) ^ (uint32)j) ^ (uint32)k).
 *               Draw d is r(d) = H(h + d), and U(d) = (float)(r(d) >> 8) * 2^-24, exact. The draws depend on the voxel's coordinates and the seed only, never on the leaf
 *               numbering: the same voxel bears the same points on any grid that holds it.
 *     Count     m = fmaxf(0.0f, fminf(v * rate, (float)K)) with one rounded multiply, K = max_per_voxel in 1 .. 16; b = (uint32)m; f = m - (float)b;
 *               c = b + (U(0) < f ? 1 : 0). A voxel that is not eligible has c = 0.
 *     Position  of point q < c, per axis a in {0, 1, 2} with the voxel's coordinate i along it: p = (float)i + U(1 + 3q + a), one rounded add; if !(p < (float)(i + 1))
 *               then p = nextafterf((float)(i + 1), -inf). So Floor(p) == i always.
 *     Order     start = append ? live : 0. Point q of voxel e takes row start + sum of c(e') over e' < e + q. Rows at or beyond capacity_rows are not written: a prefix
 *               survives, so the result is unique. d_xyz row = p; d_voxel row (d_voxel may be NULL) = e. Afterwards wanted = start + sum(c) and
 *               live = min(wanted, capacity_rows). With spec.fill != 0, rows live .. capacity_rows - 1 of d_xyz are NaN (0x7FC00000 in every word) and those of d_voxel are
 *               0xFFFFFFFF. Rows below start are untouched.
 *   birth_sim reads the sim's float field `name` and, with use_masks != 0, the sim's own masks (a sim without masks: every voxel). The sim's grid must be the object's grid.
 *   hns_grid_birth_points is the host mirror, plain C++ over HOST arrays with `start` given by the caller; works on HNS_GRID_HOST_ONLY grids and gives the same bytes;
 *   *live and *wanted (either may be NULL) are set.
 * On the device (hns_population.hip) both are count, scan, place over tiles of 2048 items: a count kernel writes one word per tile, one workgroup scans the tile table and
 * writes the counters, a place kernel recomputes its tile's counts, ranks them in index order and writes slot, or the rows; a row kernel moves and fills. No kernel waits on
 * another workgroup, and there is no atomic at all.
 * Refused with HNS_ERR_INVALID_ARGUMENT (the call and the argument in the message) before anything is launched, nothing touched: a null object, a null grid, a null array
 * with n > 0 (flags, src, dst; the field, the spec; d_xyz with capacity_rows > 0); n > capacity; a capacity, n or capacity_rows above 2^31 - 1; an at_least outside
 * 1 .. 255; a row_bytes outside the rule; d_src == d_dst; compact before any select; a K outside 1 .. 16; a rate or a threshold that is not finite, or a rate <= 0; d_xyz
 * equal to d_field or to d_voxel; a sim of another grid, or an unknown field name; an HNS_GRID_HOST_ONLY grid at create; a grid of more than 2^32 voxels.
 * HNS_ERR_NO_DEVICE where there is no HIP device. Not mirrored in hns_dist_*. */
typedef struct hns_point_population hns_point_population;
hns_point_population* hns_point_population_create(hns_grid*, uint64_t capacity, int* err);
void hns_point_population_destroy(hns_point_population*);
int hns_point_population_set_stream(hns_point_population*, void* hip_stream);
int hns_point_population_set_live(hns_point_population*, uint64_t n);
int hns_point_population_select(hns_point_population*, const unsigned char* d_flags, uint64_t n, int at_least);
int hns_point_population_compact(const hns_point_population*, const void* d_src, void* d_dst, int row_bytes, const uint32_t* fill_word);
typedef struct hns_birth_spec {
    float threshold, rate;         /* both finite, rate > 0 */
    uint32_t max_per_voxel, seed;  /* K in 1 .. 16 */
    int fill;                      /* != 0: the rows live .. capacity_rows - 1 become NaN / 0xFFFFFFFF */
} hns_birth_spec;
int hns_point_population_birth(hns_point_population*, const float* d_field, const unsigned char* d_masks, const hns_birth_spec*, float* d_xyz, uint32_t* d_voxel,
                               uint64_t capacity_rows, int append);
int hns_point_population_birth_sim(hns_point_population*, hns_sim*, const char* name, int use_masks, const hns_birth_spec*, float* d_xyz, uint32_t* d_voxel,
                                   uint64_t capacity_rows, int append);
typedef struct hns_point_population_info {
    const uint32_t* slot;      /* n entries (device) */
    const uint64_t* counters;  /* {live, wanted} (device) */
    uint64_t n, capacity;
} hns_point_population_info;
int hns_point_population_get(const hns_point_population*, hns_point_population_info*);
int hns_point_population_counts(hns_point_population*, uint64_t* live, uint64_t* wanted);
int hns_grid_birth_points(const hns_grid*, const float* field, const unsigned char* masks, const hns_birth_spec*, uint64_t start, float* xyz, uint32_t* voxel,
                          uint64_t capacity_rows, uint64_t* live, uint64_t* wanted);
/* divergence / divergence_opt (Kernel.cu:455-519) */
int hns_dev_divergence(hns_grid*, const float* vel3, float* div, float inv_dx, void* stream);
/* One colour of redBlackGaussSeidelUpdate(_opt) in place (Kernel.cu:521-623): the two-launch form. */
int hns_dev_rbgs_color(hns_grid*, const float* div, float* p, float dx, float omega, int color, void* stream);
/* `iterations` full (red, black) iterations, starting from p_a and ping-ponging p_a -> p_b -> p_a ... once per LAUNCH.
 * Bit-identical to 2*iterations calls of hns_dev_rbgs_color. How many iterations a launch holds depends on the form the
 * library picks for this grid (hns_grid_rbgs_plan: the temporally blocked form does 2 or 4 per launch, 1 for an odd one left over; "rbgs" = color: two launches per iteration), so
 * WHICH BUFFER HOLDS THE RESULT IS NOT A FUNCTION OF `iterations`: *result_in_b is 1 when it is p_b, 0 when it is p_a
 * (e.g. blocked form: iterations = 2 -> p_b, 4 -> p_b or p_a, 6 -> p_b or p_a). A caller that wants the result must pass
 * result_in_b and read it (NULL is accepted from callers that only time the solve). The other buffer holds an intermediate
 * iterate. p_a and p_b must not alias, and neither may overlap div: any overlap among the three fields is refused (HNS_ERR_INVALID_ARGUMENT, nothing launched).
 * On a grid with a LAUNCH RANGE (hns_grid_set_active_range / _leaves: a multi-GPU rank's boundary / interior / owned leaves) only the leaves
 * of the range are written, and the statement above holds for ONE launch: a temporally blocked launch advances the leaves outside the range
 * inside its tiles instead of reading them as fixed, so its result on the range equals what a WHOLE-grid sweep leaves there -- provided p within
 * 2K voxels of the range and div within 2K - 1 are current in the leaves outside it (K = iterations per launch, hns_grid_rbgs_plan). A second
 * launch reads the other buffer, whose out-of-range leaves the first never wrote: the caller must refresh those voxels in BOTH buffers between
 * launches (hns_dist does: an exchange, or its peers' mirror stores, after every launch). With nothing refreshing them, use one launch per call. */
int hns_dev_rbgs_iterate(hns_grid*, const float* div, float* p_a, float* p_b, float dx, float omega, int iterations, int* result_in_b,
                         void* stream);
/* subtractPressureGradient(_opt) (Kernel.cu:694-829); out3 may alias vel3 -- be the same pointer: the call is then in place -- since each voxel reads only its own velocity */
int hns_dev_subtract_pressure_gradient(hns_grid*, const float* vel3, const float* p, float* out3, const float* sdf, int has_collision, float inv_dx,
                                       void* stream);
/* combustion_oxygen (Kernel.cu:923-966) */
int hns_dev_combustion_oxygen(const float* fuel, const float* waste, const float* temperature, float* divergence, const float* flame,
                              float* out_fuel, float* out_waste, float* out_temperature, float* out_flame, float temp_gain, float expansion,
                              uint64_t n, void* stream);
/* temperature_buoyancy (Kernel.cu:831-847); out3 may alias vel3 (be the same pointer: in place) */
int hns_dev_temperature_buoyancy(const float* vel3, const float* temperature, float* out3, float dt, float ambient, float strength, uint64_t n,
                                 void* stream);
/* vorticityConfinement (Kernel.cu:970-1024), out-of-place (the reference's in-place launch races when factor_scale >= 1): out3 must not alias vel3, any overlap of the
 * two fields is refused (HNS_ERR_INVALID_ARGUMENT, nothing launched) */
int hns_dev_vorticity_confinement(hns_grid*, const float* vel3, float* out3, float dt, float inv_dx, float confinement_scale, float factor_scale,
                                  void* stream);
/* enforceCollisionBoundaries (Kernel.cu:77-116), in place */
int hns_dev_enforce_collision_boundaries(hns_grid*, float* vel3, const float* sdf, float voxel_size, void* stream);

/* Halo support for leaf-partitioned multi-GPU runs: copy whole leaves (512*ncomp floats each; ncomp 1 = float field,
 * 3 = Vec3f field) between a field and a packed buffer. leaf_ids is a DEVICE array of n leaf indices. */
int hns_dev_pack_leaves(const float* field, const int32_t* leaf_ids, uint64_t n, float* packed, int ncomp, void* stream);
int hns_dev_unpack_leaves(const float* packed, const int32_t* leaf_ids, uint64_t n, float* field, int ncomp, void* stream);
/* hns_sim_stats on caller-owned device memory: ncomp records over ALL leaves of the grid (values: leaf_count x 512 x ncomp floats; masks: leaf_count
 * x 64 bytes in device memory, or NULL = every voxel) into d_out, DEVICE memory. The table of per-leaf partial records is kept with the grid (arena
 * pool, made on first use) and shared with hns_dev_residual: calls on one grid must follow each other on one stream. */
int hns_dev_field_stats(hns_grid*, const float* values, int ncomp, const unsigned char* masks, hns_stats* d_out, void* stream);
/* The residual of the pressure solve as the quantity the reference's sweep itself defines: the Gauss-Seidel correction, in the reference's
 * association (Kernel.cu:621),
 *   c = ((pxp + pxm + pyp + pym + pzp + pzm) - div * dx*dx) * 0.166666667f - p
 * all in f32, absent neighbours read as 0 -- omega * c is what the next sweep would add to p. Taken over the leaves of the grid's launch range, all
 * 512 voxels each (the solve ignores active masks, so this does too). In divergence units the residual is -6 c / dx^2. d_out (DEVICE memory)
 * receives ONE record: exactly hns_leaf_stats of the field c over those leaves, same tree. c_out (or NULL; leaf_count x 512 floats) receives c on
 * the leaves of the range, so that tests can see the field. One wave per leaf: p and its six face layers staged in LDS as in the gradient
 * subtraction, the divergence streamed in 16-byte pieces -- 8 B/voxel. The partial table is the grid's (hns_dev_field_stats). */
int hns_dev_residual(hns_grid*, const float* div, const float* p, float dx, float* c_out, hns_stats* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------ */
/* Leaf-partitioned multi-GPU core substep (new: the reference is single-GPU). One hns_dist per rank = per GPU.      */
/* Rank r owns the r-th of `world` equal ranges of the global leaf list in slab order (hns_dist_partition_axis below), */
/* keeps one layer of ghost leaves and refreshes exactly the ghost voxels the next kernel can read (hns_dist_*.hip). */
/* Owned results are bit-identical to the single-domain hns_sim_core_substep -- as long as every tap of an advection   */
/* back-trace that leaves the 27-leaf neighbourhood of its voxel's leaf (|u| dt / dx above ~8 voxels) still lands in   */
/* a leaf this rank holds (owned or ghost: a rank holds ONE layer of ghost leaves). A far tap whose leaf is not here   */
/* may exist on another rank: it is detected on the device and the next hns_dist_*_substep / hns_dist_synchronize /    */
/* hns_dist_download returns HNS_ERR_RUNTIME saying so; hns_dist_upload clears it. (Far taps deep inside a rank are    */
/* answered through the origin hash like on one GPU; a far tap beyond the true edge of the domain is reported too --   */
/* the rank cannot tell it from one beyond its ghost layer. The single-GPU path has no such limit.)                    */
/* ------------------------------------------------------------------------------------------------------------ */

typedef struct hns_dist hns_dist;

typedef struct {
	int world, rank, peers, sweeps_per_exchange;
	uint64_t boundary_leaves, interior_leaves, ghost_leaves; /* local leaf order: [boundary | interior | ghosts] */
	/* per halo region type {advection inputs (whole leaves, global leaf 0 = the element-0 mirror among them), L1 reach 1, div (2k-1), p (2k)}: */
	uint64_t region_voxels_sent[4]; /* voxels this rank sends per exchange of that type (a property of the plan)   */
	uint64_t bytes_sent[4];         /* payload bytes this rank sent during the last substep                          */
	uint64_t messages_sent, exchanges; /* point-to-point messages / exchange rounds of the last substep              */
	uint64_t halo_peers; /* peers this rank exchanges div / p / reach-1 halo voxels with (slab partition: the rank before and the rank behind it);
	                        `peers` also counts ranks it only shares the element-0 mirror of the caller's leaf 0 with (its owner: every rank) */
	uint64_t packed_exchanges; /* exchanges of the last substep whose messages the sweep wrote itself as it stored (no pack launch) */
	uint64_t chained;          /* 1 once connected if this rank runs the CHAINED substep (ipc / local transports, 16^3-block ranks, sweeps_per_exchange = 2: every kernel stores
	                              its boundary values into the peers' ghost voxels itself, no exchanges); 0 = the exchanged substep */
} hns_dist_stats;

/* sweeps_per_exchange (1..4, 0 = default 4): the pressure loop refreshes the ghosts of p after every k-th fused sweep and
 * sweeps the ghost leaves locally in between. n_scalars float fields are advected (the metric's core substep uses 1). */
#define HNS_DIST_DEFAULT 0u
#define HNS_DIST_PLAN_ONLY 1u /* build the partition plan on the host only (inspection / CPU tests); compute calls then fail */
#define HNS_DIST_LEAF_ORDER 2u /* rank r owns leaves [n*r/world, n*(r+1)/world) of the caller's list whatever the domain (the rule of rounds 1-4) */
hns_dist* hns_dist_create(const int32_t* global_leaf_origins_xyz, uint64_t n_leaves, int world, int rank, float voxel_size, int n_scalars,
                          int sweeps_per_exchange, unsigned flags, int* err);
void hns_dist_destroy(hns_dist*);
/* Transport, RCCL over xGMI (one process per GPU): rank 0 calls hns_dist_unique_id and hands the 128 bytes to every rank
 * by any means (torch.distributed broadcast, MPI, a file); every rank then calls hns_dist_connect_rccl (collective). */
int hns_dist_unique_id(void* out128);
int hns_dist_connect_rccl(hns_dist*, const void* unique_id128);
/* Transport, one-sided over mapped peer memory (one process per GPU, xGMI peer access; also between processes sharing one
 * GPU): every rank calls hns_dist_ipc_export, the HNS_DIST_IPC_BLOB_BYTES-byte blobs travel by any host means, every rank
 * calls hns_dist_connect_ipc with all `world` blobs in rank order. A rank then PUTS its messages into the peer's receive
 * buffer / ghost voxels with a copy kernel; the two sides meet through sequence-numbered flags in device memory (bounded
 * waits: a peer that does not answer within 20 s makes the next call fail instead of hanging the device). */
#define HNS_DIST_IPC_BLOB_BYTES 2048
int hns_dist_ipc_export(hns_dist*, void* out_blob);
int hns_dist_connect_ipc(hns_dist*, const void* blobs_of_all_ranks);
/* Transport, local: all `world` ranks live in this process on ONE device; a message is a device copy out of the peer's
 * send buffer. Same plan, kernels, streams and events as the RCCL path (tests; per-rank overhead without a wire). */
int hns_dist_connect_local(hns_dist* const* ranks, int world);
/* Transport, loopback (TIMING ONLY, results are meaningless): this rank alone, every message answered with the rank's own
 * payload of the same size. Measures what one rank costs next to the single-GPU substep before any wire time. */
int hns_dist_connect_loopback(hns_dist*);
/* The same with every message carried by RCCL (a one-rank communicator, sends and receives to itself in the groups the
 * multi-rank path issues): what a single-GPU box can check of the RCCL path. Leaves what the copy-based loopback leaves. */
int hns_dist_connect_loopback_rccl(hns_dist*);
uint64_t hns_dist_owned_leaves(const hns_dist*);
/* Which leaves a rank owns (round 5): the leaves in SLAB order -- by leaf coordinate along the axis whose cuts cross the fewest leaves, the
 * caller's order inside a plane -- cut into `world` equal ranges, so that a rank exchanges halos with the rank before and the rank behind
 * it only (BASELINE config 5 in 8 ranks: 2 halo peers instead of 7). Where the x cut selects the same leaf sets as contiguous ranges of the
 * caller's list (box domains made of whole 128-voxel NanoVDB nodes per rank) the caller's order is kept: hns_dist_partition_axis = -1 and
 * hns_dist_first_owned_leaf = the first leaf of the contiguous run. Otherwise hns_dist_partition_axis = 0 / 1 / 2, hns_dist_first_owned_leaf
 * = ~0, and hns_dist_owned_leaf_ids lists the owned leaves (positions in the caller's list) in the order hns_dist_upload / _download expect. */
uint64_t hns_dist_first_owned_leaf(const hns_dist*);
int hns_dist_owned_leaf_ids(const hns_dist*, int64_t* out_global_ids); /* hns_dist_owned_leaves entries */
int hns_dist_partition_axis(const hns_dist*);
/* sweeps_per_exchange to create the ranks with for the chained one-sided substep (ipc / local transports) of `world` ranks over n_leaves leaves: 2 = the
 * temporally blocked chained sweep, two iterations per launch, where every rank's range is large enough for 16^3 blocks under the current options; else 1 */
int hns_dist_one_sided_sweeps(uint64_t n_leaves, int world);
int hns_dist_info(const hns_dist*, hns_dist_stats* out);
/* The plan (also on PLAN_ONLY handles): global id of every local leaf in local order [boundary | interior | ghosts]; the
 * rank of peer i (-1 beyond the last); and per peer, halo region type (0..3 as in hns_dist_stats) and direction the
 * local leaves whose voxels travel plus a 64-byte mask each (byte x*8+y, bit z). Any output pointer may be NULL. */
int hns_dist_local_leaves(const hns_dist*, int64_t* out_global_ids);
int hns_dist_peer_rank(const hns_dist*, int peer);
int hns_dist_peer_region(const hns_dist*, int peer, int type, int is_send, int32_t* leaves, unsigned char* masks, uint64_t* n_leaves, uint64_t* n_voxels);
/* Host arrays over the OWNED leaves in the order of hns_dist_owned_leaf_ids (vel3: 512*3 floats per leaf, each scalar 512 per leaf).
 * Collective in effect: every rank uploads before the next substep (the first exchange then carries the new fields).
 * Synchronous. download: any pointer may be NULL; `pressure` receives the last solve's p. */
int hns_dist_upload(hns_dist*, const float* vel3, const float* const* scalars, void* stream);
int hns_dist_download(hns_dist*, float* vel3, float* const* scalars, float* pressure, void* stream);
/* Diagnostics: one field over ALL local leaves, ghosts included, in local order (hns_dist_local_leaves), as the device holds it
 * now; which = -2: the last solve's p, -1: velocity (3 floats per voxel), s >= 0: scalar s. Synchronous. With
 * hns_dist_peer_region it lets a driver check that a rank's ghost voxels equal their owners' values (DistRank.ghost_check). */
int hns_dist_download_local(hns_dist*, int which, float* out, void* stream);
/* One core substep of this rank, asynchronous on `stream` and on the rank's communication stream (RCCL transport, or world 1). */
int hns_dist_core_substep(hns_dist*, int iterations, float dt, void* stream);
/* The same for locally connected ranks: all of them advance together, phase by phase, on `stream`. */
int hns_dist_local_core_substep(hns_dist* const* ranks, int world, int iterations, float dt, void* stream);
/* hipEvent bracketing of the pressure loops (halo exchanges included), as hns_sim_timing / hns_sim_pressure_time. */
int hns_dist_timing(hns_dist*, int max_solves);
/* The whole Compute_Sim substep on the partitioned domain (reference HNanoSolver.cu:150-356; single GPU: hns_sim_substep): collision,
 * advect_vector, vorticity confinement, divergence, combustion, buoyancy, the pressure solve, gradient subtraction, collision, and the
 * advection of every float field except collision_sdf. field_index[5]: the positions of fuel, waste, temperature, flame and
 * collision_sdf (-1: none) among the rank's scalars in hns_dist_upload order. Every kernel boundary a stencil crosses is a halo
 * exchange (vorticity confinement reads whole ghost leaves of u*); the pointwise kernels run on the owned leaves. Owned results are
 * bit-identical to hns_sim_substep on the whole domain (tests/test_dist_gpu.py). factor_scale must stay within 0..6. */
int hns_dist_sim_substep(hns_dist*, int iterations, float dt, const hns_combustion_params*, const int* field_index, int has_collision, void* stream);
int hns_dist_local_sim_substep(hns_dist* const* ranks, int world, int iterations, float dt, const hns_combustion_params*, const int* field_index, int has_collision,
                               void* stream);
int hns_dist_pressure_time(hns_dist*, float* total_ms, long long* sweeps);
int hns_dist_synchronize(hns_dist*, void* stream); /* waits for `stream` and the communication stream */

/* Timing helper: runs `iterations` fused RB-SOR iterations `reps` times on `stream`, bracketing each launch group with
 * hipEvents on that stream, and returns the mean milliseconds per fused-iteration launch. */
int hns_dev_time_rbgs(hns_grid*, const float* div, float* p_a, float* p_b, float dx, float omega, int iterations, int reps, float* ms_per_launch,
                      void* stream);

/* Which kernel form hns_dev_rbgs_iterate / the operators' pressure loops use for `iterations` iterations on this grid under the
 * current options, as text (e.g. "k_rbgs_block<2,2>: 2 iterations per launch on 16^3-voxel blocks"), and how many kernel launches
 * that is. For bench / profile labels; `description` may be null. */
int hns_grid_rbgs_plan(hns_grid*, int iterations, char* description, uint64_t description_bytes, int* launches, int* iterations_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* HNS_H */
