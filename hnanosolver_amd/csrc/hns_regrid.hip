// hns_regrid.hip -- what the HNanoSolver SOP does to the domain between two cooks, on the device: dilate the velocity's active topology by `padding`
// voxels, unite it with the collision SDF's leaves (reference src/SOP/HNanoSolver/SOP_HNanoSolver.cpp:186-199) and carry every field into the new leaf
// set, filled the way HNS::IndexGridBuilder fills leaves a source lacks (src/Utils/GridBuilder.hpp:99-154). The host chain that does the same
// (hns_sim_download -> hns_dilate_leaf_masks -> hns_union_leaves -> hns_gather_leaves -> new grid -> hns_sim_upload) moves every field over PCIe
// twice; here only leaf origins cross (12 bytes per leaf each way) plus, when a collision SDF source is given, that source.
//
// hns_sim_regrid_sourced first adds a frame's SOURCES into the fields (SOP_HNanoSolver.cpp:159-179: compSum of the emitter into the feedback grids,
// before the domain is built from the summed velocity). Only the source leaves cross PCIe; the sum is formed in the field phase, the velocity
// source's leaves and masks join the domain through the candidate and mask phases (dilation distributes over the union, so nothing is pre-merged).
//
// hns_sim_regrid_seeded unites the velocity's topology with the seeds of a device-resident point set (hns_seed.hip) before the dilation: one more entry of the source
// list, of a kind that comes from the device and has no values. Its leaves and masks are dilation seeds exactly as the velocity source's are (phases 1 and 3) and take part
// in nothing else; the two sets are never merged. Only the seeds' leaf count crosses PCIe.
//
// The collision SDF is one more entry of the same source list (Source), of its own kind: its leaves join the domain undilated, its masks are ORed
// in undilated and its values replace collision_sdf instead of being added. Every entry is validated, staged, uploaded and hashed by origin
// (duplicates are refused) the same way, and all but the velocity's (the mask waves find its leaves) are indexed into the new grid by one kernel.
//
//   1. candidates  one thread per (old leaf, offset in the (2R+1)^3 leaf neighbourhood), R = ceil(p / 8), one per SDF leaf and one per (velocity source
//                  leaf, offset): a hit (the leaf's active voxels reach the candidate's box, hns_dilate.hpp) claims a slot of a fresh claim table
//                  (hns_originhash.hpp), which is then compacted. Each source's leaves go into an index table of their own
//   2. order       the origins come to the host, are sorted into OpenVDB leaf order and become a new hns_grid through the usual path (Topology::prepare,
//                  hns_grid_upload: hash, nbr27, launch order); the source values are uploaded meanwhile
//   3. masks       one wave per new leaf gathers the masks of the old leaves and velocity source leaves within reach (their origin hashes), dilates
//                  each separably into its own box, ORs them across the wave and ORs in the SDF leaf's mask; the same wave records which old leaf and
//                  which velocity source leaf (if any) has this origin. Every other source's leaves are indexed into the new grid
//   4. fields      velocity and every float field, 16 bytes per load and store, from the old leaf (collision_sdf: the SDF leaf, when an SDF is given)
//                  or the fill (zeros; bytes 0x01 for collision_sdf), into a fresh arena from the pool; a field with a velocity or float source gets
//                  (old or +0) + (source or +0) instead
//   5. commit      the duplicate refusals the device raised; then the sim moves onto the new grid and the old arena goes back to the pool. Nothing
//                  before this step touches the sim's state
//
// hns_sim_deactivate, at the end of a frame, clears the mask bits of voxels whose listed fields are all within tolerance (the reference's commented-out
// deactivate, GridBuilder.hpp:213-214), so that the next regrid can drop leaves no active voxel reaches: one wave per leaf, a ballot per 64 voxels.
//
// Everything that decides a result is order-free: hash slots hold the smallest thing that identifies a candidate (its thread id), the compacted
// order is discarded by the sort, the mask OR is commutative and a source hash is only ever asked for an origin it holds once. Two runs give the
// same bytes.
#include <algorithm>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "hns_device.hpp"
#include "hns_dilate.hpp"
#include "hns_seed.hpp"

namespace hns {
namespace {

constexpr uint64_t kMaxCandidates = uint64_t(1) << 23;  // distinct leaves the candidate hash may hold (the grid limit is 2^22: Topology::prepare)
constexpr int kCopyFields = 16;                          // float fields per copy or add launch
constexpr uint32_t kSdfFill = 0x01010101u;               // collision_sdf where no leaf has a value: memset(..., 1, ...) (GridBuilder.hpp:108)

__device__ __forceinline__ void load_mask(const unsigned char* masks, int l, uint64_t (&m)[8]) {
	const uint64_t* w = masks ? (const uint64_t*)(masks + 64 * (size_t)l) : nullptr;
#pragma unroll
	for (int x = 0; x < 8; ++x) m[x] = w ? w[x] : ~0ull;
}

// A set of leaves whose masks are dilated into the domain besides the sim's own: [kVsrcSeeds] the velocity source's, [kPointSeeds] the seeds of a point set.
constexpr int kVsrcSeeds = 0, kPointSeeds = 1, kSeedSets = 2;
struct MaskedLeaves {
	const int4* origins;
	const unsigned char* masks;  // null: every voxel active
	uint64_t n_dil;               // (leaf, offset) pairs
};

// The candidate a thread id stands for: ids [0, n_dil) are (old leaf, offset) pairs, ids [n_dil, n_dil + n_sdf) the SDF leaves, then the (leaf, offset)
// pairs of seeds[0] and behind them those of seeds[1].
struct Candidates {
	const int4* old_origins;
	const unsigned char* old_masks;  // null: every voxel active
	const int4* sdf;
	MaskedLeaves seeds[kSeedSets];
	uint64_t n_dil, n_sdf;
	__host__ __device__ uint64_t total() const { return n_dil + n_sdf + seeds[0].n_dil + seeds[1].n_dil; }
	int side, R, p;
	unsigned long long* table;
	uint32_t mask;
	unsigned long long cap;
	unsigned long long* count;  // (claim_slot states it)
};

// l: the old or seed-set leaf whose active voxels (`masks`) must reach the candidate, -1 for an SDF leaf
__device__ __forceinline__ bool cand_origin(const Candidates& c, uint64_t t, int& x, int& y, int& z, int& l, int (&d)[3], const unsigned char*& masks) {
	const int4* origins = c.old_origins;
	masks = c.old_masks;
	if (t >= c.n_dil) {
		if (t < c.n_dil + c.n_sdf) {
			const int4 o = c.sdf[t - c.n_dil];
			x = o.x, y = o.y, z = o.z, l = -1;
			return true;
		}
		t -= c.n_dil + c.n_sdf;
		const int k = t < c.seeds[0].n_dil ? 0 : 1;
		if (k) t -= c.seeds[0].n_dil;
		origins = c.seeds[k].origins, masks = c.seeds[k].masks;
	}
	const uint64_t K = (uint64_t)c.side * c.side * c.side;
	l = (int)(t / K);
	const int k = (int)(t - (uint64_t)l * K);
	d[0] = k / (c.side * c.side) - c.R, d[1] = (k / c.side) % c.side - c.R, d[2] = k % c.side - c.R;
	const int4 o = origins[l];
	const int64_t nx = (int64_t)o.x + 8 * d[0], ny = (int64_t)o.y + 8 * d[1], nz = (int64_t)o.z + 8 * d[2];
	if (nx < INT32_MIN || nx > INT32_MAX - 7 || ny < INT32_MIN || ny > INT32_MAX - 7 || nz < INT32_MIN || nz > INT32_MAX - 7) return false;
	x = (int)nx, y = (int)ny, z = (int)nz;
	return true;
}

__global__ __launch_bounds__(256) void k_regrid_candidates(Candidates c) {
	const uint64_t total = c.total();
	for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
		int x, y, z, l, d[3] = {0, 0, 0};
		const unsigned char* ms;
		if (!cand_origin(c, t, x, y, z, l, d, ms)) continue;
		if (l >= 0) {  // a hit iff the leaf's active voxels, dilated by p, reach the candidate's box (hns_dilate_leaves' slab test)
			uint64_t m[8], out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
			load_mask(ms, l, m);
			if (!dilate_into(m, -8 * d[0], -8 * d[1], -8 * d[2], c.p, out)) continue;
		}
		claim_slot(c.table, c.mask, c.cap, c.count, hash_origin(x, y, z) & c.mask, (unsigned long long)t, [&](unsigned long long cur) {
			int qx, qy, qz, ql, qd[3];
			const unsigned char* qm;
			cand_origin(c, cur, qx, qy, qz, ql, qd, qm);  // (an id in the table always stands for a valid origin)
			return qx == x && qy == y && qz == z;
		});
	}
}

// one thread per slot, whole waves
__global__ __launch_bounds__(256) void k_regrid_compact(Candidates c, int4* __restrict__ out) {
	const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	const unsigned long long t = s <= c.mask ? c.table[s] : kEmptySlot;
	const uint32_t i = wave_compact(t != kEmptySlot, &c.count[2]);
	if (t == kEmptySlot) return;
	int x, y, z, l, d[3];
	const unsigned char* m;
	cand_origin(c, t, x, y, z, l, d, m);
	out[i] = make_int4(x, y, z, 0);
}

// A source's leaves into its index table of `mask + 1` (>= 2 n) slots. Two leaves on one origin raise *dup.
__global__ __launch_bounds__(256) void k_regrid_src_hash(const int4* __restrict__ origins, int n, int* __restrict__ table, uint32_t mask, int* __restrict__ dup) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i < n && insert_origin(origins, table, mask, i) >= 0) *dup = 1;
}

// idx[new leaf] = the source leaf with its origin; two such leaves on one origin raise *dup. Leaves outside the new grid are skipped (every SDF leaf
// is a leaf of the new grid; a float source's may not be).
__global__ __launch_bounds__(256) void k_regrid_src_index(GridDev ng, const int4* __restrict__ origins, int n, int* __restrict__ idx, int* __restrict__ dup) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int4 o = origins[i];
	const int b = d_find_leaf(ng, o.x, o.y, o.z);
	if (b >= 0 && atomicCAS(&idx[b], -1, i) != -1) *dup = 1;
}

// The seed sets of k_regrid_masks by origin (h.table null: none) with their masks (null: every voxel active)
struct SeedHashes {
	OriginIndex h[kSeedSets];
	const unsigned char* masks[kSeedSets];
};

// A float source's indices under point seeds: a leaf the unseeded regrid would not hold takes nothing from the source (k_regrid_masks: unseeded)
__global__ __launch_bounds__(256) void k_regrid_src_unseeded(int* __restrict__ idx, const int* __restrict__ unseeded, int n_new) {
	const int b = blockIdx.x * 256 + threadIdx.x;
	if (b < n_new && !unseeded[b]) idx[b] = -1;
}

// One wave per new leaf: its dilated mask (OR over the old leaves and the leaves of either seed set within reach, then the SDF leaf's mask), the old leaf with
// its origin (map, -1 = new) and, with a velocity source (sh.h[kVsrcSeeds].table != null), its leaf with that origin (vmap, -1 = none).
// With point seeds a leaf may be in the domain through them alone: the unseeded regrid would not hold it, so it takes no value from anywhere -- map and vmap are -1
// there and unseeded[leaf] (given with point seeds) is 0, for the float sources' indices. The leaf is in the unseeded domain iff an old or velocity source leaf
// contributed to its mask (hns_dilate_leaf_masks' test) or it is an SDF leaf.
__global__ __launch_bounds__(256) void k_regrid_masks(GridDev og, const unsigned char* __restrict__ old_masks, const int4* __restrict__ new_origins, int n_new, int p, int R,
                                                      const int* __restrict__ sdf_idx, const unsigned char* __restrict__ sdf_masks, SeedHashes sh,
                                                      uint64_t* __restrict__ new_masks, int* __restrict__ map, int* __restrict__ vmap, int* __restrict__ unseeded) {
	const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (b >= n_new) return;
	const int4 o = new_origins[b];
	const int side = 2 * R + 1, K = side * side * side, centre = (K - 1) / 2;
	uint64_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	int own = -1, vown = -1;
	bool reached = false;  // by an old or a velocity source leaf
	for (int k = lane; k < K; k += 64) {
		const int d[3] = {k / (side * side) - R, (k / side) % side - R, k % side - R};
		const int64_t nx = (int64_t)o.x + 8 * d[0], ny = (int64_t)o.y + 8 * d[1], nz = (int64_t)o.z + 8 * d[2];
		const bool in_range = nx >= INT32_MIN && nx <= INT32_MAX && ny >= INT32_MIN && ny <= INT32_MAX && nz >= INT32_MIN && nz <= INT32_MAX;
		int l = -1;
		if (og.n_leaves > 0 && in_range) l = d_find_leaf(og, (int)nx, (int)ny, (int)nz);
		int sl[kSeedSets];
#pragma unroll
		for (int q = 0; q < kSeedSets; ++q) sl[q] = sh.h[q].table && in_range ? find_origin(sh.h[q], (int)nx, (int)ny, (int)nz) : -1;
		if (k == centre) own = l, vown = sl[kVsrcSeeds];
		uint64_t m[8];
		if (l >= 0) {
			load_mask(old_masks, l, m);
			reached |= dilate_into(m, 8 * d[0], 8 * d[1], 8 * d[2], p, acc);
		}
#pragma unroll
		for (int q = 0; q < kSeedSets; ++q)
			if (sl[q] >= 0) {
				load_mask(sh.masks[q], sl[q], m);
				const bool hit = dilate_into(m, 8 * d[0], 8 * d[1], 8 * d[2], p, acc);
				if (q == kVsrcSeeds) reached |= hit;
			}
	}
	const int si = sdf_idx ? sdf_idx[b] : -1;
	const bool in_unseeded = !sh.h[kPointSeeds].table || __ballot(reached) != 0 || si >= 0;
	if (lane == centre % 64) {  // (the lane that met the leaf's own origin)
		map[b] = in_unseeded ? own : -1;
		if (sh.h[kVsrcSeeds].table) vmap[b] = in_unseeded ? vown : -1;
		if (unseeded) unseeded[b] = in_unseeded;
	}
#pragma unroll
	for (int x = 0; x < 8; ++x) acc[x] = wave_or64(acc[x], true);
	if (lane < 8) {
		uint64_t w = 0;
#pragma unroll
		for (int x = 0; x < 8; ++x) w = lane == x ? acc[x] : w;
		if (si >= 0) w |= sdf_masks ? ((const uint64_t*)(sdf_masks + 64 * (size_t)si))[lane] : ~0ull;
		new_masks[(size_t)b * 8 + lane] = w;
	}
}

// The fields of one copy or add launch, blockIdx.y = field.
struct FieldSet {
	const float4* a[kCopyFields];   // the old field (collision_sdf with an SDF: the SDF's leaves)
	const int* map_a[kCopyFields];  // new leaf -> leaf of a, -1 = none
	const float4* b[kCopyFields];   // add: the source's leaves
	const int* map_b[kCopyFields];  // add: new leaf -> source leaf, -1 = none
	float4* dst[kCopyFields];
	uint32_t fill[kCopyFields];     // copy: the bytes of a new leaf that a lacks
};

// NC = floats per voxel (3: the velocity, AoS). Each thread moves four 16-byte pieces, all four loads in flight before the stores.
template <int NC>
__global__ __launch_bounds__(256) void k_regrid_copy(FieldSet fs, uint32_t n_f4) {
	constexpr uint32_t per_leaf = 128u * NC;
	const int f = blockIdx.y;
	const float4* __restrict__ src = fs.a[f];
	float4* __restrict__ dst = fs.dst[f];
	const int* __restrict__ map = fs.map_a[f];
	const float fv = __uint_as_float(fs.fill[f]);
	const uint32_t base = blockIdx.x * 1024u + threadIdx.x;
	float4 v[4];
#pragma unroll
	for (int j = 0; j < 4; ++j) {
		const uint32_t e = base + 256u * j;
		v[j] = make_float4(fv, fv, fv, fv);
		if (e < n_f4) {
			const uint32_t leaf = e / per_leaf;
			const int l = map[leaf];
			if (l >= 0) v[j] = src[(size_t)l * per_leaf + (e - leaf * per_leaf)];
		}
	}
#pragma unroll
	for (int j = 0; j < 4; ++j) {
		const uint32_t e = base + 256u * j;
		if (e < n_f4) dst[e] = v[j];
	}
}

// A sourced field (compSum, then the gather): (old or +0) + (source or +0) in f32, the k_regrid_copy layout. All eight loads in flight before the adds.
template <int NC>
__global__ __launch_bounds__(256) void k_regrid_add(FieldSet fs, uint32_t n_f4) {
	constexpr uint32_t per_leaf = 128u * NC;
	const int f = blockIdx.y;
	const float4* __restrict__ a = fs.a[f];
	const float4* __restrict__ b = fs.b[f];
	float4* __restrict__ dst = fs.dst[f];
	const int* __restrict__ map_a = fs.map_a[f];
	const int* __restrict__ map_b = fs.map_b[f];
	const uint32_t base = blockIdx.x * 1024u + threadIdx.x;
	float4 va[4], vb[4];
#pragma unroll
	for (int j = 0; j < 4; ++j) {
		const uint32_t e = base + 256u * j;
		va[j] = vb[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (e < n_f4) {
			const uint32_t leaf = e / per_leaf, r = e - leaf * per_leaf;
			const int la = map_a[leaf], lb = map_b[leaf];
			if (la >= 0) va[j] = a[(size_t)la * per_leaf + r];
			if (lb >= 0) vb[j] = b[(size_t)lb * per_leaf + r];
		}
	}
#pragma unroll
	for (int j = 0; j < 4; ++j) {
		const uint32_t e = base + 256u * j;
		if (e < n_f4) dst[e] = make_float4(va[j].x + vb[j].x, va[j].y + vb[j].y, va[j].z + vb[j].z, va[j].w + vb[j].w);
	}
}

// nf fields of nc floats per voxel: k_regrid_add where they have a source to add, else k_regrid_copy
int launch_fields(const FieldSet& fs, int nf, int nc, bool add, uint64_t n_new, hipStream_t st) {
	if (!nf) return HNS_OK;
	const uint32_t n_f4 = (uint32_t)(n_new * 128u * (uint64_t)nc);
	void (*k)(FieldSet, uint32_t) = nc == 3 ? (add ? k_regrid_add<3> : k_regrid_copy<3>) : (add ? k_regrid_add<1> : k_regrid_copy<1>);
	k<<<dim3((n_f4 + 1023u) / 1024u, (unsigned)nf), 256, 0, st>>>(fs, n_f4);
	HNS_HIP(hipGetLastError());
	return HNS_OK;
}

// (Scratch, the device allocations of one regrid: hns_pool.hpp)

// One entry of the regrid's source list: the collision SDF or one source of hns_sim_regrid_sourced, validated, and where its leaves live on the
// device. The kinds differ in three places only: the velocity's leaves are dilated candidates (phase 1) and its masks are dilated into the new
// ones (phase 3), the SDF's leaves and masks join as they are; the SDF's values replace collision_sdf, with the 0x01 byte fill (phase 4), a
// velocity or float source is added to its field. A float source's masks never enter the domain. The seeds of a point set (kPoints) come from the device
// (hns_seed.hip: origins and masks point into the scratch, l holds the leaf count only) and have no values: they are treated like the velocity's in phases 1 and 3
// and are in no field's sum; their origins are distinct by construction, so their duplicate flag never rises.
struct Source {
	enum Kind { kVelocity, kFloat, kSdf, kPoints } kind = kFloat;
	hns_leaf_source l{};  // the caller's entry (the SDF's: its arguments of hns_sim_regrid)
	int index = -1;       // in the caller's list (-1: the SDF)
	int field = -1;       // float field index (the SDF's: collision_sdf), -1 = the velocity
	std::vector<int32_t> o4;  // the origins as int4 (host staging of the upload)
	int4* origins = nullptr;
	int* table = nullptr;  // its index table (OriginIndex)
	uint32_t mask = 0;
	unsigned char* masks = nullptr;  // where they enter the domain (velocity, SDF); null = every voxel active
	float* values = nullptr;
	int* idx = nullptr;  // new leaf -> source leaf, -1 = none (phase 3)
	const char* name() const { return l.name ? l.name : "(null)"; }
};

// 8-aligned origins, checked alike for the SDF and every source (the other checks of a source do not apply to the SDF: it has no leaf limit, and
// regrid_entry refuses its NULL arrays)
int check_origins(const Source& q, const char* who) {
	for (uint64_t k = 0; k < 3 * q.l.n_leaves; ++k)
		if (q.l.origins[k] & 7) {
			if (q.kind == Source::kSdf)
				set_error("%s: SDF leaf origin %llu is not 8-aligned", who, (unsigned long long)(k / 3));
			else
				set_error("%s: source %d ('%s'): leaf origin %llu is not 8-aligned", who, q.index, q.name(), (unsigned long long)(k / 3));
			return HNS_ERR_TOPOLOGY;
		}
	return HNS_OK;
}

// One regrid of s: its source list, its device scratch and what each phase hands the next. The sim is only touched by commit().
struct Regrid {
	hns_sim* s;
	int p, R;
	hipStream_t st;
	const char* who;
	std::vector<Source> srcs;  // the SDF first, when given, then the caller's sources (before the scratch: its staging outlives the device work)
	Source* vsrc = nullptr;    // the velocity's source, if any
	Source* sdf = nullptr;
	Source* points = nullptr;  // the seeds of the point set, if any
	Scratch scratch;
	std::unique_ptr<hns_grid, void (*)(hns_grid*)> ng{nullptr, hns_grid_destroy};
	Candidates c{};
	int4* compact = nullptr;
	int* dup = nullptr;  // one duplicate flag per source
	uint64_t n_new = 0;
	int* map = nullptr;  // new leaf -> old leaf, -1 = new
	int* unseeded = nullptr;  // with point seeds: is the new leaf one of the unseeded domain's?
	void* new_masks = nullptr;
	void* new_fields = nullptr;
	size_t i_masks = 0, i_fields = 0;  // their blocks in scratch.held

	Regrid(hns_sim* sim, int padding, hipStream_t stream, const char* w) : s(sim), p(padding), R((padding + 7) / 8), st(stream), who(w), scratch(sim->device) {}

	// ---- 0. the source list, checked; `sdf_src` is the SDF (given iff its values are); with_points: an entry for the seeds of a point set, filled by seeds() ----
	int sources(const hns_leaf_source& sdf_src, const hns_leaf_source* src, int n_src, bool with_points) {
		if (sdf_src.values) {
			Source q;
			q.kind = Source::kSdf, q.l = sdf_src, q.field = s->find("collision_sdf");
			if (q.field < 0) {
				set_error("%s: a collision SDF source was given but the sim has no field 'collision_sdf'", who);
				return HNS_ERR_INVALID_ARGUMENT;
			}
			HNS_TRY(check_origins(q, who));
			srcs.push_back(q);
		}
		if (n_src < 0 || (n_src > 0 && !src)) {
			set_error("%s: bad source list", who);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		std::vector<char> taken(s->names.size() + 1, 0);  // [names.size()]: the velocity
		for (int i = 0; i < n_src; ++i) {
			const hns_leaf_source& l = src[i];
			const char* nm = l.name ? l.name : "(null)";
			if (l.ncomp != 1 && l.ncomp != 3) {
				set_error("%s: source %d ('%s'): ncomp %d (1 or 3)", who, i, nm, l.ncomp);
				return HNS_ERR_INVALID_ARGUMENT;
			}
			const int f = l.name ? s->find(l.name) : -1;
			if (l.name && !strcmp(l.name, "collision_sdf")) {
				set_error("%s: source %d: 'collision_sdf' cannot be a source (the SDF comes from the collision input, never from the feedback)", who, i);
				return HNS_ERR_INVALID_ARGUMENT;
			}
			if (l.ncomp == 1 && f < 0) {
				set_error("%s: source %d: the sim has no float field '%s'", who, i, nm);
				return HNS_ERR_INVALID_ARGUMENT;
			}
			if (l.ncomp == 3 && f >= 0) {
				set_error("%s: source %d: ncomp 3 under the float field name '%s'", who, i, nm);
				return HNS_ERR_INVALID_ARGUMENT;
			}
			const size_t slot = l.ncomp == 3 ? s->names.size() : (size_t)f;
			if (taken[slot]) {
				if (l.ncomp == 3)
					set_error("%s: source %d: a second velocity source", who, i);
				else
					set_error("%s: source %d: a second source for '%s'", who, i, nm);
				return HNS_ERR_INVALID_ARGUMENT;
			}
			taken[slot] = 1;
			if (l.n_leaves && (!l.origins || !l.values)) {
				set_error("%s: source %d ('%s'): origins or values NULL with %llu leaves", who, i, nm, (unsigned long long)l.n_leaves);
				return HNS_ERR_INVALID_ARGUMENT;
			}
			if (l.n_leaves > (uint64_t(1) << 22)) {
				set_error("%s: source %d ('%s'): %llu leaves exceed the 2^22-leaf limit", who, i, nm, (unsigned long long)l.n_leaves);
				return HNS_ERR_INVALID_ARGUMENT;
			}
			Source q;
			q.kind = l.ncomp == 3 ? Source::kVelocity : Source::kFloat, q.l = l, q.index = i, q.field = l.ncomp == 3 ? -1 : f;
			HNS_TRY(check_origins(q, who));
			srcs.push_back(q);
		}
		if (with_points) {
			Source q;
			q.kind = Source::kPoints, q.l.name = "(points)";
			srcs.push_back(q);
		}
		for (Source& q : srcs) {
			if (q.kind == Source::kVelocity) vsrc = &q;
			if (q.kind == Source::kSdf) sdf = &q;
			if (q.kind == Source::kPoints) points = &q;
		}
		return HNS_OK;
	}

	// ---- the seeds of the point set, on the device (hns_seed.hip); timed with the candidates ----
	int seeds(const float* d_xyz, uint64_t n, uint64_t* skipped) {
		if (!points) return HNS_OK;  // (candidates() opens the first phase where it always did)
		HNS_HIP(hipEventRecord(s->rev[0], st));
		SeedSet S;
		HNS_TRY(seed_leaves(scratch, d_xyz, n, st, who, &S));
		points->l.n_leaves = S.n_leaves, points->origins = S.origins, points->masks = S.masks;
		if (skipped) *skipped = S.skipped;
		return HNS_OK;
	}

	// ---- 1. candidates: every source's origins (and masks where they enter the domain) go up and into its origin hash; the candidate hash ----
	int candidates() {
		const hns_grid* og = s->grid;
		const uint64_t K = (uint64_t)(2 * R + 1) * (2 * R + 1) * (2 * R + 1);
		c.old_origins = (const int4*)og->d_origins, c.old_masks = s->d_masks.as<unsigned char>();
		c.n_dil = (uint64_t)og->topo.n_leaves * K, c.n_sdf = sdf ? sdf->l.n_leaves : 0;
		c.seeds[kVsrcSeeds].n_dil = vsrc ? vsrc->l.n_leaves * K : 0, c.seeds[kPointSeeds].n_dil = points ? points->l.n_leaves * K : 0;
		c.side = 2 * R + 1, c.R = R, c.p = p;
		const uint64_t total = c.total();
		c.cap = std::min<uint64_t>(total, kMaxCandidates);
		const uint64_t T = hash_slots(2 * c.cap);
		c.mask = (uint32_t)(T - 1);
		for (Source& q : srcs) {
			const uint64_t n = q.l.n_leaves;
			q.mask = (uint32_t)(hash_slots(2 * n) - 1);
			if (q.kind == Source::kPoints) continue;  // (already on the device)
			q.o4.assign((size_t)n * 4, 0);
			for (uint64_t i = 0; i < n; ++i)
				for (int a = 0; a < 3; ++a) q.o4[4 * i + a] = q.l.origins[3 * i + a];
		}
		HNS_TRY(scratch.carve([&](auto&& slice) {
			slice(c.table, 8 * T);
			slice(compact, 16 * std::max<uint64_t>(c.cap, 1));
			slice(c.count, 256);
		}));
		if (!srcs.empty())  // (an allocation of their own: the arena pool then serves a regrid with sources as it serves one without)
			HNS_TRY(scratch.carve([&](auto&& slice) {
				slice(dup, 4 * srcs.size());
				for (Source& q : srcs) {
					const uint64_t n1 = std::max<uint64_t>(q.l.n_leaves, 1);
					slice(q.table, 4 * ((uint64_t)q.mask + 1));
					if (q.kind == Source::kPoints) continue;
					slice(q.origins, 16 * n1);
					if (q.kind != Source::kFloat && q.l.masks) slice(q.masks, 64 * n1);
					slice(q.values, 2048 * (uint64_t)q.l.ncomp * n1);
				}
			}));
		c.sdf = sdf ? sdf->origins : nullptr;
		if (vsrc) c.seeds[kVsrcSeeds].origins = vsrc->origins, c.seeds[kVsrcSeeds].masks = vsrc->masks;
		if (points) c.seeds[kPointSeeds].origins = points->origins, c.seeds[kPointSeeds].masks = points->masks;
		if (!points) HNS_HIP(hipEventRecord(s->rev[0], st));
		HNS_HIP(hipMemsetAsync(c.table, 0xFF, 8 * T, st));
		HNS_HIP(hipMemsetAsync(c.count, 0, 256, st));
		if (!srcs.empty()) HNS_HIP(hipMemsetAsync(dup, 0, 4 * srcs.size(), st));
		for (size_t i = 0; i < srcs.size(); ++i) {
			Source& q = srcs[i];
			const uint64_t n = q.l.n_leaves;
			HNS_HIP(hipMemsetAsync(q.table, 0xFF, 4 * ((size_t)q.mask + 1), st));
			if (!n) continue;
			if (q.kind != Source::kPoints) {
				HNS_HIP(hipMemcpyAsync(q.origins, q.o4.data(), 16 * n, hipMemcpyHostToDevice, st));
				if (q.masks) HNS_HIP(hipMemcpyAsync(q.masks, q.l.masks, 64 * n, hipMemcpyHostToDevice, st));
			}
			k_regrid_src_hash<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(q.origins, (int)n, q.table, q.mask, dup + i);
			HNS_HIP(hipGetLastError());
		}
		if (total) {
			k_regrid_candidates<<<(unsigned)std::min<uint64_t>((total + 255) / 256, 1u << 20), 256, 0, st>>>(c);
			HNS_HIP(hipGetLastError());
			k_regrid_compact<<<(unsigned)(T / 256 ? T / 256 : 1), 256, 0, st>>>(c, compact);
			HNS_HIP(hipGetLastError());
		}
		HNS_HIP(hipEventRecord(s->rev[1], st));
		unsigned long long counts[3] = {0, 0, 0};
		HNS_HIP(hipMemcpyAsync(counts, c.count, sizeof(counts), hipMemcpyDeviceToHost, st));
		HNS_HIP(hipStreamSynchronize(st));
		if (counts[1] || counts[2] > (uint64_t(1) << 22)) {
			set_error("%s: the new domain exceeds the 2^22-leaf (2^31-voxel) limit of 32-bit voxel indices", who);
			return HNS_ERR_TOPOLOGY;
		}
		n_new = counts[2];
		if (n_new == 0) {  // SOP_HNanoSolver.cpp: "No active voxels"
			set_error("%s: No active voxels in the new domain", who);
			return HNS_ERR_RUNTIME;
		}
		return HNS_OK;
	}

	// ---- 2. order + grid: the origins to the host, OpenVDB leaf order, the new grid; the source values go up meanwhile ----
	int order() {
		std::vector<int32_t> xyz;
		HNS_TRY(download_origins(compact, (size_t)n_new, st, &xyz));
		for (Source& q : srcs)  // issued before the sort, so that they can overlap it
			if (q.l.n_leaves && q.kind != Source::kPoints) HNS_HIP(hipMemcpyAsync(q.values, q.l.values, 2048 * (size_t)q.l.ncomp * q.l.n_leaves, hipMemcpyHostToDevice, st));
		sort_leaf_origins(xyz.data(), (size_t)n_new);
		ng.reset(new hns_grid);
		ng->voxel_size = s->grid->voxel_size;
		HNS_TRY(ng->topo.prepare(xyz.data(), (int64_t)n_new));
		ng->n_active = n_new;
		HNS_TRY(hns_grid_upload(ng.get()));
		HNS_HIP(hipEventRecord(s->rev[2], st));
		return HNS_OK;
	}

	// ---- 3. masks: one wave per new leaf; every source but the velocity's and the points' (whose leaves the waves find) indexed into the new grid ----
	int masks() {
		HNS_TRY(scratch.carve([&](auto&& slice) {
			slice(map, 4 * n_new);
			if (points) slice(unseeded, 4 * n_new);
		}));
		HNS_TRY(scratch.get(64 * n_new, &new_masks));
		i_masks = scratch.held.size() - 1;
		if (!srcs.empty())
			HNS_TRY(scratch.carve([&](auto&& slice) {
				for (Source& q : srcs)
					if (q.kind != Source::kPoints) slice(q.idx, 4 * n_new);
			}));
		for (size_t i = 0; i < srcs.size(); ++i) {
			Source& q = srcs[i];
			if (q.kind == Source::kVelocity || q.kind == Source::kPoints) continue;
			HNS_HIP(hipMemsetAsync(q.idx, 0xFF, 4 * n_new, st));  // (a source without leaves: every leaf is fill)
			if (!q.l.n_leaves) continue;
			k_regrid_src_index<<<(unsigned)((q.l.n_leaves + 255) / 256), 256, 0, st>>>(ng->dev(), q.origins, (int)q.l.n_leaves, q.idx, dup + i);
			HNS_HIP(hipGetLastError());
		}
		SeedHashes sh{};
		if (vsrc) sh.h[kVsrcSeeds] = OriginIndex{vsrc->origins, vsrc->table, vsrc->mask}, sh.masks[kVsrcSeeds] = vsrc->masks;
		if (points) sh.h[kPointSeeds] = OriginIndex{points->origins, points->table, points->mask}, sh.masks[kPointSeeds] = points->masks;
		k_regrid_masks<<<(unsigned)((n_new + 3) / 4), 256, 0, st>>>(s->grid->dev(), s->d_masks.as<unsigned char>(), (const int4*)ng->d_origins, (int)n_new, p, R, sdf ? sdf->idx : nullptr,
		                                                           sdf ? sdf->masks : nullptr, sh, (uint64_t*)new_masks, map, vsrc ? vsrc->idx : nullptr, unseeded);
		HNS_HIP(hipGetLastError());
		for (Source& q : srcs) {
			if (!points || q.kind != Source::kFloat) continue;
			k_regrid_src_unseeded<<<(unsigned)((n_new + 255) / 256), 256, 0, st>>>(q.idx, unseeded, (int)n_new);
			HNS_HIP(hipGetLastError());
		}
		HNS_HIP(hipEventRecord(s->rev[3], st));
		return HNS_OK;
	}

	// entry j of a field launch: dst from `old` through map, or (q the SDF) from the SDF's leaves; with a velocity or float source q added
	void field(FieldSet& fs, int j, const float* old, float* dst, const Source* q, uint32_t fill) const {
		const bool from_sdf = q && q->kind == Source::kSdf, add = q && !from_sdf;
		fs.a[j] = (const float4*)(from_sdf ? q->values : old), fs.map_a[j] = from_sdf ? q->idx : map;
		fs.b[j] = add ? (const float4*)q->values : nullptr, fs.map_b[j] = add ? q->idx : nullptr;
		fs.dst[j] = (float4*)dst, fs.fill[j] = fill;
	}

	// ---- 4. fields: into a fresh arena, the velocity, then the float fields copied and those with a source added, kCopyFields per launch ----
	int fields() {
		hns_sim shell;  // the new layout, built over the new arena (the sim itself keeps the old one until the end)
		shell.names = s->names;
		HNS_TRY(scratch.get(hns_sim_arena_need(s, n_new * 512u), &new_fields));
		i_fields = scratch.held.size() - 1;
		hns_sim_layout(&shell, new_fields, n_new * 512u);
		std::vector<const Source*> src_of(s->names.size(), nullptr);
		for (const Source& q : srcs)
			if (q.field >= 0) src_of[(size_t)q.field] = &q;
		const int i_sdf = s->find("collision_sdf");
		FieldSet fs{};
		field(fs, 0, s->vel, shell.vel, vsrc, 0u);
		HNS_TRY(launch_fields(fs, 1, 3, vsrc != nullptr, n_new, st));
		for (const bool add : {false, true}) {
			int nf = 0;
			for (size_t f = 0; f < s->names.size(); ++f) {
				const Source* q = src_of[f];
				if ((q && q->kind == Source::kFloat) != add) continue;
				field(fs, nf++, s->cur[f], shell.cur[f], q, (int)f == i_sdf ? kSdfFill : 0u);
				if (nf == kCopyFields) {
					HNS_TRY(launch_fields(fs, nf, 1, add, n_new, st));
					nf = 0;
				}
			}
			HNS_TRY(launch_fields(fs, nf, 1, add, n_new, st));
		}
		HNS_HIP(hipEventRecord(s->rev[4], st));
		return HNS_OK;
	}

	// ---- 5. commit: the duplicate origins the device found refuse the regrid; else the sim moves onto the new grid ----
	int commit(hns_grid** out) {
		std::vector<int> dups(srcs.size(), 0);
		if (!srcs.empty()) HNS_HIP(hipMemcpyAsync(dups.data(), dup, 4 * srcs.size(), hipMemcpyDeviceToHost, st));
		HNS_HIP(hipStreamSynchronize(st));
		for (size_t i = 0; i < srcs.size(); ++i) {
			if (!dups[i]) continue;
			if (srcs[i].kind == Source::kSdf)
				set_error("%s: duplicate SDF leaf origin", who);
			else
				set_error("%s: source %d ('%s'): duplicate leaf origin", who, srcs[i].index, srcs[i].name());
			return HNS_ERR_TOPOLOGY;
		}
		std::swap(s->arena, scratch.held[i_fields]);  // the old state goes back to the pool with the scratch
		std::swap(s->d_masks, scratch.held[i_masks]);
		hns_sim_layout(s, new_fields, n_new * 512u);
		s->grid = ng.release();
		s->forget();
		hns_sim_drop_hierarchy(s);  // (hns_sim_set_solve_method: the next solve builds the new grid's)
		s->solved = false;  // (the divergence / pressure scratch holds no defined values: hns_sim_residual refuses until the next solve)
		s->regrid_timed = true;
		*out = s->grid;
		return HNS_OK;
	}
};

// The regrid proper (include/hns.h); `who` names the entry point in messages.
// The point set whose seeds join the velocity's topology (n == 0: none); *skipped (or null): the points that do not seed
struct SeedPoints {
	const float* d_xyz;
	uint64_t n;
	uint64_t* skipped;
};

int regrid(hns_sim* s, int p, const hns_leaf_source* src, int n_src, const hns_leaf_source& sdf, const SeedPoints& pts, hipStream_t st, hns_grid** out, const char* who) {
	const hns_grid* og = s->grid;
	if (og->first_active != 0 || og->n_active != (uint64_t)og->topo.n_leaves) {
		set_error("%s: the grid's launch range is not the whole grid (a multi-GPU rank's grid cannot be regridded)", who);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	DeviceScope on(s->device);
	Regrid r(s, p, st, who);
	HNS_TRY(r.sources(sdf, src, n_src, pts.n > 0));
	if (!s->rev[0])
		for (hipEvent_t& e : s->rev) HNS_HIP(hipEventCreate(&e));
	s->regrid_timed = false;
	HNS_TRY(r.seeds(pts.d_xyz, pts.n, pts.skipped));
	HNS_TRY(r.candidates());
	HNS_TRY(r.order());
	HNS_TRY(r.masks());
	HNS_TRY(r.fields());
	return r.commit(out);
}

// ---- hns_sim_deactivate: the end of a frame, one wave per leaf ----
// Mask byte x*8+y, bit z is voxel x*64+y*8+z, so little-endian word k of a leaf's mask holds voxels 64k .. 64k+63: in round k lane L tests voxel
// 64k+L and the wave's ballot is the new word. `pend[k]` (wave-uniform) holds the voxels of word k that are active and within every tolerance so
// far; a round whose pend is 0 loads nothing. Per round a float field is 256 contiguous bytes, the velocity 768 (Vec3f AoS).

struct ActField {  // one row of the device table
	const float* p;
	float tol;
	int ncomp;
};
constexpr int kActRows = 16;  // rows per table-writing launch (their kernel argument)
struct ActRows {
	ActField f[kActRows];
};

// Writes rows of the table from the kernel argument (no host staging, so the call stays asynchronous); zeroes the packed count when asked.
__global__ __launch_bounds__(64) void k_deactivate_table(ActRows rows, int n, ActField* dst, unsigned long long* count) {
	if ((int)threadIdx.x < n) dst[threadIdx.x] = rows.f[threadIdx.x];
	if (count && threadIdx.x == 0) *count = 0;
}

// Raw buffer loads over one leaf of a field, a round to skip at kActSkip, and the mask words through readlane64: hns_device.hpp ("one wave over one leaf").

// masks_in null: every voxel active (it may equal masks_out). count: += active voxels | (leaves holding one) << 40, one atomic per such wave.
__global__ __launch_bounds__(256) void k_deactivate(const ActField* __restrict__ tab, int n_tab, const uint64_t* masks_in, uint64_t* masks_out, uint64_t n_leaves,
                                                    unsigned long long* count) {
	const uint64_t leaf = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (leaf >= n_leaves) return;  // (whole waves)
	const int lane = (int)(threadIdx.x & 63);
	const uint64_t word = masks_in && lane < 8 ? masks_in[8 * leaf + (uint64_t)lane] : ~0ull;
	uint64_t old[8], pend[8];
#pragma unroll
	for (int k = 0; k < 8; ++k) pend[k] = old[k] = readlane64(word, k);
	for (int f = 0; f < n_tab; ++f) {
		const ActField e = tab[f];
		if (e.ncomp == 1) {
			const v4i r = field_rsrc(e.p + 512 * leaf, 2048u);
			float x[8];
#pragma unroll
			for (int k = 0; k < 8; ++k) x[k] = hns_buffer_load_f32(r, pend[k] ? 4 * (64 * k + lane) : kActSkip, 0, 0);
#pragma unroll
			for (int k = 0; k < 8; ++k) pend[k] &= __ballot(fabsf(x[k]) <= e.tol);
		} else {
			const v4i r = field_rsrc(e.p + 1536 * leaf, 6144u);
			v3f x[8];
#pragma unroll
			for (int k = 0; k < 8; ++k) x[k] = hns_buffer_load_v3f32(r, pend[k] ? 12 * (64 * k + lane) : kActSkip, 0, 0);
#pragma unroll
			for (int k = 0; k < 8; ++k) pend[k] &= __ballot(fabsf(x[k].x) <= e.tol && fabsf(x[k].y) <= e.tol && fabsf(x[k].z) <= e.tol);
		}
		if (!(pend[0] | pend[1] | pend[2] | pend[3] | pend[4] | pend[5] | pend[6] | pend[7])) break;  // every active voxel is kept already
	}
	uint64_t mine = 0;
	unsigned pop = 0;
#pragma unroll
	for (int k = 0; k < 8; ++k) {
		const uint64_t w = old[k] & ~pend[k];
		pop += (unsigned)__popcll(w);
		if (lane == k) mine = w;
	}
	if (lane < 8) masks_out[8 * leaf + (uint64_t)lane] = mine;
	if (count && lane == 0 && pop) atomicAdd(count, (unsigned long long)pop | 1ull << 40);
}

}  // namespace
}  // namespace hns

using namespace hns;

extern "C" int hns_sim_set_active_masks(hns_sim* s, const unsigned char* masks, void* stream) {
	if (!s) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_active_masks: null sim");
	const uint64_t n_leaves = s->n / 512u;
	if (!masks) {  // every voxel active: the state a sim starts in
		s->d_masks.release();
		return HNS_OK;
	}
	if (!n_leaves) return HNS_OK;
	HNS_TRY(s->d_masks.reserve(64 * n_leaves, s->device));
	HNS_HIP(hipMemcpyAsync(s->d_masks.p, masks, 64 * n_leaves, hipMemcpyHostToDevice, (hipStream_t)stream));
	return HNS_OK;
}

extern "C" int hns_sim_active_masks(hns_sim* s, unsigned char* out, void* stream) {
	if (!s || !out) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_active_masks: null argument");
	const uint64_t n_leaves = s->n / 512u;
	if (!s->d_masks) {
		memset(out, 0xFF, 64 * n_leaves);
		return HNS_OK;
	}
	HNS_HIP(hipMemcpyAsync(out, s->d_masks.p, 64 * n_leaves, hipMemcpyDeviceToHost, (hipStream_t)stream));
	HNS_HIP(hipStreamSynchronize((hipStream_t)stream));
	return HNS_OK;
}

namespace {
hns_grid* regrid_entry(hns_sim* s, int padding_voxels, const hns_leaf_source* sources, int n_sources, const SeedPoints& pts, const int32_t* sdf_origins, uint64_t n_sdf,
                       const unsigned char* sdf_masks, const float* sdf_values, void* stream, int* err, const char* who) {
	int rc = HNS_OK;
	hns_grid* g = nullptr;
	if (pts.skipped) *pts.skipped = 0;
	if (!s || !s->grid || padding_voxels < 0 || padding_voxels > 1024 || (n_sdf && (!sdf_origins || !sdf_values))) {
		set_error("%s: bad arguments", who);
		rc = HNS_ERR_INVALID_ARGUMENT;
	} else if (pts.n && !pts.d_xyz) {
		set_error("%s: d_seed_xyz is null with %llu seeds", who, (unsigned long long)pts.n);
		rc = HNS_ERR_INVALID_ARGUMENT;
	} else if (pts.n > kMaxSeedPoints) {
		set_error("%s: n_seeds is above 2^31 - 1", who);
		rc = HNS_ERR_INVALID_ARGUMENT;
	} else if (s->cached) {
		set_error("%s: the sim belongs to a grid's cook cache", who);
		rc = HNS_ERR_INVALID_ARGUMENT;
	} else {
		const hns_leaf_source sdf{"collision_sdf", 1, sdf_origins, n_sdf, sdf_masks, sdf_values};
		rc = regrid(s, padding_voxels, sources, n_sources, sdf, pts, (hipStream_t)stream, &g, who);
	}
	if (err) *err = rc;
	return rc == HNS_OK ? g : nullptr;
}
}  // namespace

extern "C" hns_grid* hns_sim_regrid(hns_sim* s, int padding_voxels, const int32_t* sdf_origins, uint64_t n_sdf, const unsigned char* sdf_masks, const float* sdf_values,
                                    void* stream, int* err) {
	return regrid_entry(s, padding_voxels, nullptr, 0, SeedPoints{nullptr, 0, nullptr}, sdf_origins, n_sdf, sdf_masks, sdf_values, stream, err, "hns_sim_regrid");
}

// hns_sim_regrid after adding a frame's sources into the fields (include/hns.h): the same four phases, the sources folded into them.
extern "C" hns_grid* hns_sim_regrid_sourced(hns_sim* s, int padding_voxels, const hns_leaf_source* sources, int n_sources, const int32_t* sdf_origins, uint64_t n_sdf,
                                            const unsigned char* sdf_masks, const float* sdf_values, void* stream, int* err) {
	return regrid_entry(s, padding_voxels, sources, n_sources, SeedPoints{nullptr, 0, nullptr}, sdf_origins, n_sdf, sdf_masks, sdf_values, stream, err,
	                    "hns_sim_regrid_sourced");
}

// hns_sim_regrid_sourced with the seeds of a device-resident point set united into the velocity's topology before the dilation (include/hns.h)
extern "C" hns_grid* hns_sim_regrid_seeded(hns_sim* s, int padding_voxels, const hns_leaf_source* sources, int n_sources, const float* d_seed_xyz, uint64_t n_seeds,
                                           uint64_t* seeds_skipped, const int32_t* sdf_origins, uint64_t n_sdf, const unsigned char* sdf_masks, const float* sdf_values,
                                           void* stream, int* err) {
	return regrid_entry(s, padding_voxels, sources, n_sources, SeedPoints{d_seed_xyz, n_seeds, seeds_skipped}, sdf_origins, n_sdf, sdf_masks, sdf_values, stream, err,
	                    "hns_sim_regrid_seeded");
}

// hipEvent split of the last hns_sim_regrid: {candidates (with the seeds of a point set, where given), origins to the host + sort + grid tables, masks, field copy} in milliseconds
extern "C" int hns_sim_regrid_times(hns_sim* s, float* ms4) {
	if (!s || !ms4) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_regrid_times: null argument");
	if (!s->regrid_timed) return fail(HNS_ERR_RUNTIME, "hns_sim_regrid_times: no regrid has completed on this sim");
	for (int i = 0; i < 4; ++i) HNS_HIP(hipEventElapsedTime(&ms4[i], s->rev[i], s->rev[i + 1]));
	return HNS_OK;
}

// The end of a frame (include/hns.h): clears the active bits of voxels whose listed fields are all within tolerance. Fields are never touched.
extern "C" int hns_sim_deactivate(hns_sim* s, const hns_activity_field* fields, int n_fields, uint64_t* counts, void* stream) {
	const char* who = "hns_sim_deactivate";
	if (!s || !s->grid) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_deactivate: null sim");
	if (s->cached) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_deactivate: the sim belongs to a grid's cook cache");
	std::vector<int> field_of;
	HNS_TRY(check_activity_fields(s, fields, n_fields, who, &field_of));
	const uint64_t n_leaves = s->n / 512u;
	if (!n_leaves) {
		if (counts) counts[0] = counts[1] = 0;
		return HNS_OK;
	}
	DeviceScope on(s->device);
	const hipStream_t st = (hipStream_t)stream;
	HNS_TRY(s->d_act.reserve(16 + sizeof(ActField) * (s->names.size() + 1), s->device));  // the packed count, then a row per field the sim could list (its float fields and the velocity)
	unsigned long long* d_count = s->d_act.as<unsigned long long>();
	ActField* d_tab = (ActField*)(s->d_act.as<char>() + 16);
	Pooled first_masks;  // all active until now: the kernel reads no masks and writes the first ones, which the sim takes once the launches went out
	if (!s->d_masks) HNS_TRY(first_masks.get(64 * n_leaves, s->device));
	unsigned char* masks = s->d_masks ? s->d_masks.as<unsigned char>() : first_masks.as<unsigned char>();
	int rc = HNS_OK;
	for (int i0 = 0; i0 < n_fields && rc == HNS_OK; i0 += kActRows) {
		ActRows rows{};
		const int n = std::min(kActRows, n_fields - i0);
		for (int j = 0; j < n; ++j) {
			const int f = field_of[(size_t)(i0 + j)];
			rows.f[j] = ActField{f < 0 ? s->vel : s->cur[(size_t)f], fields[i0 + j].tolerance, fields[i0 + j].ncomp};
		}
		k_deactivate_table<<<1, 64, 0, st>>>(rows, n, d_tab + i0, counts && i0 == 0 ? d_count : nullptr);
		if (hipGetLastError() != hipSuccess) rc = fail(HNS_ERR_HIP, "hns_sim_deactivate: table launch failed");
	}
	if (rc == HNS_OK) {
		k_deactivate<<<(unsigned)((n_leaves + 3) / 4), 256, 0, st>>>(d_tab, n_fields, s->d_masks.as<const uint64_t>(), (uint64_t*)masks, n_leaves,
		                                                            counts ? d_count : nullptr);
		if (hipGetLastError() != hipSuccess) rc = fail(HNS_ERR_HIP, "hns_sim_deactivate: kernel launch failed");
	}
	if (rc != HNS_OK) return rc;  // nothing ran: the masks are as they were
	if (first_masks) s->d_masks = std::move(first_masks);
	s->drop_ahead();  // (the end of a frame: the next substep belongs to another one)
	if (counts) {
		unsigned long long packed = 0;
		HNS_HIP(hipMemcpyAsync(&packed, d_count, sizeof(packed), hipMemcpyDeviceToHost, st));
		HNS_HIP(hipStreamSynchronize(st));
		counts[0] = packed & ((1ull << 40) - 1), counts[1] = packed >> 40;
	}
	return HNS_OK;
}
