// hns_regrid.hip -- what the HNanoSolver SOP does to the domain between two cooks, on the device: dilate the velocity's active topology by `padding`
// voxels, unite it with the collision SDF's leaves (reference src/SOP/HNanoSolver/SOP_HNanoSolver.cpp:186-199) and carry every field into the new leaf
// set, filled the way HNS::IndexGridBuilder fills leaves a source lacks (src/Utils/GridBuilder.hpp:99-154). The host chain that does the same
// (hns_sim_download -> hns_dilate_leaf_masks -> hns_union_leaves -> hns_gather_leaves -> new grid -> hns_sim_upload) moves every field over PCIe
// twice; here only leaf origins cross (12 bytes per leaf each way) plus, when a collision SDF source is given, that source.
//
//   1. candidates  one thread per (old leaf, offset in the (2R+1)^3 leaf neighbourhood), R = ceil(p / 8), and one per SDF leaf: a hit (the old leaf's
//                  active voxels reach the candidate's box, hns_dilate.hpp) goes into a fresh origin hash with compare-and-swap, then the hash is compacted
//   2. order       the origins come to the host, are sorted into OpenVDB leaf order and become a new hns_grid through the usual path (Topology::prepare,
//                  hns_grid_upload: hash, nbr27, launch order)
//   3. masks       one wave per new leaf gathers the masks of the old leaves within reach (old grid's origin hash), dilates each separably into its own
//                  box, ORs them across the wave and ORs in the SDF leaf's mask; the same wave records which old leaf (if any) has this origin
//   4. fields      velocity and every float field, 16 bytes per load and store, from the old leaf or the fill (zeros; bytes 0x01 for collision_sdf),
//                  into a fresh arena from the pool; the old arena goes back to the pool
//
// Everything that decides a result is order-free: hash slots hold the smallest thing that identifies a candidate (its thread id), the compacted
// order is discarded by the sort, and the mask OR is commutative. Two runs give the same bytes.
#include <algorithm>
#include <cstring>
#include <vector>

#include "hns_device.hpp"
#include "hns_dilate.hpp"

#define HNS_TRY_RC(call)           \
	do {                            \
		int rc__ = (call);          \
		if (rc__ != HNS_OK) return rc__; \
	} while (0)

namespace hns {
namespace {

constexpr unsigned long long kEmptySlot = ~0ull;
constexpr uint64_t kMaxCandidates = uint64_t(1) << 23;  // distinct leaves the candidate hash may hold (the grid limit is 2^22: Topology::prepare)
constexpr int kCopyFields = 16;                          // float fields per copy launch

__device__ __forceinline__ void load_mask(const unsigned char* masks, int l, uint64_t (&m)[8]) {
	const uint64_t* w = masks ? (const uint64_t*)(masks + 64 * (size_t)l) : nullptr;
#pragma unroll
	for (int x = 0; x < 8; ++x) m[x] = w ? w[x] : ~0ull;
}

// The candidate a thread id stands for: ids [0, n_dil) are (old leaf, offset) pairs, ids [n_dil, n_dil + n_sdf) the SDF leaves.
struct Candidates {
	const int4* old_origins;
	const unsigned char* old_masks;  // null: every voxel active
	const int4* sdf;
	uint64_t n_dil, n_sdf;
	int side, R, p;
	unsigned long long* table;
	uint32_t mask;
	unsigned long long cap;
	unsigned long long* count;  // [0] slots reserved, [1] overflow, [2] compacted leaves
};

__device__ __forceinline__ bool cand_origin(const Candidates& c, uint64_t t, int& x, int& y, int& z, int& l, int (&d)[3]) {
	if (t >= c.n_dil) {
		const int4 o = c.sdf[t - c.n_dil];
		x = o.x, y = o.y, z = o.z, l = -1;
		return true;
	}
	const uint64_t K = (uint64_t)c.side * c.side * c.side;
	l = (int)(t / K);
	const int k = (int)(t - (uint64_t)l * K);
	d[0] = k / (c.side * c.side) - c.R, d[1] = (k / c.side) % c.side - c.R, d[2] = k % c.side - c.R;
	const int4 o = c.old_origins[l];
	const int64_t nx = (int64_t)o.x + 8 * d[0], ny = (int64_t)o.y + 8 * d[1], nz = (int64_t)o.z + 8 * d[2];
	if (nx < INT32_MIN || nx > INT32_MAX - 7 || ny < INT32_MIN || ny > INT32_MAX - 7 || nz < INT32_MIN || nz > INT32_MAX - 7) return false;
	x = (int)nx, y = (int)ny, z = (int)nz;
	return true;
}

__global__ __launch_bounds__(256) void k_regrid_candidates(Candidates c) {
	const uint64_t total = c.n_dil + c.n_sdf;
	for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
		int x, y, z, l, d[3] = {0, 0, 0};
		if (!cand_origin(c, t, x, y, z, l, d)) continue;
		if (l >= 0) {  // a hit iff the old leaf's active voxels, dilated by p, reach the candidate's box (hns_dilate_leaves' slab test)
			uint64_t m[8], out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
			load_mask(c.old_masks, l, m);
			if (!dilate_into(m, -8 * d[0], -8 * d[1], -8 * d[2], c.p, out)) continue;
		}
		uint32_t s = d_hash_origin(x, y, z) & c.mask;
		bool reserved = false;
		for (;;) {
			unsigned long long cur = c.table[s];
			if (cur == kEmptySlot) {
				if (!reserved) {  // at most `cap` slots are ever taken: the table (>= 2 cap) always has an empty slot ahead
					if (atomicAdd(&c.count[0], 1ull) >= c.cap) {
						c.count[1] = 1;
						break;
					}
					reserved = true;
				}
				cur = atomicCAS(&c.table[s], kEmptySlot, (unsigned long long)t);
				if (cur == kEmptySlot) break;
			}
			int qx, qy, qz, ql, qd[3];
			cand_origin(c, cur, qx, qy, qz, ql, qd);  // (an id in the table always stands for a valid origin)
			if (qx == x && qy == y && qz == z) break;
			s = (s + 1) & c.mask;
		}
	}
}

__global__ __launch_bounds__(256) void k_regrid_compact(Candidates c, int4* __restrict__ out) {
	const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (s > c.mask) return;
	const unsigned long long t = c.table[s];
	if (t == kEmptySlot) return;
	int x, y, z, l, d[3];
	cand_origin(c, t, x, y, z, l, d);
	out[atomicAdd(&c.count[2], 1ull)] = make_int4(x, y, z, 0);
}

// sdf_idx[new leaf] = the SDF leaf with its origin; two SDF leaves on one origin raise *dup
__global__ __launch_bounds__(256) void k_regrid_sdf_index(GridDev ng, const int4* __restrict__ sdf, int n_sdf, int* __restrict__ sdf_idx, int* __restrict__ dup) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n_sdf) return;
	const int4 o = sdf[i];
	const int b = d_find_leaf(ng, o.x, o.y, o.z);  // (present: every SDF leaf is a leaf of the new grid)
	if (b >= 0 && atomicCAS(&sdf_idx[b], -1, i) != -1) *dup = 1;
}

// One wave per new leaf: its dilated mask (OR over the old leaves within reach, then the SDF leaf's mask) and the old leaf with its origin (map, -1 = new).
__global__ __launch_bounds__(256) void k_regrid_masks(GridDev og, const unsigned char* __restrict__ old_masks, const int4* __restrict__ new_origins, int n_new, int p, int R,
                                                      const int* __restrict__ sdf_idx, const unsigned char* __restrict__ sdf_masks, uint64_t* __restrict__ new_masks,
                                                      int* __restrict__ map) {
	const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (b >= n_new) return;
	const int4 o = new_origins[b];
	const int side = 2 * R + 1, K = side * side * side, centre = (K - 1) / 2;
	uint64_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	for (int k = lane; k < K; k += 64) {
		const int d[3] = {k / (side * side) - R, (k / side) % side - R, k % side - R};
		const int64_t nx = (int64_t)o.x + 8 * d[0], ny = (int64_t)o.y + 8 * d[1], nz = (int64_t)o.z + 8 * d[2];
		int l = -1;
		if (og.n_leaves > 0 && nx >= INT32_MIN && nx <= INT32_MAX && ny >= INT32_MIN && ny <= INT32_MAX && nz >= INT32_MIN && nz <= INT32_MAX)
			l = d_find_leaf(og, (int)nx, (int)ny, (int)nz);
		if (k == centre) map[b] = l;
		if (l < 0) continue;
		uint64_t m[8];
		load_mask(old_masks, l, m);
		dilate_into(m, 8 * d[0], 8 * d[1], 8 * d[2], p, acc);
	}
#pragma unroll
	for (int x = 0; x < 8; ++x) {
		uint32_t lo = (uint32_t)acc[x], hi = (uint32_t)(acc[x] >> 32);
#pragma unroll
		for (int w = 32; w >= 1; w >>= 1) {
			lo |= __shfl_xor(lo, w);
			hi |= __shfl_xor(hi, w);
		}
		acc[x] = (uint64_t)hi << 32 | lo;
	}
	if (lane < 8) {
		uint64_t w = 0;
#pragma unroll
		for (int x = 0; x < 8; ++x) w = lane == x ? acc[x] : w;
		const int si = sdf_idx ? sdf_idx[b] : -1;
		if (si >= 0) w |= sdf_masks ? ((const uint64_t*)(sdf_masks + 64 * (size_t)si))[lane] : ~0ull;
		new_masks[(size_t)b * 8 + lane] = w;
	}
}

struct CopySet {
	const float4* src[kCopyFields];
	float4* dst[kCopyFields];
	const int* map[kCopyFields];  // new leaf -> source leaf, -1 = fill
	uint32_t fill[kCopyFields];
};

// blockIdx.y = field; NC = floats per voxel (3: the velocity, AoS). Each thread moves four 16-byte pieces, all four loads in flight before the stores.
template <int NC>
__global__ __launch_bounds__(256) void k_regrid_copy(CopySet cs, uint32_t n_f4) {
	constexpr uint32_t per_leaf = 128u * NC;
	const int f = blockIdx.y;
	const float4* __restrict__ src = cs.src[f];
	float4* __restrict__ dst = cs.dst[f];
	const int* __restrict__ map = cs.map[f];
	const float fv = __uint_as_float(cs.fill[f]);
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

// device allocations of one regrid, returned to the pool however it ends (hns_arena_put waits for the device first)
struct Scratch {
	std::vector<std::pair<void*, size_t>> held;
	int device;
	explicit Scratch(int dev) : device(dev) {}
	int get(size_t bytes, void** p) {
		size_t got = 0;
		const int rc = hns_arena_get(bytes, device, p, &got);
		if (rc == HNS_OK) held.emplace_back(*p, got);
		return rc;
	}
	void keep(void* p) {  // ownership passes to the sim
		for (size_t i = 0; i < held.size(); ++i)
			if (held[i].first == p) held.erase(held.begin() + (long)i);
	}
	~Scratch() {
		for (auto& h : held) hns_arena_put(h.first, h.second, device);
	}
};

struct CurrentDevice {
	int prev = -1;
	explicit CurrentDevice(int device) {
		if (hipGetDevice(&prev) != hipSuccess || prev == device || hipSetDevice(device) != hipSuccess) prev = -1;
	}
	~CurrentDevice() {
		if (prev >= 0) (void)hipSetDevice(prev);
	}
};

size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

int copy_fields(const CopySet& cs, int nf, int nc, uint64_t n_new, hipStream_t st) {
	if (!nf || !n_new) return HNS_OK;
	const uint32_t n_f4 = (uint32_t)(n_new * 128u * (uint64_t)nc);
	const dim3 grid((n_f4 + 1023u) / 1024u, (unsigned)nf);
	if (nc == 3)
		k_regrid_copy<3><<<grid, 256, 0, st>>>(cs, n_f4);
	else
		k_regrid_copy<1><<<grid, 256, 0, st>>>(cs, n_f4);
	HNS_HIP(hipGetLastError());
	return HNS_OK;
}

// The regrid proper; the sim is only touched at the very end, when everything has succeeded.
int regrid(hns_sim* s, int p, const int32_t* sdf_origins, uint64_t n_sdf, const unsigned char* sdf_masks, const float* sdf_values, hipStream_t st, hns_grid** out) {
	hns_grid* og = s->grid;
	const bool have_src = sdf_values != nullptr;
	const int i_sdf = s->find("collision_sdf");
	if (og->first_active != 0 || og->n_active != (uint64_t)og->topo.n_leaves)
		return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_regrid: the grid's launch range is not the whole grid (a multi-GPU rank's grid cannot be regridded)");
	if (have_src && i_sdf < 0) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_regrid: a collision SDF source was given but the sim has no field 'collision_sdf'");
	for (uint64_t i = 0; i < 3 * n_sdf; ++i)
		if (sdf_origins[i] & 7) {
			set_error("hns_sim_regrid: SDF leaf origin %llu is not 8-aligned", (unsigned long long)(i / 3));
			return HNS_ERR_TOPOLOGY;
		}
	CurrentDevice on(s->device);
	if (!s->rev[0])
		for (hipEvent_t& e : s->rev) HNS_HIP(hipEventCreate(&e));
	s->regrid_timed = false;
	Scratch scratch(s->device);

	// ---- 1. candidates ----
	const uint64_t n_old = (uint64_t)og->topo.n_leaves;
	const int R = (p + 7) / 8, side = 2 * R + 1;
	const uint64_t n_dil = n_old * (uint64_t)side * side * side;
	const uint64_t cap = std::min<uint64_t>(n_dil + n_sdf, kMaxCandidates);
	uint64_t T = 16;
	while (T < 2 * cap) T <<= 1;
	std::vector<int32_t> sdf4((size_t)n_sdf * 4, 0);
	for (uint64_t i = 0; i < n_sdf; ++i)
		for (int a = 0; a < 3; ++a) sdf4[4 * i + a] = sdf_origins[3 * i + a];
	const size_t sz1[4] = {pad256(8 * T), pad256(16 * (cap ? cap : 1)), pad256(16 * (n_sdf ? n_sdf : 1)), 256};
	void* p1 = nullptr;
	HNS_TRY_RC(scratch.get(sz1[0] + sz1[1] + sz1[2] + sz1[3], &p1));
	char* q = (char*)p1;
	Candidates c;
	c.table = (unsigned long long*)q, q += sz1[0];
	int4* compact = (int4*)q;
	q += sz1[1];
	int4* d_sdf = (int4*)q;
	q += sz1[2];
	c.count = (unsigned long long*)q;
	c.old_origins = (const int4*)og->d_origins, c.old_masks = s->d_masks, c.sdf = d_sdf;
	c.n_dil = n_dil, c.n_sdf = n_sdf, c.side = side, c.R = R, c.p = p;
	c.mask = (uint32_t)(T - 1), c.cap = cap;
	HNS_HIP(hipEventRecord(s->rev[0], st));
	HNS_HIP(hipMemsetAsync(c.table, 0xFF, 8 * T, st));
	HNS_HIP(hipMemsetAsync(c.count, 0, 256, st));
	if (n_sdf) HNS_HIP(hipMemcpyAsync(d_sdf, sdf4.data(), 16 * n_sdf, hipMemcpyHostToDevice, st));
	if (n_dil + n_sdf) {
		const uint64_t blocks = std::min<uint64_t>((n_dil + n_sdf + 255) / 256, 1u << 20);
		k_regrid_candidates<<<(unsigned)blocks, 256, 0, st>>>(c);
		HNS_HIP(hipGetLastError());
		k_regrid_compact<<<(unsigned)(T / 256 ? T / 256 : 1), 256, 0, st>>>(c, compact);
		HNS_HIP(hipGetLastError());
	}
	HNS_HIP(hipEventRecord(s->rev[1], st));
	unsigned long long counts[3] = {0, 0, 0};
	HNS_HIP(hipMemcpyAsync(counts, c.count, sizeof(counts), hipMemcpyDeviceToHost, st));
	HNS_HIP(hipStreamSynchronize(st));
	if (counts[1] || counts[2] > (uint64_t(1) << 22)) return fail(HNS_ERR_TOPOLOGY, "hns_sim_regrid: the new domain exceeds the 2^22-leaf (2^31-voxel) limit of 32-bit voxel indices");
	const uint64_t n_new = counts[2];
	if (n_new == 0) return fail(HNS_ERR_RUNTIME, "hns_sim_regrid: No active voxels in the new domain");  // SOP_HNanoSolver.cpp: "No active voxels"

	// ---- 2. order + grid ----
	std::vector<int32_t> c4((size_t)n_new * 4);
	HNS_HIP(hipMemcpyAsync(c4.data(), compact, 16 * n_new, hipMemcpyDeviceToHost, st));
	HNS_HIP(hipStreamSynchronize(st));
	std::vector<int32_t> xyz((size_t)n_new * 3);
	for (uint64_t i = 0; i < n_new; ++i)
		for (int a = 0; a < 3; ++a) xyz[3 * i + a] = c4[4 * i + a];
	sort_leaf_origins(xyz.data(), (size_t)n_new);
	struct GridOwner {
		hns_grid* g = new hns_grid;
		~GridOwner() {
			if (g) hns_grid_destroy(g);
		}
	} ng;
	ng.g->voxel_size = og->voxel_size;
	HNS_TRY_RC(ng.g->topo.prepare(xyz.data(), (int64_t)n_new));
	ng.g->n_active = n_new;
	HNS_TRY_RC(hns_grid_upload(ng.g));
	HNS_HIP(hipEventRecord(s->rev[2], st));

	// ---- 3. masks ----
	const size_t sz2[5] = {pad256(4 * n_new), pad256(4 * n_new), pad256(64 * (n_sdf ? n_sdf : 1)), pad256(2048 * (have_src && n_sdf ? n_sdf : 1)), 256};
	void *p2 = nullptr, *p_masks = nullptr;
	HNS_TRY_RC(scratch.get(sz2[0] + sz2[1] + sz2[2] + sz2[3] + sz2[4], &p2));
	HNS_TRY_RC(scratch.get(64 * n_new, &p_masks));
	q = (char*)p2;
	int* map = (int*)q;
	q += sz2[0];
	int* sdf_idx = (int*)q;
	q += sz2[1];
	unsigned char* d_sdf_masks = (unsigned char*)q;
	q += sz2[2];
	float* d_sdf_values = (float*)q;
	q += sz2[3];
	int* dup = (int*)q;
	HNS_HIP(hipMemsetAsync(dup, 0, 4, st));
	if (n_sdf || have_src) HNS_HIP(hipMemsetAsync(sdf_idx, 0xFF, 4 * n_new, st));  // (a source without leaves: every leaf is fill)
	if (n_sdf) {
		if (sdf_masks) HNS_HIP(hipMemcpyAsync(d_sdf_masks, sdf_masks, 64 * n_sdf, hipMemcpyHostToDevice, st));
		if (have_src) HNS_HIP(hipMemcpyAsync(d_sdf_values, sdf_values, 2048 * n_sdf, hipMemcpyHostToDevice, st));
		k_regrid_sdf_index<<<(unsigned)((n_sdf + 255) / 256), 256, 0, st>>>(ng.g->dev(), d_sdf, (int)n_sdf, sdf_idx, dup);
		HNS_HIP(hipGetLastError());
	}
	k_regrid_masks<<<(unsigned)((n_new + 3) / 4), 256, 0, st>>>(og->dev(), s->d_masks, (const int4*)ng.g->d_origins, (int)n_new, p, R, n_sdf ? sdf_idx : nullptr,
	                                                           sdf_masks ? d_sdf_masks : nullptr, (uint64_t*)p_masks, map);
	HNS_HIP(hipGetLastError());
	HNS_HIP(hipEventRecord(s->rev[3], st));

	// ---- 4. fields ----
	hns_sim shell;  // the new layout, built over the new arena (the sim itself keeps the old one until the end)
	shell.names = s->names;
	void* p_fields = nullptr;
	HNS_TRY_RC(scratch.get(hns_sim_arena_need(s, n_new * 512u), &p_fields));
	hns_sim_layout(&shell, p_fields, n_new * 512u);
	const uint32_t sdf_fill = 0x01010101u;  // memset(..., 1, ...) (GridBuilder.hpp:108)
	CopySet vs{};
	vs.src[0] = (const float4*)s->vel, vs.dst[0] = (float4*)shell.vel, vs.map[0] = map, vs.fill[0] = 0;
	HNS_TRY_RC(copy_fields(vs, 1, 3, n_new, st));
	for (size_t f0 = 0; f0 < s->names.size(); f0 += kCopyFields) {
		CopySet cs{};
		int nf = 0;
		for (size_t f = f0; f < s->names.size() && nf < kCopyFields; ++f, ++nf) {
			const bool sdf = (int)f == i_sdf;
			const bool from_src = sdf && have_src;
			cs.src[nf] = from_src ? (const float4*)d_sdf_values : (const float4*)s->cur[f];
			cs.map[nf] = from_src ? sdf_idx : map;
			cs.dst[nf] = (float4*)shell.cur[f];
			cs.fill[nf] = sdf ? sdf_fill : 0u;
		}
		HNS_TRY_RC(copy_fields(cs, nf, 1, n_new, st));
	}
	HNS_HIP(hipEventRecord(s->rev[4], st));
	int dup_h = 0;
	HNS_HIP(hipMemcpyAsync(&dup_h, dup, 4, hipMemcpyDeviceToHost, st));
	HNS_HIP(hipStreamSynchronize(st));
	if (dup_h) return fail(HNS_ERR_TOPOLOGY, "hns_sim_regrid: duplicate SDF leaf origin");

	// ---- the sim moves onto the new grid ----
	size_t fields_bytes = 0, masks_bytes = 0;
	for (const auto& h : scratch.held) {
		if (h.first == p_fields) fields_bytes = h.second;
		if (h.first == p_masks) masks_bytes = h.second;
	}
	scratch.keep(p_fields);
	scratch.keep(p_masks);
	scratch.held.emplace_back(s->arena, s->arena_bytes);  // the old state goes back to the pool with the scratch
	if (s->d_masks) scratch.held.emplace_back(s->d_masks, s->masks_bytes);
	s->arena = p_fields, s->arena_bytes = fields_bytes;
	hns_sim_layout(s, p_fields, n_new * 512u);
	s->d_masks = (unsigned char*)p_masks, s->masks_bytes = masks_bytes;
	s->grid = ng.g;
	ng.g = nullptr;
	s->sig_vel = s->dig_vel = 0;
	std::fill(s->sig_cur.begin(), s->sig_cur.end(), 0);
	std::fill(s->dig_cur.begin(), s->dig_cur.end(), 0);
	s->regrid_timed = true;
	*out = s->grid;
	return HNS_OK;
}

}  // namespace
}  // namespace hns

using namespace hns;

extern "C" int hns_sim_set_active_masks(hns_sim* s, const unsigned char* masks, void* stream) {
	if (!s) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_active_masks: null sim");
	const uint64_t n_leaves = s->n / 512u;
	if (!masks) {  // every voxel active: the state a sim starts in
		if (s->d_masks) hns_arena_put(s->d_masks, s->masks_bytes, s->device);
		s->d_masks = nullptr, s->masks_bytes = 0;
		return HNS_OK;
	}
	if (!n_leaves) return HNS_OK;
	if (!s->d_masks) {
		void* p = nullptr;
		size_t got = 0;
		HNS_TRY_RC(hns_arena_get(64 * n_leaves, s->device, &p, &got));
		s->d_masks = (unsigned char*)p, s->masks_bytes = got;
	}
	HNS_HIP(hipMemcpyAsync(s->d_masks, masks, 64 * n_leaves, hipMemcpyHostToDevice, (hipStream_t)stream));
	return HNS_OK;
}

extern "C" int hns_sim_active_masks(hns_sim* s, unsigned char* out, void* stream) {
	if (!s || !out) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_active_masks: null argument");
	const uint64_t n_leaves = s->n / 512u;
	if (!s->d_masks) {
		memset(out, 0xFF, 64 * n_leaves);
		return HNS_OK;
	}
	HNS_HIP(hipMemcpyAsync(out, s->d_masks, 64 * n_leaves, hipMemcpyDeviceToHost, (hipStream_t)stream));
	HNS_HIP(hipStreamSynchronize((hipStream_t)stream));
	return HNS_OK;
}

extern "C" hns_grid* hns_sim_regrid(hns_sim* s, int padding_voxels, const int32_t* sdf_origins, uint64_t n_sdf, const unsigned char* sdf_masks, const float* sdf_values,
                                    void* stream, int* err) {
	int rc = HNS_OK;
	hns_grid* g = nullptr;
	if (!s || !s->grid || padding_voxels < 0 || padding_voxels > 1024 || (n_sdf && (!sdf_origins || !sdf_values)))
		rc = fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_regrid: bad arguments");
	else if (s->cached)
		rc = fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_regrid: the sim belongs to a grid's cook cache");
	else
		rc = regrid(s, padding_voxels, sdf_origins, n_sdf, sdf_masks, sdf_values, (hipStream_t)stream, &g);
	if (err) *err = rc;
	return rc == HNS_OK ? g : nullptr;
}

// hipEvent split of the last hns_sim_regrid: {candidates, origins to the host + sort + grid tables, masks, field copy} in milliseconds
extern "C" int hns_sim_regrid_times(hns_sim* s, float* ms4) {
	if (!s || !ms4) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_regrid_times: null argument");
	if (!s->regrid_timed) return fail(HNS_ERR_RUNTIME, "hns_sim_regrid_times: no regrid has completed on this sim");
	for (int i = 0; i < 4; ++i) HNS_HIP(hipEventElapsedTime(&ms4[i], s->rev[i], s->rev[i + 1]));
	return HNS_OK;
}
