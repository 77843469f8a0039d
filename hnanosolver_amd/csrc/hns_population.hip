// hns_population.hip -- birth and death of points on the device (include/hns.h: "BIRTH AND DEATH OF POINTS" states the rules): a stream of items, each with a small count,
// expanded into rows in item order with the counts kept on the device. Death: a flag byte per point, a slot per kept point, and the row move that compacts any attribute
// array through the slots. Birth: a count of 0 .. 16 per voxel of a field, and the positions of the newborn (hns_birth.hpp, shared with the host mirror).
//
// Count, scan, place over tiles of kPopTile consecutive items, every dependence a launch boundary:
//   k_pop_count_flags   one workgroup per tile. A wave takes 64 consecutive points per round: the kept ones are a ballot, their number a popcount
//   k_pop_count_births  one workgroup per tile of four leaves. A thread takes the eight voxels of one z-row (one mask byte, 32 contiguous bytes of the field); the tile's
//                       count is a workgroup sum
//   k_pop_scan          one workgroup: an exclusive scan along the tile table in place, kPopScanChunk tiles per round with a carry (k_order_scan's shape with a single row);
//                       it starts at `start` (live of an append, else 0) and writes the counters: wanted = start + the sum, live = min(wanted, cap)
//   k_pop_place_slots   recomputes the tile's ballots; rank = the tile's start + the waves before + the rounds before + the kept lanes below: index order
//   k_pop_place_births  recomputes the tile's counts (birth_count: the one function both kernels call); a thread's first row = the tile's start + the counts of the threads
//                       before it (block_scan), thread order being voxel order; then the rows. A tile's births are contiguous rows
//   k_pop_fill_births   rows live .. capacity_rows - 1 of xyz and voxel: NaN, 0xFFFFFFFF
//   k_pop_rows          k_order_rows' layout -- adjacent lanes take adjacent words of a row --: dst row slot[r] = src row r, and with FILL the rows live .. n - 1 of dst
//   k_pop_set_live      one thread: the counters of set_live
// Every thread that needs live reads it from the device word: the host never learns a count unless it asks. No atomics at all, no scratch. Rows are 64-bit where a sum of
// counts can pass 2^32 (16 births a voxel); the tile table saturates at 0xFFFFFFFF, which is beyond every capacity_rows (<= 2^31 - 1): such a tile writes nothing.
#include "hns_birth.hpp"
#include "hns_blockscan.hpp"
#include "hns_points.hpp"

namespace hns {
namespace {

constexpr int kPopBlock = 256;                          // threads of every kernel here: four waves
constexpr int kPopWaves = kPopBlock / 64;
constexpr int kPopItems = 8;                            // items per thread of a tile
constexpr int kPopTile = kPopBlock * kPopItems;         // 2048 items: what device.POINT_POPULATION_TILE states to the tests
constexpr int kPopScanItems = 4;                        // table entries per thread and round of k_pop_scan
constexpr int kPopScanChunk = kPopBlock * kPopScanItems;  // 1024 tiles per round: device.POINT_POPULATION_SCAN_TILES
constexpr int kPopTileLeaves = kPopTile / 512;          // a wave of a birth tile is one leaf
static_assert(kPopBlock == kBlockScanThreads && kPopWaves == kBlockScanWaves, "block_scan (hns_blockscan.hpp) scans a workgroup of this size");
static_assert(kPopTileLeaves == kPopWaves && kPopItems == 8, "k_pop_*_births: wave w of a tile is leaf 4 * tile + w, thread = mask byte, item = bit z");

constexpr unsigned kDropped = 0xFFFFFFFFu;
constexpr int kLdsPop = kPopWaves * 4;  // every kernel with LDS here: the waves' totals

// ---- death: flags -> slots -----------------------------------------------------------------------------------------------------------------------------------------------

// the kept lanes of round j of wave w of the tile: points tile0 + 512 w + 64 j .. + 63
__device__ __forceinline__ unsigned long long kept_ballot(const unsigned char* __restrict__ flags, unsigned n, unsigned at_least, unsigned p) {
	return __ballot(p < n && (unsigned)flags[p] >= at_least);
}

__global__ __launch_bounds__(kPopBlock) void k_pop_count_flags(const unsigned char* __restrict__ flags, const unsigned n, const unsigned at_least, unsigned* __restrict__ table) {
	__shared__ unsigned s_wave[kPopWaves];
	static_assert(sizeof(s_wave) == kLdsPop, "k_pop_count_flags: LDS");
	const unsigned t = threadIdx.x, lane = t & 63u, w = t >> 6;
	const unsigned first = blockIdx.x * (unsigned)kPopTile + w * (unsigned)(64 * kPopItems) + lane;
	unsigned count = 0;
#pragma unroll
	for (int j = 0; j < kPopItems; ++j) count += (unsigned)__popcll(kept_ballot(flags, n, at_least, first + (unsigned)(64 * j)));
	if (lane == 0) s_wave[w] = count;
	__syncthreads();
	if (t == 0) {
		unsigned sum = 0;
#pragma unroll
		for (int k = 0; k < kPopWaves; ++k) sum += s_wave[k];
		table[blockIdx.x] = sum;
	}
}

__global__ __launch_bounds__(kPopBlock) void k_pop_place_slots(const unsigned char* __restrict__ flags, const unsigned n, const unsigned at_least,
                                                               const unsigned* __restrict__ scanned, unsigned* __restrict__ slot) {
	__shared__ unsigned s_wave[kPopWaves];
	static_assert(sizeof(s_wave) == kLdsPop, "k_pop_place_slots: LDS");
	const unsigned t = threadIdx.x, lane = t & 63u, w = t >> 6;
	const unsigned first = blockIdx.x * (unsigned)kPopTile + w * (unsigned)(64 * kPopItems) + lane;
	const unsigned long long below = (1ull << lane) - 1ull;
	unsigned long long kept[kPopItems];
	unsigned count = 0;
#pragma unroll
	for (int j = 0; j < kPopItems; ++j) {
		kept[j] = kept_ballot(flags, n, at_least, first + (unsigned)(64 * j));
		count += (unsigned)__popcll(kept[j]);
	}
	if (lane == 0) s_wave[w] = count;
	__syncthreads();
	unsigned at = scanned[blockIdx.x];  // (a select's table never saturates: its sum is <= n < 2^31)
#pragma unroll
	for (int k = 0; k < kPopWaves; ++k) at += (unsigned)k < w ? s_wave[k] : 0u;
#pragma unroll
	for (int j = 0; j < kPopItems; ++j) {
		const unsigned p = first + (unsigned)(64 * j);
		if (p < n) slot[p] = (kept[j] >> lane) & 1ull ? at + (unsigned)__popcll(kept[j] & below) : kDropped;
		at += (unsigned)__popcll(kept[j]);
	}
}

// ---- the scan of a tile table, and the counters ---------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned saturated(unsigned long long at) { return at > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)at; }

// table[i] = start + the counts of the tiles below i; counters = {min(wanted, cap), wanted = start + the sum}; start = append ? live : 0
__global__ __launch_bounds__(kPopBlock) void k_pop_scan(unsigned* __restrict__ table, const unsigned n_tiles, unsigned long long* __restrict__ counters, const int append,
                                                        const unsigned long long cap) {
	__shared__ unsigned s_wave[kPopWaves];
	static_assert(sizeof(s_wave) == kLdsPop, "k_pop_scan: LDS");
	const unsigned t = threadIdx.x;
	unsigned long long carry = append ? counters[0] : 0ull;
	for (unsigned chunk = 0; chunk < n_tiles; chunk += (unsigned)kPopScanChunk) {
		const unsigned i0 = chunk + t * (unsigned)kPopScanItems;
		unsigned a[kPopScanItems], mine = 0;
#pragma unroll
		for (int k = 0; k < kPopScanItems; ++k) {
			a[k] = i0 + (unsigned)k < n_tiles ? table[i0 + (unsigned)k] : 0u;
			mine += a[k];
		}
		unsigned sum;  // (a round's sum: at most 1024 tiles of 2048 * 16)
		unsigned long long at = carry + block_scan(mine, s_wave, sum);
#pragma unroll
		for (int k = 0; k < kPopScanItems; ++k) {
			if (i0 + (unsigned)k < n_tiles) table[i0 + (unsigned)k] = saturated(at);
			at += a[k];
		}
		carry += sum;
	}
	__syncthreads();  // (every thread has read live before thread 0 writes it)
	if (t == 0) {
		counters[0] = carry < cap ? carry : cap;
		counters[1] = carry;
	}
}

__global__ void k_pop_set_live(unsigned long long* __restrict__ counters, const unsigned long long n) { counters[0] = counters[1] = n; }

// ---- birth: a field -> rows ------------------------------------------------------------------------------------------------------------------------------------------------

// WIDE: the field is 16-byte aligned, a z-row is two 16-byte loads
template <bool WIDE>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float (&v)[8]) {
	if (WIDE) {
		const float4 a = ((const float4*)p)[0], b = ((const float4*)p)[1];
		v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
	} else {
#pragma unroll
		for (int z = 0; z < 8; ++z) v[z] = p[z];
	}
}

// thread t of tile b: the z-row (x, y) = (t >> 3) & 7, t & 7 of leaf 4 b + (t >> 6), voxels e0 .. e0 + 7. -> the counts of its eight voxels, their hashes, and the sum
template <bool WIDE>
__device__ __forceinline__ unsigned row_counts(const GridDev& g, const float* __restrict__ field, const unsigned char* __restrict__ masks, const hns_birth_spec& sp,
                                               unsigned& e0, int (&ijk)[3], unsigned (&c)[8], unsigned (&h)[8]) {
	const unsigned t = threadIdx.x, leaf = blockIdx.x * (unsigned)kPopTileLeaves + (t >> 6), byte = t & 63u;
	e0 = leaf * 512u + byte * 8u;
	unsigned sum = 0;
#pragma unroll
	for (int z = 0; z < 8; ++z) c[z] = 0, h[z] = 0;
	if (leaf < (unsigned)g.n_leaves) {
		const int4 o = g.origins[leaf];
		ijk[0] = o.x + (int)(byte >> 3), ijk[1] = o.y + (int)(byte & 7u), ijk[2] = o.z;
		const unsigned bits = masks ? masks[(size_t)leaf * 64 + byte] : 0xFFu;
		float v[8];
		load_row<WIDE>(field + e0, v);
#pragma unroll
		for (int z = 0; z < 8; ++z) {
			c[z] = birth_count(v[z], (bits >> z) & 1u, ijk[0], ijk[1], ijk[2] + z, sp, &h[z]);
			sum += c[z];
		}
	}
	return sum;
}

template <bool WIDE>
__global__ __launch_bounds__(kPopBlock) void k_pop_count_births(const GridDev g, const float* __restrict__ field, const unsigned char* __restrict__ masks,
                                                                const hns_birth_spec sp, unsigned* __restrict__ table) {
	__shared__ unsigned s_wave[kPopWaves];
	static_assert(sizeof(s_wave) == kLdsPop, "k_pop_count_births: LDS");
	unsigned e0, c[8], h[8], sum;
	int ijk[3];
	const unsigned mine = row_counts<WIDE>(g, field, masks, sp, e0, ijk, c, h);
	(void)block_scan(mine, s_wave, sum);
	if (threadIdx.x == 0) table[blockIdx.x] = sum;
}

template <bool WIDE>
__global__ __launch_bounds__(kPopBlock) void k_pop_place_births(const GridDev g, const float* __restrict__ field, const unsigned char* __restrict__ masks,
                                                                const hns_birth_spec sp, const unsigned* __restrict__ scanned, float* __restrict__ xyz,
                                                                unsigned* __restrict__ voxel, const unsigned long long cap) {
	__shared__ unsigned s_wave[kPopWaves];
	static_assert(sizeof(s_wave) == kLdsPop, "k_pop_place_births: LDS");
	const unsigned long long tile_row = scanned[blockIdx.x];
	if (tile_row >= cap) return;  // (the whole workgroup: the rows of this tile and of every later one lie beyond the cap)
	unsigned e0, c[8], h[8], sum;
	int ijk[3];
	const unsigned mine = row_counts<WIDE>(g, field, masks, sp, e0, ijk, c, h);
	unsigned long long row = tile_row + block_scan(mine, s_wave, sum);
#pragma unroll
	for (int z = 0; z < 8; ++z) {
		for (unsigned q = 0; q < c[z]; ++q, ++row) {
			if (row >= cap) return;
			float* __restrict__ x = xyz + 3 * row;  // row < cap <= 2^31 - 1
			x[0] = birth_position(ijk[0], h[z], q, 0);
			x[1] = birth_position(ijk[1], h[z], q, 1);
			x[2] = birth_position(ijk[2] + z, h[z], q, 2);
			if (voxel) voxel[row] = e0 + (unsigned)z;
		}
	}
}

// rows live .. cap - 1: adjacent lanes take adjacent words of xyz
__global__ __launch_bounds__(kPopBlock) void k_pop_fill_births(const unsigned long long* __restrict__ counters, unsigned* __restrict__ xyz, unsigned* __restrict__ voxel,
                                                               const unsigned cap) {
	const unsigned long long live = counters[0];
	const unsigned row0 = blockIdx.x * (unsigned)kPopBlock;
	const unsigned rows = cap - row0 < (unsigned)kPopBlock ? cap - row0 : (unsigned)kPopBlock;
	if ((unsigned long long)row0 + rows <= live) return;
	for (unsigned l = threadIdx.x; l < rows * 3u; l += (unsigned)kPopBlock)
		if (row0 + l / 3u >= live) xyz[(size_t)row0 * 3 + l] = kBirthNaN;
	if (voxel && threadIdx.x < rows && row0 + threadIdx.x >= live) voxel[row0 + threadIdx.x] = kBirthNoVoxel;
}

// ---- rows through the slots --------------------------------------------------------------------------------------------------------------------------------------------------

// dst row slot[r] = src row r for the kept r < n; FILL: every word of dst rows live .. n - 1 = fill. A workgroup takes 256 rows; adjacent lanes adjacent words
template <bool FILL>
__global__ __launch_bounds__(kPopBlock) void k_pop_rows(const unsigned* __restrict__ slot, const unsigned long long* __restrict__ counters, const unsigned* __restrict__ src,
                                                        unsigned* __restrict__ dst, const unsigned n, const unsigned W, const unsigned fill) {
	const unsigned long long live = FILL ? counters[0] : 0ull;
	const unsigned row0 = blockIdx.x * (unsigned)kPopBlock;
	const unsigned rows = n - row0 < (unsigned)kPopBlock ? n - row0 : (unsigned)kPopBlock;
	for (unsigned l = threadIdx.x; l < rows * W; l += (unsigned)kPopBlock) {
		const unsigned rl = l / W, w = l - rl * W, r = row0 + rl;
		const unsigned to = slot[r];  // kDropped, or < live <= n
		if (to != kDropped) dst[(size_t)to * W + w] = src[(size_t)r * W + w];
		if (FILL && r >= live) dst[(size_t)r * W + w] = fill;  // (a moved row lands below live: no word is written twice)
	}
}

inline unsigned pop_tiles(uint64_t items) { return (unsigned)((items + kPopTile - 1) / kPopTile); }

}  // namespace
}  // namespace hns

using namespace hns;

struct hns_point_population {
	hns_grid* grid = nullptr;
	int device = -1;
	uint64_t capacity = 0, n_leaves = 0;
	hipStream_t stream = nullptr;
	// one pooled allocation: the slots, the tile table, the counters {live, wanted}
	Pooled arena;
	uint32_t *slot = nullptr, *table = nullptr;
	unsigned long long* counters = nullptr;
	uint64_t n = 0;  // of the last select
	bool selected = false;
};

namespace {

int check_population(const hns_point_population* o, const char* who) {
	if (!o) return refuse(who, "null point population");
	return check_grid(o->grid, who);
}

int birth(const char* who, hns_point_population* o, const float* d_field, const unsigned char* d_masks, const hns_birth_spec* sp, float* d_xyz, uint32_t* d_voxel,
          uint64_t capacity_rows, int append) {
	if (const char* what = birth_spec_refusal(sp)) return refuse(who, what);
	if (capacity_rows > kMaxPoints) return refuse(who, "capacity_rows is above 2^31 - 1");
	if (!o->n_leaves) return refuse(who, "the grid has no leaves");
	if (!d_field) return refuse(who, "null d_field");
	if (capacity_rows && !d_xyz) return refuse(who, "null d_xyz");
	if (d_xyz && ((const void*)d_xyz == (const void*)d_field || (const void*)d_xyz == (const void*)d_voxel)) return refuse(who, "d_xyz is d_field or d_voxel");
	const hipStream_t st = o->stream;
	const unsigned tiles = pop_tiles(o->n_leaves * 512);
	const dim3 block(kPopBlock);
	const GridDev g = o->grid->dev();
	const unsigned long long cap = capacity_rows;
	if (((uintptr_t)d_field & 15) == 0) {
		hipLaunchKernelGGL((k_pop_count_births<true>), dim3(tiles), block, 0, st, g, d_field, d_masks, *sp, o->table);
		hipLaunchKernelGGL(k_pop_scan, dim3(1), block, 0, st, o->table, tiles, o->counters, append ? 1 : 0, cap);
		hipLaunchKernelGGL((k_pop_place_births<true>), dim3(tiles), block, 0, st, g, d_field, d_masks, *sp, (const uint32_t*)o->table, d_xyz, d_voxel, cap);
	} else {
		hipLaunchKernelGGL((k_pop_count_births<false>), dim3(tiles), block, 0, st, g, d_field, d_masks, *sp, o->table);
		hipLaunchKernelGGL(k_pop_scan, dim3(1), block, 0, st, o->table, tiles, o->counters, append ? 1 : 0, cap);
		hipLaunchKernelGGL((k_pop_place_births<false>), dim3(tiles), block, 0, st, g, d_field, d_masks, *sp, (const uint32_t*)o->table, d_xyz, d_voxel, cap);
	}
	if (sp->fill && capacity_rows)
		hipLaunchKernelGGL(k_pop_fill_births, dim3((unsigned)((capacity_rows + kPopBlock - 1) / kPopBlock)), block, 0, st, (const unsigned long long*)o->counters,
		                   (unsigned*)d_xyz, d_voxel, (unsigned)capacity_rows);
	return launch_status(who);
}

}  // namespace

extern "C" {

hns_point_population* hns_point_population_create(hns_grid* g, uint64_t capacity, int* err) {
	const char* who = "hns_point_population_create";
	return make_object<hns_point_population>(who, err, true, g, capacity, "; hns_grid_birth_points is the host's", [&](hns_point_population* o) {
		const uint64_t L = (uint64_t)g->topo.n_leaves;
		if (L * 512 > (uint64_t(1) << 32)) return refuse(who, "the grid's voxel indices do not fit 32 bits (leaves * 512 > 2^32)");
		o->grid = g, o->capacity = capacity, o->n_leaves = L;
		const size_t cap = (size_t)std::max<uint64_t>(capacity, 1), tiles = std::max<size_t>(pop_tiles(std::max<uint64_t>(capacity, L * 512)), 1);
		HNS_TRY(carve(o->arena, g->device, [&](const Slice& slice) { slice(o->slot, 4 * cap), slice(o->table, 4 * tiles), slice(o->counters, 16); }));
		if (hipMemsetAsync(o->counters, 0, 16, nullptr) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
			return fail(HNS_ERR_HIP, "hns_point_population_create: clearing the counters failed");
		return (int)HNS_OK;
	});
}

void hns_point_population_destroy(hns_point_population* o) {
	if (!o) return;
	delete o;  // (its block goes back to the pool, which waits for the device first)
}

int hns_point_population_set_stream(hns_point_population* o, void* hip_stream) {
	return set_object_stream(o, hip_stream, "hns_point_population_set_stream", "null point population");
}

int hns_point_population_set_live(hns_point_population* o, uint64_t n) {
	const char* who = "hns_point_population_set_live";
	HNS_TRY(check_population(o, who));
	if (n > kMaxPoints) return refuse(who, "n is above 2^31 - 1");
	hipLaunchKernelGGL(k_pop_set_live, dim3(1), dim3(1), 0, o->stream, o->counters, (unsigned long long)n);
	return launch_status(who);
}

int hns_point_population_select(hns_point_population* o, const unsigned char* d_flags, uint64_t n, int at_least) {
	const char* who = "hns_point_population_select";
	HNS_TRY(check_population(o, who));
	if (n > kMaxPoints) return refuse(who, "n is above 2^31 - 1");
	HNS_TRY(check_capacity(who, n, o->capacity));
	if (at_least < 1 || at_least > 255) {
		set_error("%s: at_least %d (1 .. 255)", who, at_least);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (n && !d_flags) return refuse(who, "null d_flags");
	const hipStream_t st = o->stream;
	o->n = n, o->selected = true;
	if (!n) {
		HNS_HIP(hipMemsetAsync(o->counters, 0, 16, st));
		return HNS_OK;
	}
	const unsigned tiles = pop_tiles(n), un = (unsigned)n;
	const dim3 block(kPopBlock);
	hipLaunchKernelGGL(k_pop_count_flags, dim3(tiles), block, 0, st, d_flags, un, (unsigned)at_least, o->table);
	hipLaunchKernelGGL(k_pop_scan, dim3(1), block, 0, st, o->table, tiles, o->counters, 0, ~0ull);
	hipLaunchKernelGGL(k_pop_place_slots, dim3(tiles), block, 0, st, d_flags, un, (unsigned)at_least, (const uint32_t*)o->table, o->slot);
	return launch_status(who);
}

int hns_point_population_compact(const hns_point_population* o, const void* d_src, void* d_dst, int row_bytes, const uint32_t* fill_word) {
	const char* who = "hns_point_population_compact";
	HNS_TRY(check_population(o, who));
	HNS_TRY(check_rows(who, o->selected, "select", o->n, d_src, d_dst, row_bytes));
	if (!o->n) return HNS_OK;
	const dim3 grid((unsigned)((o->n + kPopBlock - 1) / kPopBlock)), block(kPopBlock);
	const unsigned W = (unsigned)(row_bytes / 4);
	if (fill_word)
		hipLaunchKernelGGL((k_pop_rows<true>), grid, block, 0, o->stream, (const uint32_t*)o->slot, (const unsigned long long*)o->counters, (const unsigned*)d_src,
		                   (unsigned*)d_dst, (unsigned)o->n, W, *fill_word);
	else
		hipLaunchKernelGGL((k_pop_rows<false>), grid, block, 0, o->stream, (const uint32_t*)o->slot, (const unsigned long long*)o->counters, (const unsigned*)d_src,
		                   (unsigned*)d_dst, (unsigned)o->n, W, 0u);
	return launch_status(who);
}

int hns_point_population_birth(hns_point_population* o, const float* d_field, const unsigned char* d_masks, const hns_birth_spec* sp, float* d_xyz, uint32_t* d_voxel,
                               uint64_t capacity_rows, int append) {
	const char* who = "hns_point_population_birth";
	HNS_TRY(check_population(o, who));
	return birth(who, o, d_field, d_masks, sp, d_xyz, d_voxel, capacity_rows, append);
}

int hns_point_population_birth_sim(hns_point_population* o, hns_sim* s, const char* name, int use_masks, const hns_birth_spec* sp, float* d_xyz, uint32_t* d_voxel,
                                   uint64_t capacity_rows, int append) {
	const char* who = "hns_point_population_birth_sim";
	HNS_TRY(check_population(o, who));
	HNS_TRY(check_sim(s, who));
	if (s->grid != o->grid) return refuse(who, "the sim's grid is not the object's grid");
	const int f = name ? s->find(name) : -1;
	if (f < 0) {
		set_error("%s: the sim has no float field '%s'", who, name ? name : "(null)");
		return HNS_ERR_INVALID_ARGUMENT;
	}
	return birth(who, o, s->cur[(size_t)f], use_masks ? s->d_masks.as<unsigned char>() : nullptr, sp, d_xyz, d_voxel, capacity_rows, append);
}

int hns_point_population_get(const hns_point_population* o, hns_point_population_info* info) {
	if (!o) return refuse("hns_point_population_get", "null point population");
	if (!info) return refuse("hns_point_population_get", "null info");
	*info = hns_point_population_info{o->slot, (const uint64_t*)o->counters, o->n, o->capacity};
	return HNS_OK;
}

int hns_point_population_counts(hns_point_population* o, uint64_t* live, uint64_t* wanted) {
	const char* who = "hns_point_population_counts";
	HNS_TRY(check_population(o, who));
	unsigned long long c[2] = {0, 0};
	HNS_HIP(hipMemcpyAsync(c, o->counters, 16, hipMemcpyDeviceToHost, o->stream));
	HNS_HIP(hipStreamSynchronize(o->stream));
	if (live) *live = c[0];
	if (wanted) *wanted = c[1];
	return HNS_OK;
}

}  // extern "C"
