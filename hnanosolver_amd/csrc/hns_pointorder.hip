// hns_pointorder.hip -- the leaf order of a device-resident point set (include/hns.h: "THE LEAF ORDER OF A POINT SET" states the definition): a stable sort of the points by
// the voxel, or the leaf, of their cell as a permutation with per-leaf ranges, and the row moves that carry per-point attributes through it. The point kernels
// (hns_points.hip, hns_splat.hip) run some five times faster on points in this order; nothing else under csrc/ sorts on the device.
//
// A least-significant-digit radix sort of (key, index) pairs, 8-bit digits, over tiles of kOrderTile consecutive points; 1 .. 4 passes, fixed by the grid and the level:
//   k_order_keys     one thread per point and round: seeds_f, the cell and the leaf lookup of hns_points.hpp (point_cell), the key; fused with the first pass's tile histogram
//   k_order_hist     the tile histograms of a later pass (the tiles hold other points after every scatter)
//   k_order_totals   one workgroup per digit: the sum of its row of the [digit][tile] table
//   k_order_scan     one workgroup per digit: the digit's base from the totals of the digits below, then an exclusive scan along its row of the table, in place
//   k_order_scatter  one workgroup per tile. A wave takes 64 consecutive points per round, so rank order is index order: the rank of a point among its wave's equal
//                    digits comes from ballots over the digit's bits and the lanes below, the counts of earlier rounds and waves sit in LDS, tiles are taken in index
//                    order by the scan. The tile is then put in digit order in LDS, so that the global stores of a digit's run are contiguous.
//   k_order_ranges   one thread per rank: where the leaf-level key changes from a to b the wave stores leaf_start[a + 1 .. b], each entry exactly once, plain stores
//   k_order_rows     gather / scatter of rows of 1 .. 16 words through perm: adjacent lanes take adjacent words of a row
// No kernel waits on another workgroup: every dependence is a launch boundary. The only atomics are integer adds in LDS (a tile's histogram counts: sums of integers, unique
// whatever the order); no float atomics, no scratch. Every index below is bounded by n < 2^31 and by the tile: the histograms count exactly the points the scatter places.
#include "hns_blockscan.hpp"
#include "hns_points.hpp"

namespace hns {
namespace {

constexpr int kOrderBlock = 256;                          // threads of every kernel here: four waves
constexpr int kOrderWaves = kOrderBlock / 64;
constexpr int kOrderItems = 8;                            // points per thread of a tile
constexpr int kOrderTile = kOrderBlock * kOrderItems;     // 2048 points: what device.POINT_ORDER_TILE states to the tests
constexpr int kRadix = 256;                               // 8-bit digits; one digit per thread of a workgroup
constexpr int kScanItems = 4;                             // table entries per thread and round of k_order_scan
constexpr int kScanChunk = kOrderBlock * kScanItems;      // 1024 tiles per round: device.POINT_ORDER_SCAN_TILES
static_assert(kRadix == kOrderBlock, "k_order_scan and k_order_scatter give every digit one thread");
static_assert(kOrderBlock == kBlockScanThreads && kOrderWaves == kBlockScanWaves, "block_scan (hns_blockscan.hpp) scans a workgroup of this size");

// LDS per kernel, stated and held
constexpr int kLdsKeys = kRadix * 4;                                                                        // k_order_keys, k_order_hist: the tile's histogram
constexpr int kLdsScan = kOrderWaves * 4;                                                                   // k_order_scan: the waves' totals
constexpr int kLdsScatter = kOrderWaves * kRadix * 4 + kRadix * 4 + 2 * kOrderTile * 4 + kOrderWaves * 4;  // k_order_scatter: 21,520 bytes, seven workgroups a CU
static_assert(kLdsScatter <= 22 * 1024, "k_order_scatter: LDS per workgroup");

// the voxel key of point p (include/hns.h: "Voxel key"); n_leaves = L
__device__ __forceinline__ unsigned point_key(const GridDev& g, const float* __restrict__ xyz, unsigned p) {
	const f3 x = ld3(xyz, (int)p);
	if (!(seeds_f(x.x) && seeds_f(x.y) && seeds_f(x.z))) return 512u * ((unsigned)g.n_leaves + 1u);
	Cursor none{-1, 0, 0, 0};
	const Cell C = point_cell<false>(g, none, x.x, x.y, x.z);  // (only the lower corner is used: the other seven lookups are dead code)
	return C.t[0] < 0 ? 512u * (unsigned)g.n_leaves : (unsigned)C.t[0];
}

// one count into the tile's histogram. Coherent points put a whole wave on one digit: then one lane adds the wave's count instead of 64 adds to one address
__device__ __forceinline__ void hist_add(unsigned* s_hist, unsigned digit, bool valid) {
	const unsigned long long live = __ballot(valid);
	if (!live) return;
	const unsigned first = (unsigned)__shfl((int)digit, __ffsll((long long)live) - 1);
	if (__all(!valid || digit == first)) {
		if (valid && (live & ((1ull << (threadIdx.x & 63)) - 1)) == 0) atomicAdd(&s_hist[digit], (unsigned)__popcll(live));
	} else if (valid) {
		atomicAdd(&s_hist[digit], 1u);
	}
}

// the tile's histogram leaves LDS: its column of the [digit][tile] table
__device__ __forceinline__ void hist_store(const unsigned* s_hist, unsigned* __restrict__ hist, unsigned n_tiles) { hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = s_hist[threadIdx.x]; }

__global__ __launch_bounds__(kOrderBlock) void k_order_keys(const GridDev g, const float* __restrict__ xyz, const unsigned n, const int level, unsigned* __restrict__ keys,
                                                            unsigned* __restrict__ hist, const unsigned n_tiles) {
	__shared__ unsigned s_hist[kRadix];
	static_assert(sizeof(s_hist) == kLdsKeys, "k_order_keys: LDS");
	s_hist[threadIdx.x] = 0;
	__syncthreads();
	const unsigned base = blockIdx.x * (unsigned)kOrderTile + threadIdx.x;
	for (int j = 0; j < kOrderItems; ++j) {
		const unsigned p = base + (unsigned)(j * kOrderBlock);
		const bool valid = p < n;
		unsigned key = 0;
		if (valid) {
			key = point_key(g, xyz, p);
			key = level ? key : key >> 9;
			keys[p] = key;
		}
		hist_add(s_hist, key & (kRadix - 1), valid);
	}
	__syncthreads();
	hist_store(s_hist, hist, n_tiles);
}

__global__ __launch_bounds__(kOrderBlock) void k_order_hist(const unsigned* __restrict__ keys, const unsigned n, const int shift, unsigned* __restrict__ hist,
                                                            const unsigned n_tiles) {
	__shared__ unsigned s_hist[kRadix];
	static_assert(sizeof(s_hist) == kLdsKeys, "k_order_hist: LDS");
	s_hist[threadIdx.x] = 0;
	__syncthreads();
	const unsigned base = blockIdx.x * (unsigned)kOrderTile + threadIdx.x;
#pragma unroll
	for (int j = 0; j < kOrderItems; ++j) {
		const unsigned p = base + (unsigned)(j * kOrderBlock);
		const bool valid = p < n;
		const unsigned key = valid ? keys[p] : 0u;
		hist_add(s_hist, (key >> shift) & (kRadix - 1), valid);
	}
	__syncthreads();
	hist_store(s_hist, hist, n_tiles);
}

// total[d] = the sum of row d of the table: how many points hold digit d. One workgroup per digit, a plain store (512 k atomic adds of the tiles into 256 words took
// 36 us a pass at 2^22 points: profiles/point_order_ab.txt)
__global__ __launch_bounds__(kOrderBlock) void k_order_totals(const unsigned* __restrict__ hist, unsigned* __restrict__ total, const unsigned n_tiles) {
	__shared__ unsigned s_wave[kOrderWaves];
	static_assert(sizeof(s_wave) == kLdsScan, "k_order_totals: LDS");
	const unsigned* __restrict__ row = hist + (size_t)blockIdx.x * n_tiles;
	unsigned mine = 0, sum;
	for (unsigned i = threadIdx.x; i < n_tiles; i += (unsigned)kOrderBlock) mine += row[i];
	(void)block_scan(mine, s_wave, sum);
	if (threadIdx.x == 0) total[blockIdx.x] = sum;
}

// row d of the table: counts of digit d per tile -> where the tile's first point of digit d goes
__global__ __launch_bounds__(kOrderBlock) void k_order_scan(unsigned* __restrict__ hist, const unsigned* __restrict__ total, const unsigned n_tiles) {
	__shared__ unsigned s_wave[kOrderWaves];
	static_assert(sizeof(s_wave) == kLdsScan, "k_order_scan: LDS");
	const unsigned d = blockIdx.x, t = threadIdx.x;
	unsigned carry;
	(void)block_scan(t < d ? total[t] : 0u, s_wave, carry);  // every point of a smaller digit comes first
	unsigned* __restrict__ row = hist + (size_t)d * n_tiles;
	for (unsigned chunk = 0; chunk < n_tiles; chunk += (unsigned)kScanChunk) {
		const unsigned i0 = chunk + t * (unsigned)kScanItems;
		unsigned a[kScanItems], mine = 0;
#pragma unroll
		for (int k = 0; k < kScanItems; ++k) {
			a[k] = i0 + (unsigned)k < n_tiles ? row[i0 + (unsigned)k] : 0u;
			mine += a[k];
		}
		unsigned sum;
		unsigned at = carry + block_scan(mine, s_wave, sum);
#pragma unroll
		for (int k = 0; k < kScanItems; ++k) {
			if (i0 + (unsigned)k < n_tiles) row[i0 + (unsigned)k] = at;
			at += a[k];
		}
		carry += sum;
	}
}

// FIRST: the pass behind k_order_keys, whose index is the point's own
template <bool FIRST>
__global__ __launch_bounds__(kOrderBlock) void k_order_scatter(const unsigned* __restrict__ keys_in, const unsigned* __restrict__ idx_in, const unsigned n, const int shift,
                                                               const unsigned* __restrict__ scanned, const unsigned n_tiles, unsigned* __restrict__ keys_out,
                                                               unsigned* __restrict__ idx_out) {
	__shared__ unsigned s_cnt[kOrderWaves][kRadix];  // per wave and digit: the count so far, then where the wave's first point of the digit lies in the tile
	__shared__ unsigned s_base[kRadix];              // global position of the digit's run minus its start in the tile
	__shared__ unsigned s_key[kOrderTile], s_idx[kOrderTile];
	__shared__ unsigned s_wave[kOrderWaves];
	static_assert(sizeof(s_cnt) + sizeof(s_base) + sizeof(s_key) + sizeof(s_idx) + sizeof(s_wave) == kLdsScatter, "k_order_scatter: LDS");
	const unsigned t = threadIdx.x, lane = t & 63u, w = t >> 6;
	const unsigned tile0 = blockIdx.x * (unsigned)kOrderTile;
#pragma unroll
	for (int k = 0; k < kOrderWaves; ++k) s_cnt[k][t] = 0;
	__syncthreads();
	// wave w holds points tile0 + 512 w .. + 511, round j the 64 consecutive ones from 64 j on: within the tile, index order is (wave, round, lane) order
	const unsigned first = tile0 + w * (unsigned)(64 * kOrderItems) + lane;
	const unsigned long long below = (1ull << lane) - 1ull;
	unsigned key[kOrderItems], idx[kOrderItems], off[kOrderItems];
#pragma unroll
	for (int j = 0; j < kOrderItems; ++j) {
		const unsigned p = first + (unsigned)(64 * j);
		key[j] = p < n ? keys_in[p] : 0u;
		idx[j] = FIRST ? p : (p < n ? idx_in[p] : 0u);
	}
#pragma unroll
	for (int j = 0; j < kOrderItems; ++j) {
		const bool valid = first + (unsigned)(64 * j) < n;
		const unsigned digit = (key[j] >> shift) & (kRadix - 1);
		unsigned long long same = __ballot(valid);  // the valid lanes of equal digit
#pragma unroll
		for (int b = 0; b < 8; ++b) {
			const bool bit = (digit >> b) & 1u;
			const unsigned long long set = __ballot(bit);
			same &= bit ? set : ~set;
		}
		const unsigned rank = (unsigned)__popcll(same & below);
		const unsigned before = s_cnt[w][digit];
		wave_sync();  // (every lane has read the count before its digit's lowest lane raises it)
		if (valid && rank == 0) s_cnt[w][digit] = before + (unsigned)__popcll(same);
		wave_sync();
		off[j] = before + rank;
	}
	__syncthreads();
	{  // thread t is digit t: its run's start in the tile, the waves' starts inside the run, and where the run goes
		unsigned c[kOrderWaves], mine = 0;
#pragma unroll
		for (int k = 0; k < kOrderWaves; ++k) mine += c[k] = s_cnt[k][t];
		unsigned sum;
		unsigned at = block_scan(mine, s_wave, sum);
		s_base[t] = scanned[(size_t)t * n_tiles + blockIdx.x] - at;
#pragma unroll
		for (int k = 0; k < kOrderWaves; ++k) {
			s_cnt[k][t] = at;
			at += c[k];
		}
	}
	__syncthreads();
#pragma unroll
	for (int j = 0; j < kOrderItems; ++j) {
		if (first + (unsigned)(64 * j) < n) {
			const unsigned at = s_cnt[w][(key[j] >> shift) & (kRadix - 1)] + off[j];  // < the tile's count <= kOrderTile
			s_key[at] = key[j];
			s_idx[at] = idx[j];
		}
	}
	__syncthreads();
	const unsigned count = n - tile0 < (unsigned)kOrderTile ? n - tile0 : (unsigned)kOrderTile;
#pragma unroll
	for (int j = 0; j < kOrderItems; ++j) {
		const unsigned e = (unsigned)(j * kOrderBlock) + t;
		if (e < count) {
			const unsigned k = s_key[e];
			const unsigned at = s_base[(k >> shift) & (kRadix - 1)] + e;  // < n: base of the digit's run + position in the run
			keys_out[at] = k;
			idx_out[at] = s_idx[e];
		}
	}
}

// leaf_start over the sorted keys; shift: 9 at level 1 (voxel keys), 0 at level 0. top = L + 2
__global__ __launch_bounds__(kOrderBlock) void k_order_ranges(const unsigned* __restrict__ keys, const unsigned n, const int shift, const unsigned top,
                                                              unsigned* __restrict__ leaf_start) {
	const unsigned r = blockIdx.x * (unsigned)kOrderBlock + threadIdx.x, lane = threadIdx.x & 63u;
	const bool valid = r < n;
	const unsigned b = valid ? keys[r] >> shift : 0u;
	const unsigned lo = valid && r > 0 ? (keys[r - 1] >> shift) + 1u : 0u;
	// entries lo .. b get r (none where the key did not change: lo = b + 1); behind the last rank, entries b + 1 .. top get n. The wave stores each stretch together
	unsigned long long edges = __ballot(valid && lo <= b);
	while (edges) {
		const int src = __ffsll((long long)edges) - 1;
		edges &= edges - 1;
		const unsigned from = (unsigned)__shfl((int)lo, src), to = (unsigned)__shfl((int)b, src), rank = (unsigned)__shfl((int)r, src);
		for (unsigned q = from + lane; q <= to; q += 64u) leaf_start[q] = rank;
	}
	const unsigned long long last = __ballot(valid && r == n - 1u);
	if (last) {
		const unsigned from = (unsigned)__shfl((int)b, __ffsll((long long)last) - 1) + 1u;
		for (unsigned q = from + lane; q <= top; q += 64u) leaf_start[q] = n;
	}
}

// rows of W words through perm. SCATTER: dst row perm[r] = src row r; else dst row r = src row perm[r]. A workgroup takes 256 rows; adjacent lanes adjacent words
template <bool SCATTER>
__global__ __launch_bounds__(kOrderBlock) void k_order_rows(const unsigned* __restrict__ perm, const unsigned* __restrict__ src, unsigned* __restrict__ dst, const unsigned n,
                                                            const unsigned W) {
	const unsigned row0 = blockIdx.x * (unsigned)kOrderBlock;
	const unsigned rows = n - row0 < (unsigned)kOrderBlock ? n - row0 : (unsigned)kOrderBlock;
	for (unsigned l = threadIdx.x; l < rows * W; l += (unsigned)kOrderBlock) {
		const unsigned rl = l / W, w = l - rl * W, r = row0 + rl;
		const size_t here = (size_t)r * W + w, there = (size_t)perm[r] * W + w;
		if (SCATTER)
			dst[there] = src[here];
		else
			dst[here] = src[there];
	}
}

// passes of a sort: ceil(bits of the largest key / 8)
int order_passes(uint64_t n_leaves, int level) {
	const uint64_t top = level ? 512 * (n_leaves + 1) : n_leaves + 1;
	int bits = 0;
	while (bits < 32 && (top >> bits)) ++bits;
	return std::max(1, (bits + 7) / 8);
}

inline unsigned order_tiles(uint64_t n) { return (unsigned)((n + kOrderTile - 1) / kOrderTile); }

}  // namespace
}  // namespace hns

using namespace hns;

namespace {  // (struct hns_point_order and check_order: hns_points.hpp, shared with hns_splat_binned.hip)

template <bool SCATTER>
int move_rows(const hns_point_order* o, const void* d_src, void* d_dst, int row_bytes, const char* who) {
	HNS_TRY(check_order(o, who));
	HNS_TRY(check_rows(who, o->sorted, "sort", o->n, d_src, d_dst, row_bytes));
	if (!o->n) return HNS_OK;
	hipLaunchKernelGGL((k_order_rows<SCATTER>), dim3((unsigned)((o->n + kOrderBlock - 1) / kOrderBlock)), dim3(kOrderBlock), 0, o->stream, o->perm, (const unsigned*)d_src,
	                   (unsigned*)d_dst, (unsigned)o->n, (unsigned)(row_bytes / 4));
	return launch_status(who);
}

}  // namespace

extern "C" {

hns_point_order* hns_point_order_create(hns_grid* g, uint64_t capacity, int* err) {
	const char* who = "hns_point_order_create";
	return make_object<hns_point_order>(who, err, true, g, capacity, "; hns_grid_sort_points is the host's", [&](hns_point_order* o) {
		const uint64_t L = (uint64_t)g->topo.n_leaves;
		if ((L + 2) * 512 > (uint64_t(1) << 32)) return refuse(who, "the grid's voxel keys do not fit 32 bits ((leaves + 2) * 512 > 2^32)");
		o->grid = g, o->capacity = capacity, o->n_leaves = L;
		const size_t cap = (size_t)std::max<uint64_t>(capacity, 1), tiles = order_tiles(cap);
		return carve(o->arena, g->device, [&](const Slice& slice) {
			slice(o->perm, 4 * cap), slice(o->keys, 4 * cap), slice(o->ka, 4 * cap), slice(o->ia, 4 * cap), slice(o->kb, 4 * cap), slice(o->ib, 4 * cap);
			slice(o->leaf_start, 4 * (size_t)(L + 3)), slice(o->hist, 4 * (size_t)kRadix * tiles), slice(o->total, 4 * (size_t)kRadix);
		});
	});
}

void hns_point_order_destroy(hns_point_order* o) {
	if (!o) return;
	delete o;  // (its two blocks go back to the pool, which waits for the device first)
}

int hns_point_order_set_stream(hns_point_order* o, void* hip_stream) { return set_object_stream(o, hip_stream, "hns_point_order_set_stream", "null point order"); }

int hns_point_order_sort(hns_point_order* o, const float* d_xyz, uint64_t n, int level) {
	const char* who = "hns_point_order_sort";
	HNS_TRY(check_order(o, who));
	if (n > kMaxPoints) return refuse(who, "n is above 2^31 - 1");
	HNS_TRY(check_capacity(who, n, o->capacity));
	if (level != 0 && level != 1) {
		set_error("%s: level %d (0: by leaf, 1: by voxel)", who, level);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (n && !d_xyz) return refuse(who, "xyz is null");
	const hipStream_t st = o->stream;
	const unsigned L = (unsigned)o->n_leaves;
	o->n = n, o->level = level, o->sorted = true, o->cells_fresh = false;
	if (!n) {
		HNS_HIP(hipMemsetAsync(o->leaf_start, 0, 4 * (size_t)(L + 3), st));
		return HNS_OK;
	}
	const int passes = order_passes(L, level);
	const unsigned tiles = order_tiles(n), un = (unsigned)n;
	const dim3 block(kOrderBlock);
	hipLaunchKernelGGL(k_order_keys, dim3(tiles), block, 0, st, o->grid->dev(), d_xyz, un, level, o->kb, o->hist, tiles);
	const uint32_t *kin = o->kb, *iin = nullptr;
	for (int p = 0; p < passes; ++p) {
		if (p) hipLaunchKernelGGL(k_order_hist, dim3(tiles), block, 0, st, kin, un, 8 * p, o->hist, tiles);
		hipLaunchKernelGGL(k_order_totals, dim3(kRadix), block, 0, st, (const uint32_t*)o->hist, o->total, tiles);
		hipLaunchKernelGGL(k_order_scan, dim3(kRadix), block, 0, st, o->hist, (const uint32_t*)o->total, tiles);
		const bool last = p == passes - 1;
		uint32_t *kout = last ? o->keys : (p & 1 ? o->kb : o->ka), *iout = last ? o->perm : (p & 1 ? o->ib : o->ia);
		if (p)
			hipLaunchKernelGGL((k_order_scatter<false>), dim3(tiles), block, 0, st, kin, iin, un, 8 * p, (const uint32_t*)o->hist, tiles, kout, iout);
		else
			hipLaunchKernelGGL((k_order_scatter<true>), dim3(tiles), block, 0, st, kin, iin, un, 0, (const uint32_t*)o->hist, tiles, kout, iout);
		kin = kout, iin = iout;
	}
	hipLaunchKernelGGL(k_order_ranges, dim3((un + kOrderBlock - 1) / kOrderBlock), block, 0, st, (const uint32_t*)o->keys, un, level ? 9 : 0, L + 2, o->leaf_start);
	return launch_status(who);
}

int hns_point_order_get(const hns_point_order* o, hns_point_order_info* info) {
	if (!o) return refuse("hns_point_order_get", "null point order");
	if (!info) return refuse("hns_point_order_get", "null info");
	*info = hns_point_order_info{o->perm, o->keys, o->leaf_start, o->n, o->n_leaves, o->capacity, o->level};
	return HNS_OK;
}

int hns_point_order_gather(const hns_point_order* o, const void* d_src, void* d_dst, int row_bytes) { return move_rows<false>(o, d_src, d_dst, row_bytes, "hns_point_order_gather"); }

int hns_point_order_scatter(const hns_point_order* o, const void* d_src, void* d_dst, int row_bytes) { return move_rows<true>(o, d_src, d_dst, row_bytes, "hns_point_order_scatter"); }

}  // extern "C"
