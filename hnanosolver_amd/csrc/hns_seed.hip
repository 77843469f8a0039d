// hns_seed.hip -- the seeds of a device-resident point set (include/hns.h: hns_point_leaves states the definition): the leaves under the eight taps of every point's
// cell and, per leaf, exactly the tap bits -- what a point emitter needs the domain to hold before it splats. hns_sim_regrid_seeded (hns_regrid.hip) dilates the set into the
// next domain without it crossing PCIe; hns_dev_point_leaves brings it to the host in OpenVDB leaf order.
//
// Two passes over the points, because the number of leaves is not known beforehand, both shaped to issue almost no atomic where points are coherent (an emitter):
//   k_seed_keys     one thread per point: its 1, 2, 4 or 8 leaves as 63-bit keys into a claim table (hns_originhash.hpp: claim_slot). Equal keys are merged within the wave
//                   BEFORE memory is touched
//   k_seed_compact  every occupied slot gets a leaf index (wave_compact) and writes its origin
//   k_seed_masks    one thread per point: the leaf index of each of its leaves by loads alone, then the tap bits as at most eight 64-bit ORs (two when the cell lies inside
//                   one leaf), merged within the wave like the keys and each skipped when a load shows its bits already set
// Bits are only ever set, so a stale load can only cause an OR that was not needed (as for the keys: claim_slot). Everything that decides the result is order-free: a
// set of keys, ORs of bits; the compacted order is discarded by whoever sorts. Integer atomics only, no LDS.
#include <cstring>

#include "hns_device.hpp"
#include "hns_seed.hpp"

namespace hns {
namespace {

constexpr int kMergeRounds = 8;  // distinct keys (mask words) a wave merges per slot before its lanes insert (OR) on their own

// The key table: a claim table of mask + 1 >= 2 min(8n, 2^23) slots. count: [0..2] as claim_slot states them ([2]: leaves), [3] points that do not seed.
struct SeedTable {
	unsigned long long* keys;
	int* leaf;  // slot -> leaf index, written by k_seed_compact for occupied slots only
	uint32_t mask;
	unsigned long long reserve;  // reservations allowed: below the table size, so a probe always meets an empty slot
	unsigned long long* count;
};

// three leaf coordinates (cell >> 3, in [-2^20, 2^20)) biased by 2^20, 21 bits each: never kEmptySlot
__device__ __forceinline__ unsigned long long leaf_key(int lx, int ly, int lz) {
	return (unsigned long long)(unsigned)(lx + (1 << 20)) << 42 | (unsigned long long)(unsigned)(ly + (1 << 20)) << 21 | (unsigned long long)(unsigned)(lz + (1 << 20));
}
__device__ __forceinline__ int4 key_origin(unsigned long long k) {
	return make_int4(((int)(k >> 42) - (1 << 20)) * 8, ((int)(k >> 21 & 0x1fffffu) - (1 << 20)) * 8, ((int)(k & 0x1fffffu) - (1 << 20)) * 8, 0);
}
__device__ __forceinline__ uint32_t key_slot(unsigned long long k, uint32_t mask) {
	const int4 o = key_origin(k);
	return hash_origin(o.x, o.y, o.z) & mask;
}

// The cell of a seeding point: lower corner (i, j, k), which axes cross into the next leaf, the lower leaf's coordinates.
struct SeedCell {
	int i, j, k, lx, ly, lz;
	bool cx, cy, cz;
	// is leaf slot c = di*4 + dj*2 + dk one of the cell's distinct leaves?
	__device__ __forceinline__ bool has(int c) const { return (!(c & 4) || cx) && (!(c & 2) || cy) && (!(c & 1) || cz); }
	__device__ __forceinline__ unsigned long long key(int c) const { return leaf_key(lx + (c >> 2), ly + ((c >> 1) & 1), lz + (c & 1)); }
};
__device__ __forceinline__ bool seed_cell(const float* __restrict__ xyz, unsigned p, SeedCell& C) {
	const float x = xyz[3 * (size_t)p], y = xyz[3 * (size_t)p + 1], z = xyz[3 * (size_t)p + 2];
	if (!(seeds_f(x) && seeds_f(y) && seeds_f(z))) return false;
	C.i = __float2int_rd(x), C.j = __float2int_rd(y), C.k = __float2int_rd(z);
	C.lx = C.i >> 3, C.ly = C.j >> 3, C.lz = C.k >> 3;
	C.cx = (C.i & 7) == 7, C.cy = (C.j & 7) == 7, C.cz = (C.k & 7) == 7;
	return true;
}

__global__ __launch_bounds__(256) void k_seed_keys(const float* __restrict__ xyz, const unsigned n, const SeedTable t) {
	const unsigned p = blockIdx.x * 256u + threadIdx.x;
	const int lane = (int)(threadIdx.x & 63u);
	SeedCell C{};
	const bool seeds = p < n && seed_cell(xyz, p, C);
	// whole waves from here on: nothing above returns
	for (int c = 0; c < 8; ++c) {
		bool pending = seeds && C.has(c);
		if (!__ballot(pending)) continue;
		const unsigned long long key = pending ? C.key(c) : kEmptySlot;
		bool mine = false;  // this lane inserts for every lane of the wave that held its key
		for (int r = 0; r < kMergeRounds; ++r) {
			const unsigned long long left = __ballot(pending);
			if (!left) break;
			const int first = __ffsll((long long)left) - 1;
			if (pending && key == readlane64(key, first)) {
				pending = false;
				mine = lane == first;
			}
		}
		if (mine || pending) claim_slot(t.keys, t.mask, t.reserve, t.count, key_slot(key, t.mask), key, [key](unsigned long long cur) { return cur == key; });
	}
	unsigned skip = p < n && !seeds ? 1u : 0u;
#pragma unroll
	for (int m = 1; m < 64; m *= 2) skip += (unsigned)__shfl_xor((int)skip, m);
	if (lane == 0 && skip) atomicAdd(&t.count[3], (unsigned long long)skip);
}

// One thread per slot. Leaves beyond `cap` (the refusal's case) are counted and not written.
__global__ __launch_bounds__(256) void k_seed_compact(const SeedTable t, int4* __restrict__ origins, const unsigned long long cap) {
	const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	const unsigned long long key = s <= t.mask ? t.keys[s] : kEmptySlot;
	const uint32_t l = wave_compact(key != kEmptySlot, &t.count[2]);
	if (key == kEmptySlot || l >= cap) return;
	origins[l] = key_origin(key);
	t.leaf[s] = (int)l;
}

__device__ __forceinline__ int find_key(const SeedTable& t, unsigned long long key) {
	for (uint32_t s = key_slot(key, t.mask);; s = (s + 1) & t.mask)
		if (t.keys[s] == key) return t.leaf[s];  // (every key asked for was inserted by k_seed_keys)
}

// masks: leaf x 8 words; word x holds the bytes y = 0 .. 7 of layer x, bit z of each. The two z-taps of a row share a byte, the two y-rows of a layer a word: a point has
// one word per (x-layer, leaf split along y, leaf split along z), eight at most and two when its cell lies inside one leaf. A leaf's mask is ONE 64-byte line, so the ORs
// of coherent points -- a wave inside one leaf -- would queue on that line: as for the keys, the lanes of a wave that hold the same word merge their bits first (kMergeRounds
// distinct words per slot, the rest on their own), and the lane that stands for a word issues one load and, where bits are missing, one OR.
__global__ __launch_bounds__(256) void k_seed_masks(const float* __restrict__ xyz, const unsigned n, const SeedTable t, unsigned long long* __restrict__ masks) {
	const unsigned p = blockIdx.x * 256u + threadIdx.x;
	const int lane = (int)(threadIdx.x & 63u);
	SeedCell C{};
	const bool seeds = p < n && seed_cell(xyz, p, C);
	// whole waves from here on: nothing above returns
	int L[8];
#pragma unroll
	for (int c = 0; c < 8; ++c) L[c] = seeds && C.has(c) ? find_key(t, C.key(c)) : -1;
	const unsigned y0 = (unsigned)C.j & 7u, z0 = (unsigned)C.k & 7u;
#pragma unroll
	for (int dx = 0; dx < 2; ++dx) {
		const unsigned x = ((unsigned)C.i + (unsigned)dx) & 7u;
		const int di = C.cx ? dx : 0;
#pragma unroll
		for (int sy = 0; sy < 2; ++sy) {
#pragma unroll
			for (int sz = 0; sz < 2; ++sz) {
				bool pending = seeds && (!sy || C.cy) && (!sz || C.cz);
				if (!__ballot(pending)) continue;
				const unsigned long long zb = C.cz ? (sz ? 0x01ull : 0x80ull) : 3ull << z0;                        // the z-taps in this leaf, as bits of a row's byte
				unsigned long long bits = C.cy ? zb << (sy ? 0 : 56) : (zb | zb << 8) << (8u * y0);  // the y-rows in this leaf
				const unsigned word = pending ? (unsigned)L[di * 4 + sy * 2 + sz] * 8u + x : ~0u;        // (fewer than 2^23 leaves)
				bool mine = false;
				for (int r = 0; r < kMergeRounds; ++r) {
					const unsigned long long left = __ballot(pending);
					if (!left) break;
					const int first = __ffsll((long long)left) - 1;
					const bool same = pending && word == (unsigned)__builtin_amdgcn_readlane((int)word, first);
					const unsigned long long all = wave_or64(bits, same);
					if (same) pending = false;
					if (lane == first) mine = true, bits = all;
				}
				if (mine || pending) {
					unsigned long long* w = masks + word;
					if ((load_fresh(w) & bits) != bits) (void)__hip_atomic_fetch_or(w, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				}
			}
		}
	}
}

}  // namespace

int seed_leaves(Scratch& scratch, const float* d_xyz, uint64_t n, hipStream_t st, const char* who, SeedSet* out) {
	*out = SeedSet{};
	if (n == 0) return HNS_OK;
	const uint64_t cap = std::min<uint64_t>(8 * n, kMaxSeedLeaves);
	const uint64_t T = hash_slots(2 * cap);
	SeedTable t{};
	t.mask = (uint32_t)(T - 1);
	// A thread holds at most one reservation it may still give back, and fewer than 2^22 threads are in flight: with 2^23 or fewer distinct leaves count[0] stays below
	// 2^23 + 2^22 < T, so the overflow flag rises only for a set that is refused anyway.
	t.reserve = std::min<uint64_t>(8 * n, kMaxSeedLeaves + kMaxSeedLeaves / 2);
	HNS_TRY(scratch.carve([&](auto&& slice) {
		slice(t.keys, 8 * T);
		slice(t.leaf, 4 * T);
		slice(out->origins, 16 * cap);
		slice(t.count, 256);
	}));
	HNS_HIP(hipMemsetAsync(t.keys, 0xFF, 8 * T, st));
	HNS_HIP(hipMemsetAsync(t.count, 0, 256, st));
	const unsigned blocks = (unsigned)((n + 255) / 256);
	k_seed_keys<<<blocks, 256, 0, st>>>(d_xyz, (unsigned)n, t);
	HNS_HIP(hipGetLastError());
	k_seed_compact<<<(unsigned)((T + 255) / 256), 256, 0, st>>>(t, out->origins, cap);
	HNS_HIP(hipGetLastError());
	unsigned long long counts[4] = {0, 0, 0, 0};
	HNS_HIP(hipMemcpyAsync(counts, t.count, sizeof(counts), hipMemcpyDeviceToHost, st));
	HNS_HIP(hipStreamSynchronize(st));
	if (counts[1] || counts[2] > kMaxSeedLeaves) {
		set_error("%s: the points hold more than 2^23 distinct leaves", who);
		return HNS_ERR_TOPOLOGY;
	}
	out->n_leaves = counts[2], out->skipped = counts[3];
	if (!out->n_leaves) return HNS_OK;
	HNS_TRY(scratch.carve([&](auto&& slice) { slice(out->masks, 64 * out->n_leaves); }));
	HNS_HIP(hipMemsetAsync(out->masks, 0, 64 * out->n_leaves, st));
	k_seed_masks<<<blocks, 256, 0, st>>>(d_xyz, (unsigned)n, t, (unsigned long long*)out->masks);
	HNS_HIP(hipGetLastError());
	return HNS_OK;
}

}  // namespace hns

using namespace hns;

extern "C" int hns_dev_point_leaves(int device, const float* d_xyz, uint64_t n, int32_t* origins_out, unsigned char* masks_out, uint64_t cap, uint64_t* n_leaves,
                                    uint64_t* skipped, void* stream) {
	const char* who = "hns_dev_point_leaves";
	if (!n_leaves) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dev_point_leaves: n_leaves is null");
	*n_leaves = 0;
	if (skipped) *skipped = 0;
	if (n > kMaxSeedPoints) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dev_point_leaves: n is above 2^31 - 1");
	if (n && !d_xyz) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dev_point_leaves: xyz is null");
	const int devices = hns_device_count();
	if (devices == 0) return fail(HNS_ERR_NO_DEVICE, "hns_dev_point_leaves: no HIP device (there is no CPU fallback)");
	if (device < 0 || device >= devices) {
		set_error("%s: device %d (there are %d)", who, device, devices);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	DeviceScope on(device);
	const hipStream_t st = (hipStream_t)stream;
	Scratch scratch(device);
	SeedSet S;
	HNS_TRY(seed_leaves(scratch, d_xyz, n, st, who, &S));
	*n_leaves = S.n_leaves;
	if (skipped) *skipped = S.skipped;
	if (!S.n_leaves || S.n_leaves > cap || !origins_out) {  // (the query of the two-call idiom, or nothing to write)
		HNS_HIP(hipStreamSynchronize(st));
		return HNS_OK;
	}
	std::vector<unsigned char> m(masks_out ? (size_t)S.n_leaves * 64 : 0);
	if (masks_out) HNS_HIP(hipMemcpyAsync(m.data(), S.masks, 64 * S.n_leaves, hipMemcpyDeviceToHost, st));
	std::vector<int32_t> xyz;
	HNS_TRY(download_origins(S.origins, (size_t)S.n_leaves, st, &xyz));
	std::vector<uint32_t> perm;
	leaf_order(xyz.data(), (size_t)S.n_leaves, &perm);
	for (uint64_t r = 0; r < S.n_leaves; ++r) {
		memcpy(origins_out + 3 * r, xyz.data() + 3 * (size_t)perm[r], 12);
		if (masks_out) memcpy(masks_out + 64 * r, m.data() + 64 * (size_t)perm[r], 64);
	}
	return HNS_OK;
}
