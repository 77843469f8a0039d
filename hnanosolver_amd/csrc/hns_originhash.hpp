// hns_originhash.hpp -- the origin hash ("The origin hash"): every sparse lookup of the library, stated once. A table of a power of two of slots, at least
// twice the entries it may hold, is probed linearly from hash_origin(origin) & mask; entries are never removed, so a probe ends at the entry or at an empty slot. Two kinds:
//   an INDEX table (int slots, -1 = empty) holds positions in an int4 origin list: a grid's leaves, a source's leaves, a seed set's leaves. find_origin, insert_origin
//   a CLAIM table (64-bit slots, all ones = empty) holds whatever identifies an entry to its owner, for a set whose size is not known beforehand: the regrid's candidates (a
//   thread id), a point set's leaves (a 63-bit key). claim_slot, wave_compact
// Topology::find_leaf / build_tables (hns_topology.cpp) state the index probe once more on the host, on purpose: they are the independent builder the device tables are held to.
#pragma once

#include "hns_internal.hpp"

namespace hns {

// leaf coordinates (origin >> 3) mixed with three odd 32-bit constants
HNS_HD uint32_t hash_origin(int32_t x, int32_t y, int32_t z) {
	uint32_t h = (uint32_t)(x >> 3) * 0x9E3779B1u;
	h ^= (uint32_t)(y >> 3) * 0x85EBCA77u;
	h ^= (uint32_t)(z >> 3) * 0xC2B2AE3Du;
	h ^= h >> 15;
	h *= 0x2C1B3C6Du;
	h ^= h >> 12;
	return h;
}

// slots of a table: the smallest power of two >= max(16, at_least). Callers ask for twice what the table may hold (a grid: 2n + 2), so a probe always meets an empty slot.
HNS_HD uint64_t hash_slots(uint64_t at_least) {
	uint64_t T = 16;
	while (T < at_least) T <<= 1;
	return T;
}

#ifdef __HIPCC__

struct OriginIndex {
	const int4* origins;
	const int* table;  // null: no such set (whoever may hold none tests it before asking)
	uint32_t mask;
};

// the entry with origin (x, y, z), -1 = none
__device__ __forceinline__ int find_origin(const OriginIndex& ix, int x, int y, int z) {
	uint32_t s = hash_origin(x, y, z) & ix.mask;
	for (;;) {
		const int l = ix.table[s];
		if (l < 0) return -1;
		const int4 o = ix.origins[l];
		if (o.x == x && o.y == y && o.z == z) return l;
		s = (s + 1) & ix.mask;
	}
}

// Entry i of `origins` into its index table. -1: slot taken; else the entry already present with the same origin (which of two equal entries meets the other depends on the
// race: report something symmetric). Read before you swap: the compare-and-swap is issued only on a slot seen empty, and an occupied slot can be compared safely.
__device__ __forceinline__ int insert_origin(const int4* __restrict__ origins, int* __restrict__ table, uint32_t mask, int i) {
	const int4 o = origins[i];
	uint32_t s = hash_origin(o.x, o.y, o.z) & mask;
	for (;;) {
		int cur = table[s];
		if (cur < 0) {
			cur = atomicCAS(&table[s], -1, i);
			if (cur < 0) return -1;
		}
		const int4 q = origins[cur];
		if (q.x == o.x && q.y == o.y && q.z == o.z) return cur;
		s = (s + 1) & mask;
	}
}

constexpr unsigned long long kEmptySlot = ~0ull;

// a load that another CU's atomic is visible to (the per-CU cache is passed by): what "read before you swap / OR" reads
__device__ __forceinline__ unsigned long long load_fresh(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Puts `value` into a claim table unless an entry that stands for the same thing (same(occupant)) is there. count (zeroed with the table): [0] slots reserved, [1] the overflow
// flag, [2] entries compacted (wave_compact's counter). A thread reserves a slot in count[0] before its first swap and refuses, raising count[1], once `cap` are reserved: with
// cap below the table size a probe always meets an empty slot. A thread that then finds its entry present gives the reservation back, so count[0] never exceeds the occupied
// slots plus one per thread in flight, and the flag can rise only when the distinct entries and the threads in flight together exceed cap. Entries never leave the table: one
// that was seen is present, and a stale load can only cost a swap that was not needed.
template <class Same>
__device__ __forceinline__ void claim_slot(unsigned long long* table, uint32_t mask, unsigned long long cap, unsigned long long* count, uint32_t home_slot,
                                           unsigned long long value, Same same) {
	bool reserved = false;
	for (uint32_t s = home_slot;; s = (s + 1) & mask) {
		unsigned long long cur = load_fresh(table + s);
		if (cur == kEmptySlot) {
			if (!reserved) {
				if (atomicAdd(&count[0], 1ull) >= cap) {
					count[1] = 1;
					return;
				}
				reserved = true;
			}
			cur = atomicCAS(table + s, kEmptySlot, value);
			if (cur == kEmptySlot) return;
		}
		if (same(cur)) {
			if (reserved) atomicAdd(&count[0], ~0ull);
			return;
		}
	}
}

// One thread per slot, whole waves: the index of an occupied slot's entry among all occupied ones, in no particular order (whoever sorts discards it). One atomic per wave.
// (a table has fewer than 2^32 slots)
__device__ __forceinline__ uint32_t wave_compact(bool occupied, unsigned long long* counter) {
	const unsigned long long full = __ballot(occupied);
	if (!full) return 0;
	const int lane = (int)(threadIdx.x & 63u);
	uint32_t base = 0;
	if (lane == 0) base = (uint32_t)atomicAdd(counter, (unsigned long long)__popcll(full));
	return (uint32_t)__builtin_amdgcn_readfirstlane((int)base) + (uint32_t)__popcll(full & ((1ull << lane) - 1ull));
}

#endif  // __HIPCC__

}  // namespace hns
