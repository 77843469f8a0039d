// hns_dilate.hpp -- dilateVoxels(p, NN_FACE_EDGE_VERTEX) of leaf masks (SOP_HNanoSolver.cpp:190-193), one pair of leaves at a time. Shared by the
// host function hns_dilate_leaf_masks (hns_leafio.cpp) and the device regrid (hns_regrid.hip), so that both compute the same bits the same way.
//
// p iterations of 26-neighbour dilation = the Chebyshev ball of radius p = a box, so it separates into three 1-D dilations (z, then y, then x). A mask is
// eight 64-bit words: word x holds bytes y = 0..7 (byte x*8+y of the hns_leafio layout, little endian), bit z of each byte.
#pragma once

#include "hns_internal.hpp"

namespace hns {

// bits [lo, hi] of a byte (clamped to 0..7), 0 when empty
HNS_HD uint32_t dil_bits(int lo, int hi) {
	lo = lo < 0 ? 0 : lo;
	hi = hi > 7 ? 7 : hi;
	return lo > hi ? 0u : (0xFFu >> (7 - hi)) & (0xFFu << lo);
}
// 0x01 in bytes [lo, hi] of a word (clamped to 0..7), 0 when empty
HNS_HD uint64_t dil_bytes(int lo, int hi) {
	lo = lo < 0 ? 0 : lo;
	hi = hi > 7 ? 7 : hi;
	return lo > hi ? 0ull : (~0ull >> (8 * (7 - hi))) & (~0ull << (8 * lo)) & 0x0101010101010101ull;
}

// ORs into `out` the active voxels of mask `m`, dilated by p and cropped to a leaf whose origin is (ox, oy, oz) voxels BELOW m's leaf (off = m's origin
// minus the receiving leaf's origin, a multiple of 8 per axis): receiving voxel v gets a bit iff some active u of m has |off + u - v| <= p on every axis.
// Returns whether anything was contributed, i.e. whether an active voxel of m lies within p of the receiving leaf's box (the test hns_dilate_leaves does).
HNS_HD bool dilate_into(const uint64_t (&m)[8], int ox, int oy, int oz, int p, uint64_t (&out)[8]) {
	const uint64_t ones = 0x0101010101010101ull;
	if (ox - p > 7 || ox + 7 + p < 0 || oy - p > 7 || oy + 7 + p < 0 || oz - p > 7 || oz + 7 + p < 0) return false;  // out of reach on some axis
	uint64_t a[8];
#pragma unroll
	for (int x = 0; x < 8; ++x) a[x] = 0;
#pragma unroll
	for (int u = 0; u < 8; ++u) {  // z: bit u of every byte lights bits [oz + u - p, oz + u + p]
		const uint64_t span = (uint64_t)dil_bits(oz + u - p, oz + u + p) * ones;
#pragma unroll
		for (int x = 0; x < 8; ++x) a[x] |= (((m[x] >> u) & ones) * 0xFFu) & span;
	}
	uint64_t b[8];
#pragma unroll
	for (int x = 0; x < 8; ++x) b[x] = 0;
#pragma unroll
	for (int u = 0; u < 8; ++u) {  // y: byte u lands in bytes [oy + u - p, oy + u + p]
		const uint64_t spread = dil_bytes(oy + u - p, oy + u + p);
#pragma unroll
		for (int x = 0; x < 8; ++x) b[x] |= ((a[x] >> (8 * u)) & 0xFFu) * spread;
	}
	uint64_t any = 0;
#pragma unroll
	for (int v = 0; v < 8; ++v) {  // x: word u lands in words [ox + u - p, ox + u + p]
		uint64_t w = 0;
#pragma unroll
		for (int u = 0; u < 8; ++u) w |= (ox + u - p <= v && v <= ox + u + p) ? b[u] : 0ull;
		out[v] |= w;
		any |= w;
	}
	return any != 0;
}

}  // namespace hns
