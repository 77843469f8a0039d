// hns_blockscan.hpp -- the exclusive prefix sum over a workgroup of 256 threads, stated once for the kernel files that scan: hns_pointorder.hip (digit rows of the radix
// sort, a tile's digit runs) and hns_population.hip (the tile table of a select or a birth, a tile's births).
#pragma once

#include "hns_internal.hpp"

namespace hns {

constexpr int kBlockScanThreads = 256;                  // the workgroup block_scan is written for: four waves
constexpr int kBlockScanWaves = kBlockScanThreads / 64;

// exclusive prefix of v over the workgroup's 256 threads and, in every thread, the sum; s_wave: kBlockScanWaves words nobody else uses between the call's two barriers
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* s_wave, unsigned& sum) {
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	unsigned incl = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned up = (unsigned)__shfl_up((int)incl, d);
		if (lane >= d) incl += up;
	}
	__syncthreads();  // (the previous call's reads of s_wave are over)
	if (lane == 63) s_wave[w] = incl;
	__syncthreads();
	unsigned before = 0;
	sum = 0;
#pragma unroll
	for (int k = 0; k < kBlockScanWaves; ++k) {
		const unsigned c = s_wave[k];
		before += k < w ? c : 0u;
		sum += c;
	}
	return before + incl - v;
}

}  // namespace hns
