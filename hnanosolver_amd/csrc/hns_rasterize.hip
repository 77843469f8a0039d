// hns_rasterize.hip -- points rasterised into fields with a radius: the radial kernel of hns_dev_splat_points / hns_sim_splat_points (include/hns.h: hns_splat_spec states
// the footprint). The arithmetic is hns_points.hpp's, the accumulator, the finish kernel and the launcher are hns_splat.hip's; this file holds the one kernel in which a
// GROUP of lanes shares a point, so that the adds of one wave instruction go to contiguous accumulator addresses.
#include "hns_points.hpp"

namespace hns {
namespace {

constexpr int kMaskMergeRounds = 8;  // distinct mask words a wave merges per x-slab before its lanes OR on their own (as k_seed_masks, hns_seed.hip)

__device__ __forceinline__ unsigned wave_or32(unsigned bits, bool take) {
	unsigned x = take ? bits : 0u;
#pragma unroll
	for (int w = 32; w >= 1; w >>= 1) x |= (unsigned)__shfl_xor((int)x, w);
	return x;
}

// G lanes per point (G = EB^2, EB the power of two at or above ceil(2 * the spec's radius)): lane t of a group is column (y, z) = (t / EB, t % EB) of the point's box, z
// fastest, and the group walks the box along x. So the lanes of one row hold a z-run: adjacent voxels of one leaf row (x<<6 | y<<3 | z), accumulator pieces 8 S bytes apart.
// The up to eight leaves under the box are looked up once per point -- lane c of the group takes leaf c (with fewer than eight lanes: c, c + G, ..) -- and handed round by
// shuffles; a column needs two of them, one per leaf along x. Adds, touched words, rejections: as k_splat_points. Mask bits of lanes that share a 32-bit word are merged
// before one lane ORs them. status (radial): 2 the whole non-empty footprint landed, 1 a part of it, 0 nothing. Nothing returns early: shuffles and ballots see whole waves.
template <int G>
__global__ __launch_bounds__(kSplatBlock) void k_splat_radial(const GridDev g, const SplatChannels ch, const float* __restrict__ xyz, const float* __restrict__ radii,
                                                               const float bound, const unsigned n, const double scale, unsigned long long* __restrict__ acc, const int S,
                                                               int* __restrict__ touched, unsigned* __restrict__ masks, unsigned char* __restrict__ status,
                                                               unsigned long long* __restrict__ rejected) {
	constexpr int EB = G == 1 ? 1 : G == 4 ? 2 : G == 16 ? 4 : 8;
	static_assert(EB * EB == G, "G is 1, 4, 16 or 64");
	const unsigned p = blockIdx.x * (unsigned)(kSplatBlock / G) + threadIdx.x / (unsigned)G;
	const int lane = (int)(threadIdx.x & 63u), t = (int)(threadIdx.x % (unsigned)G), ly = t / EB, lz = t % EB;
	f3 pos = {0.0f, 0.0f, 0.0f};
	float r = 0.0f;
	bool ok = false;
	if (p < n) {
		pos = ld3(xyz, (int)p);
		r = radii ? radii[p] : bound;
		ok = radial_point(pos.x, pos.y, pos.z, r, bound);
	}
	const int E = ok ? radial_extent(r) : 0;
	const int i0 = ok ? radial_lo(pos.x, r) : 0, j0 = ok ? radial_lo(pos.y, r) : 0, k0 = ok ? radial_lo(pos.z, r) : 0;
	const float inv = radial_inv(r);
	const int ox = i0 & ~7, oy = j0 & ~7, oz = k0 & ~7;
	const bool cx = ((i0 + E - 1) & ~7) != ox, cy = ((j0 + E - 1) & ~7) != oy, cz = ((k0 + E - 1) & ~7) != oz;  // the box reaches into the next leaf (E <= 8: at most one)

	// the leaves under the box, leaf c = di*4 + dj*2 + dk: one lookup per leaf and point
	constexpr int NL = G >= 8 ? 1 : 8 / G;
	int mine[NL];
#pragma unroll
	for (int a = 0; a < NL; ++a) {
		const int c = t + a * G;
		const bool need = ok && c < 8 && (!(c & 4) || cx) && (!(c & 2) || cy) && (!(c & 1) || cz);
		mine[a] = need ? d_find_leaf(g, (c & 4) ? plus8(ox) : ox, (c & 2) ? plus8(oy) : oy, (c & 1) ? plus8(oz) : oz) : -1;
	}
	const int j = j0 + ly, k = k0 + lz;
	const int c0 = ((j & ~7) != oy ? 2 : 0) | ((k & ~7) != oz ? 1 : 0), c1 = c0 | 4;  // this column's leaf below and above the leaf face along x
	int L0 = -1, L1 = -1;
#pragma unroll
	for (int a = 0; a < NL; ++a) {
		const int base = lane & ~(G - 1);
		const int v0 = G == 1 ? mine[a] : __shfl(mine[a], base + c0 % G), v1 = G == 1 ? mine[a] : __shfl(mine[a], base + c1 % G);
		if (a == c0 / G) L0 = v0;
		if (a == c1 / G) L1 = v1;
	}

	float v[kSplatChannels];
#pragma unroll
	for (int q = 0; q < kSplatChannels; ++q)
		v[q] = ok && q < ch.n ? (ch.c[q].val ? ch.c[q].val[(size_t)p * (unsigned)ch.c[q].stride + (unsigned)ch.c[q].off] : 1.0f) : 0.0f;
	const bool column = ok && ly < E && lz < E;
	int in_footprint = 0, landed = 0;
	unsigned rej = 0;
#pragma unroll
	for (int dx = 0; dx < EB; ++dx) {
		const bool act = column && dx < E;
		if (!__ballot(act)) break;  // (the same answer in every lane)
		const int i = i0 + dx;
		float w = 0.0f;
		const bool in = act && radial_weight((float)i - pos.x, (float)j - pos.y, (float)k - pos.z, inv, &w);
		const int leaf = (i & ~7) != ox ? L1 : L0;
		const bool land = in && leaf >= 0;
		in_footprint += in, landed += land;
		const unsigned vox = (unsigned)leaf * 512u + (((unsigned)i & 7u) << 6 | ((unsigned)j & 7u) << 3 | ((unsigned)k & 7u));  // (used where land)
		if (land) {
			touched[leaf] = 1;
#pragma unroll
			for (int q = 0; q < kSplatChannels; ++q) {
				if (q >= ch.n) break;
				long long term;
				if (!splat_term(w * v[q], scale, &term))
					++rej;
				else if (term)
					atomicAdd(acc + (size_t)vox * (unsigned)S + (unsigned)q, (unsigned long long)term);
			}
		}
		if (masks) {  // (the same answer in every lane)
			bool pending = land && w > 0.0f, issue = false;
			unsigned bits = 1u << (vox & 31u);
			const unsigned word = pending ? vox >> 5 : ~0u;
			for (int round = 0; round < (G == 1 ? 0 : kMaskMergeRounds); ++round) {  // (one point a lane: its one voxel has a word of its own but for coincidences)
				const unsigned long long left = __ballot(pending);
				if (!left) break;
				const int first = __ffsll((long long)left) - 1;
				const bool same = pending && word == (unsigned)__builtin_amdgcn_readlane((int)word, first);
				const unsigned all = wave_or32(bits, same);
				if (same) pending = false;
				if (lane == first) issue = true, bits = all;
			}
			if (issue || pending) atomicOr(masks + word, bits);
		}
	}
#pragma unroll
	for (int m = 1; m < G; m *= 2) in_footprint += __shfl_xor(in_footprint, m), landed += __shfl_xor(landed, m);
	if (status && p < n && t == 0) status[p] = (unsigned char)(in_footprint > 0 && landed == in_footprint ? 2 : landed > 0 ? 1 : 0);
	if (rejected) {  // one add per wave that has something to report
#pragma unroll
		for (int m = 1; m < 64; m *= 2) rej += (unsigned)__shfl_xor((int)rej, m);
		if (lane == 0 && rej) atomicAdd(rejected, (unsigned long long)rej);
	}
}

template <int G>
void launch(hipStream_t st, const GridDev& g, const SplatChannels& ch, const float* xyz, const float* radii, float bound, unsigned n, double scale, unsigned long long* acc,
            int S, int* touched, unsigned* masks, unsigned char* status, unsigned long long* rejected) {
	const unsigned per_block = (unsigned)(kSplatBlock / G);
	hipLaunchKernelGGL(k_splat_radial<G>, dim3((n + per_block - 1u) / per_block), dim3(kSplatBlock), 0, st, g, ch, xyz, radii, bound, n, scale, acc, S, touched, masks, status,
	                   rejected);
}

}  // namespace

int splat_radial_group(float radius) {
	const int e = radial_extent(radius);
	const int eb = e <= 1 ? 1 : e <= 2 ? 2 : e <= 4 ? 4 : 8;
	return eb * eb;
}

void launch_splat_radial(hipStream_t st, const GridDev& g, const SplatChannels& ch, const float* xyz, const float* radii, float bound, unsigned n, double scale,
                         unsigned long long* acc, int S, int* touched, unsigned* masks, unsigned char* status, unsigned long long* rejected) {
	switch (splat_radial_group(bound)) {
	case 1: launch<1>(st, g, ch, xyz, radii, bound, n, scale, acc, S, touched, masks, status, rejected); break;
	case 4: launch<4>(st, g, ch, xyz, radii, bound, n, scale, acc, S, touched, masks, status, rejected); break;
	case 16: launch<16>(st, g, ch, xyz, radii, bound, n, scale, acc, S, touched, masks, status, rejected); break;
	default: launch<64>(st, g, ch, xyz, radii, bound, n, scale, acc, S, touched, masks, status, rejected); break;
	}
}

}  // namespace hns
