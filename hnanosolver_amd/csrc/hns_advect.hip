// hns_advect.hip -- BFECC semi-Lagrangian advection kernels (reference src/Cuda/Kernel.cu:118-453).
//
// One 8^3 leaf per 512-thread workgroup, one voxel per thread (coordinate = leaf origin + thread id: no 12 B/voxel
// coordinate stream). The reference walks the NanoVDB tree for each of its 23-31 taps per voxel; here a tap is
//     slot = 9*dx + 3*dy + dz (leaf offset of the tap relative to the workgroup's leaf, each in {0,1,2})
//     index = s_base[slot] + local offset          (s_base = the 27 neighbour leaves' base indices, staged in LDS)
// computed once per axis for the two planes of a trilinear stencil and combined for its 8 corners, branch-free. Taps
// farther than one leaf away (|u| dt/dx > 8) take a generic path -- the neighbour's own neighbour table up to two leaves away, the origin hash beyond; wave-divergent but rare.
// The arithmetic (Floor, lerp order z->y->x, fused Vec3f lerps, unfused float lerps, weight-product form of
// advect_scalars, clamp set and order) is the reference's, so results stay bit-identical to the oracle.
#include <cstdlib>
#include <cstring>

#include "hns_device.hpp"

namespace hns {

struct Taps {
	int t[8];  // flat voxel index of corner (di,dj,dk) at t[di*4+dj*2+dk], -1 = outside the domain
	float fx, fy, fz;
};

// ---- 32-bit addressed field access ---------------------------------------------------------------------------------
// The advection kernels issue ~590 vector ALU instructions per voxel against 23 loads and are bound by VALU issue, not by
// memory; a large share of those instructions only guards and addresses the taps: a 64-bit multiply-add per address,
// an index clamp and three "value or 0" selects per out-of-domain-capable tap (IndexSampler<T,0>, Stencils.hpp:83,88).
// While a field is below 4 GiB all of that is a property of the load instead: a buffer descriptor over the whole field
// takes a 32-bit byte offset, and the hardware returns 0 for offsets past the end. Taps are therefore carried as the
// byte offset of the voxel in a float field (voxel * 4; a Vec3f tap is at three times that), and a tap outside the
// domain is any offset >= kOutside: absent neighbour leaves get kOutside as their base, so no select is needed at all.
// (descriptor and loads: hns_device.hpp, "raw buffer access")
constexpr unsigned kOutside = 0xFFFFE000u;        // float-field byte offsets at or above this read as 0 (and 3x it still lies past a Vec3f field)
constexpr uint64_t kNarrowBytes = 0xFFFF0000ull;  // largest Vec3f field the 32-bit path accepts (and largest 16-byte-per-voxel field of the q4 path)

__device__ __forceinline__ f3 ldv(const v4i& r, unsigned o4) {  // Vec3f of the voxel at float-offset o4; 0 outside
	const v3f v = hns_buffer_load_v3f32(r, (int)(o4 + (o4 << 1)), 0, 0);
	return f3{v.x, v.y, v.z};
}
__device__ __forceinline__ float lds1(const v4i& r, unsigned o4) { return hns_buffer_load_f32(r, (int)o4, 0, 0); }

// The two z-corners of a trilinear column, float field: when they are neighbours in memory (same leaf, k & 7 != 7) one
// 8-byte load fetches both; otherwise the second comes from its own load, which only the few lanes whose column
// straddles a leaf face execute. A load instruction costs the L1 the same 16 cycles per wave whatever its width, and
// the scalar gathers are what bounds advect_scalars, so halving them is the point. Reading 4 bytes past `lo` is safe:
// the descriptor's bounds check covers the end of the field.
__device__ __forceinline__ void ld_zpair(const v4i& r, unsigned lo, unsigned hi, float& a, float& b) {
	const v2f32 v = hns_buffer_load_v2f32(r, (int)lo, 0, 0);
	a = v.x;
	b = v.y;
	if (hi != lo + 4u) b = lds1(r, hi);
}

// The workgroup's leaf tables in LDS: nbr27 (for the far path) and, in the generic kernels, the neighbours' base indices leaf*512 (-1 = absent) ...
struct GenericTabs {
	int nbr[27], base[27];
	__device__ __forceinline__ void set(int t, int nb) { nbr[t] = nb, base[t] = nb < 0 ? -1 : nb * 512; }
};
// ... in the 32-bit kernels their base byte offsets in a float field (kOutside = absent), twice:
// b4p holds the same byte bases again in a table padded to 4 x 4 x 4, entry (ax*4 + ay)*4 + az for the neighbour leaf
// (ax, ay, az) in 0..2 -- its byte index ax<<6 | ay<<4 | az<<2 is shifts and ORs of the tap's coordinates, where 9*ax + 3*ay + az cost
// four quarter-rate multiplies per trilinear sample (make_taps_b).
constexpr int kPadTab = 48;
struct NarrowTabs {
	int nbr[27];
	unsigned b4[27], b4p[kPadTab];
	__device__ __forceinline__ void set(int t, int nb) {
		const int ax = t / 9, ay = (t - 9 * ax) / 3, az = t - 9 * ax - 3 * ay;
		nbr[t] = nb, b4[t] = b4p[(ax * 4 + ay) * 4 + az] = nb < 0 ? kOutside : (unsigned)nb * 2048u;
	}
};

// position of voxel n of the leaf at `org`
__device__ __forceinline__ int3 voxel_ijk(const int4 org, int n) { return int3{org.x + (n >> 6), org.y + ((n >> 3) & 7), org.z + (n & 7)}; }

// What a thread knows about its leaf and its voxel (thread n of the leaf's workgroup). The constructor sets what the voxel's own values need: their loads can be issued
// before stage() fetches and stages the tables (k_advect_vector_n, which see).
template <class Tabs>
struct LeafVoxel {
	Tabs& tabs;
	const int n, leaf, idx;
	int4 org;
	int3 c;            // the voxel's coordinate
	float px, py, pz;  // and as floats
	__device__ __forceinline__ LeafVoxel(const GridDev& g, Tabs& t) : tabs(t), n(threadIdx.x), leaf(launch_leaf(g, blockIdx.x)), idx(leaf * 512 + n) {}
	__device__ __forceinline__ void stage(const GridDev& g) {
		org = g.origins[leaf];
		if (threadIdx.x < 27) tabs.set(threadIdx.x, g.nbr27[leaf * 27 + threadIdx.x]);
		__syncthreads();
		c = voxel_ijk(org, n);
		px = (float)c.x, py = (float)c.y, pz = (float)c.z;
	}
};
typedef LeafVoxel<GenericTabs> GenericCtx;
typedef LeafVoxel<NarrowTabs> NarrowCtx;

// ---- the pieces every sampler is made of ------------------------------------------------------------------------------------
// corner q of setupInterpolation's order 000,100,010,110,001,... of (x,y,z) (Kernel.cu:163-196) is tap tap_of(q) of the order (di,dj,dk) at t[di*4+dj*2+dk], and back
__device__ __forceinline__ constexpr int tap_of(int q) { return ((q & 1) << 2) | (q & 2) | (q >> 2); }
// its offset in a box with rows YS and slices XS apart
template <int XS = 100, int YS = 10>
__device__ __forceinline__ constexpr int box_corner(int q) { return (q & 1) * XS + ((q >> 1) & 1) * YS + (q >> 2); }
// the eight weight products of setupInterpolation (Kernel.cu:163-196), in its order
__device__ __forceinline__ void tri_weights(float tx, float ty, float tz, float (&w)[8]) {
	const float itx = 1.0f - tx, ity = 1.0f - ty, itz = 1.0f - tz;
	const float w00 = itx * ity, w10 = tx * ity, w01 = itx * ty, w11 = tx * ty;
	w[0] = w00 * itz, w[1] = w10 * itz, w[2] = w01 * itz, w[3] = w11 * itz, w[4] = w00 * tz, w[5] = w10 * tz, w[6] = w01 * tz, w[7] = w11 * tz;
}
// (tri_nest / tri_nest_yx, TrilinearSampler's nest over eight corners with one of the three lerps: hns_device.hpp)
// BFECC's limiter (Kernel.cu:219-233, 334-352, 396-431 per component): the corrected value clamped to the range of the voxel, its six face neighbours and the first sample.
// float or v4f32. The caller forms phiCorr: advect_scalar's is unfused, advect_scalars' is fmaf(0.5, error, phiForward), as in the reference.
template <class T>
__device__ __forceinline__ T bfecc_limit(T phiOrig, const T (&nbr)[6], T phiForward, T phiCorr) {
	T mn = phiOrig, mx = phiOrig;
#pragma unroll
	for (int d = 0; d < 6; ++d) {
		mn = __builtin_elementwise_min(mn, nbr[d]);
		mx = __builtin_elementwise_max(mx, nbr[d]);
	}
	mn = __builtin_elementwise_min(mn, phiForward);
	mx = __builtin_elementwise_max(mx, phiForward);
	return __builtin_elementwise_max(mn, __builtin_elementwise_min(phiCorr, mx));
}
// advect_vector's (Kernel.cu:396-431): correction, then the limiter per component. nbr(d): the velocity at face neighbour d in the order -x,+x,-y,+y,-z,+z, 0 outside the domain
template <class Fetch>
__device__ __forceinline__ f3 bfecc_limit_v(const f3& vo, const f3& vf, const f3& vb, Fetch nbr) {
	float nx[6], ny[6], nz[6];
#pragma unroll
	for (int d = 0; d < 6; ++d) {
		const f3 t = nbr(d);
		nx[d] = t.x, ny[d] = t.y, nz[d] = t.z;
	}
	return f3{bfecc_limit(vo.x, nx, vf.x, vf.x + 0.5f * (vo.x - vb.x)), bfecc_limit(vo.y, ny, vf.y, vf.y + 0.5f * (vo.y - vb.y)),
	          bfecc_limit(vo.z, nz, vf.z, vf.z + 0.5f * (vo.z - vb.z))};
}

struct TapsB {
	unsigned o[8];  // float-field byte offset of corner (di,dj,dk) at o[di*4+dj*2+dk]; >= kOutside: outside the domain
	float fx, fy, fz;
};

// Floor (Stencils.hpp:25-43) + the eight corner indices of TrilinearSampler::stencil (Stencils.hpp:104-114)
__device__ __forceinline__ Taps make_taps(const GridDev& g, const GenericCtx& C, float x, float y, float z) {
	Taps T;
	const int4 org = C.org;
	const int i = __float2int_rd(x), j = __float2int_rd(y), k = __float2int_rd(z);
	T.fx = x - (float)i;
	T.fy = y - (float)j;
	T.fz = z - (float)k;
	// leaf offsets (+1) of the two planes per axis; near <=> all in {0,1,2}
	const int ax0 = (i >> 3) - (org.x >> 3) + 1, ax1 = ((i + 1) >> 3) - (org.x >> 3) + 1;
	const int ay0 = (j >> 3) - (org.y >> 3) + 1, ay1 = ((j + 1) >> 3) - (org.y >> 3) + 1;
	const int az0 = (k >> 3) - (org.z >> 3) + 1, az1 = ((k + 1) >> 3) - (org.z >> 3) + 1;
	const bool near = ((unsigned)ax0 <= 2u) & ((unsigned)ax1 <= 2u) & ((unsigned)ay0 <= 2u) & ((unsigned)ay1 <= 2u) & ((unsigned)az0 <= 2u) &
	                  ((unsigned)az1 <= 2u);
	if (near) {
		const int sx[2] = {ax0 * 9, ax1 * 9}, sy[2] = {ay0 * 3, ay1 * 3}, sz[2] = {az0, az1};
		const int lx[2] = {(i & 7) << 6, ((i + 1) & 7) << 6}, ly[2] = {(j & 7) << 3, ((j + 1) & 7) << 3}, lz[2] = {k & 7, (k + 1) & 7};
#pragma unroll
		for (int c = 0; c < 8; ++c) {
			const int di = c >> 2, dj = (c >> 1) & 1, dk = c & 1;
			const int b = C.tabs.base[sx[di] + sy[dj] + sz[dk]];
			T.t[c] = b < 0 ? -1 : b + (lx[di] | ly[dj] | lz[dk]);
		}
	} else {
		int any = 0;
		far_cell_taps(g, C.tabs.nbr, org, i, j, k, T.t);
#pragma unroll
		for (int c = 0; c < 8; ++c) any |= T.t[c];
		// a multi-GPU rank: a tap beyond the 27-leaf neighbourhood whose leaf is not HERE may exist on another rank (hns_dist reports
		// it); one that resolves to a local leaf -- owned or ghost, both hold current values -- is answered as the single domain answers it
		if (any < 0 && g.far_flag) *g.far_flag = 1;
	}
	return T;
}

// the same for the 32-bit path: byte offsets, and an absent leaf needs no test (its base is kOutside).
// Round 4: the kernels that call this keep the VALU 86 % busy (4 cycles per wave instruction; SQ_ACTIVE_INST_VALU) next to a texture
// addresser at 84 %, and a good half of their instructions address taps. So: d = cell - (corner of the 3 x 3 x 3 leaves around the
// workgroup's leaf) per axis, "near" <=> every d in [0, 22] (cell and cell + 1 inside the 24 voxels: ONE max3 and ONE compare instead of
// six range tests), neighbour slot and voxel-in-leaf are bit fields of d, the table is padded so that its index is ORs (s_b4p), and
// the eight offsets are add3's of three precombined terms.
__device__ __forceinline__ TapsB make_taps_b(const GridDev& g, const NarrowCtx& C, float x, float y, float z) {
	TapsB T;
	const int4 org = C.org;
	const int i = __float2int_rd(x), j = __float2int_rd(y), k = __float2int_rd(z);
	T.fx = x - (float)i;
	T.fy = y - (float)j;
	T.fz = z - (float)k;
	const unsigned dx = (unsigned)(i - (org.x - 8)), dy = (unsigned)(j - (org.y - 8)), dz = (unsigned)(k - (org.z - 8));
	if (max(dx, max(dy, dz)) < 23u) {
		const unsigned ex = dx + 1u, ey = dy + 1u, ez = dz + 1u;
		// table byte index (d >> 3) << {6, 4, 2} and voxel-in-leaf byte offset (d & 7) << {8, 5, 2}, for the cell (0) and cell + 1 (1)
		const unsigned X[2] = {(dx & 24u) << 3, (ex & 24u) << 3}, Y[2] = {(dy & 24u) << 1, (ey & 24u) << 1}, Z[2] = {(dz & 24u) >> 1, (ez & 24u) >> 1};
		const unsigned lx[2] = {(dx & 7u) << 8, (ex & 7u) << 8}, ly[2] = {(dy & 7u) << 5, (ey & 7u) << 5}, lz[2] = {(dz & 7u) << 2, (ez & 7u) << 2};
		const unsigned XY[4] = {X[0] | Y[0], X[0] | Y[1], X[1] | Y[0], X[1] | Y[1]};
		const unsigned lxy[4] = {lx[0] | ly[0], lx[0] | ly[1], lx[1] | ly[0], lx[1] | ly[1]};
		const char* tab = reinterpret_cast<const char*>(C.tabs.b4p);
#pragma unroll
		for (int c = 0; c < 8; ++c) {
			const int dij = c >> 1, dk = c & 1;
			T.o[c] = *reinterpret_cast<const unsigned*>(tab + (XY[dij] | Z[dk])) + lxy[dij] + lz[dk];
		}
	} else {
		int any = 0, ft[8];
		far_cell_taps(g, C.tabs.nbr, org, i, j, k, ft);  // (round 6: through the neighbour tables up to two leaves away, the hash beyond)
#pragma unroll
		for (int c = 0; c < 8; ++c) {
			any |= ft[c];
			T.o[c] = ft[c] < 0 ? kOutside : (unsigned)ft[c] << 2;
		}
		if (any < 0 && g.far_flag) *g.far_flag = 1;  // a multi-GPU rank: a far tap whose leaf is not here may exist on another rank (see make_taps)
	}
	return T;
}

// value or 0 outside the domain (IndexSampler<T,0>, Stencils.hpp:81-89), without a branch
__device__ __forceinline__ float ldz(const float* __restrict__ f, int idx) {
	const float v = f[idx < 0 ? 0 : idx];
	return idx < 0 ? 0.0f : v;
}

// IndexSampler<float,1> (Stencils.hpp:140-152)
__device__ __forceinline__ float tri_f_t(const float* __restrict__ f, const Taps& T) {
	float c[8];
#pragma unroll
	for (int q = 0; q < 8; ++q) c[q] = ldz(f, T.t[q]);
	return tri_nest(c, T.fx, T.fy, T.fz, lerp_f);
}

// IndexSampler<Vec3f,1> on the device branch, per component (Stencils.hpp:131-135); eight 12-byte taps
__device__ __forceinline__ f3 tri_v_t(const float* __restrict__ u, const Taps& T) {
	float x[8], y[8], z[8];
#pragma unroll
	for (int q = 0; q < 8; ++q) {
		const f3 c = ld3z(u, T.t[q]);
		x[q] = c.x, y[q] = c.y, z[q] = c.z;
	}
	return f3{tri_nest(x, T.fx, T.fy, T.fz, lerp_c), tri_nest(y, T.fx, T.fy, T.fz, lerp_c), tri_nest(z, T.fx, T.fy, T.fz, lerp_c)};
}

// One Vec3f lerp of the device branch, fmaf(w, b - a, a) per component (Stencils.hpp:131-135), written on the (x, y) pair and on z: a
// 12-byte load lands x and y in an aligned register pair, so the pair goes through v_pk_add_f32 / v_pk_fma_f32 as it is (the same IEEE
// operations per component). Left to the SLP vectoriser the seven lerps of a sample paired components of DIFFERENT taps and paid 16
// register moves per sample for it.
struct V3 {
	v2f32 xy;
	float z;
};
__device__ __forceinline__ V3 lerp_v3(const V3& a, const V3& b, float w) {
	V3 r;
	r.xy = __builtin_elementwise_fma(v2f32{w, w}, b.xy - a.xy, a.xy);
	r.z = __fmaf_rn(w, b.z - a.z, a.z);
	return r;
}
__device__ __forceinline__ f3 tri_v_b(const v4i& ru, const TapsB& T) {
	V3 c[8];
#pragma unroll
	for (int q = 0; q < 8; ++q) {
		const v3f v = hns_buffer_load_v3f32(ru, (int)(T.o[q] + (T.o[q] << 1)), 0, 0);
		c[q].xy = v2f32{v.x, v.y};
		c[q].z = v.z;
	}
	const V3 r = tri_nest(c, T.fx, T.fy, T.fz, lerp_v3);
	return f3{r.xy.x, r.xy.y, r.z};
}

__device__ __forceinline__ float tri_f_b(const v4i& rf, const TapsB& T) {
	float c[8];
#pragma unroll
	for (int q = 0; q < 8; ++q) c[q] = lds1(rf, T.o[q]);
	return tri_nest(c, T.fx, T.fy, T.fz, lerp_f);
}

// flat index of the face neighbour of voxel n of the workgroup's leaf along AXIS in direction DIR, -1 = outside
template <int AXIS, int DIR>
__device__ __forceinline__ int nbr_idx(const int* s_base, int leaf, int n) {
	constexpr int shift = AXIS == 0 ? 6 : (AXIS == 1 ? 3 : 0);
	constexpr int stride = 1 << shift;
	constexpr int dslot = AXIS == 0 ? 9 : (AXIS == 1 ? 3 : 1);
	const int c = (n >> shift) & 7;
	const bool inside = DIR > 0 ? c != 7 : c != 0;
	const int b = s_base[13 + DIR * dslot];
	const int in_leaf = leaf * 512 + n + DIR * stride;
	const int out_leaf = b < 0 ? -1 : b + n - DIR * 7 * stride;
	return inside ? in_leaf : out_leaf;
}

// the six face neighbours in the reference's order -x,+x,-y,+y,-z,+z (Kernel.cu:219,334-342,410-421)
__device__ __forceinline__ void nbr6(const int* s_base, int leaf, int n, int (&t)[6]) {
	t[0] = nbr_idx<0, -1>(s_base, leaf, n);
	t[1] = nbr_idx<0, 1>(s_base, leaf, n);
	t[2] = nbr_idx<1, -1>(s_base, leaf, n);
	t[3] = nbr_idx<1, 1>(s_base, leaf, n);
	t[4] = nbr_idx<2, -1>(s_base, leaf, n);
	t[5] = nbr_idx<2, 1>(s_base, leaf, n);
}

// ---------------------------------------------------------------------------------------------------------------
// advect_vector (reference Kernel.cu:354-453): BFECC self-advection of the velocity, clamped
// ---------------------------------------------------------------------------------------------------------------

// float-field byte offset of LDS-tile halo entry h (hns_device.hpp); >= kOutside where that neighbour leaf is absent
__device__ __forceinline__ unsigned halo_off(const unsigned* s_b4, int h) {
	int slot, local;
	halo_entry(h, slot, local);
	return s_b4[slot] + ((unsigned)local << 2);
}

// ---- the leaf and ONE voxel around it as a 10 x 10 x 10 box in LDS (round 6) ------------------------------------------------------------------
// BFECC's second sample is taken at back + u(back) * s, which is the voxel's own position up to s * (u(back) - u(own)): a fraction of a voxel wherever the
// velocity is smooth. Its eight taps then lie among the voxel and its 26 neighbours -- values the workgroup holds anyway once the tile the clamp needs
// (own leaf + six face layers, 896 voxels) is completed by the twelve edges and eight corners (104 more). Where the sample lands inside the box the kernel reads
// the second sample's taps from LDS: 8 of the kernel's 17 gathers (26 L1 tag lookups per wave each, the unit that bounds it: profiles/floors.py) are gone
// for 12 % more staging. Outside (a steep velocity gradient) the taps are gathered as before. Same values, same arithmetic: bit-identical.
// Box cell of voxel (x, y, z) relative to the leaf origin, each in [-1, 8]: ((x + 1) * 10 + y + 1) * 10 + z + 1; three component planes of kBox floats.
constexpr int kBox = 1000, kBoxShell = kBox - 512;
// k_advect_vector_n pads its rows from 10 to 24 floats (kVY; a plane = kVP floats): a wave's taps are an 8 (y) x 8 (z) window of one x-slice, and with rows 24 apart the four rows of
// a 32-lane group fall on banks c, c + 24, c + 16, c + 8 (+ 0..7): every bank once. With rows 10 apart six lanes of every group collide (46 % of the kernel's LDS cycles were conflicts).
constexpr int kVY = 24, kVX = 10 * kVY, kVP = 10 * kVX;
// Only 10 of a row's 24 floats are used, so a second component's rows lie in the gaps: x rows at 24 r and y rows at 24 r + 12 share one plane, z has a plane of its own --
// two planes (19,200 B), not three. A load reads ONE component for all lanes, so every component keeps the bank pattern above, shifted uniformly (y by 12 banks).
// Component offsets from a cell: x 0, y kVCy, z kVCz; the box is kVBox floats.
constexpr int kVCy = kVY / 2, kVCz = kVP, kVBox = 2 * kVP;
static_assert(kVCy + 10 <= kVY, "velocity box: the y rows (10 floats from kVCy) run into the next x row");
// shell cell h in [0, 488): the two full x-slabs (2 x 100), the y = -1 / 8 rows of the inner x (2 x 80), the z = -1 / 8 ends of the inner rows (2 x 64):
// slot of its leaf in the 27-table, voxel inside that leaf, box cell
template <int XS = 100, int YS = 10>  // strides of the box the cell number is for
__device__ __forceinline__ void box_shell_entry(int h, int& slot, int& local, int& cell) {
	int bx, by, bz;
	if (h < 200) {
		const int side = h >= 100, r = h - 100 * side;
		bx = 9 * side, by = r / 10, bz = r - 10 * by;
	} else if (h < 360) {
		const int q = h - 200, side = q >= 80, r = q - 80 * side;
		bx = 1 + r / 10, by = 9 * side, bz = r - 10 * (bx - 1);
	} else {
		const int q = h - 360, side = q >> 6, r = q & 63;
		bx = 1 + (r >> 3), by = 1 + (r & 7), bz = 9 * side;
	}
	slot = ((bx + 7) >> 3) * 9 + ((by + 7) >> 3) * 3 + ((bz + 7) >> 3);
	local = (((bx + 7) & 7) << 6) | (((by + 7) & 7) << 3) | ((bz + 7) & 7);
	cell = bx * XS + by * YS + bz;
}
// the shell cell that thread h stages (the first 488 threads; 0 for the others) and the float-field byte offset of the voxel under it (>= kOutside where that leaf is absent)
template <int XS = 100, int YS = 10>
__device__ __forceinline__ unsigned box_shell_off(const unsigned* s_b4, int h, int& cell) {
	unsigned off = 0u;
	cell = 0;
	if (h < kBoxShell) {
		int slot, local;
		box_shell_entry<XS, YS>(h, slot, local, cell);
		off = s_b4[slot] + ((unsigned)local << 2);
	}
	return off;
}
// box cell of own voxel n, and the step from a cell to its face neighbour d in the reference's order -x,+x,-y,+y,-z,+z (Kernel.cu:219,334-342,410-421)
template <int XS = 100, int YS = 10>
__device__ __forceinline__ int box_own(int n) { return ((n >> 6) + 1) * XS + (((n >> 3) & 7) + 1) * YS + (n & 7) + 1; }
template <int XS = 100, int YS = 10>
__device__ __forceinline__ constexpr int box_nbr(int d) { return (d & 1 ? 1 : -1) * (d < 2 ? XS : (d < 4 ? YS : 1)); }

// Stage the velocity box, components y and z at CY and CZ floats from x (three planes, or kVCy / kVCz): every thread its own voxel (value vo), the first 488 the shell cell `cell` with the voxel at `off` (box_shell_off).
// What a shell cell outside the domain holds is the caller's choice of `off`: unmapped it reads 0 (advect_vector: the descriptor's bounds check), mapped to element g.oob that
// element (advect_scalars, Kernel.cu:225). In two halves, load and store: the store waits for the load, and a kernel that has gathers to issue puts them in between
// (k_advect_scalars_n<false, true>: with the store in front of them the kernel was 2.3 % slower, profiles/advect_refactor_ab.txt). The caller's barrier completes the box.
template <int XS, int YS, int CY, int CZ>
__device__ __forceinline__ f3 velocity_box_load(float* s_box, const v4i& ru, int n, const f3& vo, unsigned off) {
	const int ob = box_own<XS, YS>(n);
	s_box[ob] = vo.x, s_box[ob + CY] = vo.y, s_box[ob + CZ] = vo.z;
	f3 h = {0.0f, 0.0f, 0.0f};
	if (n < kBoxShell) h = ldv(ru, off);
	return h;
}
template <int CY, int CZ>
__device__ __forceinline__ void velocity_box_store(float* s_box, int n, int cell, const f3& h) {
	if (n < kBoxShell) s_box[cell] = h.x, s_box[cell + CY] = h.y, s_box[cell + CZ] = h.z;
}
__device__ __forceinline__ V3 box_v3(const float* s_box, int a) {
	V3 r;
	r.xy = v2f32{s_box[a], s_box[a + kVCy]};
	r.z = s_box[a + kVCz];
	return r;
}
__device__ __forceinline__ f3 box_f3(const float* s_box, int a) {
	const V3 t = box_v3(s_box, a);
	return f3{t.xy.x, t.xy.y, t.z};
}
// TrilinearSampler over the box (rows kVY apart): a = cell of the lower corner
__device__ __forceinline__ f3 tri_v_box(const float* s_box, int a, float fx, float fy, float fz) {
	V3 c[8];
#pragma unroll
	for (int q = 0; q < 8; ++q) c[q] = box_v3(s_box, a + box_corner<kVX, kVY>(tap_of(q)));
	const V3 r = tri_nest(c, fx, fy, fz, lerp_v3);
	return f3{r.xy.x, r.xy.y, r.z};
}
// The velocity at (sx, sy, sz), advect_vector's sample: out of the box where the whole wave's cells lie inside it, else gathered.
// (either sample: the FIRST one too lands in the box where the flow moves less than a voxel per step -- then the wave gathers nothing at all. Per WAVE here: with a lane
// outside, all of them gather -- measured 2.4 % faster through the plume's transient than a per-lane split; advect_scalars splits per lane)
__device__ __forceinline__ f3 sample_velocity(const GridDev& g, const NarrowCtx& C, const v4i& ru, const float* s_box, float sx, float sy, float sz) {
	const int i = __float2int_rd(sx), j = __float2int_rd(sy), k = __float2int_rd(sz);
	const unsigned rx = (unsigned)(i - (C.org.x - 1)), ry = (unsigned)(j - (C.org.y - 1)), rz = (unsigned)(k - (C.org.z - 1));  // cell and cell + 1 inside the box <=> each in [0, 8]
	if (__all(max(rx, max(ry, rz)) <= 8u)) return tri_v_box(s_box, (int)(rx * (unsigned)kVX + ry * (unsigned)kVY + rz), sx - (float)i, sy - (float)j, sz - (float)k);
	return tri_v_b(ru, make_taps_b(g, C, sx, sy, sz));
}

// ---- the collision SDF of the leaf and one voxel around it, a fourth box (k_advect_vector_n<true>, k_advect_scalars_n<.., .., true>) -------------------------
// With a collider every trial position is tested against the SDF first (its nested-lerp sample < 0: Kernel.cu:142-155, 211-214, 377-382, 390-394) and advect_vector blends
// the result by the voxel's own SDF value and the gradient over its six face neighbours (:433-450). All of those lie in the box wherever the velocity sample itself does, so the
// kernels stage the SDF as they stage the velocity: own value per thread, shell by the first 488 threads, through a descriptor of the float field with the UNMAPPED shell offsets --
// a cell outside the domain holds 0, as IndexSampler<float, 1> (ldz in tri_f_t) and sdf_normal (ld0) read it. Same values, same arithmetic as the generic kernels: bit-identical.
__device__ __forceinline__ float sdf_box_load(float* s_sdf, const v4i& rs, int n, int ob, float own, unsigned off) {
	s_sdf[ob] = own;
	float h = 0.0f;
	if (n < kBoxShell) h = lds1(rs, off);
	return h;
}
__device__ __forceinline__ void sdf_box_store(float* s_sdf, int n, int cell, float h) {
	if (n < kBoxShell) s_sdf[cell] = h;
}
// IndexSampler<float,1> over a box (a = cell of the lower corner): tri_f_b's arithmetic
template <int XS, int YS>
__device__ __forceinline__ float tri_f_box(const float* s_f, int a, float fx, float fy, float fz) {
	float c[8];
#pragma unroll
	for (int q = 0; q < 8; ++q) c[q] = s_f[a + box_corner<XS, YS>(tap_of(q))];
	return tri_nest(c, fx, fy, fz, lerp_f);
}
// advect_vector's epilogue with a collider (Kernel.cu:433-450) for the voxel at box cell ob. (sv < 0 is false for -0 and NaN, sv < 0.1 false for NaN: in this order)
template <int XS, int YS>
__device__ __forceinline__ f3 collide_velocity(const float* s_sdf, int ob, f3 vc, float inv_dx) {
	const float sv = s_sdf[ob];
	if (sv < 0.0f) {
		vc.x = vc.y = vc.z = 0.0f;
	} else if (sv < 0.1f) {
		float nb[6];
#pragma unroll
		for (int d = 0; d < 6; ++d) nb[d] = s_sdf[ob + box_nbr<XS, YS>(d)];
		vc = no_slip_blend(vc, sdf_normal_of(nb, inv_dx), 1.0f - (sv / 1.5f));
	}
	return vc;
}

// 32-bit addressed form: same loads and arithmetic as the generic kernel below. COLL: with a collision SDF (rows of its box kVY apart, as the velocity's, so one cell number
// serves both). The test is per lane; where it sends a lane back -- pass 0 to the voxel's own position, pass 1 to the (possibly reset) back position -- the wave samples again at
// the positions it then has, a full eight-tap sample also where the weights are 0 (0 x inf = NaN, in the reference as here).
template <bool COLL>
__device__ __forceinline__ void advect_vector_n(const GridDev& g, const float* __restrict__ u, float* __restrict__ out, const float* __restrict__ sdf, float* s_sdf, const float scaled_dt,
                                                const float inv_dx) {
	__shared__ NarrowTabs tabs;
	__shared__ float s_box[kVBox];
	// the voxel's own velocity needs the leaf number only: its load is issued before the neighbour table is fetched and staged (one memory
	// round trip less in front of the first gathers; the kernel is bound by the length of that chain)
	NarrowCtx C(g, tabs);
	const v4i ru = field_rsrc(u, (unsigned)g.n_leaves * 6144u);
	const f3 vo = ldv(ru, (unsigned)C.idx << 2);
	v4i rs = {0, 0, 0, 0};
	float so = 0.0f;
	if constexpr (COLL) {
		rs = field_rsrc(sdf, (unsigned)g.n_leaves * 2048u);
		so = lds1(rs, (unsigned)C.idx << 2);
	}
	C.stage(g);
	int cell;
	const unsigned off = box_shell_off<kVX, kVY>(tabs.b4, C.n, cell);
	const int ob = box_own<kVX, kVY>(C.n);
	const f3 hv = velocity_box_load<kVX, kVY, kVCy, kVCz>(s_box, ru, C.n, vo, off);
	if constexpr (COLL) sdf_box_store(s_sdf, C.n, cell, sdf_box_load(s_sdf, rs, C.n, ob, so, off));
	velocity_box_store<kVCy, kVCz>(s_box, C.n, cell, hv);
	float sx = C.px - scaled_dt * vo.x, sy = C.py - scaled_dt * vo.y, sz = C.pz - scaled_dt * vo.z;  // backPos (Kernel.cu:374)
	float rx = C.px, ry = C.py, rz = C.pz;                                                            // COLL: where a collision sends the trace back to
	f3 vf = {0.0f, 0.0f, 0.0f}, vb = {0.0f, 0.0f, 0.0f};
	__syncthreads();  // box complete
#pragma unroll 1
	for (int pass = 0; pass < 2; ++pass) {
		f3 v;
		if constexpr (COLL) {  // Kernel.cu:377-382 / :390-394
			const int i = __float2int_rd(sx), j = __float2int_rd(sy), k = __float2int_rd(sz);
			const unsigned cx = (unsigned)(i - (C.org.x - 1)), cy = (unsigned)(j - (C.org.y - 1)), cz = (unsigned)(k - (C.org.z - 1));
			const bool boxed = __all(max(cx, max(cy, cz)) <= 8u);  // per wave, as sample_velocity
			const int a = (int)(cx * (unsigned)kVX + cy * (unsigned)kVY + cz);
			float d;
			if (boxed)
				d = tri_f_box<kVX, kVY>(s_sdf, a, sx - (float)i, sy - (float)j, sz - (float)k);
			else  // (sample_velocity builds these taps again for a lane that stays: held across the SDF gathers for it, their eight offsets take the kernel from 58 registers to 64 and three spills)
				d = tri_f_b(rs, make_taps_b(g, C, sx, sy, sz));
			if (d < 0.0f) sx = rx, sy = ry, sz = rz;
			v = sample_velocity(g, C, ru, s_box, sx, sy, sz);
		} else {
			v = sample_velocity(g, C, ru, s_box, sx, sy, sz);
		}
		if (pass == 0) {
			vf = v;
			if constexpr (COLL) rx = sx, ry = sy, rz = sz;  // fwdPos2 falls back to backPos
			sx = sx + scaled_dt * v.x, sy = sy + scaled_dt * v.y, sz = sz + scaled_dt * v.z;  // Kernel.cu:387
		} else {
			vb = v;
		}
	}
	f3 vc = bfecc_limit_v(vo, vf, vb, [&](int d) { return box_f3(s_box, ob + box_nbr<kVX, kVY>(d)); });
	if constexpr (COLL) vc = collide_velocity<kVX, kVY>(s_sdf, ob, vc, inv_dx);
	st3(out, C.idx, vc);
}
// Two kernels of ONE name: this one without a collision field, and below it the template that takes the SDF. The first keeps the symbol (and with it the registers and LDS that
// tests/test_kernel_resources.py pins by symbol) it had before there was a second; a launch picks between them by its argument list.
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_advect_vector_n(const GridDev g, const float* __restrict__ u, float* __restrict__ out, const float scaled_dt) {
	advect_vector_n<false>(g, u, out, nullptr, nullptr, scaled_dt, 0.0f);
}
// LDS: the velocity box, the SDF box and the tables. Four workgroups per CU (eight waves per SIMD) need a quarter of gfx950's 160 KB each.
constexpr int kVectorCollLds = (kVBox + kVP) * 4 + (int)sizeof(NarrowTabs);
static_assert(kVectorCollLds <= 160 * 1024 / 4, "k_advect_vector_n<true>: four workgroups per CU no longer fit the LDS");
template <bool COLL>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_advect_vector_n(const GridDev g, const float* __restrict__ u, float* __restrict__ out,
                                                                                                const float* __restrict__ sdf, const float scaled_dt, const float inv_dx) {
	static_assert(COLL, "without a collision field: the kernel of the same name that takes no SDF");
	__shared__ float s_sdf[kVP];
	advect_vector_n<true>(g, u, out, sdf, s_sdf, scaled_dt, inv_dx);
}

template <bool COLL>
__global__ __launch_bounds__(512) void k_advect_vector(const GridDev g, const float* __restrict__ u, float* __restrict__ out,
                                                       const float* __restrict__ sdf, const float scaled_dt, const float inv_dx) {
	__shared__ GenericTabs tabs;
	GenericCtx C(g, tabs);
	C.stage(g);
	const int idx = C.idx;

	const f3 vo = ld3(u, idx);
	// forward pass (backtrace) then backward check: the same sampling code twice, kept as a 2-trip loop so that the
	// far-tap path is emitted once
	float sx = C.px - scaled_dt * vo.x, sy = C.py - scaled_dt * vo.y, sz = C.pz - scaled_dt * vo.z;  // backPos (Kernel.cu:374)
	float rx = C.px, ry = C.py, rz = C.pz;                                                            // where a collision sends the trace back to
	f3 vf = {0.0f, 0.0f, 0.0f}, vb = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
	for (int pass = 0; pass < 2; ++pass) {
		Taps T = make_taps(g, C, sx, sy, sz);
		if (COLL) {
			if (tri_f_t(sdf, T) < 0.0f) {  // Kernel.cu:377-382 / :390-394
				sx = rx, sy = ry, sz = rz;
				T = make_taps(g, C, sx, sy, sz);
			}
		}
		const f3 v = tri_v_t(u, T);
		if (pass == 0) {
			vf = v;
			rx = sx, ry = sy, rz = sz;  // fwdPos2 falls back to backPos
			sx = sx + scaled_dt * v.x, sy = sy + scaled_dt * v.y, sz = sz + scaled_dt * v.z;  // Kernel.cu:387
		} else {
			vb = v;
		}
	}
	int nb[6];
	nbr6(tabs.base, C.leaf, C.n, nb);
	f3 vc = bfecc_limit_v(vo, vf, vb, [&](int d) { return ld3z(u, nb[d]); });

	if (COLL) {  // Kernel.cu:433-450
		const float sv = sdf[idx];
		if (sv < 0.0f) {
			vc.x = vc.y = vc.z = 0.0f;
		} else if (sv < 0.1f) {
			const f3 nrm = sdf_normal(g, tabs.nbr, C.org, sdf, C.c.x, C.c.y, C.c.z, inv_dx);
			vc = no_slip_blend(vc, nrm, 1.0f - (sv / 1.5f));
		}
	}
	st3(out, idx, vc);
}

// ---------------------------------------------------------------------------------------------------------------
// advect_scalar (reference Kernel.cu:269-352): single field, nested-lerp trilinear
// ---------------------------------------------------------------------------------------------------------------

// 32-bit addressed form (no collision field)
__global__ __launch_bounds__(512) void k_advect_scalar_n(const GridDev g, const float* __restrict__ u, const float* __restrict__ in, float* __restrict__ out,
                                                         const float scaled_dt) {
	__shared__ NarrowTabs tabs;
	NarrowCtx C(g, tabs);
	C.stage(g);
	const int n = C.n;
	const unsigned bytes1 = (unsigned)g.n_leaves * 2048u, own = (unsigned)C.idx << 2;
	const v4i ru = field_rsrc(u, bytes1 * 3u), rf = field_rsrc(in, bytes1);

	__shared__ float s_tile[kTile];  // clamp neighbours through LDS (see k_advect_vector_n)
	const float phiOrig = lds1(rf, own);
	s_tile[n] = phiOrig;
	if (n < 384) s_tile[512 + n] = lds1(rf, halo_off(tabs.b4, n));
	const f3 vc = ldv(ru, own);
	float sx = C.px - scaled_dt * vc.x, sy = C.py - scaled_dt * vc.y, sz = C.pz - scaled_dt * vc.z;
	float phiForward = 0.0f, phiBackward = 0.0f;
#pragma unroll 1
	for (int pass = 0; pass < 2; ++pass) {
		const TapsB T = make_taps_b(g, C, sx, sy, sz);
		const float phi = tri_f_b(rf, T);
		if (pass == 0) {
			phiForward = phi;
			const f3 vf = tri_v_b(ru, T);  // same eight taps as phiForward
			sx = sx + scaled_dt * vf.x, sy = sy + scaled_dt * vf.y, sz = sz + scaled_dt * vf.z;
		} else {
			phiBackward = phi;
		}
	}
	const float error = phiOrig - phiBackward;
	__syncthreads();
	const float nv[6] = {s_tile[tile_nbr<0, -1>(n)], s_tile[tile_nbr<0, 1>(n)], s_tile[tile_nbr<1, -1>(n)], s_tile[tile_nbr<1, 1>(n)], s_tile[tile_nbr<2, -1>(n)], s_tile[tile_nbr<2, 1>(n)]};
	out[C.idx] = bfecc_limit(phiOrig, nv, phiForward, phiForward + 0.5f * error);
}

template <bool COLL>
__global__ __launch_bounds__(512) void k_advect_scalar(const GridDev g, const float* __restrict__ u, const float* __restrict__ in,
                                                       float* __restrict__ out, const float* __restrict__ sdf, const float scaled_dt) {
	__shared__ GenericTabs tabs;
	GenericCtx C(g, tabs);
	C.stage(g);
	const int idx = C.idx;

	const float phiOrig = in[idx];
	const f3 vc = ld3(u, idx);
	float sx = C.px - scaled_dt * vc.x, sy = C.py - scaled_dt * vc.y, sz = C.pz - scaled_dt * vc.z;
	float rx = C.px, ry = C.py, rz = C.pz;
	float phiForward = 0.0f, phiBackward = 0.0f;
#pragma unroll 1
	for (int pass = 0; pass < 2; ++pass) {
		Taps T = make_taps(g, C, sx, sy, sz);
		if (COLL) {
			if (tri_f_t(sdf, T) < 0.0f) {
				sx = rx, sy = ry, sz = rz;
				T = make_taps(g, C, sx, sy, sz);
			}
		}
		const float phi = tri_f_t(in, T);
		if (pass == 0) {
			phiForward = phi;
			const f3 vf = tri_v_t(u, T);  // same eight taps as phiForward
			rx = sx, ry = sy, rz = sz;
			sx = sx + scaled_dt * vf.x, sy = sy + scaled_dt * vf.y, sz = sz + scaled_dt * vf.z;
		} else {
			phiBackward = phi;
		}
	}
	const float error = phiOrig - phiBackward;
	int nb[6];
	nbr6(tabs.base, C.leaf, C.n, nb);
	float nv[6];
#pragma unroll
	for (int d = 0; d < 6; ++d) nv[d] = ldz(in, nb[d]);
	out[idx] = bfecc_limit(phiOrig, nv, phiForward, phiForward + 0.5f * error);
}

// ---------------------------------------------------------------------------------------------------------------
// advect_scalars (reference Kernel.cu:118-266): one backtrace shared by up to HNS_MAX_SCALARS fields,
// weight-product trilinear, out-of-domain taps read ELEMENT g.oob (0 in the reference: Kernel.cu:133,192,225)
// ---------------------------------------------------------------------------------------------------------------

#define HNS_MAX_SCALARS 8
struct ScalarPtrs {
	const float* in[HNS_MAX_SCALARS];
	float* out[HNS_MAX_SCALARS];
	int n;
	// k_advect_scalars_n<true> (round 6): four more fields that arrive as ONE 16-byte element per voxel -- {fuel, waste, temperature, flame} as the fused
	// divergence / combustion kernel leaves them (hns_pressure.hip: CombustFuse) -- and leave as four float arrays like every other field
	const float* q4;
	float* q4_out[4];
};

// advect_scalar (Kernel.cu:269-352) over up to HNS_MAX_SCALARS fields with ONE back-trace: k_advect_scalar_n's arithmetic per field (nested lerps, 0 outside the domain,
// unfused correction), so every output is bit-identical to one k_advect_scalar_n launch per field (P.q4 unused). What does not depend on the field is done once per voxel --
// own velocity, table staging, back position, both sets of eight tap offsets and the eight 12-byte velocity gathers (26 L1 tag lookups each, the unit these kernels are bound
// by) -- where S launches of k_advect_scalar_n do it S times.
// The two z-corners of a tap column come as one 8-byte load (ld_zpair): 9 + 8 S gathers per voxel against 25 S. The offsets are unmapped, so the pair of an absent leaf lies
// wholly past the descriptor and reads 0, and hi == lo + 4 cannot hold across two leaves (leaf bases are multiples of 2048): the same values as eight 4-byte loads
// (measured against those: profiles/advect_multi_ab.txt). Two tiles alternate so that one barrier per field suffices (as s_box[2] of k_advect_scalars_n).
// Eight waves per SIMD: at 62 registers four workgroups share a CU; left to itself the compiler takes 67 = three, 7-10 % slower at S = 2 ... 8 (the same file, 2).
__device__ __forceinline__ float tri_f_zpair(const v4i& rf, const TapsB& T) {  // tri_f_b with z-paired loads
	float c[8];
#pragma unroll
	for (int m = 0; m < 4; ++m) ld_zpair(rf, T.o[2 * m], T.o[2 * m + 1], c[2 * m], c[2 * m + 1]);
	return tri_nest(c, T.fx, T.fy, T.fz, lerp_f);
}
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_advect_scalar_multi_n(const GridDev g, const float* __restrict__ u, const ScalarPtrs P, const float scaled_dt) {
	__shared__ NarrowTabs tabs;
	NarrowCtx C(g, tabs);
	const int n = C.n;
	const unsigned bytes1 = (unsigned)g.n_leaves * 2048u, own = (unsigned)C.idx << 2;
	const v4i ru = field_rsrc(u, bytes1 * 3u);
	const f3 vc = ldv(ru, own);  // (issued before the neighbour table is staged: see k_advect_vector_n)
	C.stage(g);
	// the back-trace, once: B = taps of the back position, F = taps of the forward position (a 2-trip loop so that the far-tap path is emitted once)
	float sx = C.px - scaled_dt * vc.x, sy = C.py - scaled_dt * vc.y, sz = C.pz - scaled_dt * vc.z;
	TapsB B, F;
#pragma unroll 1
	for (int pass = 0; pass < 2; ++pass) {
		F = make_taps_b(g, C, sx, sy, sz);
		if (pass == 0) {
			B = F;
			const f3 vf = tri_v_b(ru, B);
			sx = sx + scaled_dt * vf.x, sy = sy + scaled_dt * vf.y, sz = sz + scaled_dt * vf.z;
		}
	}
	const unsigned ho = n < 384 ? halo_off(tabs.b4, n) : 0u;
	__shared__ float s_tile[2][kTile];  // clamp neighbours through LDS (see k_advect_vector_n)
	for (int s = 0; s < P.n; ++s) {
		const v4i rf = field_rsrc(P.in[s], bytes1);
		float* tile = s_tile[s & 1];
		const float phiOrig = lds1(rf, own);
		tile[n] = phiOrig;
		if (n < 384) tile[512 + n] = lds1(rf, ho);
		const float phiForward = tri_f_zpair(rf, B), phiBackward = tri_f_zpair(rf, F);
		const float error = phiOrig - phiBackward;
		__syncthreads();
		const float nv[6] = {tile[tile_nbr<0, -1>(n)], tile[tile_nbr<0, 1>(n)], tile[tile_nbr<1, -1>(n)], tile[tile_nbr<1, 1>(n)], tile[tile_nbr<2, -1>(n)], tile[tile_nbr<2, 1>(n)]};
		P.out[s][C.idx] = bfecc_limit(phiOrig, nv, phiForward, phiForward + 0.5f * error);
	}
}

// setupInterpolation (Kernel.cu:163-196): indices and weights in the order 000,100,010,110,001,101,011,111 of (x,y,z)
__device__ __forceinline__ void interp_from_taps(const Taps& T, int oob, int (&ix)[8], float (&w)[8]) {
	tri_weights(T.fx, T.fy, T.fz, w);
#pragma unroll
	for (int q = 0; q < 8; ++q) ix[q] = T.t[tap_of(q)] < 0 ? oob : T.t[tap_of(q)];
}
// velF = velF + v * w (Kernel.cu:201-206), unfused
__device__ __forceinline__ void add_weighted(f3& a, const f3& v, float w) { a.x = a.x + w * v.x, a.y = a.y + w * v.y, a.z = a.z + w * v.z; }

// One sample point of advect_scalars in the 32-bit kernels. Where BOX allows it and the point's cell and cell + 1 lie inside the leaf's 10^3 box (per lane): true, and the box
// cell of the lower corner -- corner q of the interpolation order is box cell `cell + box_corner(q)`. Else the eight float-field byte offsets in interpolation order, a tap
// outside the domain mapped to element oob4 / 4 (Kernel.cu:133,192,225). Either way the weights of setupInterpolation.
template <bool BOX>
__device__ __forceinline__ bool sample_setup(const GridDev& g, const NarrowCtx& C, float x, float y, float z, unsigned oob4, int& cell, unsigned (&o)[8], float (&w)[8]) {
	const int i = __float2int_rd(x), j = __float2int_rd(y), k = __float2int_rd(z);
	const unsigned rx = (unsigned)(i - (C.org.x - 1)), ry = (unsigned)(j - (C.org.y - 1)), rz = (unsigned)(k - (C.org.z - 1));
	const bool boxed = BOX && max(rx, max(ry, rz)) <= 8u;
	cell = boxed ? (int)((rx * 10u + ry) * 10u + rz) : 0;
	float tx, ty, tz;
	if (boxed) {
		tx = x - (float)i, ty = y - (float)j, tz = z - (float)k;  // (make_taps_b's fractions)
#pragma unroll
		for (int q = 0; q < 8; ++q) o[q] = 0u;
	} else {
		const TapsB T = make_taps_b(g, C, x, y, z);
		tx = T.fx, ty = T.fy, tz = T.fz;
#pragma unroll
		for (int q = 0; q < 8; ++q) o[q] = T.o[tap_of(q)] >= kOutside ? oob4 : T.o[tap_of(q)];
	}
	tri_weights(tx, ty, tz, w);
	return boxed;
}

// 32-bit addressed form (no collision field). Out-of-domain taps read element g.oob, as in the generic kernel.
// Q4: besides the P.n float fields, the four fields of P.q4. A corner tap of those four is ONE 16-byte gather instead of four 4-byte (z-paired: 8-byte) ones: the
// kernel is bound by L1 accesses per gather instruction (profiles/r05_advect_notes.txt 2), and a quad of lanes costs an access whatever its width -- sixteen
// gathers for the four fields' two samples instead of thirty-two. Per field the arithmetic is the same chain of fused multiply-adds in the same order.
// (at least four waves per SIMD = two workgroups per CU: the Q4 form sits at the 128-register line, and one register over it is ONE workgroup per CU -- 585 -> 838 us at 256^3, measured)
// AHEAD (float-only form): the look-ahead launch of a substep's part C. The NEXT substep's advect_vector reads this same velocity with this same scaled_dt, so its own-velocity load,
// its table staging, its back position, its eight tap offsets and its eight 12-byte gathers are the ones made here. The kernel writes advect_vector(u) of its voxels to adv_out as
// well: both first samples are formed from the one set of taps (nested lerps for the vector, weight products for the fields: different bits); the vector's sample then waits in LDS
// while the fields are advected, and BEHIND the per-field loop the vector half takes its second sample from a velocity box (rows kVY apart, as k_advect_vector_n), clamps and stores.
// That order is the one that fits without a spill (the vector half in front of the loop: 100 registers, profiles/lookahead_ab.txt); with the two-plane velocity box and the far-tap
// path's grid fields read where that path runs (gk below) it is 64 registers and 33.8 KB of LDS: four workgroups per CU, eight waves per SIMD (profiles/lookahead_occupancy_ab.txt).
// Same loads of the same values, same arithmetic in the same association as k_advect_vector_n and k_advect_scalars_n<false>: bit-identical to the two launches.
// COLL: with a collision SDF, staged as a fourth box (see sdf_box_load; 0 outside the domain, unlike the field boxes of this kernel). The back position is tested before its
// sample is set up and falls back to the voxel's own position (Kernel.cu:142-155; the reference makes that test twice, and the repeat cannot change the outcome), the forward
// position before the second set-up and falls back to the back position (:211-214). Per lane. The fields' arithmetic is untouched.
// The SDF at (x, y, z) < 0 ? -- out of the leaf's SDF box (rows 10 apart) where the cell and cell + 1 lie inside it, else gathered
__device__ __forceinline__ bool sdf_hit(const GridDev& g, const NarrowCtx& C, const v4i& rs, const float* s_sdf, float x, float y, float z) {
	const int i = __float2int_rd(x), j = __float2int_rd(y), k = __float2int_rd(z);
	const unsigned rx = (unsigned)(i - (C.org.x - 1)), ry = (unsigned)(j - (C.org.y - 1)), rz = (unsigned)(k - (C.org.z - 1));
	float d;
	if (max(rx, max(ry, rz)) <= 8u)
		d = tri_f_box<100, 10>(s_sdf, (int)((rx * 10u + ry) * 10u + rz), x - (float)i, y - (float)j, z - (float)k);
	else  // (sample_setup builds these taps again for a lane that stays: kept for it across the SDF gathers, they spill the q4 form at its 80 registers -- 132 bytes of scratch a lane -- and cost the float form eight)
		d = tri_f_b(rs, make_taps_b(g, C, x, y, z));
	return d < 0.0f;
}
// The kernel's GridDev where it lies in the kernel-argument segment. ONLY in kernels whose FIRST parameter is the GridDev (by value: offset 0 of the segment): a field read through
// this reference is a scalar load at the point of use, where the same field of the by-value parameter is loaded at the kernel's entry and held.
__device__ __forceinline__ const GridDev& kernarg_grid() { return *reinterpret_cast<const GridDev*>((const void*)__builtin_amdgcn_kernarg_segment_ptr()); }

template <bool Q4, bool AHEAD, bool COLL>
__device__ __forceinline__ void advect_scalars_n(const GridDev& g, const float* __restrict__ u, const ScalarPtrs& P, const float scaled_dt, float* __restrict__ adv_out,
                                                 const float* __restrict__ sdf) {
	static_assert(!(Q4 && AHEAD), "the look-ahead form is float-only");
	static_assert(!(AHEAD && COLL), "with a collider the next substep rewrites the velocity before it advects it: nothing to look ahead to");
	// AHEAD: what the far-tap path needs of the grid (origins, nbr27, hash, hash_mask, far_flag) is read where that path runs, not held from the kernel's entry in nine scalar
	// registers across three inlined copies of it: at eight waves per SIMD 80 scalar registers are addressable, and with them held the kernel spilled four into a VGPR's lanes
	// -- the 65th register (profiles/lookahead_occupancy_ab.txt).
	const GridDev& gk = AHEAD ? kernarg_grid() : g;
	__shared__ NarrowTabs tabs;
	NarrowCtx C(g, tabs);
	const int n = C.n, idx = C.idx;
	const unsigned bytes1 = (unsigned)g.n_leaves * 2048u;
	const v4i ru = field_rsrc(u, bytes1 * 3u);
	const unsigned own = (unsigned)idx << 2, oob4 = (unsigned)g.oob << 2;
	const f3 vc = ldv(ru, own);  // (issued before the neighbour table is staged: see k_advect_vector_n)
	v4i rs = {0, 0, 0, 0};
	float so = 0.0f;
	if constexpr (COLL) {
		rs = field_rsrc(sdf, bytes1);
		so = lds1(rs, own);
	}
	C.stage(g);

	// the leaf and one voxel around it through LDS (see k_advect_vector_n): the velocity once, then per field; shell cell of this thread (the first 488) and where its value lies
	const int ob = box_own(n);
	int hcell;
	unsigned ho = box_shell_off(tabs.b4, n, hcell);
	__shared__ float s_sdf[COLL ? kBox : 1];
	if constexpr (COLL) sdf_box_store(s_sdf, n, hcell, sdf_box_load(s_sdf, rs, n, ob, so, ho));  // (the unmapped offset: 0 outside the domain)
	ho = ho >= kOutside ? oob4 : ho;  // out-of-domain neighbours read element g.oob here (Kernel.cu:225)
	// FIRST: the first sample's taps out of the boxes too (below). Measured (profiles/r06_advect_box_ab.txt): it pays in the q4 form, which then fits 80 registers = six waves per SIMD,
	// and costs the float-only form a fifth (one more 12-byte gather per thread for the velocity shell, and a barrier in front of its first gathers)
	constexpr bool FIRST = Q4;
	__shared__ float s_ubox[FIRST ? 3 * kBox : 1];
	if constexpr (FIRST) velocity_box_store<kBox, 2 * kBox>(s_ubox, n, hcell, velocity_box_load<100, 10, kBox, 2 * kBox>(s_ubox, ru, n, vc, ho));

	float bx = C.px - scaled_dt * vc.x, by = C.py - scaled_dt * vc.y, bz = C.pz - scaled_dt * vc.z;
	__shared__ float s_back[COLL && FIRST ? 3 * 512 : 1];
	if constexpr (COLL) {
		__syncthreads();  // SDF box complete (and the velocity box, FIRST)
		if (sdf_hit(g, C, rs, s_sdf, bx, by, bz)) bx = C.px, by = C.py, bz = C.pz;
		if constexpr (FIRST) s_back[n] = bx, s_back[n + 512] = by, s_back[n + 1024] = bz;  // (read back by this thread alone)
		asm volatile("" : "+v"(bx), "+v"(by), "+v"(bz));  // (the sample's set-up starts from the position, not from what the test kept of it)
	}
	unsigned bo[8], fo[8];
	float bw[8], fw[8];
	bool bboxed = false;  // the back sample's taps come out of the boxes (FIRST only)
	int ba = 0;           // box cell of the back cell's lower corner
	f3 vf = {0.0f, 0.0f, 0.0f};
	// AHEAD: the velocity box of k_advect_vector_n (shell cells outside the domain read 0 there -- the descriptor's bounds check -- not element g.oob), and advect_vector's
	// first sample
	__shared__ float s_vbox[AHEAD ? kVBox : 1];
	__shared__ float s_wf[AHEAD ? 3 * 512 : 1];  // (advect_vector's first sample waits here, not in three registers, while the fields are advected)
	if constexpr (AHEAD) {
		int vcell;
		const unsigned voff = box_shell_off<kVX, kVY>(tabs.b4, n, vcell);
		const f3 hv = velocity_box_load<kVX, kVY, kVCy, kVCz>(s_vbox, ru, n, vc, voff);
		// the eight taps of the back cell, gathered ONCE with the unmapped offsets: 0 outside the domain, which is what advect_vector samples
		const TapsB T = make_taps_b(gk, C, bx, by, bz);
		V3 c[8];  // (issued in the order the weight products consume them: the z lerp of a column follows as soon as its second tap has been added, and the pair's registers are free)
#pragma unroll
		for (int q = 0; q < 8; ++q) {
			const v3f v = hns_buffer_load_v3f32(ru, (int)(T.o[tap_of(q)] + (T.o[tap_of(q)] << 1)), 0, 0);
			c[tap_of(q)].xy = v2f32{v.x, v.y};
			c[tap_of(q)].z = v.z;
		}
		const float* __restrict__ uoob = u + 3 * (size_t)g.oob;
		const f3 uo = {uoob[0], uoob[1], uoob[2]};  // what advect_scalars samples outside the domain: element g.oob (a uniform address: scalar registers)
		velocity_box_store<kVCy, kVCz>(s_vbox, n, vcell, hv);
		tri_weights(T.fx, T.fy, T.fz, bw);
		// Two samples from the one set of taps. advect_scalars': the weight products, a tap outside the domain replaced by element g.oob. advect_vector's: nested lerps
		// (tri_v_b) -- column z[t >> 1] = lerp(c[t - 1], c[t]) once the odd tap t has been added.
		V3 z[4];
#pragma unroll
		for (int q = 0; q < 8; ++q) {
			const int t = tap_of(q);
			const bool outside = T.o[t] >= kOutside;
			bo[q] = outside ? oob4 : T.o[t];
			add_weighted(vf, f3{outside ? uo.x : c[t].xy.x, outside ? uo.y : c[t].xy.y, outside ? uo.z : c[t].z}, bw[q]);
			if (t & 1) z[t >> 1] = lerp_v3(c[t - 1], c[t], T.fz);
		}
		const V3 r = tri_nest_yx(z, T.fx, T.fy, lerp_v3);
		s_wf[n] = r.xy.x, s_wf[n + 512] = r.xy.y, s_wf[n + 1024] = r.z;
	} else {
		// Where the flow moves less than a voxel per step the FIRST sample point, too, lies among the voxel's 26 neighbours: its taps (velocity here, the fields' below) come out of
		// the boxes, per lane.
		bboxed = sample_setup<FIRST>(gk, C, bx, by, bz, oob4, ba, bo, bw);
		f3 vt[8];
		if (!bboxed) {
#pragma unroll
			for (int q = 0; q < 8; ++q) vt[q] = ldv(ru, bo[q]);
		}
		if constexpr (FIRST && !COLL) __syncthreads();  // velocity box complete
		if (bboxed) {
#pragma unroll
			for (int q = 0; q < 8; ++q) {
				const int a = ba + box_corner(q);
				vt[q] = f3{s_ubox[a], s_ubox[a + kBox], s_ubox[a + 2 * kBox]};
			}
		}
#pragma unroll
		for (int q = 0; q < 8; ++q) add_weighted(vf, vt[q], bw[q]);
	}
	// The second sample point is the voxel's own position up to s * (u(back) - u(own)): where it lands inside the leaf's 10^3 box (k_advect_vector_n, which see)
	// the fields' forward taps are read from the LDS box that the clamp needs anyway, not gathered
	int fa;  // box cell of the forward cell's lower corner
	float fx = bx + scaled_dt * vf.x, fy = by + scaled_dt * vf.y, fz = bz + scaled_dt * vf.z;
	if constexpr (COLL) {
		if (sdf_hit(g, C, rs, s_sdf, fx, fy, fz)) {
			if constexpr (FIRST) {
				// (the back position waits in LDS, not in three registers across the velocity sample and this test: the q4 form sits on the 80-register line and spilled two with them)
				int m = n;
				asm volatile("" : "+v"(m));
				fx = s_back[m], fy = s_back[m + 512], fz = s_back[m + 1024];
			} else {
				fx = bx, fy = by, fz = bz;
			}
		}
	}
	const bool boxed = sample_setup<true>(gk, C, fx, fy, fz, oob4, fa, fo, fw);
	// COLL and Q4: a sample has a box cell or tap offsets, never both, so from here on the cell rides in the first offset's register (the q4 form sits on the 80-register
	// line, and with the tests in front of its set-ups it spilled the back cell)
	constexpr bool SHARE = COLL && Q4;
	if constexpr (SHARE) {
		if (bboxed) bo[0] = (unsigned)ba;
		if (boxed) fo[0] = (unsigned)fa;
		asm volatile("" : "+v"(bo[0]), "+v"(fo[0]));
	}
	const int bcell = SHARE ? (int)bo[0] : ba, fcell = SHARE ? (int)fo[0] : fa;
	// per field one own value per thread and one shell value per thread of the first 488; two boxes alternate so that one barrier per field suffices
	__shared__ float s_box[2][kBox];
	if constexpr (Q4) {
		__shared__ v4f32 s_box4[kBox];
		const v4i rq = field_rsrc(P.q4, bytes1 * 4u);  // element = 16 bytes: byte offset = 4 x the float-field byte offset
		const v4f32 phiOrig = hns_buffer_load_v4f32(rq, (int)(own << 2), 0, 0);
		s_box4[ob] = phiOrig;
		if (n < kBoxShell) s_box4[hcell] = hns_buffer_load_v4f32(rq, (int)(ho << 2), 0, 0);
		v4f32 phiF = {0.0f, 0.0f, 0.0f, 0.0f}, phiB = {0.0f, 0.0f, 0.0f, 0.0f};
		if (!bboxed) {
			v4f32 c[8];
#pragma unroll
			for (int q = 0; q < 8; ++q) c[q] = hns_buffer_load_v4f32(rq, (int)(bo[q] << 2), 0, 0);
#pragma unroll
			for (int q = 0; q < 8; ++q) phiF = __builtin_elementwise_fma(c[q], v4f32{bw[q], bw[q], bw[q], bw[q]}, phiF);
		}
		if (!boxed) {
			v4f32 c[8];
#pragma unroll
			for (int q = 0; q < 8; ++q) c[q] = hns_buffer_load_v4f32(rq, (int)(fo[q] << 2), 0, 0);
#pragma unroll
			for (int q = 0; q < 8; ++q) phiB = __builtin_elementwise_fma(c[q], v4f32{fw[q], fw[q], fw[q], fw[q]}, phiB);
		}
		__syncthreads();
		if (bboxed) {
#pragma unroll
			for (int q = 0; q < 8; ++q) phiF = __builtin_elementwise_fma(s_box4[bcell + box_corner(q)], v4f32{bw[q], bw[q], bw[q], bw[q]}, phiF);
		}
		if (boxed) {
#pragma unroll
			for (int q = 0; q < 8; ++q) phiB = __builtin_elementwise_fma(s_box4[fcell + box_corner(q)], v4f32{fw[q], fw[q], fw[q], fw[q]}, phiB);
		}
		v4f32 nv[6];
#pragma unroll
		for (int d = 0; d < 6; ++d) nv[d] = s_box4[ob + box_nbr(d)];
		const v4f32 r = bfecc_limit(phiOrig, nv, phiF, __builtin_elementwise_fma(v4f32{0.5f, 0.5f, 0.5f, 0.5f}, phiOrig - phiB, phiF));
		P.q4_out[0][idx] = r.x, P.q4_out[1][idx] = r.y, P.q4_out[2][idx] = r.z, P.q4_out[3][idx] = r.w;
	}
	for (int s = 0; s < P.n; ++s) {
		const v4i rf = field_rsrc(P.in[s], bytes1);
		float* box = s_box[s & 1];
		const float phiOrig = lds1(rf, own);
		box[ob] = phiOrig;
		if (n < kBoxShell) box[hcell] = lds1(rf, ho);
		float vb[8], vf8[8];  // corner q and q+4 of the interpolation order differ only in z
		if (!bboxed) {
#pragma unroll
			for (int q = 0; q < 4; ++q) ld_zpair(rf, bo[q], bo[q + 4], vb[q], vb[q + 4]);
		}
		if (!boxed) {
#pragma unroll
			for (int q = 0; q < 4; ++q) ld_zpair(rf, fo[q], fo[q + 4], vf8[q], vf8[q + 4]);
		}
		float phiF = 0.0f, phiB = 0.0f;
		__syncthreads();
		if (bboxed) {
#pragma unroll
			for (int q = 0; q < 8; ++q) vb[q] = box[bcell + box_corner(q)];
		}
#pragma unroll
		for (int q = 0; q < 8; ++q) phiF = __fmaf_rn(vb[q], bw[q], phiF);
		if (boxed) {
#pragma unroll
			for (int q = 0; q < 8; ++q) vf8[q] = box[fcell + box_corner(q)];
		}
#pragma unroll
		for (int q = 0; q < 8; ++q) phiB = __fmaf_rn(vf8[q], fw[q], phiB);
		float nv[6];
#pragma unroll
		for (int d = 0; d < 6; ++d) nv[d] = box[ob + box_nbr(d)];
		P.out[s][idx] = bfecc_limit(phiOrig, nv, phiF, __fmaf_rn(0.5f, phiOrig - phiB, phiF));
	}
	if constexpr (AHEAD) {
		// The rest of advect_vector (k_advect_vector_n from its second pass on) comes LAST and holds no register across the field loop, where the fields' two sets of tap
		// offsets and weights held across the vector half cost sixteen. The voxel's own velocity and its back position are formed again from the box.
		__syncthreads();  // velocity box complete (with no field the loop above held no barrier)
		int m = n;
		asm volatile("" : "+v"(m));  // (the voxel's position and box cell are formed again here, not kept in registers from the top of the kernel)
		const int obv = box_own<kVX, kVY>(m);
		const int3 w = voxel_ijk(C.org, m);
		const f3 vo = box_f3(s_vbox, obv);
		const f3 wf = f3{s_wf[m], s_wf[m + 512], s_wf[m + 1024]};
		const float cx = (float)w.x - scaled_dt * vo.x, cy = (float)w.y - scaled_dt * vo.y, cz = (float)w.z - scaled_dt * vo.z;  // backPos (Kernel.cu:374)
		const f3 wb = sample_velocity(gk, C, ru, s_vbox, cx + scaled_dt * wf.x, cy + scaled_dt * wf.y, cz + scaled_dt * wf.z);  // Kernel.cu:387
		st3(adv_out, idx, bfecc_limit_v(vo, wf, wb, [&](int d) { return box_f3(s_vbox, obv + box_nbr<kVX, kVY>(d)); }));
	}
}

// Two templates of ONE name, as k_advect_vector_n: <Q4, AHEAD> without a collision field, under the symbols the resource tests pin, and <Q4, false, true> below, which takes the SDF.
// LDS of the look-ahead form: the tables, the velocity box, advect_vector's first sample and two float boxes. Four workgroups per CU (eight waves per SIMD, at 64 registers) need a
// quarter of gfx950's 160 KB each. (the q4 form: at least six waves, the float-only form at least four, as before)
constexpr int kLookaheadLds = (int)sizeof(NarrowTabs) + (kVBox + 3 * 512 + 2 * kBox) * 4;
static_assert(kLookaheadLds <= 160 * 1024 / 4, "k_advect_scalars_n<false, true>: four workgroups per CU no longer fit the LDS");
template <bool Q4, bool AHEAD = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(AHEAD ? 8 : (Q4 ? 6 : 4), 8))) void k_advect_scalars_n(const GridDev g, const float* __restrict__ u, const ScalarPtrs P, const float scaled_dt,
                                                                                                            float* __restrict__ adv_out) {
	advect_scalars_n<Q4, AHEAD, false>(g, u, P, scaled_dt, adv_out, nullptr);
}
// LDS of the q4 form with a collider: the tables, the velocity box, two float boxes, the 16-byte box, the SDF box and the back positions. Three workgroups per CU (six waves per SIMD) need a
// third of gfx950's 160 KB each.
constexpr int kScalarsQ4CollLds = (int)sizeof(NarrowTabs) + (3 * kBox + 2 * kBox + 4 * kBox + kBox + 3 * 512) * 4;
static_assert(kScalarsQ4CollLds <= 160 * 1024 / 3, "k_advect_scalars_n<true, false, true>: three workgroups per CU no longer fit the LDS");
template <bool Q4, bool AHEAD, bool COLL>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(Q4 ? 6 : 4))) void k_advect_scalars_n(const GridDev g, const float* __restrict__ u, const ScalarPtrs P, const float* __restrict__ sdf,
                                                                                                   const float scaled_dt) {
	static_assert(COLL && !AHEAD, "without a collision field: the kernel of the same name that takes no SDF");
	advect_scalars_n<Q4, false, true>(g, u, P, scaled_dt, nullptr, sdf);
}

template <bool COLL>
__global__ __launch_bounds__(512) void k_advect_scalars(const GridDev g, const float* __restrict__ u, const ScalarPtrs P,
                                                        const float* __restrict__ sdf, const float scaled_dt) {
	__shared__ GenericTabs tabs;
	GenericCtx C(g, tabs);
	C.stage(g);
	const int idx = C.idx;

	const f3 vc = ld3(u, idx);
	float sx = C.px - scaled_dt * vc.x, sy = C.py - scaled_dt * vc.y, sz = C.pz - scaled_dt * vc.z;
	float rx = C.px, ry = C.py, rz = C.pz;
	int bi[8], fi[8];
	float bw[8], fw[8];
#pragma unroll 1
	for (int pass = 0; pass < 2; ++pass) {
		Taps T = make_taps(g, C, sx, sy, sz);
		if (COLL) {  // the back-position test is made twice in the reference (Kernel.cu:142-155); the repeat cannot change the outcome
			if (tri_f_t(sdf, T) < 0.0f) {
				sx = rx, sy = ry, sz = rz;
				T = make_taps(g, C, sx, sy, sz);
			}
		}
		if (pass == 0) {
			interp_from_taps(T, g.oob, bi, bw);
			f3 vf = {0.0f, 0.0f, 0.0f};
#pragma unroll
			for (int q = 0; q < 8; ++q) add_weighted(vf, ld3(u, bi[q]), bw[q]);
			rx = sx, ry = sy, rz = sz;
			sx = sx + scaled_dt * vf.x, sy = sy + scaled_dt * vf.y, sz = sz + scaled_dt * vf.z;
		} else {
			interp_from_taps(T, g.oob, fi, fw);
		}
	}
	int nb[6];
	nbr6(tabs.base, C.leaf, C.n, nb);
#pragma unroll
	for (int d = 0; d < 6; ++d) nb[d] = nb[d] < 0 ? g.oob : nb[d];
	for (int s = 0; s < P.n; ++s) {
		const float* __restrict__ in = P.in[s];
		const float phiOrig = in[idx];
		float phiF = 0.0f, phiB = 0.0f;
#pragma unroll
		for (int q = 0; q < 8; ++q) {
			phiF = __fmaf_rn(in[bi[q]], bw[q], phiF);
			phiB = __fmaf_rn(in[fi[q]], fw[q], phiB);
		}
		float nv[6];
#pragma unroll
		for (int d = 0; d < 6; ++d) nv[d] = in[nb[d]];
		P.out[s][idx] = bfecc_limit(phiOrig, nv, phiF, __fmaf_rn(0.5f, phiOrig - phiB, phiF));
	}
}

}  // namespace hns

using namespace hns;

// the 32-bit addressed kernels apply while a Vec3f field stays below kNarrowBytes; option "advect" = generic forces the 64-bit ones (A/B, tests)
static bool narrow_fields(const hns_grid* g) {
	return !options().advect_generic.load() && (uint64_t)g->topo.n_leaves * 6144u <= hns::kNarrowBytes;
}

// which of an operator's four kernels a call gets: the generic one with its collision branch, the 32-bit addressed one with its collision branch (advect_vector and
// advect_scalars; option "collide" = generic sends those to the generic one, as before they existed), the 32-bit addressed one, or the generic one.
// A null SDF is a call without a collider whatever has_collision says.
enum class AdvectForm { collision, narrow_collision, narrow, generic };
static AdvectForm advect_form(const hns_grid* g, const float* sdf, int has_collision) {
	if (has_collision && sdf) return narrow_fields(g) && !options().collide_generic.load() ? AdvectForm::narrow_collision : AdvectForm::collision;
	return narrow_fields(g) ? AdvectForm::narrow : AdvectForm::generic;
}
// the source names of the kernels a form launches (hns_sim_substep_plan)
static const char* advect_vector_kernel(AdvectForm f) {
	switch (f) {
	case AdvectForm::collision: return "k_advect_vector<true>";
	case AdvectForm::narrow_collision: return "k_advect_vector_n<coll>";
	case AdvectForm::narrow: return "k_advect_vector_n";
	default: return "k_advect_vector<false>";
	}
}
static const char* advect_scalars_kernel(AdvectForm f) {
	switch (f) {
	case AdvectForm::collision: return "k_advect_scalars<true>";
	case AdvectForm::narrow_collision: return "k_advect_scalars_n<coll>";
	case AdvectForm::narrow: return "k_advect_scalars_n";
	default: return "k_advect_scalars<false>";
	}
}

// The launch tables of the advect_scalars kernels in the 32-bit form: leaves backwards. The gradient kernel has just written the velocity front to back; starting on its
// cached tail also leaves the head cached for the next substep's advect_vector (256^3: -1 % here, -4 % there).
static GridDev reversed(const hns_grid* g) {
	GridDev gd = g->dev();
	gd.rev = 1;
	return gd;
}

// n float fields (at most HNS_MAX_SCALARS) and no q4 element; returns the first field with a null pointer, -1 if none
static int fill_scalar_ptrs(ScalarPtrs& P, const float* const* in, float* const* out, int n) {
	int bad = -1;
	P.n = n;
	P.q4 = nullptr, P.q4_out[0] = P.q4_out[1] = P.q4_out[2] = P.q4_out[3] = nullptr;
	for (int s = 0; s < HNS_MAX_SCALARS; ++s) {
		P.in[s] = s < n ? in[s] : nullptr;
		P.out[s] = s < n ? out[s] : nullptr;
		if (s < n && (!P.in[s] || !P.out[s]) && bad < 0) bad = s;
	}
	return bad;
}

extern "C" {

int hns_dev_advect_vector(hns_grid* g, const float* vel3, float* out3, const float* sdf, int has_collision, float dt, float inv_dx, void* stream) {
	if (int rc = check_grid(g, "hns_dev_advect_vector")) return rc;
	NULLCHK(!vel3 || !out3, "hns_dev_advect_vector");
	const size_t vec_bytes = sizeof(float) * 1536 * (size_t)g->topo.n_leaves;
	if (ranges_overlap(vel3, vec_bytes, out3, vec_bytes)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dev_advect_vector: output must not alias input (out3 overlaps vel3)");
	if (g->n_active == 0) return HNS_OK;
	const float scaled_dt = dt * inv_dx;  // Kernel.cu:361
	const dim3 grid((unsigned)g->n_active), block(512);
	switch (advect_form(g, sdf, has_collision)) {
	case AdvectForm::collision: hipLaunchKernelGGL(k_advect_vector<true>, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, out3, sdf, scaled_dt, inv_dx); break;
	// (k_advect_vector_n is overloaded: <true> names the template with the SDF, the bare name two lines on the kernel without -- see at their definitions)
	case AdvectForm::narrow_collision: hipLaunchKernelGGL(k_advect_vector_n<true>, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, out3, sdf, scaled_dt, inv_dx); break;
	case AdvectForm::narrow: hipLaunchKernelGGL(k_advect_vector_n, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, out3, scaled_dt); break;
	case AdvectForm::generic: hipLaunchKernelGGL(k_advect_vector<false>, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, out3, sdf, scaled_dt, inv_dx); break;
	}
	return launch_status("hns_dev_advect_vector");
}

int hns_dev_advect_scalar(hns_grid* g, const float* vel3, const float* in, float* out, const float* sdf, int has_collision, float dt, float inv_dx,
                          void* stream) {
	if (int rc = check_grid(g, "hns_dev_advect_scalar")) return rc;
	NULLCHK(!vel3 || !in || !out, "hns_dev_advect_scalar");
	if (g->n_active == 0) return HNS_OK;
	const float scaled_dt = dt * inv_dx;
	const dim3 grid((unsigned)g->n_active), block(512);
	switch (advect_form(g, sdf, has_collision)) {
	case AdvectForm::narrow_collision:  // (no operator of the reference hands this kernel a collider: it keeps the generic form)
	case AdvectForm::collision: hipLaunchKernelGGL(k_advect_scalar<true>, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, in, out, sdf, scaled_dt); break;
	case AdvectForm::narrow: hipLaunchKernelGGL(k_advect_scalar_n, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, in, out, scaled_dt); break;
	case AdvectForm::generic: hipLaunchKernelGGL(k_advect_scalar<false>, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, in, out, sdf, scaled_dt); break;
	}
	return launch_status("hns_dev_advect_scalar");
}

int hns_dev_advect_scalars(hns_grid* g, const float* vel3, const float* const* in, float* const* out, int n, const float* sdf, int has_collision,
                           float dt, float inv_dx, void* stream) {
	if (int rc = check_grid(g, "hns_dev_advect_scalars")) return rc;
	NULLCHK(!vel3 || (n > 0 && (!in || !out)), "hns_dev_advect_scalars");
	if (g->n_active == 0 || n <= 0) return HNS_OK;
	const float scaled_dt = dt * inv_dx;
	const dim3 grid((unsigned)g->n_active), block(512);
	// the backtrace does not depend on the fields, so splitting S fields over several launches changes nothing numerically
	for (int base = 0; base < n; base += HNS_MAX_SCALARS) {
		ScalarPtrs P;
		const int bad = fill_scalar_ptrs(P, in + base, out + base, n - base < HNS_MAX_SCALARS ? n - base : HNS_MAX_SCALARS);
		if (bad >= 0) {
			set_error("hns_dev_advect_scalars: null device pointer for field %d", base + bad);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		switch (advect_form(g, sdf, has_collision)) {
		case AdvectForm::collision: hipLaunchKernelGGL(k_advect_scalars<true>, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, P, sdf, scaled_dt); break;
		// (k_advect_scalars_n is overloaded by its template arity: three flags name the form with the SDF, one or two the form without -- see at their definitions)
		case AdvectForm::narrow_collision: hipLaunchKernelGGL((k_advect_scalars_n<false, false, true>), grid, block, 0, (hipStream_t)stream, reversed(g), vel3, P, sdf, scaled_dt); break;
		case AdvectForm::narrow: hipLaunchKernelGGL(k_advect_scalars_n<false>, grid, block, 0, (hipStream_t)stream, reversed(g), vel3, P, scaled_dt, (float*)nullptr); break;
		case AdvectForm::generic: hipLaunchKernelGGL(k_advect_scalars<false>, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, P, sdf, scaled_dt); break;
		}
	}
	return launch_status("hns_dev_advect_scalars");
}

// advect_scalar over n fields with one back-trace per launch of up to HNS_MAX_SCALARS fields (k_advect_scalar_multi_n); with a collision field or 64-bit addressing one
// k_advect_scalar launch per field. Either way output i is bit-identical to hns_dev_advect_scalar of field i.
int hns_dev_advect_scalar_multi(hns_grid* g, const float* vel3, const float* const* in, float* const* out, int n, const float* sdf, int has_collision, float dt, float inv_dx,
                                void* stream) {
	if (int rc = check_grid(g, "hns_dev_advect_scalar_multi")) return rc;
	NULLCHK(!vel3 || (n > 0 && (!in || !out)), "hns_dev_advect_scalar_multi");
	// every refusal before the first launch: a field the kernel reads while a workgroup of the same call writes it has no defined result
	const size_t field_bytes = sizeof(float) * 512 * (size_t)g->topo.n_leaves;
	for (int i = 0; i < n; ++i) {
		if (!in[i] || !out[i]) {
			set_error("hns_dev_advect_scalar_multi: null device pointer for field %d", i);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		if (ranges_overlap(out[i], field_bytes, vel3, 3 * field_bytes)) {
			set_error("hns_dev_advect_scalar_multi: output of field %d aliases the velocity", i);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		for (int j = 0; j < n; ++j) {
			if (ranges_overlap(out[i], field_bytes, in[j], field_bytes)) {
				set_error("hns_dev_advect_scalar_multi: output of field %d aliases the input of field %d", i, j);
				return HNS_ERR_INVALID_ARGUMENT;
			}
			if (j < i && ranges_overlap(out[i], field_bytes, out[j], field_bytes)) {
				set_error("hns_dev_advect_scalar_multi: output of field %d is the output of field %d", i, j);
				return HNS_ERR_INVALID_ARGUMENT;
			}
		}
	}
	if (g->n_active == 0 || n <= 0) return HNS_OK;
	const float scaled_dt = dt * inv_dx;
	const dim3 grid((unsigned)g->n_active), block(512);
	const AdvectForm form = advect_form(g, sdf, has_collision);
	if (form == AdvectForm::narrow) {
		// the back-trace does not depend on the fields, so splitting them over several launches changes nothing numerically
		// A lone field (n = 1, or the ninth of nine) has nothing to share and goes to k_advect_scalar_n, which interleaves the field's first sample with the velocity
		// gathers: the multi-field kernel with one field measured 10-18 % slower than it at 256^3 (profiles/advect_multi_ab.txt, 1). The same bits either way.
		for (int base = 0; base < n; base += HNS_MAX_SCALARS) {
			const int m = n - base < HNS_MAX_SCALARS ? n - base : HNS_MAX_SCALARS;
			if (m == 1) {
				hipLaunchKernelGGL(k_advect_scalar_n, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, in[base], out[base], scaled_dt);
				continue;
			}
			ScalarPtrs P;
			fill_scalar_ptrs(P, in + base, out + base, m);
			hipLaunchKernelGGL(k_advect_scalar_multi_n, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, P, scaled_dt);
		}
	} else {
		for (int i = 0; i < n; ++i) {
			if (form == AdvectForm::collision || form == AdvectForm::narrow_collision)  // (as hns_dev_advect_scalar)
				hipLaunchKernelGGL(k_advect_scalar<true>, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, in[i], out[i], sdf, scaled_dt);
			else
				hipLaunchKernelGGL(k_advect_scalar<false>, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, in[i], out[i], sdf, scaled_dt);
		}
	}
	return launch_status("hns_dev_advect_scalar_multi");
}

// can this grid take the look-ahead launch (hns_dev_advect_scalars_ahead)?
bool hns_advect_ahead_ok(const hns_grid* g) { return narrow_fields(g); }

// advect_scalars over n float fields (at most HNS_MAX_SCALARS, no collision field) AND advect_vector of the same velocity into adv_out3, one launch (k_advect_scalars_n<false, true>).
// Every output is bit-identical to hns_dev_advect_scalars followed by hns_dev_advect_vector with the same arguments. Applies where the 32-bit addressed kernels do.
int hns_dev_advect_scalars_ahead(hns_grid* g, const float* vel3, const float* const* in, float* const* out, int n, float* adv_out3, float dt, float inv_dx, void* stream) {
	if (int rc = check_grid(g, "hns_dev_advect_scalars_ahead")) return rc;
	NULLCHK(!vel3 || !adv_out3 || (n > 0 && (!in || !out)), "hns_dev_advect_scalars_ahead");
	const size_t vec_bytes = sizeof(float) * 1536 * (size_t)g->topo.n_leaves;
	if (ranges_overlap(vel3, vec_bytes, adv_out3, vec_bytes)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dev_advect_scalars_ahead: adv_out3 must not alias vel3");
	if (n < 0 || n > HNS_MAX_SCALARS) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dev_advect_scalars_ahead: between 0 and 8 fields");
	if (!narrow_fields(g)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dev_advect_scalars_ahead: grid too large for 32-bit offsets (or option advect = generic)");
	if (g->n_active == 0) return HNS_OK;
	ScalarPtrs P;
	const int bad = fill_scalar_ptrs(P, in, out, n);
	if (bad >= 0) {
		set_error("hns_dev_advect_scalars_ahead: null device pointer for field %d", bad);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	hipLaunchKernelGGL((k_advect_scalars_n<false, true>), dim3((unsigned)g->n_active), dim3(512), 0, (hipStream_t)stream, reversed(g), vel3, P, dt * inv_dx, adv_out3);
	return launch_status("hns_dev_advect_scalars_ahead");
}

// advect_scalars over the four fields of `q4` (one 16-byte element per voxel in, four float arrays out) and n more float fields, one launch (hns_sim_substep). sdf: the
// collision field, null = none. Applies where hns_advect_q4_ok(g).
int hns_advect_scalars_q4(hns_grid* g, const float* vel3, const float* q4, float* const* q4_out, const float* const* in, float* const* out, int n, const float* sdf, float dt,
                          float inv_dx, void* stream) {
	if (int rc = check_grid(g, "hns_advect_scalars_q4")) return rc;
	NULLCHK(!vel3 || !q4 || !q4_out || (n > 0 && (!in || !out)), "hns_advect_scalars_q4");
	if (!hns_advect_q4_ok(g) || n > HNS_MAX_SCALARS) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_advect_scalars_q4: grid too large for 32-bit offsets, or too many fields");
	if (g->n_active == 0) return HNS_OK;
	for (int c = 0; c < 4; ++c) NULLCHK(!q4_out[c], "hns_advect_scalars_q4");
	ScalarPtrs P;
	NULLCHK(fill_scalar_ptrs(P, in, out, n) >= 0, "hns_advect_scalars_q4");
	P.q4 = q4;
	for (int c = 0; c < 4; ++c) P.q4_out[c] = q4_out[c];
	if (sdf)
		hipLaunchKernelGGL((k_advect_scalars_n<true, false, true>), dim3((unsigned)g->n_active), dim3(512), 0, (hipStream_t)stream, reversed(g), vel3, P, sdf, dt * inv_dx);
	else
		hipLaunchKernelGGL(k_advect_scalars_n<true>, dim3((unsigned)g->n_active), dim3(512), 0, (hipStream_t)stream, reversed(g), vel3, P, dt * inv_dx, (float*)nullptr);
	return launch_status("hns_advect_scalars_q4");
}
const char* hns_advect_scalars_q4_kernel(const float* sdf) { return sdf ? "k_advect_scalars_n<q4,coll>" : "k_advect_scalars_n<q4>"; }

// the kernels hns_dev_advect_vector / hns_dev_advect_scalars / hns_dev_advect_scalars_ahead launch for these arguments (hns_sim_substep_plan)
const char* hns_advect_vector_kernel(const hns_grid* g, const float* sdf, int has_collision) { return advect_vector_kernel(advect_form(g, sdf, has_collision)); }
const char* hns_advect_scalars_kernel(const hns_grid* g, const float* sdf, int has_collision) { return advect_scalars_kernel(advect_form(g, sdf, has_collision)); }
const char* hns_advect_scalars_ahead_kernel(void) { return "k_advect_scalars_n<ahead>"; }

// can this grid's fields take the q4 path (32-bit byte offsets into a 16-byte-per-voxel array)?
bool hns_advect_q4_ok(const hns_grid* g) { return narrow_fields(g) && (uint64_t)g->topo.n_leaves * 8192u <= hns::kNarrowBytes; }

}  // extern "C"
