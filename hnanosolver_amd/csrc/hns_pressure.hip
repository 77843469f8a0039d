// hns_pressure.hip -- divergence, red-black SOR (all forms) and pressure-gradient subtraction: hand-written HIP for gfx950 / CDNA4; and hns_sim_solve, the one driver of a sim's solve.
//
// One 8^3 leaf per workgroup; wave64. All arithmetic is float32 and keeps the association of the reference kernels
// (reference src/Cuda/Kernel.cu) so that results are reproducible against oracle/hns_oracle.c; build with
// -ffp-contract=off: the only fused multiply-adds are the explicit __fmaf_rn() calls, which sit where the reference
// itself calls __fmaf_rn / fmaf (Kernel.cu:241-247, Stencils.hpp:20-22,131-135).
//
// Differences in mechanism (not in arithmetic) from the reference:
//   * no per-voxel coordinate stream: a voxel's coordinate is leaf origin + thread id (saves 12 B/voxel/kernel);
//   * no NanoVDB tree walk: a tap resolves its leaf through the 27-entry neighbour table of the workgroup's leaf
//     (staged in LDS) or, beyond one leaf away, an origin hash;
//   * velocity is Vec3f AoS on the device (the host layout): one 12-byte access per tap, and every
//     2 KB leaf payload is one fully coalesced run;
//   * the red-black SOR loop runs ONE launch per iteration: a wave stages its leaves plus a two-voxel halo of
//     p in LDS, recomputes the red updates of the face-adjacent halo voxels itself (bit-identical to what the
//     neighbouring wave computes), then does black, ping-ponging p_in -> p_out. 12 B/voxel/iteration of HBM
//     traffic instead of the >=16 B of two in-place launches.
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

#include "hns_device.hpp"
#include "hns_flags.hpp"

namespace hns {

// ---------------------------------------------------------------------------------------------------------------
// divergence (reference Kernel.cu:499-519 and :455-496)
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(512) void k_divergence(const GridDev g, const float* __restrict__ u, float* __restrict__ div, const float inv_dx) {
	__shared__ int s_nbr[27];
	const LeafCtx L = stage_leaf(g, s_nbr, blockIdx.x);
	const int n = threadIdx.x;
	const int idx = L.leaf * 512 + n;
	const f3 c = ld3(u, idx);
	const float uxp = nbr_val3<0, 1, 0>(u, s_nbr, L.leaf, n), uxm = nbr_val3<0, -1, 0>(u, s_nbr, L.leaf, n);
	const float uyp = nbr_val3<1, 1, 1>(u, s_nbr, L.leaf, n), uym = nbr_val3<1, -1, 1>(u, s_nbr, L.leaf, n);
	const float uzp = nbr_val3<2, 1, 2>(u, s_nbr, L.leaf, n), uzm = nbr_val3<2, -1, 2>(u, s_nbr, L.leaf, n);
	div[idx] = divergence_of(c, uxp, uxm, uyp, uym, uzp, uzm, inv_dx);
}

// ---------------------------------------------------------------------------------------------------------------
// red-black SOR, two-launch form: one colour in place (reference Kernel.cu:591-623 / :521-588)
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_rbgs_color(const GridDev g, const float* __restrict__ div, float* p, const float dx2, const float omega,
                                                    const int color) {
	__shared__ int s_nbr[27];
	color_sweep<false>(g, s_nbr, nullptr, div, p, dx2, omega, color);  // (hns_device.hpp)
}

// ---------------------------------------------------------------------------------------------------------------
// subtractPressureGradient (reference Kernel.cu:765-829 / :694-762)
// ---------------------------------------------------------------------------------------------------------------

template <bool COLL>
__global__ __launch_bounds__(512) void k_subtract_gradient(const GridDev g, const float* u, const float* __restrict__ p, float* out,
                                                           const float* __restrict__ sdf, const float inv_dx) {
	__shared__ int s_nbr[27];
	const LeafCtx L = stage_leaf(g, s_nbr, blockIdx.x);
	const int n = threadIdx.x;
	const int idx = L.leaf * 512 + n;
	const float gx = central_gradient(nbr_val<0, 1>(p, s_nbr, L.leaf, n), nbr_val<0, -1>(p, s_nbr, L.leaf, n), inv_dx);
	const float gy = central_gradient(nbr_val<1, 1>(p, s_nbr, L.leaf, n), nbr_val<1, -1>(p, s_nbr, L.leaf, n), inv_dx);
	const float gz = central_gradient(nbr_val<2, 1>(p, s_nbr, L.leaf, n), nbr_val<2, -1>(p, s_nbr, L.leaf, n), inv_dx);
	const f3 us = ld3(u, idx);  // `out` may alias `u`: each voxel reads only its own velocity (PressureProjection.cu:64)
	f3 r = {us.x - gx, us.y - gy, us.z - gz};
	if (COLL) {  // Kernel.cu:809-826
		const float sv = sdf[idx];
		if (sv < 0.0f) {
			r.x = r.y = r.z = 0.0f;
		} else if (sv < 0.1f) {
			const int ci = L.org.x + (n >> 6), cj = L.org.y + ((n >> 3) & 7), ck = L.org.z + (n & 7);
			const f3 nrm = sdf_normal(g, s_nbr, L.org, sdf, ci, cj, ck, inv_dx);
			r = no_slip_blend(r, nrm, 1.0f - (sv / 0.1f));
		}
	}
	st3(out, idx, r);
}

// Streaming form (no collision field): one wave per leaf. The pressure of the leaf and of the six touching face layers is
// staged in LDS (own values: two 16-byte loads per lane; a face layer: one value per lane); the velocity then streams
// through as 384 fully coalesced 16-byte chunks per leaf, each float subtracting the gradient component it belongs to
// (float f of the leaf: voxel f / 3, component f % 3, taps along that axis only). Same expression per component:
// central_gradient (hns_device.hpp). The 512-thread form issues ~12 load/store instructions per wave of 64 voxels, mostly
// 12-byte and scattered 4-byte accesses; this one issues 20 per 512 voxels.
// M = NoMirror, or PhaseMirror for a chained multi-GPU rank (hns_flags.hpp): the boundary leaves' new velocity also goes, whole
// leaves, into the peers' ghost copies
template <class M>
__global__ __launch_bounds__(64) void k_subtract_gradient_s(const GridDev g, const float* u, const float* __restrict__ p, float* out, const float inv_dx, const M m) {
	__shared__ __attribute__((aligned(16))) float P[kTile];
	const int l = threadIdx.x;
	const int* __restrict__ rec = g.blk + (size_t)launch_pos(g, blockIdx.x) * 28;
	const int leaf = __builtin_amdgcn_readfirstlane(rec[0]);
	chain_begin(m, leaf);
	stage_tile_wave(P, p, rec, leaf, l);
	__syncthreads();
	const float4* src = reinterpret_cast<const float4*>(u + (size_t)leaf * 1536);
	float4* dst = reinterpret_cast<float4*>(out + (size_t)leaf * 1536);
	float4 a[6];
#pragma unroll
	for (int j = 0; j < 6; ++j) a[j] = src[l + 64 * j];
#pragma unroll
	for (int j = 0; j < 6; ++j) {
		float r[4] = {a[j].x, a[j].y, a[j].z, a[j].w};
#pragma unroll
		for (int e = 0; e < 4; ++e) {
			const int f = 4 * (l + 64 * j) + e;
			const int v = __mul24(f, 683) >> 11;  // f / 3 for f < 1536
			const int comp = f - 3 * v;
			const int shift = comp == 0 ? 6 : (comp == 1 ? 3 : 0);
			const int c = (v >> shift) & 7;
			const int x = v >> 6, y = (v >> 3) & 7, z = v & 7;
			const int ab = comp == 0 ? ((y << 3) | z) : (comp == 1 ? ((x << 3) | z) : ((x << 3) | y));
			const int plus = c != 7 ? v + (1 << shift) : 512 + 64 * (2 * comp + 1) + ab;
			const int minus = c != 0 ? v - (1 << shift) : 512 + 64 * (2 * comp) + ab;
			r[e] = r[e] - central_gradient(P[plus], P[minus], inv_dx);
		}
		dst[l + 64 * j] = make_float4(r[0], r[1], r[2], r[3]);
		chain_store_leaf16<3>(m, 0, leaf, 4 * (l + 64 * j), make_float4(r[0], r[1], r[2], r[3]));
	}
	chain_end(m, leaf);
}

// ---------------------------------------------------------------------------------------------------------------
// divergence, one wave per leaf (the production form)
// ---------------------------------------------------------------------------------------------------------------
//
// Same idea as the SOR kernels: lane = x*8+y owns a z-row, the row is read and written as 16-byte accesses (a Vec3f row
// is 96 contiguous bytes, a float row 32), lateral neighbours travel through a wave-private LDS tile, the +-z neighbours
// are in the lane's own registers. The 512-thread forms above issue 7-8 scalar taps per voxel and are bound by the
// texture addresser (one L1 access per 4 lanes per instruction); these issue ~1/5 of the accesses.

#define RT_ROW(xp, yp) (((xp) + 1) * 10 + ((yp) + 1))  // rows (x',y') in [-1,8]^2

struct RowTile {
	float4 lo[100], hi[100];
};
__device__ __forceinline__ void rt_put(RowTile& T, int R, const float (&v)[8]) {
	T.lo[R] = make_float4(v[0], v[1], v[2], v[3]);
	T.hi[R] = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void unpack8(const float4 a, const float4 b, float (&v)[8]) { v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w; }
__device__ __forceinline__ void rt_get(const RowTile& T, int R, float (&v)[8]) { unpack8(T.lo[R], T.hi[R], v); }
// the 24 floats of Vec3f row `row` of leaf `leaf` (zeros when the leaf is absent)
__device__ __forceinline__ void glb_row3(const float* u, int leaf, int row, float (&r)[24]) {
	const float4* q = reinterpret_cast<const float4*>(u + ((size_t)(leaf < 0 ? 0 : leaf) * 512 + row * 8) * 3);
	const bool ok = leaf >= 0;
#pragma unroll
	for (int k = 0; k < 6; ++k) {
		const float4 v = q[k];
		r[4 * k] = ok ? v.x : 0.0f, r[4 * k + 1] = ok ? v.y : 0.0f, r[4 * k + 2] = ok ? v.z : 0.0f, r[4 * k + 3] = ok ? v.w : 0.0f;
	}
}

// face-row duty of lane l < 32: face f = l>>3 (-x,+x,-y,+y), row i = l&7 -> neighbour slot, source row, tile row
__device__ __forceinline__ void face_duty(int l, int& slot, int& src, int& R) {
	const int f = (l >> 3) & 3, i = l & 7;
	slot = f == 0 ? 4 : (f == 1 ? 22 : (f == 2 ? 10 : 16));
	src = f == 0 ? 56 + i : (f == 1 ? i : (f == 2 ? i * 8 + 7 : i * 8));
	R = f == 0 ? RT_ROW(-1, i) : (f == 1 ? RT_ROW(8, i) : (f == 2 ? RT_ROW(i, -1) : RT_ROW(i, 8)));
}

// What hns_sim_substep fuses into the divergence launch (round 6; reference HNanoSolver.cu:181-234 runs three launches: divergence, combustion_oxygen, temperature_buoyancy).
// The lane that owns a z-row of the leaf has its eight divergences and its eight velocities in registers: it also burns the row's eight voxels
// (combustion_oxygen, Kernel.cu:923-966: div += burn * expansion), writes {fuel, waste, temperature, flame} as ONE 16-byte element per voxel (`q4`: what
// k_advect_scalars_n<true> gathers its taps from, hns_advect.hip) and the velocity with the buoyancy of the NEW temperature (temperature_buoyancy, Kernel.cu:831-847)
// into a second buffer -- the neighbours' divergences still read the un-buoyed u*. 60 B/voxel in one pass instead of 16 + 40 + 28 in three.
struct NoFuse {};
struct CombustFuse {
	const float* fuel;
	const float* waste;
	const float* temp;
	const float* flame;
	float4* q4;    // out: {fuel, waste, temperature, flame} after combustion, one element per voxel
	float* u_out;  // out: u* + buoyancy
	float temp_gain, expansion, dt, ambient, strength;
};
__device__ __forceinline__ void ld_row8(const float* f, size_t at, float (&v)[8]) {
	const float4* q = reinterpret_cast<const float4*>(f + at);
	unpack8(q[0], q[1], v);
}

// The row kernels: divergence (reference Kernel.cu:499-519; hns_device.hpp: divergence_of) with three switches, put together from the pieces below by divergence_rows.
// COAL (round 4; grids of 16k leaves and more, hns_dev_divergence): the leaf's own 6 KB are fetched in memory order -- lane l takes the
// 16-byte pieces l, 64 + l, ... so that an instruction touches 8 whole cache lines instead of a piece of each of the 48 -- and handed to
// the row owners through LDS (the wave's own 6 KB; one wave per workgroup, so only the wave's LDS order matters). Round 3 measured it
// (64.1 -> 62.9 us at 256^3, 133 -> 123 on the 66k-leaf plume, but 11.8 -> 13.4 at 128^3: 12.6 KB of LDS per wave halve the waves in
// flight where the grid is small) and dropped it; it is now switched by size instead.
// ZP (round 6, VERDICT r5 task 5): TWO waves per workgroup on the z-adjacent leaves 2q and 2q + 1 of the launch range (leaf order is z-fastest: on a box every such pair
// shares a z face); each hands the other the layer of u.z the other would gather -- 64 floats 96 bytes apart, every lane on a cache line of its own -- through LDS. The
// pair is checked against the neighbour table: leaves that are not z neighbours gather as before.
// F = CombustFuse: combustion and buoyancy of the row's voxels in the same launch (above).

// The LDS of one wave. `in`: the tiles of u.x / u.y rows its lanes read their lateral neighbours from and, COAL, the buffer that hands memory-order pieces to the lanes that
// own them (the own rows, then the four faces). `out` (FUSE) lies over it once the divergence has been read out of the tiles: the out-going q4 rows (kQ4Row float4 per
// lane), then the velocity rows (kURow per lane) -- a row's pieces plus one of padding, so that the lanes' rows start on different banks.
template <bool COAL> struct RowIn { RowTile tx, ty; };
template <> struct RowIn<true> { RowTile tx, ty; float4 own[384]; };
constexpr int kQ4Row = 8 + 1, kURow = 6 + 1;
template <bool COAL, bool FUSE> union RowWave { RowIn<COAL> in; float4 out[FUSE ? 64 * kQ4Row : 1]; };

// Leaf selection: the wave's leaf, its record (rec[1 + j] = neighbour j), whether the wave stores, and its z neighbours n_zm / n_zp. One leaf per workgroup: the block's
// launch-order record. ZP: wave wv of the block has leaf 2q + wv of the range; the second wave of an odd range's last pair shadows the first and stores nothing;
// `shared` (wave-uniform): the partner wave has the z neighbour on its side.
struct RowLeaf { const int* __restrict__ rec; int leaf; bool live; int n_zm, n_zp; bool shared; };
template <bool ZP>
__device__ __forceinline__ RowLeaf select_leaf(const GridDev& g, int wv) {
	RowLeaf L{nullptr, 0, true, -1, -1, false};
	if constexpr (ZP) {
		// pair q of the range in the chunked order of hns_device.hpp (one chunk of the pair list per XCD), walked backwards like the one-leaf form
		const int np = (g.n_active + 1) >> 1;
		const unsigned rows = (unsigned)np >> 3, b = blockIdx.x;
		const unsigned pos = (b >> 3) < rows ? (((rows - 1u - (b >> 3)) << 3) | (b & 7u)) : b;
		const int q = sched_leaf((int)pos, np, g.sched_seg > 1 ? g.sched_seg / 2 : 0);
		const int lf = g.first + 2 * q + wv;
		L.live = lf < g.first + g.n_active;
		L.leaf = L.live ? lf : g.first + 2 * q;
		L.rec = g.nbr27 + (size_t)L.leaf * 27 - 1;  // (as in the launch-order records)
	} else {
		L.rec = g.blk + (size_t)launch_pos(g, blockIdx.x) * 28;
		L.leaf = __builtin_amdgcn_readfirstlane(L.rec[0]);
	}
	L.n_zm = __builtin_amdgcn_readfirstlane(L.rec[1 + 12]), L.n_zp = __builtin_amdgcn_readfirstlane(L.rec[1 + 14]);
	if constexpr (ZP) {
		const int last = g.first + g.n_active - 1;
		L.shared = wv == 0 ? (L.leaf + 1 <= last && L.n_zp == L.leaf + 1) : (L.live && L.n_zm == L.leaf - 1);
	}
	return L;
}

// Own-row fetch: r = the 24 floats of lane l's Vec3f row of `leaf`. COAL: the leaf in memory order, through in.own.
template <bool COAL>
__device__ __forceinline__ void fetch_own_row(const float* __restrict__ u, int leaf, int l, RowIn<COAL>& in, float (&r)[24]) {
	if constexpr (COAL) {
		const float4* q = reinterpret_cast<const float4*>(u + (size_t)leaf * 1536);
		float4 v[6];
#pragma unroll
		for (int k = 0; k < 6; ++k) v[k] = q[k * 64 + l];
#pragma unroll
		for (int k = 0; k < 6; ++k) in.own[k * 64 + l] = v[k];
		wave_sync();
#pragma unroll
		for (int k = 0; k < 6; ++k) {
			const float4 w = in.own[l * 6 + k];
			r[4 * k] = w.x, r[4 * k + 1] = w.y, r[4 * k + 2] = w.z, r[4 * k + 3] = w.w;
		}
	} else {
		glb_row3(u, leaf, l, r);
	}
}

// Face fetch: h = the Vec3f row of the neighbouring leaf that lane l < 32 posts into the tiles (face_duty: neighbour `slot`, its row `src`); zeros where that leaf is absent.
// COAL (round 5): the four lateral face layers in memory order too: face f's eight Vec3f rows are 8 x 96 bytes -- one contiguous 768-byte run for the x faces, eight 96-byte
// runs for the y faces -- fetched by 48 lanes, a 16-byte piece each, ONE instruction per face (12-16 L1 accesses) instead of one row per lane (32 lanes x six instructions,
// every lane on a cache line of its own: 192 accesses); handed to the face-row lanes through in.own, which the own rows have left by then. A timing-only build without
// these loads ran 10 us faster at 256^3 (profiles/r05_divergence_face_bounds.txt).
template <bool COAL>
__device__ __forceinline__ void fetch_face_row(const float* __restrict__ u, const int* __restrict__ rec, int l, int slot, int src, RowIn<COAL>& in, float (&h)[24]) {
	if constexpr (COAL) {
		float4 fv[4];
		const int fr = l / 6, fk = l - fr * 6;  // lane -> (row of the face, piece of the row), l < 48
#pragma unroll
		for (int f = 0; f < 4; ++f) {
			const int nf = __builtin_amdgcn_readfirstlane(rec[1 + (f == 0 ? 4 : (f == 1 ? 22 : (f == 2 ? 10 : 16)))]);
			const int srow = f == 0 ? 56 + fr : (f == 1 ? fr : (f == 2 ? fr * 8 + 7 : fr * 8));
			const float4* q = reinterpret_cast<const float4*>(u + ((size_t)(nf < 0 ? 0 : nf) * 512 + srow * 8) * 3) + fk;
			fv[f] = (nf >= 0 && l < 48) ? *q : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		}
		wave_sync();  // (every lane has read its own row out of in.own)
		if (l < 48) {
#pragma unroll
			for (int f = 0; f < 4; ++f) in.own[f * 48 + l] = fv[f];
		}
		wave_sync();
		if (l < 32) {
			const int f = l >> 3, i = l & 7;
#pragma unroll
			for (int k = 0; k < 6; ++k) {
				const float4 w = in.own[f * 48 + i * 6 + k];
				h[4 * k] = w.x, h[4 * k + 1] = w.y, h[4 * k + 2] = w.z, h[4 * k + 3] = w.w;
			}
		}
	} else {
		if (l < 32) glb_row3(u, rec[1 + slot], src, h);
	}
}

// z-layer exchange: uz_m / uz_p = u.z of the voxels below the row's z = 0 / above its z = 7, which lie in the leaves n_zm / n_zp (0 outside the domain). z_gather, before the
// workgroup barrier: the two values from those leaves -- but where `shared` (select_leaf), this wave posts the layer the partner would gather into s_z instead, and
// z_take, behind the barrier, takes the partner's.
template <bool ZP>
__device__ __forceinline__ void z_gather(const float* __restrict__ u, int n_zm, int n_zp, bool shared, int wv, int l, const float (&r)[24], float (*s_z)[ZP ? 64 : 1], float& uz_m,
                                         float& uz_p) {
	uz_m = (n_zm < 0 || (ZP && shared && wv == 1)) ? 0.0f : u[((size_t)n_zm * 512 + l * 8 + 7) * 3 + 2];
	uz_p = (n_zp < 0 || (ZP && shared && wv == 0)) ? 0.0f : u[((size_t)n_zp * 512 + l * 8) * 3 + 2];
	if constexpr (ZP) s_z[wv][l] = wv == 0 ? r[23] : r[2];  // (u.z of the row's z = 7 / z = 0 voxel)
}
template <bool ZP>
__device__ __forceinline__ void z_take(bool shared, int wv, int l, const float (*s_z)[ZP ? 64 : 1], float& uz_m, float& uz_p) {
	if (ZP && shared) (wv == 0 ? uz_p : uz_m) = s_z[1 - wv][l];
}

// The eight divergences of row (x, y): lateral neighbours out of the tiles, +-z neighbours in the lane's own registers and, at the row's ends, uz_m / uz_p
__device__ __forceinline__ void row_divergence(const RowTile& TX, const RowTile& TY, int x, int y, const float (&r)[24], float uz_m, float uz_p, float inv_dx, float (&d)[8]) {
	float xp[8], xm[8], yp[8], ym[8];
	rt_get(TX, RT_ROW(x + 1, y), xp);
	rt_get(TX, RT_ROW(x - 1, y), xm);
	rt_get(TY, RT_ROW(x, y + 1), yp);
	rt_get(TY, RT_ROW(x, y - 1), ym);
#pragma unroll
	for (int z = 0; z < 8; ++z) {
		const float zpv = z < 7 ? r[3 * (z < 7 ? z + 1 : 7) + 2] : uz_p;
		const float zmv = z > 0 ? r[3 * (z > 0 ? z - 1 : 0) + 2] : uz_m;
		d[z] = divergence_of(f3{r[3 * z], r[3 * z + 1], r[3 * z + 2]}, xp[z], xm[z], yp[z], ym[z], zpv, zmv, inv_dx);
	}
}

// The row's four combustion fields (32 contiguous bytes each)
struct FuseRow { float fuel[8], waste[8], temp[8], flame[8]; };

// The fused epilogue of lane l's row: combustion (combust_voxel) into q4_row and d, then buoyancy (buoyancy_voxel) of the temperature combustion has just formed into
// ro. Branch-free: with branches the compiler carries r[] and d[] through them as whole vectors and spills.
__device__ __forceinline__ void fused_epilogue(const CombustFuse& fz, const FuseRow& c, const float (&r)[24], float (&d)[8], float4* q4_row, float (&ro)[24]) {
#pragma unroll
	for (int z = 0; z < 8; ++z) {
		const Burnt b = combust_voxel(c.fuel[z], c.waste[z], c.temp[z], c.flame[z], fz.temp_gain);
		q4_row[z] = make_float4(b.fuel, b.waste, b.temperature, b.flame);
		d[z] = combust_divergence(b, d[z], fz.expansion);
		const f3 v = buoyancy_voxel(f3{r[3 * z], r[3 * z + 1], r[3 * z + 2]}, b.temperature, fz.dt, fz.ambient, fz.strength);
		ro[3 * z] = v.x, ro[3 * z + 1] = v.y, ro[3 * z + 2] = v.z;
	}
}

// A lane's rows leave through LDS in memory order: every lane has put its row of N float4 at stage[l * (N + 1)]; the wave stores the leaf's 64 N pieces l, 64 + l, ... to
// dst -- instead of 16 bytes per lane at a 128 / 96-byte stride (measured at 256^3: 285 us for the launch, more than the three separate launches' 247).
template <int N>
__device__ __forceinline__ void rows_leave(const float4* stage, float4* dst, int l, bool live) {
	static_assert(N == 8 || N == 6, "a q4 row or a Vec3f row");
	wave_sync();
#pragma unroll
	for (int k = 0; k < N; ++k) {
		const int i = k * 64 + l, row = N == 8 ? i >> 3 : __mul24(i, 10923) >> 16;  // i / 6 for i < 384
		if (live) dst[i] = stage[row * (N + 1) + (i - row * N)];
	}
}

template <class M, bool COAL, class F, bool ZP = false>
__device__ __forceinline__ void divergence_rows(const GridDev& g, const float* __restrict__ u, float* __restrict__ div, const float inv_dx, const M& m, const F& fz) {
	constexpr bool FUSE = !std::is_same<F, NoFuse>::value;
	__shared__ __attribute__((aligned(16))) RowWave<COAL, FUSE> s_wave[ZP ? 2 : 1];
	__shared__ float s_z[ZP ? 2 : 1][ZP ? 64 : 1];
	const int wv = ZP ? __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) : 0;
	RowWave<COAL, FUSE>& W = s_wave[wv];
	const int l = threadIdx.x & 63, x = l >> 3, y = l & 7;
	const RowLeaf L = select_leaf<ZP>(g, wv);
	chain_begin(m, L.leaf);
	float r[24], h[24];
	FuseRow c;
	if constexpr (FUSE) {
		const size_t at = (size_t)L.leaf * 512 + l * 8;
		ld_row8(fz.fuel, at, c.fuel), ld_row8(fz.waste, at, c.waste), ld_row8(fz.temp, at, c.temp), ld_row8(fz.flame, at, c.flame);
	}
	fetch_own_row<COAL>(u, L.leaf, l, W.in, r);
	float uz_m, uz_p;
	z_gather<ZP>(u, L.n_zm, L.n_zp, L.shared, wv, l, r, s_z, uz_m, uz_p);
	int slot, src, RF;
	face_duty(l, slot, src, RF);
	fetch_face_row<COAL>(u, L.rec, l, slot, src, W.in, h);
	float ux[8], uy[8];  // the lane's u.x / u.y rows and, l < 32, its face row into the tiles
#pragma unroll
	for (int z = 0; z < 8; ++z) ux[z] = r[3 * z], uy[z] = r[3 * z + 1];
	rt_put(W.in.tx, RT_ROW(x, y), ux);
	rt_put(W.in.ty, RT_ROW(x, y), uy);
	if (l < 32) {
#pragma unroll
		for (int z = 0; z < 8; ++z) ux[z] = l < 16 ? h[3 * z] : h[3 * z + 1];  // x faces carry u.x, y faces u.y
		rt_put(l < 16 ? W.in.tx : W.in.ty, RF, ux);
	}
	__syncthreads();
	z_take<ZP>(L.shared, wv, l, s_z, uz_m, uz_p);
	float d[8];
	row_divergence(W.in.tx, W.in.ty, x, y, r, uz_m, uz_p, inv_dx, d);
	if constexpr (FUSE) {
		float ro[24];
		wave_sync();  // (every lane has read its neighbours' rows out of the tiles: W.out lies over them)
		fused_epilogue(fz, c, r, d, W.out + l * kQ4Row, ro);
		rows_leave<8>(W.out, fz.q4 + (size_t)L.leaf * 512, l, L.live);
		wave_sync();
#pragma unroll
		for (int k = 0; k < 6; ++k) W.out[l * kURow + k] = make_float4(ro[4 * k], ro[4 * k + 1], ro[4 * k + 2], ro[4 * k + 3]);
		rows_leave<6>(W.out, reinterpret_cast<float4*>(fz.u_out + (size_t)L.leaf * 1536), l, L.live);
	}
	const float4 lo = make_float4(d[0], d[1], d[2], d[3]), hi = make_float4(d[4], d[5], d[6], d[7]);
	float4* q = reinterpret_cast<float4*>(div + (size_t)L.leaf * 512 + l * 8);
	if (L.live) q[0] = lo, q[1] = hi;
	chain_store_row(m, 0, L.leaf, l, lo, hi);
	chain_end(m, L.leaf);
}
template <class M, bool COAL = false>
__global__ __launch_bounds__(64) void k_divergence_row(const GridDev g, const float* __restrict__ u, float* __restrict__ div, const float inv_dx, const M m) {
	divergence_rows<M, COAL, NoFuse>(g, u, div, inv_dx, m, NoFuse{});
}
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(3))) void k_divergence_combust_buoyancy_zpair(const GridDev g, const float* __restrict__ u, float* __restrict__ div, const float inv_dx,
                                                                                                                      const CombustFuse fz) {
	divergence_rows<NoMirror, true, CombustFuse, true>(g, u, div, inv_dx, NoMirror{}, fz);
}
template <bool COAL>
__global__ __launch_bounds__(128) void k_divergence_zpair(const GridDev g, const float* __restrict__ u, float* __restrict__ div, const float inv_dx) {
	divergence_rows<NoMirror, COAL, NoFuse, true>(g, u, div, inv_dx, NoMirror{}, NoFuse{});
}
// the fused launch of hns_sim_substep (CombustFuse above). Four waves per SIMD: left alone the scheduler hoists every load and takes 256 registers (one wave per SIMD)
template <bool COAL>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void k_divergence_combust_buoyancy(const GridDev g, const float* __restrict__ u, float* __restrict__ div, const float inv_dx,
                                                                                                               const CombustFuse fz) {
	divergence_rows<NoMirror, COAL, CombustFuse>(g, u, div, inv_dx, NoMirror{}, fz);
}

}  // namespace hns

using namespace hns;

// which divergence kernel a grid gets, alone (hns_dev_divergence) or fused with combustion and buoyancy (hns_divergence_combust_buoyancy, which has no block form)
enum class DivForm { block, zpair, coalesced, row };
static DivForm divergence_form(const hns_grid* g, bool fused) {
	if (!fused && (options().stencil_block.load() || !g->d_blk)) return DivForm::block;  // option "stencil" = block: A/B switch
	// option "divergence" = auto | row | coalesced: by size (k_divergence_row's COAL form from 16k leaves; loses below, see the kernel)
	const int form = options().divergence_form.load();
	// auto, from 16,384 leaves (round 6): z-adjacent leaves in pairs, the coalesced form (256^3 63 -> 58 us, 512^3 467 -> 431, 66k-leaf plume 118 -> 112;
	// below that size the pairing buys nothing and the coalesced form loses to the row form: profiles/r06_divergence_zpair_ab.txt). A range whose boundary leaves
	// are dealt out first (a chained multi-GPU rank) keeps one leaf per workgroup.
	if ((form == 3 || (form == 0 && g->n_active >= 16384)) && g->sched_pre == 0) return DivForm::zpair;
	if (form == 2 || (form == 0 && g->n_active >= 16384)) return DivForm::coalesced;
	return DivForm::row;
}
// which gradient kernel a call gets: the 512-thread one with its collision branch, the same without (option "stencil" = block: A/B switch), or the streaming one
enum class GradForm { collision, block, stream };
static GradForm gradient_form(const hns_grid* g, const float* sdf, int has_collision) {
	if (has_collision && sdf) return GradForm::collision;
	return options().stencil_block.load() != 0 || !g->d_blk ? GradForm::block : GradForm::stream;
}

// One table per stage: what a form's kernel is called in the source, how it is launched, and its workgroup's threads and leaves. hns_sim_substep_plan's names and
// the launchers below read the same entry.
struct DivArgs { GridDev gd; const float* u; float* div; float inv_dx; const CombustFuse* fz; hipStream_t st; };  // (fz: the fused forms' further arguments)
struct DivEntry { const char* kernel; unsigned threads, leaves; void (*launch)(dim3 grid, dim3 block, const DivArgs& a); };
template <auto K> static void div_plain(dim3 n, dim3 t, const DivArgs& a) { hipLaunchKernelGGL(K, n, t, 0, a.st, a.gd, a.u, a.div, a.inv_dx); }
template <auto K> static void div_row(dim3 n, dim3 t, const DivArgs& a) { hipLaunchKernelGGL(K, n, t, 0, a.st, a.gd, a.u, a.div, a.inv_dx, NoMirror{}); }
template <auto K> static void div_fused(dim3 n, dim3 t, const DivArgs& a) { hipLaunchKernelGGL(K, n, t, 0, a.st, a.gd, a.u, a.div, a.inv_dx, *a.fz); }
static const DivEntry kDivergence[2][4] = {  // [fused][DivForm] (the fused launch has no block form: divergence_form)
    {{"k_divergence", 512, 1, div_plain<k_divergence>}, {"k_divergence_zpair<true>", 128, 2, div_plain<k_divergence_zpair<true>>},
     {"k_divergence_row<NoMirror,true>", 64, 1, div_row<k_divergence_row<NoMirror, true>>}, {"k_divergence_row<NoMirror,false>", 64, 1, div_row<k_divergence_row<NoMirror, false>>}},
    {{}, {"k_divergence_combust_buoyancy_zpair", 128, 2, div_fused<k_divergence_combust_buoyancy_zpair>},
     {"k_divergence_combust_buoyancy<true>", 64, 1, div_fused<k_divergence_combust_buoyancy<true>>}, {"k_divergence_combust_buoyancy<false>", 64, 1, div_fused<k_divergence_combust_buoyancy<false>>}}};
// the launch of hns_dev_divergence (fz null) and of hns_divergence_combust_buoyancy
static int launch_divergence(hns_grid* g, const float* vel3, float* div, float inv_dx, const CombustFuse* fz, void* stream, const char* who) {
	const DivForm form = divergence_form(g, fz != nullptr);
	const DivEntry& e = kDivergence[fz != nullptr][(int)form];
	DivArgs a{g->dev(), vel3, div, inv_dx, fz, (hipStream_t)stream};
	// the row forms backwards: advect_vector has just written the velocity front to back, so its tail is what the Infinity Cache holds (256^3: 74 -> 66 us).
	a.gd.rev = form != DivForm::block;
	e.launch(dim3((unsigned)((g->n_active + e.leaves - 1) / e.leaves)), dim3(e.threads), a);
	return launch_status(who);
}

struct GradArgs { GridDev gd; const float *u, *p; float* out; const float* sdf; float inv_dx; hipStream_t st; };
struct GradEntry { const char* kernel; void (*launch)(dim3 grid, const GradArgs& a); };  // (one leaf per workgroup)
template <bool COLL> static void grad_block(dim3 n, const GradArgs& a) { hipLaunchKernelGGL(k_subtract_gradient<COLL>, n, dim3(512), 0, a.st, a.gd, a.u, a.p, a.out, a.sdf, a.inv_dx); }
static void grad_stream(dim3 n, const GradArgs& a) { hipLaunchKernelGGL(k_subtract_gradient_s<NoMirror>, n, dim3(64), 0, a.st, a.gd, a.u, a.p, a.out, a.inv_dx, NoMirror{}); }
static const GradEntry kGradient[3] = {  // [GradForm]
    {"k_subtract_gradient<true>", grad_block<true>}, {"k_subtract_gradient<false>", grad_block<false>}, {"k_subtract_gradient_s<NoMirror>", grad_stream}};

extern "C" {

// the source names of the kernels the launchers below pick for these arguments (hns_sim_substep_plan)
const char* hns_divergence_kernel(const hns_grid* g, bool fused) { return kDivergence[fused][(int)divergence_form(g, fused)].kernel; }
const char* hns_subtract_gradient_kernel(const hns_grid* g, const float* sdf, int has_collision) { return kGradient[(int)gradient_form(g, sdf, has_collision)].kernel; }

int hns_dev_divergence(hns_grid* g, const float* vel3, float* div, float inv_dx, void* stream) {
	if (int rc = check_grid(g, "hns_dev_divergence")) return rc;
	NULLCHK(!vel3 || !div, "hns_dev_divergence");
	if (g->n_active == 0) return HNS_OK;
	return launch_divergence(g, vel3, div, inv_dx, nullptr, stream, "hns_dev_divergence");
}

// divergence + combustion_oxygen + temperature_buoyancy as one launch (hns_sim_substep; see CombustFuse). Same form choice and launch order as hns_dev_divergence.
int hns_divergence_combust_buoyancy(hns_grid* g, const float* vel3, float* div, float inv_dx, const float* fuel, const float* waste, const float* temperature,
                                    const float* flame, float* q4, float* vel3_out, float temp_gain, float expansion, float dt, float ambient, float strength,
                                    void* stream) {
	if (int rc = check_grid(g, "hns_divergence_combust_buoyancy")) return rc;
	NULLCHK(!vel3 || !div || !fuel || !waste || !temperature || !flame || !q4 || !vel3_out, "hns_divergence_combust_buoyancy");
	if (vel3 == vel3_out) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_divergence_combust_buoyancy: the buoyed velocity must not alias the velocity the divergence reads");
	if (g->n_active == 0) return HNS_OK;
	if (!g->d_blk) return fail(HNS_ERR_RUNTIME, "hns_divergence_combust_buoyancy: the grid has no launch tables");
	const CombustFuse fz{fuel, waste, temperature, flame, reinterpret_cast<float4*>(q4), vel3_out, temp_gain, expansion, dt, ambient, strength};
	return launch_divergence(g, vel3, div, inv_dx, &fz, stream, "hns_divergence_combust_buoyancy");
}

// the same kernels as ONE launch of a chained multi-GPU rank (hns_flags.hpp: PhaseMirror): boundary leaves first, their
// results also stored into the peers' ghost voxels
int hns_chain_divergence(hns_grid* g, const float* vel3, float* div, float inv_dx, const hns::PhaseMirror* m, void* stream) {
	if (int rc = check_grid(g, "hns_chain_divergence")) return rc;
	if (g->n_active == 0 || !g->d_blk) return fail(HNS_ERR_RUNTIME, "hns_chain_divergence: empty launch range");
	GridDev gd = g->dev();
	gd.rev = 1;  // (as hns_dev_divergence; walked backwards the boundary leaves come last, which the chain does not mind)
	hipLaunchKernelGGL(k_divergence_row<PhaseMirror>, dim3((unsigned)g->n_active), dim3(64), 0, (hipStream_t)stream, gd, vel3, div, inv_dx, *m);
	return launch_status("hns_chain_divergence");
}
int hns_chain_subtract_pressure_gradient(hns_grid* g, const float* vel3, const float* p, float* out3, float inv_dx, const hns::PhaseMirror* m, void* stream) {
	if (int rc = check_grid(g, "hns_chain_subtract_pressure_gradient")) return rc;
	if (g->n_active == 0 || !g->d_blk) return fail(HNS_ERR_RUNTIME, "hns_chain_subtract_pressure_gradient: empty launch range");
	hipLaunchKernelGGL(k_subtract_gradient_s<PhaseMirror>, dim3((unsigned)g->n_active), dim3(64), 0, (hipStream_t)stream, g->dev(), vel3, p, out3, inv_dx, *m);
	return launch_status("hns_chain_subtract_pressure_gradient");
}

int hns_dev_rbgs_color(hns_grid* g, const float* div, float* p, float dx, float omega, int color, void* stream) {
	if (int rc = check_grid(g, "hns_dev_rbgs_color")) return rc;
	NULLCHK(!div || !p, "hns_dev_rbgs_color");
	if (color != 0 && color != 1) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dev_rbgs_color: color must be 0 (red) or 1 (black)");
	if (g->n_active == 0) return HNS_OK;
	hipLaunchKernelGGL(k_rbgs_color, dim3((unsigned)g->n_active), dim3(256), 0, (hipStream_t)stream, g->dev(), div, p, dx * dx, omega, color);
	return launch_status("hns_dev_rbgs_color");
}

// One full (red, black) iteration src -> dst in the reference's own decomposition: copy, then one launch per colour in place (k_rbgs_color). The independent
// cross-check of the temporally blocked kernels (option "rbgs" = color), and what sweeps a grid they cannot (more than 2 M leaves).
static int launch_color_iteration(hns_grid* g, const GridDev& gd, const float* div, const float* src, float* dst, float dx2, float omega, hipStream_t st) {
	HNS_HIP(hipMemcpyAsync(dst, src, sizeof(float) * 512 * (size_t)g->topo.n_leaves, hipMemcpyDeviceToDevice, st));
	hipLaunchKernelGGL(k_rbgs_color, dim3((unsigned)g->n_active), dim3(256), 0, st, gd, div, dst, dx2, omega, 0);
	hipLaunchKernelGGL(k_rbgs_color, dim3((unsigned)g->n_active), dim3(256), 0, st, gd, div, dst, dx2, omega, 1);
	return HNS_OK;
}

int hns_dev_rbgs_iterate(hns_grid* g, const float* div, float* p_a, float* p_b, float dx, float omega, int iterations, int* result_in_b,
                         void* stream) {
	return hns_rbgs_iterate(g, div, p_a, p_b, dx, omega, iterations, result_in_b, stream, false);
}

// Walks the solve's schedule (hns_internal.hpp: SorSchedule; hns_grid_rbgs_plan below describes the same value), ping-ponging p_a / p_b once per step:
// *result_in_b is the parity of the steps. Blocked (hns_sorblock.hip): one launch per step, p read and written once per launch. A launch range -- a multi-GPU rank's
// boundary / interior leaves -- must never go through the colour form: its copy of the whole field would undo what the launch over the neighbouring range has stored.
// from_zero: the solve starts from p = 0 (the reference never warm-starts, HNanoSolver.cu:113 / PressureProjection.cu:35) and p_a's content is irrelevant: the first
// blocked launch does not read it (its ZERO kernel), the colour form is handed zeros, and a solve that launches nothing leaves p_a = 0.
int hns_rbgs_iterate(hns_grid* g, const float* div, float* p_a, float* p_b, float dx, float omega, int iterations, int* result_in_b, void* stream,
                     bool from_zero) {
	if (int rc = check_grid(g, "hns_dev_rbgs_iterate")) return rc;
	NULLCHK(!div || !p_a || !p_b, "hns_dev_rbgs_iterate");
	const size_t field_bytes = sizeof(float) * 512 * (size_t)g->topo.n_leaves;
	if (ranges_overlap(p_a, field_bytes, p_b, field_bytes)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dev_rbgs_iterate: p_a and p_b must be distinct buffers (they overlap)");
	if (ranges_overlap(div, field_bytes, p_a, field_bytes) || ranges_overlap(div, field_bytes, p_b, field_bytes))
		return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dev_rbgs_iterate: div overlaps p_a or p_b");
	if (iterations < 0) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dev_rbgs_iterate: negative iteration count");
	const SorSchedule s = hns_rbgs_schedule(g, iterations);
	if (result_in_b) *result_in_b = s.steps() & 1;
	hipStream_t st = (hipStream_t)stream;
	if (g->n_active == 0 || iterations == 0) {
		if (from_zero) HNS_HIP(hipMemsetAsync(p_a, 0, field_bytes, st));
		return HNS_OK;
	}
	const float dx2 = dx * dx;  // Kernel.cu:608
	float* src = p_a;
	float* dst = p_b;
	if (s.lb) {
		for (int i = 0; i < s.steps(); ++i, std::swap(src, dst))
			if (int rc = hns_rbgs_block_launch(g, s.lb, s.step(i), from_zero && i == 0, div, src, dst, dx2, omega, stream)) return rc;
	} else {
		if (from_zero) HNS_HIP(hipMemsetAsync(src, 0, field_bytes, st));  // the colour form reads its input
		const GridDev gd = g->dev();
		for (int i = 0; i < s.steps(); ++i, std::swap(src, dst))
			if (int rc = launch_color_iteration(g, gd, div, src, dst, dx2, omega, st)) return rc;
	}
	return launch_status("hns_dev_rbgs_iterate");
}

}  // extern "C"

// What has to hold before a sim's solve launches anything (hns_sim_pressure_solve, hns_sim_substep): a control reads the residual on the host at every check, and a
// hierarchy that a regrid dropped is built on the host -- neither on a capturing stream.
int hns_solve_preflight(hns_sim* s, void* stream, const char* who) {
	if (s->control && stream_is_capturing(stream)) {
		set_error("%s: a solve control is set (the host reads the residual at every check) and the stream is capturing", who);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	return s->mg ? hns_mg_ready(s, stream, who) : HNS_OK;
}

// The pressure solve of a device-resident sim: p = 0, then `iterations` x (red, black) (HNanoSolver.cu:256-272 / PressureProjection.cu:51-60) -- or, under
// hns_sim_set_solve_method, `iterations` V-cycles with the method's own omega. With no control that is one piece; a control (hns_sim_set_solve_control: `iterations`
// is then the maximum) cuts it into pieces of check_every with the residual behind each. A piece is the same sequence of launches whatever came before it, so the
// pressure after j iterations is the uncontrolled solve's, bit for bit.
int hns_sim_solve(hns_sim* s, int iterations, float voxel_size, float omega, void* stream) {
	hns_sim::Control* const ctl = s->control;
	DeviceScope on(ctl || s->mg ? s->device : -1);  // (the plain solve leaves the current device to hns_rbgs_iterate's check)
	float *cur = s->p_a, *other = s->p_b;
	// k iterations further; first: from p = 0, which the first sweep knows without reading *cur (never warm-started, HNanoSolver.cu:113)
	auto step = [&](int k, bool first) {
		if (s->mg) return hns_mg_cycles(s, &cur, &other, voxel_size, k, first, stream);
		int in_b = 0;
		HNS_TRY(hns_rbgs_iterate(s->grid, s->div, cur, other, voxel_size, omega, k, &in_b, stream, first));
		if (in_b) std::swap(cur, other);
		return (int)HNS_OK;
	};
	if (ctl) HNS_TRY(hns_control_begin(s));
	HNS_TRY(s->solve_begin(stream));
	if (ctl) HNS_TRY(hns_control_check(s, nullptr, 0, voxel_size, stream, nullptr));
	int done = 0;
	bool met = false;
	do {  // (at least one piece, be it of no iterations: the step still leaves p = 0, which hns_project_non_divergent relies on)
		const int k = ctl ? std::min(ctl->c.check_every, iterations - done) : iterations;
		HNS_TRY(step(k, done == 0));
		done += k;
		if (ctl) HNS_TRY(hns_control_check(s, cur, done, voxel_size, stream, &met));
	} while (done < iterations && !met);
	HNS_TRY(s->solve_end(stream, done));
	s->p_result = cur;
	s->solved = true;
	return HNS_OK;
}

extern "C" {

int hns_grid_rbgs_plan(hns_grid* g, int iterations, char* description, uint64_t description_bytes, int* launches, int* iterations_per_launch) {
	if (int rc = check_grid(g, "hns_grid_rbgs_plan")) return rc;
	if (iterations < 0) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_grid_rbgs_plan: negative iteration count");
	const SorSchedule s = hns_rbgs_schedule(g, iterations);
	if (description && description_bytes) {
		if (s.lb)
			snprintf(description, description_bytes, "k_rbgs_block%s<%d,%d>: %d red+black iterations per launch on %s blocks with a %d-voxel halo, p read and written once per launch%s", s.lb == 2 ? "_xy" : "",
			         s.lb, s.k_max, s.k_max, s.lb == 1 ? "one-leaf (8^3-voxel)" : "16^3-voxel", 2 * s.k_max, s.lb == 2 ? " (rows in LDS, three workgroups per CU, the sweep threads fetch their own rows)" : "");
		else
			snprintf(description, description_bytes, "k_rbgs_color: two launches per iteration, in place (the reference's decomposition)");
	}
	if (launches) *launches = s.launches();
	if (iterations_per_launch) *iterations_per_launch = s.iterations_per_launch();
	return HNS_OK;
}

int hns_dev_time_rbgs(hns_grid* g, const float* div, float* p_a, float* p_b, float dx, float omega, int iterations, int reps, float* ms_per_launch,
                      void* stream) {
	if (int rc = check_grid(g, "hns_dev_time_rbgs")) return rc;
	if (!ms_per_launch || iterations <= 0 || reps <= 0) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dev_time_rbgs: bad arguments");
	struct Events {  // destroyed on every return path
		hipEvent_t e0 = nullptr, e1 = nullptr;
		~Events() {
			if (e0) (void)hipEventDestroy(e0);
			if (e1) (void)hipEventDestroy(e1);
		}
	} ev;
	HNS_HIP(hipEventCreate(&ev.e0));
	HNS_HIP(hipEventCreate(&ev.e1));
	double total = 0.0;
	for (int r = 0; r < reps; ++r) {
		HNS_HIP(hipEventRecord(ev.e0, (hipStream_t)stream));
		if (int rc = hns_dev_rbgs_iterate(g, div, p_a, p_b, dx, omega, iterations, nullptr, stream)) return rc;
		HNS_HIP(hipEventRecord(ev.e1, (hipStream_t)stream));
		HNS_HIP(hipEventSynchronize(ev.e1));
		float ms = 0.0f;
		HNS_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
		total += ms;
	}
	*ms_per_launch = (float)(total / ((double)reps * iterations));
	return HNS_OK;
}

int hns_dev_subtract_pressure_gradient(hns_grid* g, const float* vel3, const float* p, float* out3, const float* sdf, int has_collision, float inv_dx,
                                       void* stream) {
	if (int rc = check_grid(g, "hns_dev_subtract_pressure_gradient")) return rc;
	NULLCHK(!vel3 || !p || !out3, "hns_dev_subtract_pressure_gradient");
	if (g->n_active == 0) return HNS_OK;
	// (a wave-per-leaf row form like k_divergence_row was measured for this kernel too: 118 us vs 111 us at 256^3 -- not kept)
	// (also measured and not kept for this kernel: the six taps through an LDS tile as in the advection kernels, 125 vs 116 us --
	// at 470 MB per launch it streams from HBM and the extra barrier costs more than the loads it saves)
	// (with a collision field the 512-thread form stays: the two forms measured within 6 % of each other, first line above)
	kGradient[(int)gradient_form(g, sdf, has_collision)].launch(dim3((unsigned)g->n_active), GradArgs{g->dev(), vel3, p, out3, sdf, inv_dx, (hipStream_t)stream});
	return launch_status("hns_dev_subtract_pressure_gradient");
}

}  // extern "C"
