// hns_splat.hip -- point values added into fields: the transpose of k_sample_points (hns_points.hip). The same cell, the same eight taps, weights in place of the lerp
// nest, and an accumulation whose result does not depend on the order the adds retire in: every term is rounded ONCE to a multiple of the quantum 2^Q and added as a 64-bit
// integer (include/hns.h: hns_dev_splat_points states the arithmetic). Integer addition modulo 2^64 is associative, so two runs, and the host mirror below, give the same
// bytes. No float atomics. One thread per point adds into an accumulator kept with the grid; a second launch, one wave per touched leaf, adds the accumulator into the
// fields and leaves it zero for the next call.
#include "hns_points.hpp"

#include <cmath>
#include <cstring>

using namespace hns;

namespace {

constexpr int kSplatChannels = 4;   // components one launch accumulates: the channels of a voxel's piece of the accumulator (32 bytes: one L2 sector pair)
constexpr int kMaxSplatFields = 8;  // fields of one call
constexpr int kSplatBlock = 256;

// one component of a field and of its point values: element e of either is at [e * stride + off] (a float field: 1, 0; component c of a Vec3f AoS field: 3, c)
struct SplatChannel {
	const float* val;
	float* field;
	int stride, off;
	int wide;  // finish: the field is a 16-byte aligned float array, four voxels per access
};
struct SplatChannels {
	SplatChannel c[kSplatChannels];
	int n;
};

// ---- the arithmetic, stated once for the kernel and the host mirror (-ffp-contract=off: every line is one rounded operation) ---------------------------------------

// w[di*4+dj*2+dk] = (wx[di] * wy[dj]) * wz[dk]
__host__ __device__ inline void splat_weights(float fx, float fy, float fz, float (&w)[8]) {
	const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy}, wz[2] = {1.0f - fz, fz};
	for (int c = 0; c < 8; ++c) w[c] = (wx[c >> 2] * wy[(c >> 1) & 1]) * wz[c & 1];
}

// Is the term t accepted, and as which multiple of the quantum? scale = 2^-Q: the product is exact in f64 (a power of two, |t| < 2^128, scale <= 2^40), so the test is the
// header's "t finite and |t| * 2^-Q < 2^62" (a NaN and an inf fail the comparison), and k = rint of it, ties to even.
__host__ __device__ inline bool splat_term(float t, double scale, long long* k) {
	const double x = (double)t * scale;
	if (!(fabs(x) < 0x1p62)) return false;
#ifdef __HIP_DEVICE_COMPILE__
	*k = __double2ll_rn(x);
#else
	*k = (long long)std::nearbyint(x);  // (the default rounding mode: to nearest, ties to even)
#endif
	return true;
}

// what a non-zero accumulator adds to its voxel: quantum = 2^Q
__host__ __device__ inline float splat_total(unsigned long long a, double quantum) { return (float)((double)(long long)a * quantum); }

// ---- kernels -----------------------------------------------------------------------------------------------------------------------------------------------------------

// One thread per point: the cell once (point_cell; CURSOR as there -- a splat takes one cell per point and launches without one), then up to four channels into the
// accumulator acc[voxel * S + channel]. The adds are atomics without a return value: nothing waits for them, a point's (up to 32) are in flight together, and the four of a
// tap fall into one 32-byte piece. touched[leaf] = 1 for every leaf a tap landed in (plain stores of one value). masks (or null): bit `voxel` of the sim's active masks
// (leaf x 64 bytes, byte x*8+y, bit z, read as 32-bit words) set for every landed tap of positive weight. status, masks: written by the first launch of a call only.
template <bool CURSOR>
__global__ __launch_bounds__(kSplatBlock) void k_splat_points(const GridDev g, const SplatChannels ch, const float* __restrict__ xyz, const unsigned n, const double scale,
                                                               unsigned long long* __restrict__ acc, const int S, int* __restrict__ touched, unsigned* __restrict__ masks,
                                                               unsigned char* __restrict__ status, unsigned long long* __restrict__ rejected) {
	const unsigned p = blockIdx.x * (unsigned)kSplatBlock + threadIdx.x;
	unsigned rej = 0;
	if (p < n) {
		const f3 pos = ld3(xyz, (int)p);
		Cell C;
		if (finite_f(pos.x) && finite_f(pos.y) && finite_f(pos.z)) {
			Cursor none{-1, 0, 0, 0};
			C = point_cell<CURSOR>(g, none, pos.x, pos.y, pos.z);
		} else {  // lands nowhere
#pragma unroll
			for (int c = 0; c < 8; ++c) C.t[c] = -1;
			C.fx = C.fy = C.fz = 0.0f;
		}
		float v[kSplatChannels];
#pragma unroll
		for (int q = 0; q < kSplatChannels; ++q) v[q] = q < ch.n ? ch.c[q].val[(size_t)p * (unsigned)ch.c[q].stride + (unsigned)ch.c[q].off] : 0.0f;
		float w[8];
		splat_weights(C.fx, C.fy, C.fz, w);
		int landed = 0;
#pragma unroll
		for (int c = 0; c < 8; ++c) {
			const int t = C.t[c];
			if (t < 0) continue;
			++landed;
			if (c == 0 || (t >> 9) != (C.t[c - 1] >> 9)) touched[t >> 9] = 1;
			if (masks && w[c] > 0.0f) atomicOr(masks + ((unsigned)t >> 5), 1u << ((unsigned)t & 31u));
#pragma unroll
			for (int q = 0; q < kSplatChannels; ++q) {
				if (q >= ch.n) break;
				long long k;
				if (!splat_term(w[c] * v[q], scale, &k))
					++rej;
				else if (k)
					atomicAdd(acc + (size_t)t * (unsigned)S + (unsigned)q, (unsigned long long)k);
			}
		}
		if (status) status[p] = (unsigned char)landed;
	}
	if (rejected) {  // one add per wave that has something to report (whole waves get here: nothing above returns)
#pragma unroll
		for (int m = 1; m < 64; m *= 2) rej += (unsigned)__shfl_xor((int)rej, m);
		if ((threadIdx.x & 63u) == 0 && rej) atomicAdd(rejected, (unsigned long long)rej);
	}
}

// One wave per leaf, four leaves per workgroup. An untouched leaf costs its flag load. Lane l takes voxels 4l .. 4l + 3 of each half of the leaf: their S channels are 32 S
// contiguous bytes of the accumulator, read and zeroed in 16-byte pieces; a float field takes its four values as one 16-byte access, a Vec3f component one by one. Only
// voxels with a non-zero accumulator change (a 16-byte store rewrites the others of its four with the bits it read).
template <int S>
__global__ __launch_bounds__(256) void k_splat_finish(const SplatChannels ch, unsigned long long* __restrict__ acc, int* __restrict__ touched, const unsigned n_leaves,
                                                      const double quantum) {
	const unsigned leaf = blockIdx.x * 4u + (threadIdx.x >> 6);
	if (leaf >= n_leaves) return;  // (whole waves)
	if (!touched[leaf]) return;
	const unsigned lane = threadIdx.x & 63u;
#pragma unroll
	for (int r = 0; r < 2; ++r) {
		const size_t v0 = (size_t)leaf * 512u + (unsigned)r * 256u + lane * 4u;
		ulonglong2* a = reinterpret_cast<ulonglong2*>(acc + v0 * S);
		unsigned long long x[4 * S];  // x[j * S + q]: channel q of voxel v0 + j
#pragma unroll
		for (int i = 0; i < 2 * S; ++i) {
			const ulonglong2 u = a[i];
			x[2 * i] = u.x, x[2 * i + 1] = u.y;
		}
#pragma unroll
		for (int i = 0; i < 2 * S; ++i) a[i] = make_ulonglong2(0ull, 0ull);
#pragma unroll
		for (int q = 0; q < S; ++q) {
			if (q >= ch.n) break;
			const SplatChannel e = ch.c[q];
			if (!(x[q] | x[S + q] | x[2 * S + q] | x[3 * S + q])) continue;
			if (e.wide) {
				float4* f = reinterpret_cast<float4*>(e.field + v0);
				float4 y = *f;
				if (x[q]) y.x = y.x + splat_total(x[q], quantum);
				if (x[S + q]) y.y = y.y + splat_total(x[S + q], quantum);
				if (x[2 * S + q]) y.z = y.z + splat_total(x[2 * S + q], quantum);
				if (x[3 * S + q]) y.w = y.w + splat_total(x[3 * S + q], quantum);
				*f = y;
			} else {
#pragma unroll
				for (int j = 0; j < 4; ++j)
					if (x[j * S + q]) {
						float* f = e.field + (v0 + (unsigned)j) * (unsigned)e.stride + (unsigned)e.off;
						*f = *f + splat_total(x[j * S + q], quantum);
					}
			}
		}
	}
	if (lane == 0) touched[leaf] = 0;
}

// ---- the accumulator -----------------------------------------------------------------------------------------------------------------------------------------------------

size_t splat_acc_bytes(const hns_grid* g, int channels) { return sizeof(unsigned long long) * 512u * (size_t)g->topo.n_leaves * (size_t)channels; }

// The grid's accumulator with room for `channels` channels: int64 channels over all voxels, then one touched word per leaf. All zero between calls; a fresh block (whatever
// the pool left in it) and one a failed call left half used are cleared on `stream` before the first launch.
int splat_accumulator(hns_grid* g, int channels, hipStream_t st) {
	std::lock_guard<std::mutex> lock(g->build_mutex);
	if (!g->d_splat || g->splat_channels < channels) {
		if (g->d_splat) hns_arena_put(g->d_splat, g->splat_bytes, g->device);  // (waits for the device: nothing still adds into it)
		g->d_splat = nullptr, g->splat_bytes = 0, g->splat_channels = 0;
		HNS_TRY(hns_arena_get(splat_acc_bytes(g, channels) + sizeof(int) * (size_t)g->topo.n_leaves, g->device, &g->d_splat, &g->splat_bytes));
		g->splat_channels = channels;
		g->splat_dirty = true;
	}
	if (g->splat_dirty) {
		HNS_HIP(hipMemsetAsync(g->d_splat, 0, splat_acc_bytes(g, g->splat_channels) + sizeof(int) * (size_t)g->topo.n_leaves, st));
		g->splat_dirty = false;
	}
	return HNS_OK;
}

// ---- argument checks shared by the device call and the host mirror -------------------------------------------------------------------------------------------------------

int invalid(const char* fmt, const char* who, int i = 0, int j = 0) {
	set_error(fmt, who, i, j);
	return HNS_ERR_INVALID_ARGUMENT;
}

// what is refused whatever n is
int check_splat_lists(const char* who, const void* fields, const int* ncomp, int n_fields, const void* values, uint64_t n, int log2_quantum) {
	if (n_fields < 1 || n_fields > kMaxSplatFields) return invalid("%s: n_fields is %d (must be 1 .. 8)", who, n_fields);
	if (!fields || !ncomp || !values) return refuse(who, "null list (fields, ncomp or values)");
	for (int i = 0; i < n_fields; ++i)
		if (ncomp[i] != 1 && ncomp[i] != 3) return invalid("%s: ncomp[%d] is %d (must be 1 or 3)", who, i, ncomp[i]);
	if (n > kMaxPoints) return refuse(who, "n is above 2^31 - 1");
	if (log2_quantum < -40 || log2_quantum > 0) return invalid("%s: log2_quantum is %d (must be -40 .. 0)", who, log2_quantum);
	return HNS_OK;
}

// the pointers of a call with n > 0
int check_splat_pointers(const char* who, float* const* fields, int n_fields, const float* xyz, const float* const* values, const void* status, const void* rejected) {
	if (!xyz) return refuse(who, "xyz is null");
	for (int i = 0; i < n_fields; ++i) {
		if (!fields[i]) return invalid("%s: fields[%d] is null", who, i);
		if (!values[i]) return invalid("%s: values[%d] is null", who, i);
	}
	for (int i = 0; i < n_fields; ++i) {
		if ((const void*)fields[i] == (const void*)xyz) return invalid("%s: fields[%d] is xyz", who, i);
		if ((const void*)fields[i] == status) return invalid("%s: fields[%d] is status", who, i);
		if ((const void*)fields[i] == rejected) return invalid("%s: fields[%d] is d_rejected", who, i);
		for (int j = 0; j < n_fields; ++j) {
			if (fields[i] == values[j]) return invalid("%s: fields[%d] is values[%d]", who, i, j);
			if (j < i && fields[i] == fields[j]) return invalid("%s: fields[%d] is fields[%d]", who, i, j);
		}
	}
	return HNS_OK;
}

// ---- launcher --------------------------------------------------------------------------------------------------------------------------------------------------------------

// fields / ncomp / values: HOST arrays of n_fields entries; masks: null, or the active masks of a sim on this grid. Every refusal comes before the first launch.
int splat_points(const char* who, hns_grid* g, float* const* fields, const int* ncomp, int n_fields, const float* xyz, const float* const* values, uint64_t n,
                 int log2_quantum, unsigned char* masks, unsigned char* status, uint64_t* d_rejected, void* stream) {
	if (int rc = check_grid(g, who)) return rc;
	HNS_TRY(check_splat_lists(who, fields, ncomp, n_fields, values, n, log2_quantum));
	if (n == 0) return HNS_OK;  // (no point, no device pointer looked at: an empty array's may well be null)
	HNS_TRY(check_splat_pointers(who, fields, n_fields, xyz, values, status, d_rejected));
	const hipStream_t st = (hipStream_t)stream;
	if (g->topo.n_leaves == 0) {  // no leaf: nothing lands
		if (status) HNS_HIP(hipMemsetAsync(status, 0, n, st));
		return HNS_OK;
	}
	std::vector<SplatChannel> all;
	for (int i = 0; i < n_fields; ++i)
		for (int c = 0; c < ncomp[i]; ++c) all.push_back(SplatChannel{values[i], fields[i], ncomp[i], c, ncomp[i] == 1 && ((uintptr_t)fields[i] & 15u) == 0});
	HNS_TRY(splat_accumulator(g, std::min<int>(kSplatChannels, (int)all.size()), st));
	const int S = g->splat_channels;
	unsigned long long* acc = (unsigned long long*)g->d_splat;
	int* touched = (int*)((char*)g->d_splat + splat_acc_bytes(g, S));
	const double scale = std::ldexp(1.0, -log2_quantum), quantum = std::ldexp(1.0, log2_quantum);
	const unsigned n_leaves = (unsigned)g->topo.n_leaves;
	const dim3 pgrid((unsigned)((n + kSplatBlock - 1) / kSplatBlock)), lgrid((n_leaves + 3u) / 4u);
	for (size_t base = 0; base < all.size(); base += kSplatChannels) {  // (a channel's sum does not depend on the others: more launches change nothing numerically)
		SplatChannels ch{};
		ch.n = (int)std::min<size_t>(kSplatChannels, all.size() - base);
		for (int q = 0; q < ch.n; ++q) ch.c[q] = all[base + (size_t)q];
		const bool first = base == 0;
		hipLaunchKernelGGL(k_splat_points<false>, pgrid, dim3(kSplatBlock), 0, st, g->dev(), ch, xyz, (unsigned)n, scale, acc, S, touched,
		                   first ? (unsigned*)masks : nullptr, first ? status : nullptr, (unsigned long long*)d_rejected);
		switch (S) {
		case 1: hipLaunchKernelGGL(k_splat_finish<1>, lgrid, dim3(256), 0, st, ch, acc, touched, n_leaves, quantum); break;
		case 2: hipLaunchKernelGGL(k_splat_finish<2>, lgrid, dim3(256), 0, st, ch, acc, touched, n_leaves, quantum); break;
		case 3: hipLaunchKernelGGL(k_splat_finish<3>, lgrid, dim3(256), 0, st, ch, acc, touched, n_leaves, quantum); break;
		default: hipLaunchKernelGGL(k_splat_finish<4>, lgrid, dim3(256), 0, st, ch, acc, touched, n_leaves, quantum); break;
		}
		if (int rc = launch_status(who)) {
			g->splat_dirty = true;  // whatever ran may have left sums behind: the next call clears first
			return rc;
		}
	}
	return HNS_OK;
}

// Floor with the GPU's conversion (__float2int_rd: saturating, NaN -> 0), on the host
int floor_sat(float x) {
	if (x != x) return 0;
	if (x >= 2147483648.0f) return INT32_MAX;
	if (x < -2147483648.0f) return INT32_MIN;
	return (int)std::floor(x);
}

}  // namespace

void hns_grid_free_splat(hns_grid* g) {
	std::lock_guard<std::mutex> lock(g->build_mutex);
	if (g->d_splat) hns_arena_put(g->d_splat, g->splat_bytes, g->device);
	g->d_splat = nullptr, g->splat_bytes = 0, g->splat_channels = 0, g->splat_dirty = false;
}

extern "C" {

int hns_dev_splat_points(hns_grid* g, float* const* fields, const int* ncomp, int n_fields, const float* xyz, const float* const* values, uint64_t n, int log2_quantum,
                         unsigned char* status, uint64_t* d_rejected, void* stream) {
	return splat_points("hns_dev_splat_points", g, fields, ncomp, n_fields, xyz, values, n, log2_quantum, nullptr, status, d_rejected, stream);
}

int hns_sim_splat_points(hns_sim* s, const char* const* names, int n_names, const float* velocity_values, const float* xyz, const float* const* values, uint64_t n,
                         int log2_quantum, int activate, unsigned char* status, uint64_t* d_rejected, void* stream) {
	const char* who = "hns_sim_splat_points";
	if (int rc = check_sim(s, who)) return rc;
	if (n_names < 0) return refuse(who, "n_names is negative");
	if (n_names > 0 && (!names || !values)) return refuse(who, "null list (names or values)");
	std::vector<int> which;
	for (int i = 0; i < n_names; ++i) {
		const int k = names[i] ? s->find(names[i]) : -1;
		if (k < 0) {
			set_error("%s: names[%d]: no float field named '%s' in this sim", who, i, names[i] ? names[i] : "?");
			return HNS_ERR_INVALID_ARGUMENT;
		}
		if (s->names[(size_t)k] == "collision_sdf") return invalid("%s: names[%d]: collision_sdf takes no point values (it comes from the collision input)", who, i);
		if (std::find(which.begin(), which.end(), k) != which.end()) {
			set_error("%s: names[%d]: field '%s' is listed twice", who, i, names[i]);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		which.push_back(k);
	}
	std::vector<float*> fields;
	std::vector<const float*> vals;
	std::vector<int> ncomp;
	for (size_t i = 0; i < which.size(); ++i) fields.push_back(s->cur[(size_t)which[i]]), vals.push_back(values[i]), ncomp.push_back(1);
	if (velocity_values) fields.push_back(s->vel), vals.push_back(velocity_values), ncomp.push_back(3);
	if (fields.empty()) return refuse(who, "nothing to write (no names and velocity_values is null)");
	HNS_TRY(splat_points(who, s->grid, fields.data(), ncomp.data(), (int)fields.size(), xyz, vals.data(), n, log2_quantum, activate ? s->d_masks : nullptr, status,
	                     d_rejected, stream));
	if (n) {  // the written buffers no longer hold what a cook handed back; a rewritten velocity is not the one a substep looked ahead from
		for (int k : which) s->handed_cur[(size_t)k] = hns_sim::Handed{};
		if (velocity_values) s->forget(hns_sim::kVelocity);
	}
	return HNS_OK;
}

// Host mirror: brute force, the same integers. One accumulator of n_voxels words, one component after the other.
int hns_grid_splat_points(const hns_grid* g, float* const* fields, const int* ncomp, int n_fields, const float* xyz, const float* const* values, uint64_t n,
                          int log2_quantum, unsigned char* masks, int activate, unsigned char* status, uint64_t* rejected) {
	const char* who = "hns_grid_splat_points";
	if (!g) return refuse(who, "null grid");
	HNS_TRY(check_splat_lists(who, fields, ncomp, n_fields, values, n, log2_quantum));
	if (n == 0) return HNS_OK;
	HNS_TRY(check_splat_pointers(who, fields, n_fields, xyz, values, status, rejected));
	HNS_TRY(hns_grid_host_tables(g));
	const Topology& T = g->topo;
	std::vector<int64_t> tap((size_t)n * 8);  // flat voxel index, -1: did not land
	std::vector<float> weight((size_t)n * 8);
	for (uint64_t p = 0; p < n; ++p) {
		const float* x = xyz + 3 * p;
		const bool finite = std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]);
		const int i = floor_sat(x[0]), j = floor_sat(x[1]), k = floor_sat(x[2]);
		float w[8];
		splat_weights(x[0] - (float)i, x[1] - (float)j, x[2] - (float)k, w);
		int landed = 0;
		for (int c = 0; c < 8; ++c) {  // (corner coordinates wrap at the end of the int32 range, as point_cell's do)
			const int32_t ci = (int32_t)((uint32_t)i + (uint32_t)(c >> 2)), cj = (int32_t)((uint32_t)j + (uint32_t)((c >> 1) & 1)), ck = (int32_t)((uint32_t)k + (uint32_t)(c & 1));
			const uint64_t off = finite ? T.offset(ci, cj, ck) : 0;
			tap[8 * p + c] = (int64_t)off - 1;
			weight[8 * p + c] = w[c];
			if (!off) continue;
			++landed;
			if (masks && activate && w[c] > 0.0f) masks[(off - 1) >> 3] |= (unsigned char)(1u << ((off - 1) & 7u));
		}
		if (status) status[p] = (unsigned char)landed;
	}
	const double scale = std::ldexp(1.0, -log2_quantum), quantum = std::ldexp(1.0, log2_quantum);
	std::vector<uint64_t> acc((size_t)T.n_leaves * 512u);
	uint64_t rej = 0;
	for (int f = 0; f < n_fields; ++f)
		for (int comp = 0; comp < ncomp[f]; ++comp) {
			std::fill(acc.begin(), acc.end(), 0);
			for (uint64_t p = 0; p < n; ++p) {
				const float v = values[f][p * (uint64_t)ncomp[f] + (uint64_t)comp];
				for (int c = 0; c < 8; ++c) {
					if (tap[8 * p + c] < 0) continue;
					long long k;
					if (!splat_term(weight[8 * p + c] * v, scale, &k))
						++rej;
					else
						acc[(size_t)tap[8 * p + c]] += (uint64_t)k;
				}
			}
			for (size_t e = 0; e < acc.size(); ++e)
				if (acc[e]) {
					float* dst = fields[f] + e * (size_t)ncomp[f] + (size_t)comp;
					*dst = *dst + splat_total(acc[e], quantum);
				}
		}
	if (rejected) *rejected += rej;
	return HNS_OK;
}

}  // extern "C"
