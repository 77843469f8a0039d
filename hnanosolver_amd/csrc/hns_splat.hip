// hns_splat.hip -- point values added into fields: the transpose of k_sample_points (hns_points.hip). The same cell, the same eight taps, weights in place of the lerp
// nest, and an accumulation whose result does not depend on the order the adds retire in: every term is rounded ONCE to a multiple of the quantum 2^Q and added as a 64-bit
// integer (include/hns.h: hns_dev_splat_points states the arithmetic). Integer addition modulo 2^64 is associative, so two runs, and the host mirror below, give the same
// bytes. No float atomics. One thread per point adds into an accumulator kept with the grid; a second launch, one wave per touched leaf, adds the accumulator into the
// fields and leaves it zero for the next call. Under a spec (include/hns.h: hns_splat_spec) the first launch is the radial kernel of hns_rasterize.hip, and a pass carries
// a weight channel W that the second launch divides by in place of adding (the average).
#include "hns_points.hpp"

#include <cmath>
#include <cstring>

using namespace hns;

namespace {

constexpr int kMaxSplatFields = 8;  // fields of one call

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
		for (int q = 0; q < kSplatChannels; ++q)  // (a channel without point values is the weight channel of an average: every point's value is 1.0f)
			v[q] = q < ch.n ? (ch.c[q].val ? ch.c[q].val[(size_t)p * (unsigned)ch.c[q].stride + (unsigned)ch.c[q].off] : 1.0f) : 0.0f;
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
// voxels with a non-zero accumulator change (a 16-byte store rewrites the others of its four with the bits it read). ch.average: channel 0 is the weight channel W, which
// has no field; the voxels whose W accumulator is non-zero change, and they become Vsum / max(Wsum, min_weight) (splat_average) in place of field + Vsum.
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
			if (ch.average && q == 0) continue;
			const SplatChannel e = ch.c[q];
			unsigned long long gate[4];  // the accumulator that says whether voxel v0 + j changes: the channel's own, or W
#pragma unroll
			for (int j = 0; j < 4; ++j) gate[j] = splat_gate(ch.average, x[j * S + q], x[j * S]);
			if (!(gate[0] | gate[1] | gate[2] | gate[3])) continue;
			auto value = [&](float old, int j) { return splat_finished(ch.average, old, x[j * S + q], x[j * S], quantum, ch.min_weight); };
			if (e.wide) {
				float4* f = reinterpret_cast<float4*>(e.field + v0);
				float4 y = *f;
				if (gate[0]) y.x = value(y.x, 0);
				if (gate[1]) y.y = value(y.y, 1);
				if (gate[2]) y.z = value(y.z, 2);
				if (gate[3]) y.w = value(y.w, 3);
				*f = y;
			} else {
#pragma unroll
				for (int j = 0; j < 4; ++j)
					if (gate[j]) {
						float* f = e.field + (v0 + (unsigned)j) * (unsigned)e.stride + (unsigned)e.off;
						*f = value(*f, j);
					}
			}
		}
	}
	if (lane == 0) touched[leaf] = 0;
}

}  // namespace

namespace hns {  // (hns_points.hpp declares what hns_splat_binned.hip shares: the accumulator, the checks, the passes, the sim's field lists)

// ---- the accumulator -----------------------------------------------------------------------------------------------------------------------------------------------------

size_t splat_acc_bytes(const hns_grid* g, int channels) { return sizeof(unsigned long long) * 512u * (size_t)g->topo.n_leaves * (size_t)channels; }

// The grid's accumulator with room for `channels` channels: int64 channels over all voxels, then one touched word per leaf. All zero between calls; a fresh block (whatever
// the pool left in it) and one a failed call left half used are cleared on `stream` before the first launch.
int splat_accumulator(hns_grid* g, int channels, hipStream_t st) {
	std::lock_guard<std::mutex> lock(g->build_mutex);
	if (!g->d_splat || g->splat_channels < channels) {
		g->splat_channels = 0;  // (a narrower block goes back first, behind a wait for the device: nothing still adds into it)
		HNS_TRY(g->d_splat.get(splat_acc_bytes(g, channels) + sizeof(int) * (size_t)g->topo.n_leaves, g->device));
		g->splat_channels = channels;
		g->splat_dirty = true;
	}
	if (g->splat_dirty) {
		HNS_HIP(hipMemsetAsync(g->d_splat.p, 0, splat_acc_bytes(g, g->splat_channels) + sizeof(int) * (size_t)g->topo.n_leaves, st));
		g->splat_dirty = false;
	}
	return HNS_OK;
}

// ---- argument checks shared by the device call and the host mirror -------------------------------------------------------------------------------------------------------

static int invalid(const char* fmt, const char* who, int i = 0, int j = 0) {
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

const hns_splat_spec kDefaultSpec = {0, 0, 0.0f, nullptr, 0.0f};

// what the setters and the host mirror refuse in a spec
static int check_splat_spec(const char* who, const hns_splat_spec& sp) {
	if (sp.kernel != 0 && sp.kernel != 1) return invalid("%s: spec.kernel is %d (must be 0 trilinear or 1 radial)", who, sp.kernel);
	if (sp.mode != 0 && sp.mode != 1) return invalid("%s: spec.mode is %d (must be 0 add or 1 average)", who, sp.mode);
	if (sp.kernel == 1 && !(0.0f < sp.radius && sp.radius <= 4.0f)) return refuse(who, "spec.radius of a radial spec must lie in (0, 4]");
	if (sp.kernel == 0 && sp.d_radius) return refuse(who, "spec.d_radius is given but spec.kernel is 0 (trilinear)");
	if (!(sp.min_weight >= 0.0f && sp.min_weight < INFINITY)) return refuse(who, "spec.min_weight must be finite and >= 0");
	return HNS_OK;
}

// The passes of a call: add -- up to four value channels each; average -- the weight channel W first, then up to three value channels
std::vector<SplatChannels> splat_passes(const std::vector<SplatChannel>& all, const hns_splat_spec& sp) {
	std::vector<SplatChannels> passes;
	const size_t per = sp.mode ? kSplatChannels - 1 : kSplatChannels;
	for (size_t base = 0; base < all.size(); base += per) {
		SplatChannels ch{};
		ch.average = sp.mode, ch.min_weight = sp.min_weight;
		if (sp.mode) ch.c[ch.n++] = SplatChannel{nullptr, nullptr, 0, 0, 0};
		for (size_t q = base; q < std::min(all.size(), base + per); ++q) ch.c[ch.n++] = all[q];
		passes.push_back(ch);
	}
	return passes;
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

// The field, value and component lists of a sim call (hns_sim_splat_points, hns_point_order_splat_sim) from its names: every refusal that is about the names. which: the
// float fields the call writes
int sim_splat_fields(const char* who, const hns_sim* s, const char* const* names, int n_names, const float* velocity_values, const float* const* values,
                     std::vector<float*>& fields, std::vector<const float*>& vals, std::vector<int>& ncomp, std::vector<int>& which) {
	if (n_names > 0 && !values) return refuse(who, "null list (values)");
	HNS_TRY(sim_fields(who, "names", s, n_names, names_at(names), "takes no point values (it comes from the collision input)", false, which));
	for (size_t i = 0; i < which.size(); ++i) fields.push_back(s->cur[(size_t)which[i]]), vals.push_back(values[i]), ncomp.push_back(1);
	if (velocity_values) fields.push_back(s->vel), vals.push_back(velocity_values), ncomp.push_back(3);
	if (fields.empty()) return refuse(who, "nothing to write (no names and velocity_values is null)");
	return HNS_OK;
}

// a sim call with n > 0 has run: the written buffers no longer hold what a cook handed back; a rewritten velocity is not the one a substep looked ahead from
void sim_splat_wrote(hns_sim* s, const std::vector<int>& which, bool velocity) {
	for (int k : which) s->wrote_field(k);
	if (velocity) s->forget(hns_sim::kVelocity);
}

}  // namespace hns

namespace {

// ---- launcher --------------------------------------------------------------------------------------------------------------------------------------------------------------

// fields / ncomp / values: HOST arrays of n_fields entries; masks: null, or the active masks of a sim on this grid. Every refusal comes before the first launch.
int splat_points(const char* who, hns_grid* g, const hns_splat_spec& sp, float* const* fields, const int* ncomp, int n_fields, const float* xyz,
                 const float* const* values, uint64_t n, int log2_quantum, unsigned char* masks, unsigned char* status, uint64_t* d_rejected, void* stream) {
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
	HNS_TRY(splat_accumulator(g, std::min<int>(kSplatChannels, (int)all.size() + (sp.mode ? 1 : 0)), st));
	const int S = g->splat_channels;
	unsigned long long* acc = g->d_splat.as<unsigned long long>();
	int* touched = (int*)(g->d_splat.as<char>() + splat_acc_bytes(g, S));
	const double scale = std::ldexp(1.0, -log2_quantum), quantum = std::ldexp(1.0, log2_quantum);
	const unsigned n_leaves = (unsigned)g->topo.n_leaves;
	const dim3 pgrid((unsigned)((n + kSplatBlock - 1) / kSplatBlock)), lgrid((n_leaves + 3u) / 4u);
	bool first = true;
	for (const SplatChannels& ch : splat_passes(all, sp)) {  // (a channel's sum does not depend on the others: more launches change nothing numerically)
		if (sp.kernel)
			launch_splat_radial(st, g->dev(), ch, xyz, sp.d_radius, sp.radius, (unsigned)n, scale, acc, S, touched, first ? (unsigned*)masks : nullptr, first ? status : nullptr,
			                    (unsigned long long*)d_rejected);
		else
			hipLaunchKernelGGL(k_splat_points<false>, pgrid, dim3(kSplatBlock), 0, st, g->dev(), ch, xyz, (unsigned)n, scale, acc, S, touched,
			                   first ? (unsigned*)masks : nullptr, first ? status : nullptr, (unsigned long long*)d_rejected);
		first = false;
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
	g->d_splat.release();
	g->splat_channels = 0, g->splat_dirty = false;
}

extern "C" {

int hns_dev_splat_points(hns_grid* g, float* const* fields, const int* ncomp, int n_fields, const float* xyz, const float* const* values, uint64_t n, int log2_quantum,
                         unsigned char* status, uint64_t* d_rejected, void* stream) {
	return splat_points("hns_dev_splat_points", g, g ? g->splat_spec : kDefaultSpec, fields, ncomp, n_fields, xyz, values, n, log2_quantum, nullptr, status, d_rejected, stream);
}

int hns_sim_splat_points(hns_sim* s, const char* const* names, int n_names, const float* velocity_values, const float* xyz, const float* const* values, uint64_t n,
                         int log2_quantum, int activate, unsigned char* status, uint64_t* d_rejected, void* stream) {
	const char* who = "hns_sim_splat_points";
	if (int rc = check_sim(s, who)) return rc;
	std::vector<float*> fields;
	std::vector<const float*> vals;
	std::vector<int> ncomp, which;
	HNS_TRY(sim_splat_fields(who, s, names, n_names, velocity_values, values, fields, vals, ncomp, which));
	HNS_TRY(splat_points(who, s->grid, s->splat_spec, fields.data(), ncomp.data(), (int)fields.size(), xyz, vals.data(), n, log2_quantum, activate ? s->d_masks.as<unsigned char>() : nullptr,
	                     status, d_rejected, stream));
	if (n) sim_splat_wrote(s, which, velocity_values != nullptr);
	return HNS_OK;
}

int hns_grid_set_splat_spec(hns_grid* g, const hns_splat_spec* spec) {
	const char* who = "hns_grid_set_splat_spec";
	if (!g) return refuse(who, "null grid");
	if (spec) HNS_TRY(check_splat_spec(who, *spec));
	g->splat_spec = spec ? *spec : kDefaultSpec;
	return HNS_OK;
}

int hns_sim_set_splat_spec(hns_sim* s, const hns_splat_spec* spec) {
	const char* who = "hns_sim_set_splat_spec";
	if (!s) return refuse(who, "null sim");
	if (spec) HNS_TRY(check_splat_spec(who, *spec));
	s->splat_spec = spec ? *spec : kDefaultSpec;
	return HNS_OK;
}

int hns_grid_get_splat_spec(const hns_grid* g, hns_splat_spec* spec) {
	if (!g || !spec) return refuse("hns_grid_get_splat_spec", "null grid or spec");
	*spec = g->splat_spec;
	return HNS_OK;
}

int hns_sim_get_splat_spec(const hns_sim* s, hns_splat_spec* spec) {
	if (!s || !spec) return refuse("hns_sim_get_splat_spec", "null sim or spec");
	*spec = s->splat_spec;
	return HNS_OK;
}

}  // extern "C"

namespace {

// Host mirror: brute force, the same integers. Every point's footprint as a list of (flat voxel or -1: did not land, weight), then one accumulator of n_voxels words, one
// component after the other; average: the weight accumulator once (it is the same in every pass: a weight's term is always accepted).
int splat_points_host(const char* who, const hns_grid* g, const hns_splat_spec* spec, float* const* fields, const int* ncomp, int n_fields, const float* xyz,
                      const float* const* values, uint64_t n, int log2_quantum, unsigned char* masks, int activate, unsigned char* status, uint64_t* rejected) {
	if (!g) return refuse(who, "null grid");
	const hns_splat_spec sp = spec ? *spec : kDefaultSpec;
	HNS_TRY(check_splat_spec(who, sp));
	HNS_TRY(check_splat_lists(who, fields, ncomp, n_fields, values, n, log2_quantum));
	if (n == 0) return HNS_OK;
	HNS_TRY(check_splat_pointers(who, fields, n_fields, xyz, values, status, rejected));
	HNS_TRY(hns_grid_host_tables(g));
	const Topology& T = g->topo;
	std::vector<size_t> first((size_t)n + 1, 0);  // point p's footprint: tap / weight [first[p], first[p + 1])
	std::vector<int64_t> tap;
	std::vector<float> weight;
	for (uint64_t p = 0; p < n; ++p) {
		const float* x = xyz + 3 * p;
		int in_footprint = 0, landed = 0;
		auto candidate = [&](uint64_t off, float w) {
			tap.push_back((int64_t)off - 1), weight.push_back(w);
			++in_footprint;
			if (!off) return;
			++landed;
			if (masks && activate && w > 0.0f) masks[(off - 1) >> 3] |= (unsigned char)(1u << ((off - 1) & 7u));
		};
		if (sp.kernel) {
			const float r = sp.d_radius ? sp.d_radius[p] : sp.radius;
			if (radial_point(x[0], x[1], x[2], r, sp.radius)) {
				const int E = radial_extent(r), i0 = radial_lo(x[0], r), j0 = radial_lo(x[1], r), k0 = radial_lo(x[2], r);
				const float inv = radial_inv(r);
				for (int i = i0; i < i0 + E; ++i)
					for (int j = j0; j < j0 + E; ++j)
						for (int k = k0; k < k0 + E; ++k) {
							float w;
							if (radial_weight((float)i - x[0], (float)j - x[1], (float)k - x[2], inv, &w)) candidate(T.offset(i, j, k), w);
						}
			}
			if (status) status[p] = (unsigned char)(in_footprint > 0 && landed == in_footprint ? 2 : landed > 0 ? 1 : 0);
		} else {
			const bool finite = std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]);
			const int i = floor_sat(x[0]), j = floor_sat(x[1]), k = floor_sat(x[2]);
			float w[8];
			splat_weights(x[0] - (float)i, x[1] - (float)j, x[2] - (float)k, w);
			for (int c = 0; c < 8; ++c) {  // (corner coordinates wrap at the end of the int32 range, as point_cell's do)
				const int32_t ci = (int32_t)((uint32_t)i + (uint32_t)(c >> 2)), cj = (int32_t)((uint32_t)j + (uint32_t)((c >> 1) & 1)), ck = (int32_t)((uint32_t)k + (uint32_t)(c & 1));
				candidate(finite ? T.offset(ci, cj, ck) : 0, w[c]);
			}
			if (status) status[p] = (unsigned char)landed;
		}
		first[(size_t)p + 1] = tap.size();
	}
	const double scale = std::ldexp(1.0, -log2_quantum), quantum = std::ldexp(1.0, log2_quantum);
	std::vector<uint64_t> acc((size_t)T.n_leaves * 512u), acc_w;
	uint64_t rej = 0;
	// the sum of the accepted terms of one channel; val null: the weight channel (value 1.0f)
	auto accumulate = [&](std::vector<uint64_t>& a, const float* val, uint64_t stride, uint64_t off) {
		std::fill(a.begin(), a.end(), 0);
		for (uint64_t p = 0; p < n; ++p) {
			const float v = val ? val[p * stride + off] : 1.0f;
			for (size_t e = first[(size_t)p]; e < first[(size_t)p + 1]; ++e) {
				if (tap[e] < 0) continue;
				long long k;
				if (!splat_term(weight[e] * v, scale, &k))
					++rej;
				else
					a[(size_t)tap[e]] += (uint64_t)k;
			}
		}
	};
	if (sp.mode) {
		acc_w.resize(acc.size());
		accumulate(acc_w, nullptr, 0, 0);
	}
	for (int f = 0; f < n_fields; ++f)
		for (int comp = 0; comp < ncomp[f]; ++comp) {
			accumulate(acc, values[f], (uint64_t)ncomp[f], (uint64_t)comp);
			for (size_t e = 0; e < acc.size(); ++e)
				splat_finish(sp.mode, acc[e], sp.mode ? acc_w[e] : 0, quantum, sp.min_weight, fields[f] + e * (size_t)ncomp[f] + (size_t)comp);
		}
	if (rejected) *rejected += rej;
	return HNS_OK;
}

}  // namespace

extern "C" {

int hns_grid_splat_points(const hns_grid* g, float* const* fields, const int* ncomp, int n_fields, const float* xyz, const float* const* values, uint64_t n,
                          int log2_quantum, unsigned char* masks, int activate, unsigned char* status, uint64_t* rejected) {
	return splat_points_host("hns_grid_splat_points", g, nullptr, fields, ncomp, n_fields, xyz, values, n, log2_quantum, masks, activate, status, rejected);
}

int hns_grid_splat_points_spec(const hns_grid* g, const hns_splat_spec* spec, float* const* fields, const int* ncomp, int n_fields, const float* xyz,
                               const float* const* values, uint64_t n, int log2_quantum, unsigned char* masks, int activate, unsigned char* status, uint64_t* rejected) {
	return splat_points_host("hns_grid_splat_points_spec", g, spec, fields, ncomp, n_fields, xyz, values, n, log2_quantum, masks, activate, status, rejected);
}

}  // extern "C"
