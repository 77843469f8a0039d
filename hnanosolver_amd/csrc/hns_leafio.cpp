// hns_leafio.cpp -- the steps either side of the path, without OpenVDB: what the reference's
// HNS::IndexGridBuilder (src/Utils/GridBuilder.hpp:87-216) and the domain dilation of SOP_HNanoSolverVerb::cook
// (src/SOP/HNanoSolver/SOP_HNanoSolver.cpp:186-199) do to OpenVDB trees, restated over raw 8^3 leaf buffers: a leaf is its
// 8-aligned origin, an optional 512-bit active mask (byte x*8+y, bit z) and 512 values in x<<6|y<<3|z order -- exactly an
// OpenVDB LeafNode's origin, value mask and buffer. Host code (the reference does this on the host with TBB).
//
// PARITY UNPINNED: OpenVDB is absent from this image, so nothing here has been checked against the reference's output; the
// tests check it against brute force. Quirks kept on purpose: leaves missing from an SDF source are
// filled with BYTES 0x01 (memset(..., 1, ...), GridBuilder.hpp:108: 0x01010101 = 2.4e-38f, not 1.0f), from any other source
// with zeros (:125-129,147-151); tile values of the sources are ignored (only leaves are probed, :105,122,144); output grids
// receive all 512 values of every domain leaf (:198-211).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <unordered_set>

#include "hns_birth.hpp"
#include "hns_dilate.hpp"
#include "hns_neighbours.hpp"
#include "hns_originhash.hpp"
#include "hns_seed.hpp"
#include "hns_stats.hpp"

using namespace hns;

namespace {

struct Key {
	int32_t x, y, z;
	bool operator==(const Key& o) const { return x == o.x && y == o.y && z == o.z; }
};
struct KeyHash {
	size_t operator()(const Key& k) const { return (size_t)hash_origin(k.x, k.y, k.z) * 0x9E3779B97F4A7C15ull ^ (size_t)(uint32_t)k.z; }
};

// OpenVDB's leaf order (LeafManager over root table -> 32^3 -> 16^3 children, x major) = NanoVDB's (tests/fields.nanovdb_order):
// signed root-tile coordinate (coord >> 12) x, y, z; then child offset in the 4096^3 node; then in the 128^3 node.
bool leaf_less(const Key& a, const Key& b) {
	auto parts = [](const Key& k, int64_t (&p)[5]) {
		p[0] = k.x >> 12, p[1] = k.y >> 12, p[2] = k.z >> 12;
		p[3] = ((int64_t)((k.x & 4095) >> 7) << 10) | ((int64_t)((k.y & 4095) >> 7) << 5) | ((k.z & 4095) >> 7);
		p[4] = ((int64_t)((k.x & 127) >> 3) << 8) | ((int64_t)((k.y & 127) >> 3) << 4) | ((k.z & 127) >> 3);
	};
	int64_t pa[5], pb[5];
	parts(a, pa);
	parts(b, pb);
	return std::lexicographical_compare(pa, pa + 5, pb, pb + 5);
}

int emit_sorted(std::vector<Key>& keys, int32_t* out, uint64_t capacity, uint64_t* n_out, const char* who) {
	std::sort(keys.begin(), keys.end(), leaf_less);
	if (n_out) *n_out = keys.size();
	if (!out) return HNS_OK;
	if (keys.size() > capacity) {
		set_error("%s: %zu leaves do not fit the output capacity %llu", who, keys.size(), (unsigned long long)capacity);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	for (size_t i = 0; i < keys.size(); ++i) out[3 * i] = keys[i].x, out[3 * i + 1] = keys[i].y, out[3 * i + 2] = keys[i].z;
	return HNS_OK;
}

int check_aligned(const int32_t* o, uint64_t n, const char* who) {
	for (uint64_t i = 0; i < 3 * n; ++i)
		if (o[i] & 7) {
			set_error("%s: leaf origin %llu is not 8-aligned", who, (unsigned long long)(i / 3));
			return HNS_ERR_TOPOLOGY;
		}
	return HNS_OK;
}

}  // namespace

// OpenVDB leaf order of an origin list in place (hns_regrid.hip): the same order as leaf_less, by one precomputed key per leaf -- root tile (20 bits per
// axis, biased), then the 15-bit child offset in the 4096^3 node and the 12-bit one in the 128^3 node.
namespace {
inline void leaf_sort_key(int32_t x, int32_t y, int32_t z, uint64_t& tile, uint32_t& node) {
	tile = ((uint64_t)((x >> 12) + (1 << 19)) << 40) | ((uint64_t)((y >> 12) + (1 << 19)) << 20) | (uint64_t)((z >> 12) + (1 << 19));
	node = ((uint32_t)(((x & 4095) >> 7) << 10 | ((y & 4095) >> 7) << 5 | ((z & 4095) >> 7)) << 12) |
	       (uint32_t)(((x & 127) >> 3) << 8 | ((y & 127) >> 3) << 4 | ((z & 127) >> 3));
}
}  // namespace

void hns::sort_leaf_origins(int32_t* xyz, size_t n) {
	struct Item {
		uint64_t tile;
		uint32_t node;
		int32_t x, y, z;
	};
	std::vector<Item> v(n);
	for (size_t i = 0; i < n; ++i) {
		const int32_t x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
		v[i] = Item{0, 0, x, y, z};
		leaf_sort_key(x, y, z, v[i].tile, v[i].node);
	}
	std::sort(v.begin(), v.end(), [](const Item& a, const Item& b) { return a.tile != b.tile ? a.tile < b.tile : a.node < b.node; });
	for (size_t i = 0; i < n; ++i) xyz[3 * i] = v[i].x, xyz[3 * i + 1] = v[i].y, xyz[3 * i + 2] = v[i].z;
}

// The same order as a permutation, for whoever carries something with each leaf (distinct origins: the keys are distinct).
void hns::leaf_order(const int32_t* xyz, size_t n, std::vector<uint32_t>* perm) {
	struct Item {
		uint64_t tile;
		uint32_t node, at;
	};
	std::vector<Item> v(n);
	for (size_t i = 0; i < n; ++i) {
		v[i].at = (uint32_t)i;
		leaf_sort_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], v[i].tile, v[i].node);
	}
	std::sort(v.begin(), v.end(), [](const Item& a, const Item& b) { return a.tile != b.tile ? a.tile < b.tile : a.node < b.node; });
	perm->resize(n);
	for (size_t i = 0; i < n; ++i) (*perm)[i] = v[i].at;
}

int hns::check_activity_fields(const hns_sim* s, const hns_activity_field* fields, int n_fields, const char* who, std::vector<int>* field_of) {
	if (n_fields < 1 || !fields) {
		set_error("%s: bad field list (%d fields%s)", who, n_fields, fields ? "" : ", NULL list");
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (field_of) field_of->assign((size_t)n_fields, -1);
	bool velocity = false;
	for (int i = 0; i < n_fields; ++i) {
		const hns_activity_field& q = fields[i];
		const char* nm = q.name ? q.name : "(null)";
		if (q.ncomp != 1 && q.ncomp != 3) {
			set_error("%s: field %d ('%s'): ncomp %d (1 or 3)", who, i, nm, q.ncomp);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		if (q.name && !strcmp(q.name, "collision_sdf")) {
			set_error("%s: field %d: 'collision_sdf' cannot be deactivated (its topology comes from the collision input)", who, i);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		if (s) {
			const int f = q.name ? s->find(q.name) : -1;
			if (q.ncomp == 1 && f < 0) {
				set_error("%s: field %d: the sim has no float field '%s'", who, i, nm);
				return HNS_ERR_INVALID_ARGUMENT;
			}
			if (q.ncomp == 3 && f >= 0) {
				set_error("%s: field %d: ncomp 3 under the float field name '%s'", who, i, nm);
				return HNS_ERR_INVALID_ARGUMENT;
			}
			if (field_of) (*field_of)[(size_t)i] = q.ncomp == 1 ? f : -1;
		} else if (q.ncomp == 1 && !q.name) {
			set_error("%s: field %d: a float field needs a name", who, i);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		if (q.ncomp == 3) {
			if (velocity) {
				set_error("%s: field %d: a second velocity entry", who, i);
				return HNS_ERR_INVALID_ARGUMENT;
			}
			velocity = true;
		} else {
			for (int j = 0; j < i; ++j)
				if (fields[j].ncomp == 1 && fields[j].name && !strcmp(fields[j].name, q.name)) {
					set_error("%s: field %d: a second entry for '%s'", who, i, nm);
					return HNS_ERR_INVALID_ARGUMENT;
				}
		}
		if (!(q.tolerance >= 0.0f)) {
			set_error("%s: field %d ('%s'): tolerance %g (>= 0, not NaN)", who, i, nm, (double)q.tolerance);
			return HNS_ERR_INVALID_ARGUMENT;
		}
	}
	return HNS_OK;
}

extern "C" {

// IndexGridBuilder::build (GridBuilder.hpp:99-154): for every leaf of the domain, the source leaf with the same origin is
// copied whole; a domain leaf the source lacks is filled (zeros, or bytes 0x01 for an SDF source).
int hns_gather_leaves(const int32_t* domain_origins, uint64_t n_domain, const int32_t* src_origins, uint64_t n_src, const float* src_values, int ncomp, int fill,
                      float* out) {
	if ((n_domain && (!domain_origins || !out)) || (n_src && (!src_origins || !src_values)) || (ncomp != 1 && ncomp != 3) ||
	    (fill != HNS_FILL_ZERO && fill != HNS_FILL_SDF))
		return fail(HNS_ERR_INVALID_ARGUMENT, "hns_gather_leaves: bad arguments");
	std::unordered_map<Key, uint64_t, KeyHash> where;
	where.reserve((size_t)n_src * 2);
	for (uint64_t i = 0; i < n_src; ++i) where[Key{src_origins[3 * i], src_origins[3 * i + 1], src_origins[3 * i + 2]}] = i;
	const size_t leaf_floats = 512u * (size_t)ncomp;
	for (uint64_t i = 0; i < n_domain; ++i) {
		float* dst = out + i * leaf_floats;
		const auto it = where.find(Key{domain_origins[3 * i], domain_origins[3 * i + 1], domain_origins[3 * i + 2]});
		if (it != where.end())
			memcpy(dst, src_values + it->second * leaf_floats, leaf_floats * sizeof(float));
		else
			memset(dst, fill == HNS_FILL_SDF ? 1 : 0, leaf_floats * sizeof(float));
	}
	return HNS_OK;
}

// IndexGridBuilder::writeIndexGrid (GridBuilder.hpp:171-213): every domain leaf receives its 512 values.
int hns_scatter_leaves(const float* flat, uint64_t n_domain, int ncomp, float* const* leaf_buffers) {
	if ((n_domain && (!flat || !leaf_buffers)) || (ncomp != 1 && ncomp != 3)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_scatter_leaves: bad arguments");
	const size_t leaf_floats = 512u * (size_t)ncomp;
	for (uint64_t i = 0; i < n_domain; ++i) {
		if (!leaf_buffers[i]) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_scatter_leaves: null leaf buffer");
		memcpy(leaf_buffers[i], flat + i * leaf_floats, leaf_floats * sizeof(float));
	}
	return HNS_OK;
}

// Leaves of the domain after dilateVoxels(padding, NN_FACE_EDGE_VERTEX, IGNORE_TILES) (SOP_HNanoSolver.cpp:190-193): a leaf is
// in the result iff some ACTIVE voxel lies within `padding` voxels (Chebyshev distance: faces, edges and vertices) of its
// box. The index grid then takes every voxel of those leaves (the domain is leaf-dense, GridBuilder.hpp:156-166,229).
// active_masks: n x 64 bytes, NULL = every voxel active. Output in OpenVDB leaf order; out may be NULL to query n_out.
int hns_dilate_leaves(const int32_t* origins, uint64_t n, const unsigned char* active_masks, int padding_voxels, int32_t* out_origins, uint64_t capacity,
                      uint64_t* n_out) {
	if ((n && !origins) || padding_voxels < 0 || padding_voxels > 1024) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dilate_leaves: bad arguments");
	if (int rc = check_aligned(origins, n, "hns_dilate_leaves")) return rc;
	const int p = padding_voxels, D = (p + 7) / 8;
	std::unordered_set<Key, KeyHash> have;
	have.reserve((size_t)n * 4);
	for (uint64_t i = 0; i < n; ++i) {
		const Key o{origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]};
		const unsigned char* m = active_masks ? active_masks + 64 * i : nullptr;
		bool any = !m;
		for (int b = 0; m && b < 64 && !any; ++b) any = m[b] != 0;
		if (!any) continue;  // a leaf without active voxels contributes nothing (it would not be a leaf of the mask tree)
		for (int dx = -D; dx <= D; ++dx)
			for (int dy = -D; dy <= D; ++dy)
				for (int dz = -D; dz <= D; ++dz) {
					const int d[3] = {dx, dy, dz};
					int lo[3], hi[3];
					bool possible = true;
					for (int a = 0; a < 3; ++a) {
						lo[a] = d[a] > 0 ? std::max(0, 8 * d[a] - p) : 0;
						hi[a] = d[a] < 0 ? std::min(7, 8 * d[a] + 7 + p) : 7;
						possible &= lo[a] <= hi[a];
					}
					if (!possible) continue;
					bool hit = !m;
					for (int x = lo[0]; m && x <= hi[0] && !hit; ++x)
						for (int y = lo[1]; y <= hi[1] && !hit; ++y) {
							const unsigned zmask = (0xFFu >> (7 - hi[2])) & (0xFFu << lo[2]);
							hit = (m[x * 8 + y] & zmask) != 0;
						}
					if (!hit) continue;
					const int64_t nx = (int64_t)o.x + 8 * dx, ny = (int64_t)o.y + 8 * dy, nz = (int64_t)o.z + 8 * dz;
					if (nx < INT32_MIN || nx > INT32_MAX - 7 || ny < INT32_MIN || ny > INT32_MAX - 7 || nz < INT32_MIN || nz > INT32_MAX - 7) continue;
					have.insert(Key{(int32_t)nx, (int32_t)ny, (int32_t)nz});
				}
	}
	std::vector<Key> keys(have.begin(), have.end());
	return emit_sorted(keys, out_origins, capacity, n_out, "hns_dilate_leaves");
}

// hns_dilate_leaves plus the dilated ACTIVE MASKS themselves: frame n+1's domain depends on them (SOP_HNanoSolver.cpp:186-199 dilates the velocity's
// active topology, and the output grids keep that topology, GridBuilder.hpp:198-214). Every leaf of the result receives the OR of what each leaf within
// reach contributes (hns_dilate.hpp: the separable box dilation); a leaf is in the result iff that OR is not empty, which is hns_dilate_leaves' test.
// Leaf set and order are hns_dilate_leaves'. out_origins / out_masks may be NULL to query *n_out.
int hns_dilate_leaf_masks(const int32_t* origins, uint64_t n, const unsigned char* active_masks, int padding_voxels, int32_t* out_origins,
                          unsigned char* out_masks, uint64_t capacity, uint64_t* n_out) {
	if ((n && !origins) || padding_voxels < 0 || padding_voxels > 1024) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dilate_leaf_masks: bad arguments");
	if (int rc = check_aligned(origins, n, "hns_dilate_leaf_masks")) return rc;
	const int p = padding_voxels, D = (p + 7) / 8;
	struct Mask {
		uint64_t w[8];
	};
	std::unordered_map<Key, Mask, KeyHash> have;
	have.reserve((size_t)n * 4);
	for (uint64_t i = 0; i < n; ++i) {
		const Key o{origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]};
		uint64_t m[8], any = 0;
		for (int x = 0; x < 8; ++x) {
			if (active_masks)
				memcpy(&m[x], active_masks + 64 * i + 8 * x, 8);
			else
				m[x] = ~0ull;
			any |= m[x];
		}
		if (!any) continue;
		for (int dx = -D; dx <= D; ++dx)
			for (int dy = -D; dy <= D; ++dy)
				for (int dz = -D; dz <= D; ++dz) {
					uint64_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
					if (!dilate_into(m, -8 * dx, -8 * dy, -8 * dz, p, c)) continue;
					const int64_t nx = (int64_t)o.x + 8 * dx, ny = (int64_t)o.y + 8 * dy, nz = (int64_t)o.z + 8 * dz;
					if (nx < INT32_MIN || nx > INT32_MAX - 7 || ny < INT32_MIN || ny > INT32_MAX - 7 || nz < INT32_MIN || nz > INT32_MAX - 7) continue;
					Mask& t = have.try_emplace(Key{(int32_t)nx, (int32_t)ny, (int32_t)nz}, Mask{{0, 0, 0, 0, 0, 0, 0, 0}}).first->second;
					for (int x = 0; x < 8; ++x) t.w[x] |= c[x];
				}
	}
	std::vector<Key> keys;
	keys.reserve(have.size());
	for (const auto& kv : have) keys.push_back(kv.first);
	if (out_masks && keys.size() > capacity) {
		set_error("hns_dilate_leaf_masks: %zu leaves do not fit the output capacity %llu", keys.size(), (unsigned long long)capacity);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (int rc = emit_sorted(keys, out_origins, capacity, n_out, "hns_dilate_leaf_masks")) return rc;
	if (out_masks)
		for (size_t i = 0; i < keys.size(); ++i) memcpy(out_masks + 64 * i, have[keys[i]].w, 64);
	return HNS_OK;
}

// openvdb::tools::compSum(a, b) over two leaf sets (SOP_HNanoSolver.cpp:159-179): every leaf of either side, masks ORed, values fl(a + b) per component
// where the side without the leaf contributes +0.0f (so a -0.0f on one side alone becomes +0.0f). Leaf order is hns_union_leaves'.
int hns_add_leaves(const int32_t* a_origins, uint64_t na, const unsigned char* a_masks, const float* a_values, const int32_t* b_origins, uint64_t nb,
                   const unsigned char* b_masks, const float* b_values, int ncomp, int32_t* out_origins, unsigned char* out_masks, float* out_values,
                   uint64_t capacity, uint64_t* n_out) {
	if ((na && (!a_origins || !a_values)) || (nb && (!b_origins || !b_values)) || (ncomp != 1 && ncomp != 3))
		return fail(HNS_ERR_INVALID_ARGUMENT, "hns_add_leaves: bad arguments");
	if (int rc = check_aligned(a_origins, na, "hns_add_leaves")) return rc;
	if (int rc = check_aligned(b_origins, nb, "hns_add_leaves")) return rc;
	std::unordered_map<Key, std::pair<int64_t, int64_t>, KeyHash> at;  // origin -> (leaf of a, leaf of b), -1 = absent
	at.reserve((size_t)(na + nb) * 2);
	for (int side = 0; side < 2; ++side) {
		const int32_t* o = side ? b_origins : a_origins;
		const uint64_t n = side ? nb : na;
		for (uint64_t i = 0; i < n; ++i) {
			auto& e = at.try_emplace(Key{o[3 * i], o[3 * i + 1], o[3 * i + 2]}, std::pair<int64_t, int64_t>{-1, -1}).first->second;
			int64_t& slot = side ? e.second : e.first;
			if (slot >= 0) {
				set_error("hns_add_leaves: duplicate leaf origin (%d, %d, %d) in input %c", o[3 * i], o[3 * i + 1], o[3 * i + 2], side ? 'b' : 'a');
				return HNS_ERR_TOPOLOGY;
			}
			slot = (int64_t)i;
		}
	}
	std::vector<Key> keys;
	keys.reserve(at.size());
	for (const auto& kv : at) keys.push_back(kv.first);
	if ((out_masks || out_values) && keys.size() > capacity) {
		set_error("hns_add_leaves: %zu leaves do not fit the output capacity %llu", keys.size(), (unsigned long long)capacity);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (int rc = emit_sorted(keys, out_origins, capacity, n_out, "hns_add_leaves")) return rc;
	const size_t leaf_floats = 512u * (size_t)ncomp;
	for (size_t i = 0; i < keys.size() && (out_masks || out_values); ++i) {
		const auto ab = at[keys[i]];
		if (out_masks)
			for (int w = 0; w < 64; ++w) {
				const unsigned char ma = ab.first < 0 ? 0 : a_masks ? a_masks[64 * ab.first + w] : 0xFF;
				const unsigned char mb = ab.second < 0 ? 0 : b_masks ? b_masks[64 * ab.second + w] : 0xFF;
				out_masks[64 * i + w] = ma | mb;
			}
		if (out_values) {
			const float* va = ab.first < 0 ? nullptr : a_values + (size_t)ab.first * leaf_floats;
			const float* vb = ab.second < 0 ? nullptr : b_values + (size_t)ab.second * leaf_floats;
			float* dst = out_values + i * leaf_floats;
			for (size_t k = 0; k < leaf_floats; ++k) dst[k] = (va ? va[k] : 0.0f) + (vb ? vb[k] : 0.0f);
		}
	}
	return HNS_OK;
}

// The seeds of a point set (include/hns.h states the definition): brute force over the eight taps of every seeding point, the leaves in OpenVDB leaf order. What
// hns_dev_point_leaves (hns_seed.hip) is checked against, byte for byte.
int hns_point_leaves(const float* xyz, uint64_t n, int32_t* origins_out, unsigned char* masks_out, uint64_t cap, uint64_t* n_leaves, uint64_t* skipped) {
	if (!n_leaves) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_point_leaves: n_leaves is null");
	*n_leaves = 0;
	if (skipped) *skipped = 0;
	if (n > kMaxSeedPoints) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_point_leaves: n is above 2^31 - 1");
	if (n && !xyz) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_point_leaves: xyz is null");
	struct Mask {
		unsigned char b[64];
	};
	std::unordered_map<Key, Mask, KeyHash> have;
	uint64_t skip = 0;
	for (uint64_t p = 0; p < n; ++p) {
		const float* q = xyz + 3 * p;
		if (!(seeds_f(q[0]) && seeds_f(q[1]) && seeds_f(q[2]))) {
			++skip;
			continue;
		}
		const int32_t c[3] = {(int32_t)std::floor(q[0]), (int32_t)std::floor(q[1]), (int32_t)std::floor(q[2])};
		for (int t = 0; t < 8; ++t) {
			const int32_t x = c[0] + (t >> 2), y = c[1] + ((t >> 1) & 1), z = c[2] + (t & 1);
			Mask& m = have.try_emplace(Key{x & ~7, y & ~7, z & ~7}, Mask{}).first->second;
			m.b[(x & 7) * 8 + (y & 7)] |= (unsigned char)(1u << (z & 7));
		}
	}
	if (skipped) *skipped = skip;
	if (have.size() > kMaxSeedLeaves) return fail(HNS_ERR_TOPOLOGY, "hns_point_leaves: the points hold more than 2^23 distinct leaves");
	*n_leaves = have.size();
	if (!origins_out || have.size() > cap) return HNS_OK;  // (the query of the two-call idiom)
	std::vector<int32_t> o;
	o.reserve(have.size() * 3);
	for (const auto& kv : have) o.insert(o.end(), {kv.first.x, kv.first.y, kv.first.z});
	sort_leaf_origins(o.data(), have.size());
	memcpy(origins_out, o.data(), o.size() * sizeof(int32_t));
	if (masks_out)
		for (size_t i = 0; i < have.size(); ++i) memcpy(masks_out + 64 * i, have[Key{o[3 * i], o[3 * i + 1], o[3 * i + 2]}].b, 64);
	return HNS_OK;
}

// The leaf order of a point set (include/hns.h states the definition): the keys by brute force over the topology's offsets, std::stable_sort, the ranges by counting.
// What hns_point_order_sort (hns_pointorder.hip) is checked against, byte for byte.
int hns_grid_sort_points(const hns_grid* g, const float* xyz, uint64_t n, int level, uint32_t* perm, uint32_t* keys, uint32_t* leaf_start) {
	const char* who = "hns_grid_sort_points";
	if (!g) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_grid_sort_points: null grid");
	if (n > kMaxSeedPoints) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_grid_sort_points: n is above 2^31 - 1");
	if (n && !xyz) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_grid_sort_points: xyz is null");
	if (n && !perm) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_grid_sort_points: perm is null");
	if (level != 0 && level != 1) {
		set_error("%s: level %d (0: by leaf, 1: by voxel)", who, level);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	const uint64_t L = (uint64_t)g->topo.n_leaves;
	if ((L + 2) * 512 > (uint64_t(1) << 32)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_grid_sort_points: the grid's voxel keys do not fit 32 bits ((leaves + 2) * 512 > 2^32)");
	if (int rc = hns_grid_host_tables(g)) return rc;
	std::vector<uint32_t> key((size_t)n);
	std::vector<uint32_t> count((size_t)L + 3, 0);  // [q + 1]: points with leaf-level key q, then their running sum
	for (uint64_t p = 0; p < n; ++p) {
		const float* q = xyz + 3 * p;
		uint32_t k = (uint32_t)(512 * (L + 1));
		if (seeds_f(q[0]) && seeds_f(q[1]) && seeds_f(q[2])) {
			const uint64_t off = g->topo.offset((int32_t)std::floor(q[0]), (int32_t)std::floor(q[1]), (int32_t)std::floor(q[2]));
			k = off ? (uint32_t)(off - 1) : (uint32_t)(512 * L);
		}
		++count[(size_t)(k >> 9) + 1];
		key[(size_t)p] = level ? k : k >> 9;
	}
	for (uint64_t p = 0; p < n; ++p) perm[p] = (uint32_t)p;
	std::stable_sort(perm, perm + n, [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
	if (keys)
		for (uint64_t r = 0; r < n; ++r) keys[r] = key[perm[r]];
	if (leaf_start) {
		leaf_start[0] = 0;
		for (uint64_t q = 1; q < L + 3; ++q) leaf_start[q] = leaf_start[q - 1] + count[(size_t)q];
	}
	return HNS_OK;
}

// Point neighbourhoods (include/hns.h: "POINT NEIGHBOURHOODS THROUGH A LEAF ORDER"): the voxel keys of hns_grid_sort_points, a cell list by counting, and for every point
// that takes part a walk over the cells of its box with the pair arithmetic of hns_neighbours.hpp. What hns_point_order_neighbours (hns_neighbours.hip) is checked
// against, byte for byte; rows in the original order.
int hns_grid_point_neighbours(const hns_grid* g, const float* xyz, uint64_t n, float radius, uint32_t* count, float* density, float* push) {
	const char* who = "hns_grid_point_neighbours";
	auto refused = [&](const char* what) {
		set_error("%s: %s", who, what);
		return HNS_ERR_INVALID_ARGUMENT;
	};
	if (!g) return refused("null grid");
	if (n > kMaxSeedPoints) return refused("n is above 2^31 - 1");
	if (!neighbour_radius(radius)) {
		set_error("%s: radius %g (0 < radius <= 2)", who, (double)radius);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (n && !xyz) return refused("xyz is null");
	if (!count && !density && !push) return refused("count, density and push are all null");
	if ((count && (const void*)count == (const void*)xyz) || (density && density == xyz) || (push && push == xyz)) return refused("an output is xyz");
	if ((count && (const void*)count == (const void*)density) || (count && (const void*)count == (const void*)push) || (density && density == push))
		return refused("two outputs are the same buffer");
	const uint64_t L = (uint64_t)g->topo.n_leaves;
	if ((L + 2) * 512 > (uint64_t(1) << 32)) return refused("the grid's voxel keys do not fit 32 bits ((leaves + 2) * 512 > 2^32)");
	if (!n) return HNS_OK;
	if (int rc = hns_grid_host_tables(g)) return rc;
	// cell list: start[v] .. start[v + 1] of `order` are the points of voxel v, in index order; a point in no cell takes no part
	const uint32_t none = 0xFFFFFFFFu;
	std::vector<uint32_t> cell((size_t)n, none), start((size_t)(512 * L + 1), 0);
	for (uint64_t p = 0; p < n; ++p) {
		const float* q = xyz + 3 * p;
		if (!(seeds_f(q[0]) && seeds_f(q[1]) && seeds_f(q[2]))) continue;
		const uint64_t off = g->topo.offset((int32_t)std::floor(q[0]), (int32_t)std::floor(q[1]), (int32_t)std::floor(q[2]));
		if (!off) continue;
		cell[(size_t)p] = (uint32_t)(off - 1);
		++start[(size_t)off];
	}
	for (size_t v = 1; v < start.size(); ++v) start[v] += start[v - 1];
	std::vector<uint32_t> order((size_t)start.back()), fill(start.begin(), start.end() - 1);
	for (uint64_t p = 0; p < n; ++p)
		if (cell[(size_t)p] != none) order[fill[cell[(size_t)p]]++] = (uint32_t)p;
	const float inv = radial_inv(radius);
	for (uint64_t p = 0; p < n; ++p) {
		NeighbourSums s;
		if (cell[(size_t)p] != none) {
			const float* x = xyz + 3 * p;
			int lo[3], hi[3];
			for (int c = 0; c < 3; ++c) neighbour_box(x[c], radius, &lo[c], &hi[c]);
			for (int i = lo[0]; i <= hi[0]; ++i)
				for (int j = lo[1]; j <= hi[1]; ++j)
					for (int k = lo[2]; k <= hi[2]; ++k) {
						const uint64_t off = g->topo.offset(i, j, k);
						if (!off) continue;
						for (uint32_t at = start[(size_t)off - 1]; at < start[(size_t)off]; ++at) {
							const uint32_t o = order[at];
							if (o == p) continue;
							const float* y = xyz + 3 * (size_t)o;
							neighbour_pair(x[0], x[1], x[2], y[0], y[1], y[2], inv, s);
						}
					}
		}
		if (count) count[p] = s.count;
		if (density) density[p] = neighbour_total(s.w);
		if (push) push[3 * p] = neighbour_total(s.px), push[3 * p + 1] = neighbour_total(s.py), push[3 * p + 2] = neighbour_total(s.pz);
	}
	return HNS_OK;
}

// Points born from a field (include/hns.h: "BIRTH AND DEATH OF POINTS"): voxel by voxel in index order, the count and the positions of hns_birth.hpp. What
// hns_point_population_birth (hns_population.hip) is checked against, byte for byte.
int hns_grid_birth_points(const hns_grid* g, const float* field, const unsigned char* masks, const hns_birth_spec* sp, uint64_t start, float* xyz, uint32_t* voxel,
                          uint64_t capacity_rows, uint64_t* live, uint64_t* wanted) {
	const char* who = "hns_grid_birth_points";
	auto refused = [&](const char* what) {
		set_error("%s: %s", who, what);
		return HNS_ERR_INVALID_ARGUMENT;
	};
	if (!g) return refused("null grid");
	if (const char* what = birth_spec_refusal(sp)) return refused(what);
	if (capacity_rows > kMaxSeedPoints) return refused("capacity_rows is above 2^31 - 1");
	if (start > kMaxSeedPoints) return refused("start is above 2^31 - 1");
	const uint64_t L = (uint64_t)g->topo.n_leaves;
	if (L * 512 > (uint64_t(1) << 32)) return refused("the grid's voxel indices do not fit 32 bits (leaves * 512 > 2^32)");
	if (L && !field) return refused("null field");
	if (capacity_rows && !xyz) return refused("null xyz");
	if (xyz && ((const void*)xyz == (const void*)field || (const void*)xyz == (const void*)voxel)) return refused("xyz is field or voxel");
	uint64_t row = start;
	for (uint64_t l = 0; l < L; ++l) {
		const int32_t* o = &g->topo.origins[4 * (size_t)l];
		for (uint32_t v = 0; v < 512; ++v) {
			const int i = o[0] + (int)(v >> 6), j = o[1] + (int)((v >> 3) & 7), k = o[2] + (int)(v & 7);
			const uint64_t e = 512 * l + v;
			uint32_t h = 0;
			const uint32_t c = birth_count(field[e], !masks || (masks[64 * l + (v >> 3)] >> (v & 7) & 1), i, j, k, *sp, &h);
			for (uint32_t q = 0; q < c; ++q, ++row) {
				if (row >= capacity_rows) continue;
				xyz[3 * row] = birth_position(i, h, q, 0), xyz[3 * row + 1] = birth_position(j, h, q, 1), xyz[3 * row + 2] = birth_position(k, h, q, 2);
				if (voxel) voxel[row] = (uint32_t)e;
			}
		}
	}
	const uint64_t alive = std::min(row, capacity_rows);
	if (sp->fill)
		for (uint64_t r = alive; r < capacity_rows; ++r) {
			const uint32_t nan = kBirthNaN;
			for (int a = 0; a < 3; ++a) memcpy(&xyz[3 * r + a], &nan, 4);
			if (voxel) voxel[r] = kBirthNoVoxel;
		}
	if (live) *live = alive;
	if (wanted) *wanted = row;
	return HNS_OK;
}

// topologyUnion of two leaf sets (SOP_HNanoSolver.cpp:189,195-197), in OpenVDB leaf order, duplicates removed.
int hns_union_leaves(const int32_t* a, uint64_t na, const int32_t* b, uint64_t nb, int32_t* out_origins, uint64_t capacity, uint64_t* n_out) {
	if ((na && !a) || (nb && !b)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_union_leaves: bad arguments");
	if (int rc = check_aligned(a, na, "hns_union_leaves")) return rc;
	if (int rc = check_aligned(b, nb, "hns_union_leaves")) return rc;
	std::unordered_set<Key, KeyHash> have;
	have.reserve((size_t)(na + nb) * 2);
	for (uint64_t i = 0; i < na; ++i) have.insert(Key{a[3 * i], a[3 * i + 1], a[3 * i + 2]});
	for (uint64_t i = 0; i < nb; ++i) have.insert(Key{b[3 * i], b[3 * i + 1], b[3 * i + 2]});
	std::vector<Key> keys(have.begin(), have.end());
	return emit_sorted(keys, out_origins, capacity, n_out, "hns_union_leaves");
}

// hns_sim_deactivate on the host, voxel by voxel: the brute force the device's ballot kernel is checked against.
int hns_deactivate_leaf_masks(uint64_t n_leaves, const unsigned char* masks_in, const hns_activity_field* fields, const float* const* values, int n_fields,
                              unsigned char* masks_out, uint64_t* counts) {
	const char* who = "hns_deactivate_leaf_masks";
	if (int rc = check_activity_fields(nullptr, fields, n_fields, who, nullptr)) return rc;
	if (n_leaves && (!masks_out || !values)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_deactivate_leaf_masks: masks_out or values NULL");
	for (int i = 0; i < n_fields && n_leaves; ++i)
		if (!values[i]) {
			set_error("%s: field %d: values NULL", who, i);
			return HNS_ERR_INVALID_ARGUMENT;
		}
	uint64_t voxels = 0, leaves = 0;
	for (uint64_t l = 0; l < n_leaves; ++l) {
		uint64_t in_leaf = 0;
		for (int w = 0; w < 64; ++w) {  // mask byte w = x*8+y holds voxels 8w .. 8w+7 (bit z)
			const unsigned char old = masks_in ? masks_in[64 * l + w] : 0xFF;
			unsigned char keep = 0;
			for (int z = 0; z < 8; ++z) {
				if (!(old >> z & 1)) continue;
				const uint64_t v = 512 * l + 8 * (uint64_t)w + (uint64_t)z;
				bool quiet = true;
				for (int i = 0; i < n_fields && quiet; ++i)
					for (int c = 0; c < fields[i].ncomp && quiet; ++c) quiet = std::fabs(values[i][v * (uint64_t)fields[i].ncomp + (uint64_t)c]) <= fields[i].tolerance;
				if (!quiet) keep |= (unsigned char)(1u << z);
			}
			masks_out[64 * l + w] = keep;
			in_leaf += (uint64_t)__builtin_popcount(keep);
		}
		voxels += in_leaf;
		leaves += in_leaf != 0;
	}
	if (counts) counts[0] = voxels, counts[1] = leaves;
	return HNS_OK;
}

// hns_sim_stats / hns_dev_field_stats / the record of hns_dev_residual on the host, voxel by voxel, through the trees of hns_stats.hpp: what the device's records are
// checked against, byte for byte.
int hns_leaf_stats(uint64_t n_leaves, const unsigned char* masks, const float* values, int ncomp, hns_stats* out) {
	if ((ncomp != 1 && ncomp != 3) || !out || (n_leaves && !values)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_leaf_stats: bad arguments");
	std::vector<hns_stats> row((size_t)std::max<uint64_t>(n_leaves, 1));
	for (int c = 0; c < ncomp; ++c) {
		for (uint64_t l = 0; l < n_leaves; ++l) {
			hns_stats lane[64];
			for (int L = 0; L < 64; ++L) {  // lane L: voxels 64k + L, k ascending
				hns_stats& a = lane[L];
				a = stats_empty();
				for (int k = 0; k < 8; ++k) {
					const int v = 64 * k + L;
					const bool on = !masks || (masks[64 * l + (uint64_t)(v >> 3)] >> (v & 7) & 1);
					const float x = values[(512 * l + (uint64_t)v) * (uint64_t)ncomp + (uint64_t)c];
					const bool use = on && !(x != x);
					hns_stats t = stats_empty();  // the voxel's term
					t.count = on, t.nan_count = on && x != x;
					if (use) t.min = t.max = x, t.max_abs = std::fabs(x), t.sum = (double)x, t.sum_sq = (double)x * (double)x;
					if (k == 0)
						a = t;
					else
						stats_combine(a, t);
				}
			}
			for (int m = 1; m < 64; m *= 2)  // the butterfly, as the tree it is
				for (int L = 0; L < 64; L += 2 * m) stats_combine(lane[L], lane[L + m]);
			row[(size_t)l] = lane[0];
		}
		if (n_leaves)
			stats_fold(row.data(), n_leaves);
		else
			row[0] = stats_empty();
		stats_finish(row[0]);
		out[c] = row[0];
	}
	return HNS_OK;
}

}  // extern "C"
