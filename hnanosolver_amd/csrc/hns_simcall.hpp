// hns_simcall.hpp -- the host code in front of the first launch of a call on a sim or on one of the objects (hns_point_order, hns_point_population, hns_point_motion,
// hns_shaping, hns_diffusion), stated once: every refusal comes before the first launch, and a refused call changes nothing. No kernel and no device function lives here.
// A new operator on a sim checks in this order: its numbers and host structs, its object (null?), the sim (check_sim), the names (sim_fields), the grid (sim_grid).
#pragma once

#include <algorithm>
#include <cstring>
#include <vector>

#include "hns_internal.hpp"

inline int check_grid(const hns_grid* g, const char* who);  // hns_device.hpp

namespace hns {

inline int refuse(const char* who, const char* what) {
	set_error("%s: %s", who, what);
	return HNS_ERR_INVALID_ARGUMENT;
}

constexpr uint64_t kMaxPoints = 0x7fffffffull;

// a sim a call may use: not null (without a device there is none to pass: hns_sim_create refused, and the caller learns why here too), not lent to a cook cache
inline int check_sim(const hns_sim* s, const char* who) {
	if (!s) {
		if (hns_device_count() == 0) {
			set_error("%s: no HIP device (there is no CPU fallback)", who);
			return HNS_ERR_NO_DEVICE;
		}
		return refuse(who, "null sim");
	}
	if (s->cached || s->in_use) return refuse(who, "the sim belongs to a grid's cook cache");
	return HNS_OK;
}

// ---- a named list of float fields ----

// The float field indices of the n names name_at(0 .. n - 1), in list order, into `which` (empty after every refusal). `list` is what the caller's argument is called
// ("names", "decays", "terms"). Refused, in this order: n below 0 (all_if_minus_one: below -1; n == -1 then yields every field), a null name, a name the sim lacks,
// collision_sdf where forbid_reason says why it may not be listed, a name listed twice. Reads s->names and nothing else.
template <class NameAt>
int sim_fields(const char* who, const char* list, const hns_sim* s, int n, const NameAt& name_at, const char* forbid_reason, bool all_if_minus_one, std::vector<int>& which) {
	which.clear();
	auto no = [&](const char* fmt, int i, const char* name) {
		which.clear();
		set_error(fmt, who, list, i, name, forbid_reason);
		return HNS_ERR_INVALID_ARGUMENT;
	};
	if (n < (all_if_minus_one ? -1 : 0)) {
		set_error("%s: n_%s is %d", who, list, n);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (n < 0)
		for (size_t i = 0; i < s->names.size(); ++i) which.push_back((int)i);
	for (int i = 0; i < n; ++i) {
		const char* name = name_at(i);
		const int k = name ? s->find(name) : -1;
		if (k < 0) return no("%s: %s[%d]: no float field named '%s' in this sim", i, name ? name : "?");
		if (forbid_reason && !strcmp(name, "collision_sdf")) return no("%s: %s[%d]: '%s' %s", i, name);
		if (std::find(which.begin(), which.end(), k) != which.end()) return no("%s: %s[%d]: field '%s' is listed twice", i, name);
		which.push_back(k);
	}
	return HNS_OK;
}
// name_at of a plain list of names (a null list has null names)
inline auto names_at(const char* const* names) {
	return [names](int i) { return names ? names[i] : nullptr; };
}

// ---- from a checked sim to its grid ----

// g: the sim's grid, usable by an object (`what`) on `device`. sized: the call addresses the sim's buffers by the grid's leaves, so they must be the grid's size.
inline int sim_grid(const char* who, const hns_sim* s, int device, const char* what, bool sized, hns_grid** g) {
	*g = s->grid;
	HNS_TRY(check_grid(*g, who));
	if ((*g)->device != device) {
		set_error("%s: the sim's grid and the %s live on different HIP devices", who, what);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (sized && (*g)->n_active && s->n != 512 * (uint64_t)(*g)->topo.n_leaves) {
		set_error("%s: the sim's buffers are not its grid's size", who);
		return HNS_ERR_RUNTIME;
	}
	return HNS_OK;
}

// ---- the objects ----

// A new T for *_create: on the grid's device (on_grid: `g` must be there and have device tables) or on the current one. capacity: of an object that holds per-point memory (else
// 0). init(o) fills the object and returns its status; o->device is set. *err (may be null) receives the status, and a failed create returns null and leaves nothing behind.
template <class T, class Init>
T* make_object(const char* who, int* err, bool on_grid, const hns_grid* g, uint64_t capacity, const char* host_twin, const Init& init) {
	auto out = [&](int rc, T* o) {
		if (err) *err = rc;
		return o;
	};
	if (on_grid && !g) return out(refuse(who, "null grid"), nullptr);
	if (capacity > kMaxPoints) return out(refuse(who, "capacity is above 2^31 - 1"), nullptr);
	if (hns_device_count() == 0) {
		set_error("%s: no HIP device (there is no CPU fallback%s)", who, host_twin);
		return out(HNS_ERR_NO_DEVICE, nullptr);
	}
	if (on_grid && !g->on_device) return out(refuse(who, "the grid is HNS_GRID_HOST_ONLY: it has no device tables"), nullptr);
	int device = on_grid ? g->device : -1;
	if (!on_grid && hipGetDevice(&device) != hipSuccess) {
		set_error("%s: no current HIP device", who);
		return out(HNS_ERR_HIP, nullptr);
	}
	DeviceScope on(device);
	T* o = new T;
	o->device = device;
	const int rc = init(o);
	if (rc != HNS_OK) {
		delete o;
		return out(rc, nullptr);
	}
	return out(HNS_OK, o);
}

template <class T>
int set_object_stream(T* o, void* hip_stream, const char* who, const char* null_what) {
	if (!o) return refuse(who, null_what);
	o->stream = (hipStream_t)hip_stream;
	return HNS_OK;
}

// n points in an object of `capacity`
inline int check_capacity(const char* who, uint64_t n, uint64_t capacity) {
	if (n <= capacity) return HNS_OK;
	set_error("%s: n %llu is above the capacity %llu", who, (unsigned long long)n, (unsigned long long)capacity);
	return HNS_ERR_INVALID_ARGUMENT;
}

// a move of n rows of row_bytes from d_src to d_dst through what the object's last `what_ran` ("sort", "select") left; ran: has one run?
inline int check_rows(const char* who, bool ran, const char* what_ran, uint64_t n, const void* d_src, const void* d_dst, int row_bytes) {
	if (!ran) {
		set_error("%s: no %s has run on this object", who, what_ran);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (row_bytes < 4 || row_bytes > 64 || row_bytes % 4) {
		set_error("%s: row_bytes %d (a multiple of 4 in 4 .. 64)", who, row_bytes);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (n && (!d_src || !d_dst)) return refuse(who, "null d_src or d_dst");
	if (n && d_src == d_dst) return refuse(who, "d_src and d_dst are the same buffer");
	return HNS_OK;
}

}  // namespace hns
