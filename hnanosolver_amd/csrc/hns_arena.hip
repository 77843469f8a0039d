// hns_arena.hip -- the process-wide pool of device allocations. Nobody calls it directly: a block is held by an hns::Pooled (hns_pool.hpp), which draws it here and gives
// it back when it goes. Its users: a sim's fields, masks, deactivation table (hns_api.hip, hns_regrid.hip), diagnostics (hns_diagnostics.hip) and multigrid levels
// (hns_multigrid.hip); a grid's tables (hns_gridbuild.hip), block records (hns_sorblock.hip), statistics table and splat accumulator (hns_splat.hip); a point order with its
// cell table (hns_pointorder.hip, hns_neighbours.hip) and a point population (hns_population.hip); a partitioned rank's fields (hns_dist_plan.hip); and the scratch of a
// regrid or a seed call (hns::Scratch).
// A sim's fields are slices of ONE device allocation, and allocations that are no longer needed go to a small
// process-wide pool instead of back to the driver. The reference pays cudaMallocAsync x 15+ and the matching frees every
// cook (HNanoSolver.cu:87-133,361-369); with separate hipMallocs here a cold cook at 256^3 spent 4.2 ms in hipFree
// alone. A sparse simulation changes its topology nearly every frame, so "cold" is its normal cook: with the pool the
// new grid's fields land in the previous grid's memory whenever that is large enough. hns_trim_memory() empties it.
#include <mutex>
#include <vector>

#include "hns_internal.hpp"

using namespace hns;

namespace {
struct Arena {
	void* p;
	size_t bytes;
	int device;
};
std::mutex g_pool_mutex;
std::vector<Arena> g_pool;  // at most kPoolMax idle arenas
constexpr size_t kPoolMax = 6;  // simulation states (GBs) and grid tables (MBs) share it; the smallest goes first

// Option "arena_fill" (tests): the whole block, headroom included, holds the chosen byte when its new owner gets it. The wait is arena_put's promise
// again: the owner may use the block on any stream. Called outside g_pool_mutex. A block that cannot be filled goes back to the driver: the caller gets none.
int arena_fill(Arena& a, int fill) {
	DeviceScope scope(a.device);
	if (hipMemset(a.p, fill, a.bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess) return HNS_OK;
	(void)hipGetLastError();
	(void)hipFree(a.p);
	a = Arena{nullptr, 0, -1};
	return fail(HNS_ERR_HIP, "arena_fill: filling a pooled block failed");
}

int arena_get(size_t need, int device, Arena& out) {
	const int fill = options().arena_fill.load(std::memory_order_relaxed);
	bool pooled = false;
	{
		std::lock_guard<std::mutex> lock(g_pool_mutex);
		int best = -1;
		for (size_t i = 0; i < g_pool.size(); ++i)
			if (g_pool[i].device == device && g_pool[i].bytes >= need && g_pool[i].bytes <= 2 * need + (64u << 20) &&
			    (best < 0 || g_pool[i].bytes < g_pool[(size_t)best].bytes))
				best = (int)i;
		if (best >= 0) {
			out = g_pool[(size_t)best];
			g_pool.erase(g_pool.begin() + best);
			pooled = true;
		}
	}
	if (pooled) return fill < 0 ? (int)HNS_OK : arena_fill(out, fill);
	out.bytes = need + need / 8;  // headroom: the next, slightly larger topology still fits
	out.device = device;
	DeviceScope scope(device);
	if (hipMalloc(&out.p, out.bytes) != hipSuccess) {
		(void)hipGetLastError();
		std::vector<Arena> drop;  // out of memory with idle arenas around: release them and retry at the exact size
		{
			std::lock_guard<std::mutex> lock(g_pool_mutex);
			drop.swap(g_pool);
		}
		for (Arena& a : drop) (void)hipFree(a.p);
		out.bytes = need;
		HNS_HIP(hipMalloc(&out.p, out.bytes));
	}
	return fill < 0 ? (int)HNS_OK : arena_fill(out, fill);
}

// The hipFree this pool replaces waits for the device; so does this: whoever draws the memory next may use it on any
// stream without ordering itself after the previous owner's queued kernels and copies. Cooks are synchronous, so the
// device is normally idle here and the wait costs microseconds.
void arena_put(const Arena& a) {
	if (!a.p) return;
	DeviceScope scope(a.device);
	(void)hipDeviceSynchronize();
	Arena evict{nullptr, 0, -1};
	{
		std::lock_guard<std::mutex> lock(g_pool_mutex);
		g_pool.push_back(a);
		if (g_pool.size() > kPoolMax) {  // drop the smallest
			size_t k = 0;
			for (size_t i = 1; i < g_pool.size(); ++i)
				if (g_pool[i].bytes < g_pool[k].bytes) k = i;
			evict = g_pool[k];
			g_pool.erase(g_pool.begin() + (long)k);
		}
	}
	if (evict.p) (void)hipFree(evict.p);
}
}  // namespace

extern "C" int hns_arena_get(size_t need, int device, void** p, size_t* bytes) {
	Arena a{nullptr, 0, -1};
	const int rc = arena_get(need, device, a);
	*p = a.p;
	*bytes = a.bytes;
	return rc;
}
extern "C" void hns_arena_put(void* p, size_t bytes, int device) { arena_put(Arena{p, bytes, device}); }

// Returns the idle pooled device memory to the driver.
extern "C" int hns_trim_memory(void) {
	std::vector<Arena> drop;
	{
		std::lock_guard<std::mutex> lock(g_pool_mutex);
		drop.swap(g_pool);
	}
	for (Arena& a : drop) HNS_HIP(hipFree(a.p));
	return HNS_OK;
}
