// pool_owner.cpp -- the owner of a pooled block, the scratch of a call and the one way to lay slices over a block (hns_pool.hpp), over a pool of this file's own: malloc / free
// with a log of every call. And the two layouts that lie under every kernel (hns_internal.hpp: hns::sim_slices, hns::grid_slices) against offsets worked by hand from
// the formulas they replaced. Host only: built with AddressSanitizer + UBSan by tests/test_pool_owner.py, never loaded into Python, never touches a GPU.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "hns_internal.hpp"

using namespace hns;

#define REQUIRE(c)                                                             \
	do {                                                                       \
		if (!(c)) {                                                            \
			std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
			return 1;                                                          \
		}                                                                      \
	} while (0)

// ---- the pool: every call logged; a get may be told to fail -----------------------------------------------------------------------------------------------------------
namespace {
struct Call {
	char what;  // 'g' / 'p'
	void* p;
	size_t bytes;
	int device;
};
std::vector<Call> g_log;
int g_fail_gets = 0;         // the next so many gets fail
constexpr size_t kSlack = 64;  // a block is this much larger than asked for, as the real pool's are

// every get of the log matched by exactly one put, of the same block, size and device, and no other put; then the log starts afresh
bool settled() {
	std::vector<Call> live;
	for (const Call& c : g_log) {
		if (c.what == 'g') {
			live.push_back(c);
			continue;
		}
		size_t i = 0;
		while (i < live.size() && live[i].p != c.p) ++i;
		if (i == live.size() || live[i].bytes != c.bytes || live[i].device != c.device) return false;
		live.erase(live.begin() + (long)i);
	}
	g_log.clear();
	return live.empty();
}
}  // namespace

extern "C" int hns_arena_get(size_t need, int device, void** p, size_t* bytes) {
	if (g_fail_gets > 0) {
		--g_fail_gets;
		*p = nullptr, *bytes = 0;
		return HNS_ERR_HIP;
	}
	*p = std::aligned_alloc(256, pad256(need + kSlack));
	*bytes = need + kSlack;
	g_log.push_back(Call{'g', *p, *bytes, device});
	return *p ? HNS_OK : HNS_ERR_HIP;
}
extern "C" void hns_arena_put(void* p, size_t bytes, int device) {
	g_log.push_back(Call{'p', p, bytes, device});
	std::free(p);
}

// ---- the owner --------------------------------------------------------------------------------------------------------------------------------------------------------
static int owner() {
	{
		Pooled none;  // an empty owner: nothing on destruction, nothing on release
		none.release();
		REQUIRE(!none && none.as<char>() == nullptr);
	}
	REQUIRE(g_log.empty());
	{
		Pooled a;
		REQUIRE(a.get(1000, 3) == HNS_OK);
		REQUIRE(a && a.bytes == 1000 + kSlack && a.device == 3 && g_log.size() == 1);
		void* const pa = a.p;
		a.as<unsigned char>()[999] = 7;  // (the typed accessor; AddressSanitizer watches the write)
		Pooled b(std::move(a));            // move-construct: no call, the source is empty
		REQUIRE(!a && a.bytes == 0 && b.p == pa && b.bytes == 1000 + kSlack && b.device == 3 && g_log.size() == 1);
		Pooled c;
		REQUIRE(c.get(500, 3) == HNS_OK && g_log.size() == 2);
		void* const pc = c.p;
		b = std::move(c);  // move-assign onto a full owner: the old block is put exactly once
		REQUIRE(g_log.size() == 3 && g_log[2].what == 'p' && g_log[2].p == pa && g_log[2].bytes == 1000 + kSlack && g_log[2].device == 3);
		REQUIRE(!c && b.p == pc);
		b = std::move(c);  // ... and an empty one onto it: put, and both are empty
		REQUIRE(g_log.size() == 4 && g_log[3].what == 'p' && g_log[3].p == pc && !b && !c);
	}
	REQUIRE(g_log.size() == 4);  // (three empty owners went)
	REQUIRE(settled());
	{
		Pooled r;
		REQUIRE(r.reserve(1000, 0) == HNS_OK && g_log.size() == 1 && g_log[0].what == 'g');
		void* const p0 = r.p;
		REQUIRE(r.reserve(10, 0) == HNS_OK && r.p == p0 && g_log.size() == 1);             // smaller: no call
		REQUIRE(r.reserve(r.bytes, 0) == HNS_OK && r.p == p0 && g_log.size() == 1);        // equal: no call
		REQUIRE(r.reserve(r.bytes + 1, 0) == HNS_OK && g_log.size() == 3);                 // larger: one put, then one get
		REQUIRE(g_log[1].what == 'p' && g_log[1].p == p0 && g_log[2].what == 'g' && g_log[2].p == r.p && r.bytes == 1000 + kSlack + 1 + kSlack);
		g_fail_gets = 1;
		REQUIRE(r.reserve(r.bytes + 1, 0) == HNS_ERR_HIP);  // a failed get inside reserve: the old block went back, the owner is empty
		REQUIRE(g_log.size() == 4 && g_log[3].what == 'p' && !r && r.bytes == 0);
		r.release(), r.release();  // release twice (of an empty owner): nothing
		REQUIRE(g_log.size() == 4);
		REQUIRE(r.get(8, 0) == HNS_OK && g_log.size() == 5);
		r.release();
		r.release();  // twice: one put
		REQUIRE(g_log.size() == 6 && g_log[5].what == 'p' && !r);
	}
	REQUIRE(g_log.size() == 6);
	return 0;
}

// ---- the scratch of a call --------------------------------------------------------------------------------------------------------------------------------------------
static int scratch() {
	REQUIRE(settled());
	Pooled kept;
	void *p0 = nullptr, *p1 = nullptr, *p2 = nullptr;
	{
		Scratch s(1);
		REQUIRE(s.get(100, &p0) == HNS_OK && s.get(200, &p1) == HNS_OK && s.get(300, &p2) == HNS_OK);
		REQUIRE(s.held.size() == 3 && s.held[1].p == p1 && s.held.back().p == p2 && g_log.size() == 3);
		kept = std::move(s.held[1]);  // handed out by move
		REQUIRE(g_log.size() == 3);
		int *a = nullptr, *b = nullptr;
		g_fail_gets = 1;
		REQUIRE(s.carve([&](const Slice& slice) { slice(a, 40), slice(b, 400); }) == HNS_ERR_HIP);  // a carve whose get fails: no block, no pointer moved
		REQUIRE(s.held.size() == 3 && !a && !b && g_log.size() == 3);
		REQUIRE(s.carve([&](const Slice& slice) { slice(a, 40), slice(b, 400); }) == HNS_OK);
		REQUIRE(s.held.size() == 4 && (void*)a == s.held[3].p && (char*)b == (char*)a + 256 && g_log.size() == 4 && g_log[3].bytes == 768 + kSlack);
		b[99] = 1;
	}
	REQUIRE(g_log.size() == 7);  // the other two and the carved one went back at scope exit
	for (size_t i = 4; i < 7; ++i) REQUIRE(g_log[i].what == 'p' && g_log[i].p != p1 && g_log[i].device == 1);
	REQUIRE(kept.p == p1 && kept.bytes == 200 + kSlack);
	kept.release();
	REQUIRE(g_log.size() == 8 && g_log[7].p == p1);
	return 0;
}

// ---- carve ------------------------------------------------------------------------------------------------------------------------------------------------------------
static int carving() {
	REQUIRE(settled());
	const size_t sizes[5] = {0, 1, 255, 256, 257};
	const size_t want[7] = {0, 0, 256, 512, 768, 1280, 1280 + 3 * 512};  // the offsets of the five, of the "3 units" slice behind them, and the room
	char* ptr[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
	float* units = nullptr;
	char* const untouched = (char*)&ptr;  // what a sizing walk must leave in place
	ptr[0] = untouched;
	auto list = [&](const Slice& slice) {
		for (int i = 0; i < 5; ++i) slice(ptr[i], sizes[i]);
		slice(units, 3, 512);
	};
	REQUIRE(carve(nullptr, list) == want[6] && ptr[0] == untouched && !ptr[1] && !units);  // sums the padded sizes, moves nothing
	std::vector<char> plain(want[6] + 256);  // memory that is not the pool's
	char* const base = (char*)pad256((size_t)plain.data());
	REQUIRE(carve(base, list) == want[6] && g_log.empty());
	for (int i = 0; i < 5; ++i) REQUIRE(ptr[i] == base + want[i] && ((size_t)ptr[i] & 255) == 0);
	REQUIRE((char*)units == base + want[5] && ((size_t)units & 255) == 0);
	REQUIRE(ptr[0] == ptr[1]);  // a zero-byte slice shares its successor's address
	for (int i = 0; i + 1 < 5; ++i) REQUIRE(ptr[i] + sizes[i] <= ptr[i + 1]);  // in order, disjoint
	REQUIRE(ptr[4] + sizes[4] <= (char*)units && (char*)units + 3 * 512 == base + want[6]);  // ... and inside the block
	bool placed[2] = {true, false};
	carve(nullptr, [&](const Slice& slice) { placed[0] = slice(ptr[1], 1); });
	carve(base, [&](const Slice& slice) { placed[1] = slice(ptr[1], 1); });
	REQUIRE(!placed[0] && placed[1]);  // what a list that uploads behind a slice goes by
	Pooled block;
	REQUIRE(carve(block, 2, list) == HNS_OK && g_log.size() == 1 && g_log[0].bytes == want[6] + kSlack && g_log[0].device == 2);
	for (int i = 0; i < 5; ++i) REQUIRE(ptr[i] == block.as<char>() + want[i]);
	units[3 * 128 - 1] = 1.0f;  // the last float of the last slice lies inside the block
	return 0;
}

// ---- the two layouts --------------------------------------------------------------------------------------------------------------------------------------------------
static int layouts() {
	REQUIRE(settled());
	std::vector<char> mem(1);  // (only its address is used)
	char* const A = mem.data();
	{
		hns_sim s;
		s.names = {"density", "fuel", "waste", "temperature", "flame"};
		REQUIRE(sim_unit(1000) == 4096);
		REQUIRE(hns_sim_arena_need(&s, 1000) == 106752);
		hns_sim_layout(&s, A, 1000);
		REQUIRE(s.n == 1000 && (char*)s.vel == A + 0 && (char*)s.adv == A + 12288 && (char*)s.tmp == A + 24576);
		REQUIRE((char*)s.div == A + 36864 && (char*)s.p_a == A + 40960 && (char*)s.p_b == A + 45056 && s.p_result == s.p_a);
		REQUIRE(s.cur.size() == 5 && s.nxt.size() == 5);
		for (size_t i = 0; i < 5; ++i) REQUIRE((char*)s.cur[i] == A + 49152 + 8192 * i && (char*)s.nxt[i] == A + 49152 + 8192 * i + 4096);
		REQUIRE((char*)s.q4 == A + 90112 && (char*)s.d_dig == A + 106496);
		REQUIRE(!s.arena);  // a layout owns nothing
		s.names = {"density"};
		REQUIRE(hns_sim_arena_need(&s, 1000) == 57600);
		hns_sim_layout(&s, A, 1000);
		REQUIRE(s.cur.size() == 1 && (char*)s.cur[0] == A + 49152 && (char*)s.nxt[0] == A + 53248 && s.q4 == nullptr && (char*)s.d_dig == A + 57344);
		REQUIRE(hns_sim_arena_need(&s, 0) == 14 * 256 + 256);  // no voxels: one element per field
	}
	const size_t want[3][7] = {{0, 256, 512, 768, 1024, 1280, 1536},   // no leaf is laid out as one
	                           {0, 256, 512, 768, 1024, 1280, 1536},   // one leaf: every table within 256 bytes (the hash: 16 slots + the status word = 68 bytes)
	                           {0, 256, 768, 1024, 1280, 1792, 2048}};  // three: nbr27 324 and blk 336 bytes take 512 each
	const int leaves[3] = {0, 1, 3};
	for (int k = 0; k < 3; ++k) {
		hns_grid g;
		g.topo.n_leaves = leaves[k];
		g.topo.hash_mask = 15;  // the smallest hash (Topology::prepare: 16 slots up to seven leaves)
		auto list = [&](const Slice& slice) { grid_slices(g, slice); };
		REQUIRE(carve(nullptr, list) == want[k][6] && g.d_origins == nullptr);
		REQUIRE(carve(A, list) == want[k][6]);
		void* const got[6] = {g.d_origins, g.d_nbr27, g.d_hash, g.d_sched_mem, g.d_blk, g.d_scratch};
		for (int i = 0; i < 6; ++i) REQUIRE((char*)got[i] == A + want[k][i]);
		REQUIRE(!g.d_arena && g.d_sched == nullptr);
	}
	REQUIRE(g_log.empty());  // sims and grids came and went: no layout touched the pool
	return 0;
}

int main() {
	if (owner() || scratch() || carving() || layouts()) return 1;
	REQUIRE(settled());  // (every part began with a settled log: over the whole run every get is matched by exactly one put)
	std::printf("pool_owner OK\n");
	return 0;
}
