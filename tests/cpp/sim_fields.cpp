// sim_fields.cpp -- the host preamble of a sim call (hns_simcall.hpp) over shell objects: the one resolver of a named float-field list, check_sim, the row-move and
// capacity checks. The error text, the device count and check_grid are this file's own. Host only: built with AddressSanitizer + UBSan by tests/test_sim_fields.py, never
// loaded into Python, never touches a GPU.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hns_simcall.hpp"

using namespace hns;

#define REQUIRE(c)                                                                                    \
	do {                                                                                              \
		if (!(c)) {                                                                                   \
			std::fprintf(stderr, "FAILED %s:%d: %s (last text: %s)\n", __FILE__, __LINE__, #c, g_text.c_str()); \
			return 1;                                                                                 \
		}                                                                                             \
	} while (0)

// ---- what the header leaves undefined ---------------------------------------------------------------------------------------------------------------------------------
namespace {
std::string g_text;  // the last refusal
int g_devices = 1;
}  // namespace

void hns::set_error(const char* fmt, ...) {
	char buf[1024];
	va_list ap;
	va_start(ap, fmt);
	std::vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	g_text = buf;
}
extern "C" int hns_device_count(void) { return g_devices; }
inline int check_grid(const hns_grid*, const char*) { return HNS_OK; }
// (the pool: a shell sim owns no block, so neither is ever called)
extern "C" int hns_arena_get(size_t, int, void**, size_t*) { std::abort(); }
extern "C" void hns_arena_put(void*, size_t, int) { std::abort(); }

namespace {
bool has(const char* word) { return g_text.find(word) != std::string::npos; }
bool begins(const char* who) { return g_text.rfind(std::string(who) + ": ", 0) == 0; }
// the last call was refused as an invalid argument under `who`
bool refused(int rc, const char* who) { return rc == HNS_ERR_INVALID_ARGUMENT && begins(who); }
}  // namespace

// ---- sim_fields -------------------------------------------------------------------------------------------------------------------------------------------------------
static int field_lists() {
	const char* who = "hns_some_call";
	hns_sim s;
	s.names = {"density", "fuel", "collision_sdf"};
	std::vector<int> which;
	auto list = [&](std::vector<const char*> names, const char* forbid, bool all, int n = -2) {
		which = {7, 7};  // (what a refusal must not leave)
		g_text.clear();
		return sim_fields(who, "names", &s, n == -2 ? (int)names.size() : n, names_at(names.empty() ? nullptr : names.data()), forbid, all, which);
	};
	// index order
	REQUIRE(list({"fuel", "density"}, nullptr, false) == HNS_OK && which == std::vector<int>({1, 0}) && g_text.empty());
	REQUIRE(list({}, nullptr, false) == HNS_OK && which.empty());
	// all fields
	REQUIRE(list({}, nullptr, true, -1) == HNS_OK && which == std::vector<int>({0, 1, 2}));
	REQUIRE(refused(list({}, nullptr, false, -1), who) && which.empty() && has("n_names is -1"));
	REQUIRE(refused(list({}, nullptr, true, -2 - 1), who) && which.empty() && has("n_names is -3"));
	REQUIRE(refused(list({}, nullptr, false, -3), who) && which.empty());
	// a null list, a null name
	REQUIRE(refused(list({}, nullptr, true, 2), who) && which.empty() && has("names[0]") && has("'?'"));
	REQUIRE(refused(list({"density", nullptr, "fuel"}, nullptr, false), who) && which.empty() && has("[1]") && has("?"));
	// an unknown name
	REQUIRE(refused(list({"density", "smoke"}, nullptr, false), who) && which.empty() && has("names[1]: no float field named 'smoke' in this sim"));
	// collision_sdf
	REQUIRE(list({"collision_sdf", "density"}, nullptr, false) == HNS_OK && which == std::vector<int>({2, 0}));
	REQUIRE(refused(list({"density", "collision_sdf"}, "is not for this call", false), who) && which.empty() && has("names[1]: 'collision_sdf' is not for this call"));
	REQUIRE(list({"density", "fuel"}, "is not for this call", false) == HNS_OK && which == std::vector<int>({0, 1}));
	// a duplicate, through both kinds of list
	const int rc = list({"fuel", "density", "fuel"}, nullptr, false);
	REQUIRE(refused(rc, who) && which.empty() && has("names[2]: field 'fuel' is listed twice"));
	const std::string plain = g_text;
	const hns_decay_spec decays[3] = {{"fuel", 1.0f, 0.0f}, {"density", 1.0f, 0.0f}, {"fuel", 2.0f, 0.0f}};
	which = {7};
	REQUIRE(sim_fields(who, "decays", &s, 3, [&](int i) { return decays[i].name; }, "x", false, which) == rc && which.empty());
	REQUIRE(begins(who) && has("decays[2]: field 'fuel' is listed twice"));
	std::string relabelled = g_text;
	relabelled.replace(relabelled.find("decays"), 6, "names");
	REQUIRE(relabelled == plain);
	REQUIRE(sim_fields(who, "decays", &s, 2, [&](int i) { return decays[i].name; }, "x", false, which) == HNS_OK && which == std::vector<int>({1, 0}));
	return 0;
}

// ---- check_sim --------------------------------------------------------------------------------------------------------------------------------------------------------
static int sims() {
	const char* who = "hns_some_call";
	hns_sim s;
	REQUIRE(check_sim(&s, who) == HNS_OK);
	s.cached = true;  // kept by a grid's cook cache ...
	REQUIRE(refused(check_sim(&s, who), who) && g_text == std::string(who) + ": the sim belongs to a grid's cook cache");
	s.cached = false, s.in_use = true;  // ... or lent to an operator call
	REQUIRE(refused(check_sim(&s, who), who) && g_text == std::string(who) + ": the sim belongs to a grid's cook cache");
	g_devices = 0;
	REQUIRE(check_sim(nullptr, who) == HNS_ERR_NO_DEVICE && begins(who) && has("no HIP device"));
	g_devices = 1;
	REQUIRE(refused(check_sim(nullptr, who), who) && has("null sim"));
	return 0;
}

// ---- sim_grid (over this file's check_grid) ------------------------------------------------------------------------------------------------------------------------------
static int grids() {
	const char* who = "hns_some_call";
	hns_grid g;
	g.device = 2, g.topo.n_leaves = 3, g.n_active = 3;
	hns_sim s;
	s.grid = &g, s.n = 512 * 3;
	hns_grid* got = nullptr;
	REQUIRE(sim_grid(who, &s, 2, "thing", true, &got) == HNS_OK && got == &g);
	REQUIRE(refused(sim_grid(who, &s, 1, "thing", true, &got), who) && has("the sim's grid and the thing live on different HIP devices"));
	s.n = 512 * 2;
	REQUIRE(sim_grid(who, &s, 2, "thing", true, &got) == HNS_ERR_RUNTIME && begins(who) && has("not its grid's size"));
	REQUIRE(sim_grid(who, &s, 2, "thing", false, &got) == HNS_OK);
	g.n_active = 0;  // an empty launch range: the call will launch nothing
	REQUIRE(sim_grid(who, &s, 2, "thing", true, &got) == HNS_OK);
	return 0;
}

// ---- check_rows, check_capacity ---------------------------------------------------------------------------------------------------------------------------------------
static int rows() {
	const char* who = "hns_some_move";
	char a[64], b[64];
	const int bad[4] = {0, 2, 6, 68}, good[2] = {4, 64};
	for (int rb : bad) REQUIRE(refused(check_rows(who, true, "sort", 5, a, b, rb), who) && has("row_bytes") && has("a multiple of 4 in 4 .. 64"));
	for (int rb : good) REQUIRE(check_rows(who, true, "sort", 5, a, b, rb) == HNS_OK);
	REQUIRE(refused(check_rows(who, true, "sort", 5, nullptr, b, 12), who) && has("null d_src or d_dst"));
	REQUIRE(refused(check_rows(who, true, "sort", 5, a, nullptr, 12), who) && has("null d_src or d_dst"));
	REQUIRE(refused(check_rows(who, true, "sort", 5, a, a, 12), who) && has("same buffer"));
	REQUIRE(check_rows(who, true, "sort", 0, nullptr, nullptr, 12) == HNS_OK);  // no row: no pointer is looked at
	REQUIRE(refused(check_rows(who, false, "sort", 5, a, b, 12), who) && has("no sort has run on this object"));
	REQUIRE(refused(check_rows(who, false, "select", 0, nullptr, nullptr, 2), who) && has("no select has run on this object"));  // before the row size
	REQUIRE(check_capacity(who, 100, 100) == HNS_OK && check_capacity(who, 0, 0) == HNS_OK);
	REQUIRE(refused(check_capacity(who, 101, 100), who) && has("n 101 is above the capacity 100"));
	REQUIRE(kMaxPoints == 0x7fffffffull);
	return 0;
}

int main() {
	if (field_lists() || sims() || grids() || rows()) return 1;
	std::printf("sim_fields OK\n");
	return 0;
}
