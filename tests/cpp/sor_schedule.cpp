// sor_schedule.cpp -- the pressure loop's launch schedule (hns_internal.hpp: hns::sor_schedule, a pure function of the block edge, the most iterations a launch does and the
// iteration count) against the two loops it replaced, restated here word for word, and against a table written by hand from the rule in include/hns.h. Host only: built with
// AddressSanitizer + UBSan by tests/test_sor_schedule.py, never loaded into Python, never touches a GPU.
#include <cstdio>
#include <vector>

#include "hns_internal.hpp"

#define REQUIRE(c)                                                                                                                      \
	do {                                                                                                                                \
		if (!(c)) {                                                                                                                     \
			std::fprintf(stderr, "FAILED %s:%d: %s (lb = %d, k_max = %d, iterations = %d)\n", __FILE__, __LINE__, #c, lb, k_max, iterations); \
			return 1;                                                                                                                   \
		}                                                                                                                               \
	} while (0)

// the loop hns_rbgs_iterate ran before it walked a schedule: the iterations of every ping-pong step, in order (a colour iteration is one step)
static std::vector<int> steps_of_the_old_iterate(int lb, int k_max, int iterations) {
	std::vector<int> steps;
	int left = iterations, launches = 0;
	while (lb && left >= 2) {
		const int k = (k_max >= 4 && left >= 4) ? 4 : 2;
		steps.push_back(k);
		left -= k, ++launches;
	}
	if (lb && left) {
		steps.push_back(1);
		--left, ++launches;
	}
	for (; left; --left, ++launches) steps.push_back(1);
	return (int)steps.size() == launches ? steps : std::vector<int>{-1};
}

// the loop hns_grid_rbgs_plan ran: kernel launches (a colour iteration is two) and iterations per launch
static void plan_of_the_old_plan(int lb, int k_max, int iterations, int* launches, int* per_launch) {
	int n = 0, k = 1, left = iterations;
	if (lb) {
		while (left >= 2) left -= (k_max >= 4 && left >= 4) ? 4 : 2, ++n;
		if (left) --left, ++n;
		k = iterations >= 2 ? k_max : 1;
	}
	n += 2 * left;
	*launches = n, *per_launch = k;
}

struct Row {
	int lb, k_max, iterations;
	std::vector<int> steps;
	int launches, per_launch;
};

int main() {
	int checked = 0;
	for (int lb = 0; lb <= 2; ++lb)
		for (int k_max : {2, 4}) {
			if (k_max == 4 && lb != 1) continue;
			for (int iterations = 0; iterations <= 64; ++iterations, ++checked) {
				const hns::SorSchedule s = hns::sor_schedule(lb, k_max, iterations);
				const std::vector<int> want = steps_of_the_old_iterate(lb, k_max, iterations);
				REQUIRE(s.steps() == (int)want.size());
				for (int i = 0; i < s.steps(); ++i) REQUIRE(s.step(i) == want[(size_t)i]);
				int launches = -1, per_launch = -1;
				plan_of_the_old_plan(lb, k_max, iterations, &launches, &per_launch);
				REQUIRE(s.launches() == launches && s.iterations_per_launch() == per_launch);
				REQUIRE(s.iterations() == iterations && s.lb == (iterations ? lb : 0));
				REQUIRE(s.one_blocked_launch() == (lb != 0 && want.size() == 1));
			}
		}
	const Row table[] = {
	    {1, 4, 7, {4, 2, 1}, 3, 4}, {1, 4, 6, {4, 2}, 2, 4},      {1, 4, 5, {4, 1}, 2, 4},      {1, 4, 3, {2, 1}, 2, 4}, {2, 2, 5, {2, 2, 1}, 3, 2}, {2, 2, 1, {1}, 1, 1},
	    {0, 2, 3, {1, 1, 1}, 6, 1}, {0, 4, 3, {1, 1, 1}, 6, 1},   {0, 0, 3, {1, 1, 1}, 6, 1},   {0, 2, 0, {}, 0, 1},     {1, 4, 0, {}, 0, 1},        {1, 2, 0, {}, 0, 1},
	    {2, 2, 0, {}, 0, 1},        {1, 2, 2, {2}, 1, 2},         {1, 4, 2, {2}, 1, 4},         {1, 4, 4, {4}, 1, 4},    {1, 4, 1, {1}, 1, 1},
	};
	for (const Row& r : table) {
		const int lb = r.lb, k_max = r.k_max, iterations = r.iterations;
		const hns::SorSchedule s = hns::sor_schedule(lb, k_max, iterations);
		REQUIRE(s.steps() == (int)r.steps.size());
		for (int i = 0; i < s.steps(); ++i) REQUIRE(s.step(i) == r.steps[(size_t)i]);
		REQUIRE(s.launches() == r.launches && s.iterations_per_launch() == r.per_launch);
		REQUIRE((s.lb != 0) == (lb != 0 && iterations != 0));
	}
	std::printf("sor_schedule OK (%d cases)\n", checked);
	return 0;
}
