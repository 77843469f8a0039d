// Yardstick (calibration, not product, never linked into libhns.so): rocprim::radix_sort_pairs on the uint32 keys profiles/micro/point_order_time.py wrote, values = the
// point indices, over the key bits our sort covers. Prints one JSON line: the median, min and max of `reps` sorts in ms, hipEvents round each.
// build: hipcc --offload-arch=gfx950 -O3 point_order_rocprim.hip -o point_order_rocprim        run: point_order_rocprim KEYS.bin BITS [REPS]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <vector>

#define CHECK(call)                                                                      \
	do {                                                                                 \
		hipError_t e = (call);                                                           \
		if (e != hipSuccess) {                                                           \
			fprintf(stderr, "%s failed: %s\n", #call, hipGetErrorString(e));             \
			return 2;                                                                    \
		}                                                                                \
	} while (0)

int main(int argc, char** argv) {
	if (argc < 3) return fprintf(stderr, "usage: %s KEYS.bin BITS [REPS]\n", argv[0]), 1;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return fprintf(stderr, "cannot read %s\n", argv[1]), 1;
	fseek(f, 0, SEEK_END);
	const size_t n = (size_t)ftell(f) / 4;
	fseek(f, 0, SEEK_SET);
	std::vector<unsigned> keys(n), idx(n);
	if (fread(keys.data(), 4, n, f) != n) return fprintf(stderr, "short read\n"), 1;
	fclose(f);
	for (size_t i = 0; i < n; ++i) idx[i] = (unsigned)i;
	const unsigned bits = (unsigned)atoi(argv[2]);
	const int reps = argc > 3 ? atoi(argv[3]) : 20;
	unsigned *k_in, *k_out, *v_in, *v_out;
	CHECK(hipMalloc(&k_in, 4 * n));
	CHECK(hipMalloc(&k_out, 4 * n));
	CHECK(hipMalloc(&v_in, 4 * n));
	CHECK(hipMalloc(&v_out, 4 * n));
	CHECK(hipMemcpy(k_in, keys.data(), 4 * n, hipMemcpyHostToDevice));
	CHECK(hipMemcpy(v_in, idx.data(), 4 * n, hipMemcpyHostToDevice));
	size_t temp_bytes = 0;
	CHECK(rocprim::radix_sort_pairs(nullptr, temp_bytes, k_in, k_out, v_in, v_out, n, 0, bits, 0));
	void* temp = nullptr;
	CHECK(hipMalloc(&temp, temp_bytes));
	hipEvent_t e0, e1;
	CHECK(hipEventCreate(&e0));
	CHECK(hipEventCreate(&e1));
	std::vector<float> ms;
	for (int rep = 0; rep < reps + 3; ++rep) {
		CHECK(hipEventRecord(e0, 0));
		CHECK(rocprim::radix_sort_pairs(temp, temp_bytes, k_in, k_out, v_in, v_out, n, 0, bits, 0));
		CHECK(hipEventRecord(e1, 0));
		CHECK(hipEventSynchronize(e1));
		float t = 0;
		CHECK(hipEventElapsedTime(&t, e0, e1));
		if (rep >= 3) ms.push_back(t);
	}
	std::vector<unsigned> out(n);
	CHECK(hipMemcpy(out.data(), k_out, 4 * n, hipMemcpyDeviceToHost));
	const bool sorted = std::is_sorted(out.begin(), out.end());
	std::sort(ms.begin(), ms.end());
	printf("{\"rocprim_radix_sort_pairs_ms\": {\"min\": %.4f, \"median\": %.4f, \"max\": %.4f}, \"n\": %zu, \"bits\": %u, \"temp_bytes\": %zu, \"sorted\": %s}\n", ms.front(),
	       ms[ms.size() / 2], ms.back(), n, bits, temp_bytes, sorted ? "true" : "false");
	return sorted ? 0 : 3;
}
