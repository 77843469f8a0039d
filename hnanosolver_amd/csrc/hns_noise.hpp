// hns_noise.hpp -- the curl noise of hns_shaping_apply (include/hns.h: "SHAPING A SIM" states it line by line): the lattice position of a voxel, the corner hash, the
// gradient table, the fades, the six partials and the curl of one octave, stated once for k_shape (hns_shaping.hip) and the host evaluation hns_shaping_curl_host, so that
// the two cannot drift. Every line is one rounded float32 operation (-ffp-contract=off); the integer arithmetic is uint32, wrapping. H is birth_hash of hns_birth.hpp.
#pragma once

#include <cmath>

#include "hns_birth.hpp"

namespace hns {

constexpr int kNoiseMaxOctaves = 4;
constexpr float kNoiseFar = 4194304.0f;  // |q| from here on: the fraction has no bits left, the octave contributes +0

// the host's constants of one octave (include/hns.h: "Host constants")
struct NoiseOctave {
	float f, a;
	uint32_t s;
};

// f_o, a_o and s_o of every octave of a spec whose numbers were checked
inline void noise_octaves(const hns_turbulence_spec& sp, NoiseOctave (&oct)[kNoiseMaxOctaves]) {
	const uint32_t base = birth_hash(sp.seed ^ 0x9E3779B9u);
	for (int o = 0; o < kNoiseMaxOctaves; ++o) {
		oct[o].f = o ? oct[o - 1].f * sp.lacunarity : sp.frequency;
		oct[o].a = o ? oct[o - 1].a * sp.gain : 1.0f;
		oct[o].s = birth_hash(base + (uint32_t)o);
	}
}

// the spec's refusals but for control*, for hns_shaping_apply and hns_shaping_curl_host alike: null, or what is wrong
inline const char* noise_spec_refusal(const hns_turbulence_spec* sp) {
	if (!std::isfinite(sp->amplitude)) return "amplitude is not finite";
	if (!std::isfinite(sp->frequency) || !(sp->frequency > 0.0f)) return "frequency is not a positive finite number";
	for (int a = 0; a < 3; ++a)
		if (!std::isfinite(sp->offset[a])) return "offset is not finite";
	if (sp->octaves < 1 || sp->octaves > kNoiseMaxOctaves) return "octaves is outside 1 .. 4";
	if (!std::isfinite(sp->lacunarity) || !(sp->lacunarity >= 1.0f)) return "lacunarity is not a finite number >= 1";
	if (!(sp->gain >= 0.0f && sp->gain <= 1.0f)) return "gain is outside 0 .. 1";
	return nullptr;
}

// component `axis` of entry n of the gradient table, +0.0f, 1.0f or -1.0f: two bits an entry (0: 0, 1: +1, 2: -1), the sixteen entries of an axis in one word
HNS_HD float noise_gradient(uint32_t n, int axis) {
	const uint32_t word = axis == 0 ? 0x09009999u : (axis == 1 ? 0xA59900A5u : 0x90A5A500u);
	const uint32_t code = (word >> (2u * n)) & 3u;
	return (float)((int)(code & 1u) - (int)(code >> 1));
}

// q, I and t of one axis; false: the octave contributes +0
HNS_HD bool noise_axis(float f, float offset, int x, int* I, float* t) {
	float q = f * (float)x;
	q = q + offset;
	if (!(fabsf(q) < kNoiseFar)) return false;  // (a NaN and an infinity included)
#ifdef __HIP_DEVICE_COMPILE__
	*I = __float2int_rd(q);
#else
	*I = (int)floorf(q);
#endif
	*t = q - (float)*I;
	return true;
}

// h of the lattice corner (x, y, z) of an octave with seed s
HNS_HD uint32_t noise_corner_hash(uint32_t s, int x, int y, int z) { return birth_hash(birth_hash(birth_hash(s ^ (uint32_t)x) ^ (uint32_t)y) ^ (uint32_t)z); }

// the eight corner hashes of cell I, h[4a + 2b + e], with the shared links of the chain hashed once: 14 H instead of 24
HNS_HD void noise_cell_hashes(uint32_t s, const int (&I)[3], uint32_t (&h)[8]) {
	for (int a = 0; a < 2; ++a) {
		const uint32_t hx = birth_hash(s ^ (uint32_t)(I[0] + a));
		for (int b = 0; b < 2; ++b) {
			const uint32_t hy = birth_hash(hx ^ (uint32_t)(I[1] + b));
			for (int e = 0; e < 2; ++e) h[4 * a + 2 * b + e] = birth_hash(hy ^ (uint32_t)(I[2] + e));
		}
	}
}

// u(t) and u'(t)
HNS_HD float noise_fade(float t) {
	float a = 6.0f * t;
	a = a - 15.0f;
	a = a * t;
	a = a + 10.0f;
	a = a * t;
	a = a * t;
	return a * t;
}
HNS_HD float noise_fade_slope(float t) {
	float b = t - 2.0f;
	b = b * t;
	b = b + 1.0f;
	float c = 30.0f * t;
	c = c * t;
	return c * b;
}

// the unfused lerp
HNS_HD float noise_lerp(float v0, float v1, float w) {
	float d = v1 - v0;
	d = w * d;
	return v0 + d;
}

// dN/d(AXIS) of one channel: d[4a + 2b + e] the corner values, g[4a + 2b + e] the corners' gradient component along AXIS, u = {u(t.x), u(t.y), u(t.z)}, slope = u'(t.AXIS).
// Every nest runs z, then y, then x, with AXIS left out of the nest over the differences.
template <int AXIS>
HNS_HD float noise_partial(const float (&d)[8], const float (&g)[8], const float (&u)[3], float slope) {
	constexpr int step = AXIS == 0 ? 4 : (AXIS == 1 ? 2 : 1);                     // the corner index moves by this along AXIS,
	constexpr int s0 = AXIS == 2 ? 2 : 1, s1 = AXIS == 0 ? 2 : 4;                 // by s0 along the faster and by s1 along the slower of the other two axes
	constexpr int w0 = AXIS == 2 ? 1 : 2, w1 = AXIS == 0 ? 1 : 0;                 // whose fades are u[w0] and u[w1]
	const float D00 = d[step] - d[0], D01 = d[step + s0] - d[s0], D10 = d[step + s1] - d[s1], D11 = d[step + s1 + s0] - d[s1 + s0];
	const float D0 = noise_lerp(D00, D01, u[w0]), D1 = noise_lerp(D10, D11, u[w0]);
	const float D = noise_lerp(D0, D1, u[w1]);
	const float g00 = noise_lerp(g[0], g[1], u[2]), g01 = noise_lerp(g[2], g[3], u[2]), g10 = noise_lerp(g[4], g[5], u[2]), g11 = noise_lerp(g[6], g[7], u[2]);
	const float g0 = noise_lerp(g00, g01, u[1]), g1 = noise_lerp(g10, g11, u[1]);
	const float L = noise_lerp(g0, g1, u[0]);
	const float m = slope * D;
	return m + L;
}

// the two partials the curl takes of channel M (nibble M of a corner's hash), along the axes A < B that are not M: d_abe = (g.x*p.x + g.y*p.y) + g.z*p.z with
// p = t - (a, b, e), then noise_partial along A and along B. tab[4n + axis]: the gradient table as floats (noise_gradient).
template <int M>
HNS_HD void noise_channel(const uint32_t (&h)[8], const float (&p)[3][2], const float (&u)[3], const float (&du)[3], const float* tab, float* dA, float* dB) {
	constexpr int A = M == 0 ? 1 : 0, B = M == 2 ? 1 : 2;
	float d[8], ga[8], gb[8];
#pragma unroll
	for (int i = 0; i < 8; ++i) {
		const float* row = tab + 4u * ((h[i] >> (4 * M)) & 15u);
		const float gx = row[0], gy = row[1], gz = row[2];
		const float dx = gx * p[0][i >> 2], dy = gy * p[1][(i >> 1) & 1], dz = gz * p[2][i & 1];
		d[i] = (dx + dy) + dz;
		ga[i] = A == 0 ? gx : gy, gb[i] = B == 1 ? gy : gz;
	}
	*dA = noise_partial<A>(d, ga, u, du[A]);
	*dB = noise_partial<B>(d, gb, u, du[B]);
}

// the curl of one octave in a cell: h[4a + 2b + e] the eight corner hashes, t the fraction
HNS_HD void noise_curl(const uint32_t (&h)[8], const float (&t)[3], const float* tab, float (&c)[3]) {
	const float u[3] = {noise_fade(t[0]), noise_fade(t[1]), noise_fade(t[2])};
	const float du[3] = {noise_fade_slope(t[0]), noise_fade_slope(t[1]), noise_fade_slope(t[2])};
	const float p[3][2] = {{t[0], t[0] - 1.0f}, {t[1], t[1] - 1.0f}, {t[2], t[2] - 1.0f}};
	float n0y, n0z, n1x, n1z, n2x, n2y;  // dN_m/d(axis)
	noise_channel<0>(h, p, u, du, tab, &n0y, &n0z);
	noise_channel<1>(h, p, u, du, tab, &n1x, &n1z);
	noise_channel<2>(h, p, u, du, tab, &n2x, &n2y);
	c[0] = n2y - n1z;
	c[1] = n0z - n2x;
	c[2] = n1x - n0y;
}

// C of the voxel ijk: the octaves in ascending order, each a multiply, then an add, from +0; an octave under the far rule contributes +0. hashes(o, I, h) fills the eight
// corner hashes of cell I of octave o (noise_cell_hashes).
template <class Hashes>
HNS_HD void noise_sum(const NoiseOctave (&oct)[kNoiseMaxOctaves], int octaves, const float (&off)[3], const int (&ijk)[3], const float* tab, Hashes&& hashes, float (&C)[3]) {
	C[0] = C[1] = C[2] = 0.0f;
#pragma unroll
	for (int o = 0; o < kNoiseMaxOctaves; ++o) {
		if (o >= octaves) continue;
		int I[3];
		float t[3], cu[3] = {0.0f, 0.0f, 0.0f};
		const bool near = noise_axis(oct[o].f, off[0], ijk[0], &I[0], &t[0]) && noise_axis(oct[o].f, off[1], ijk[1], &I[1], &t[1]) && noise_axis(oct[o].f, off[2], ijk[2], &I[2], &t[2]);
		if (near) {
			uint32_t h[8];
			hashes(o, I, h);
			noise_curl(h, t, tab, cu);
		}
		for (int a = 0; a < 3; ++a) {
			const float term = oct[o].a * cu[a];
			C[a] = C[a] + term;
		}
	}
}

// the gradient table as floats, four to an entry (the fourth unused): tab[4n + axis]
HNS_HD float noise_table_word(int w) { return (w & 3) == 3 ? 0.0f : noise_gradient((uint32_t)w >> 2, w & 3); }

}  // namespace hns
