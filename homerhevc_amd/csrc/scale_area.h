// Area-averaging downscale of 8-bit 4:2:0 pictures, defined in integers (include/homer_gpu.h section 12g).  ONE arithmetic: k_downscale (picture_io.hip) and
// hmr_gpu_scale_host compile these functions, and a caller can reproduce every sample from this comment.
//
// Every plane is scaled on its own: luma Ws x Hs -> Wd x Hd, each chroma plane Ws/2 x Hs/2 -> Wd/2 x Hd/2 (the 4:2:0 siting is kept).  Per axis, with source length S
// and destination length D:  g = gcd(S, D), s = S / g, d = D / g  (a chroma axis S/2 -> D/2 has the same s and d).  A source sample is d units wide, an output sample
// s units: output x covers [x s, (x + 1) s), source sample i covers [i d, (i + 1) d), and the tap weight is
//     w(x, i) = min((x + 1) s, (i + 1) d) - max(x s, i d)        where that is positive: i = floor(x s / d) .. floor(((x + 1) s - 1) / d)
// The weights of one output sum to s; there are at most ceil(S / D) + 1 of them.  With ONE rounding and none in between
//     out(x, y) = (sum_j sum_i wy(y, j) wx(x, i) src(i, j) + (sx sy >> 1)) / (sx sy)
// in unsigned 32-bit arithmetic (the division floors): the order of the passes cannot change a bit.  hmr_scale_check refuses what does not fit: the numerator is at
// most sx sy 255 + (sx sy >> 1), which has to stay below 2^32 - every even size up to 8192 x 4320 does.
// Equal sizes give the identity, 2 : 1 gives (a + b + c + d + 2) >> 2, and every output is within 0.5 of the real-valued area average.
#pragma once
#include <stdint.h>

#define HMR_SCALE_MAX_RATIO 8        // source length <= 8 x destination length per axis (the LDS tile of k_downscale is sized by it)
#define HMR_SCALE_MAX_LENGTH 65536   // positions x s and i d stay inside 32 bits: S d <= 65536 x 32768

// one axis, reduced
struct ScaleAxis {
	uint32_t s, d;       // S / g, D / g
	uint32_t md;         // hmr_scale_magic(d)
};

static inline uint32_t hmr_scale_gcd(uint32_t a, uint32_t b)
{
	while (b) { const uint32_t t = a % b; a = b; b = t; }
	return a;
}

// Division of any 32-bit n by a divisor `den` that is the same for a whole picture, as a multiplication: m = min(floor(2^32 / den), 2^32 - 1).
// Exact for EVERY 32-bit n:  2^32 / den - 1 <= m <= 2^32 / den, so with t = n m / 2^32 (real-valued)  n / den - n / 2^32 <= t <= n / den, and n < 2^32 gives
// n / den - 1 < t <= n / den.  q = floor(t) is therefore floor(n / den) or one less; q den <= n, so r = n - q den does not wrap and lies in [0, 2 den), and ONE
// correction q + (r >= den) gives floor(n / den).  (den = 1: m = 2^32 - 1, q = n - 1 for n > 0, corrected to n.)
static inline uint32_t hmr_scale_magic(uint32_t den) { return den <= 1 ? 0xffffffffu : (uint32_t)((1ull << 32) / den); }
__host__ __device__ inline uint32_t hmr_scale_div(uint32_t n, uint32_t den, uint32_t m)
{
#if defined(__HIP_DEVICE_COMPILE__)
	const uint32_t q = __umulhi(n, m);
#else
	const uint32_t q = (uint32_t)(((uint64_t)n * m) >> 32);
#endif
	return q + (n - q * den >= den ? 1u : 0u);
}

static inline ScaleAxis hmr_scale_axis(int S, int D)
{
	const uint32_t g = hmr_scale_gcd((uint32_t)S, (uint32_t)D);
	ScaleAxis a;
	a.s = (uint32_t)S / g; a.d = (uint32_t)D / g; a.md = hmr_scale_magic(a.d);
	return a;
}

// the first source sample output x touches, and the weight of source sample i in output x (i inside the output's taps)
__host__ __device__ inline uint32_t hmr_scale_first(const ScaleAxis &a, uint32_t x) { return hmr_scale_div(x * a.s, a.d, a.md); }
__host__ __device__ inline uint32_t hmr_scale_weight(const ScaleAxis &a, uint32_t x, uint32_t i)
{
	const uint32_t lo = x * a.s, hi = lo + a.s, b = i * a.d, e = b + a.d;
	return (hi < e ? hi : e) - (lo > b ? lo : b);
}
// one past the last source sample output x touches
__host__ __device__ inline uint32_t hmr_scale_end(const ScaleAxis &a, uint32_t x) { return hmr_scale_div((x + 1) * a.s - 1, a.d, a.md) + 1; }

// What hmr_gpu_scale_check refuses, as the field's text (NULL: accepted).  Pure arithmetic.  any_ratio: without the bound of 8 per axis, which is the kernel's (its LDS
// tile) and not the arithmetic's - hmr_gpu_scale_host takes any ratio.
static inline const char *hmr_scale_refusal(int src_w, int src_h, int dst_w, int dst_h, bool any_ratio = false)
{
	if (src_w <= 0 || (src_w & 1)) return "src_w: must be positive and even";
	if (src_h <= 0 || (src_h & 1)) return "src_h: must be positive and even";
	if (dst_w <= 0 || (dst_w & 1)) return "dst_w: must be positive and even";
	if (dst_h <= 0 || (dst_h & 1)) return "dst_h: must be positive and even";
	if (dst_w > src_w) return "dst_w: larger than src_w (no upscaling: area averaging degenerates to nearest neighbour there)";
	if (dst_h > src_h) return "dst_h: larger than src_h (no upscaling: area averaging degenerates to nearest neighbour there)";
	if (!any_ratio && (int64_t)src_w > (int64_t)HMR_SCALE_MAX_RATIO * dst_w) return "src_w: more than 8 x dst_w";
	if (!any_ratio && (int64_t)src_h > (int64_t)HMR_SCALE_MAX_RATIO * dst_h) return "src_h: more than 8 x dst_h";
	if (src_w > HMR_SCALE_MAX_LENGTH) return "src_w: above 65536";
	if (src_h > HMR_SCALE_MAX_LENGTH) return "src_h: above 65536";
	// the same reduced ratio for luma and chroma: one bound holds for both
	const uint64_t den = (uint64_t)hmr_scale_axis(src_w, dst_w).s * hmr_scale_axis(src_h, dst_h).s;
	if (den * 255 + (den >> 1) >= (1ull << 32)) return "src_w, src_h: sx * sy * 255 + (sx * sy >> 1) does not fit 32 bits for this pair of sizes";
	return nullptr;
}

// One plane over host memory, the formula as it stands: `step` bytes from sample to sample of a source row (2: one half of NV12's pairs), the output tightly packed.
static inline void hmr_scale_plane_host(const uint8_t *src, int64_t pitch, int step, int Ws, int Hs, int Wd, int Hd, uint8_t *out)
{
	const ScaleAxis ax = hmr_scale_axis(Ws, Wd), ay = hmr_scale_axis(Hs, Hd);
	const uint32_t den = ax.s * ay.s;
	for (int y = 0; y < Hd; y++)
		for (int x = 0; x < Wd; x++) {
			uint32_t sum = den >> 1;
			for (uint32_t j = (uint32_t)y * ay.s / ay.d; j * ay.d < ((uint32_t)y + 1) * ay.s; j++)
				for (uint32_t i = (uint32_t)x * ax.s / ax.d; i * ax.d < ((uint32_t)x + 1) * ax.s; i++)
					sum += hmr_scale_weight(ay, (uint32_t)y, j) * hmr_scale_weight(ax, (uint32_t)x, i) * src[(int64_t)j * pitch + (int64_t)i * step];
			out[(size_t)y * Wd + x] = (uint8_t)(sum / den);
		}
}
