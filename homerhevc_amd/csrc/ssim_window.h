// SSIM of 8-bit 4:2:0 pictures, defined in integers (include/homer_gpu.h section 12h).  ONE arithmetic: k_ssim (picture_io.hip) and hmr_gpu_ssim_host (picture_host.cpp) compile these
// functions, and a caller can reproduce every sum from this comment.
//
// Every plane is measured on its own: luma W x H, each chroma plane W/2 x H/2; a and b are the two pictures' samples of the plane.  W and H are multiples of 8, so a
// plane is an exact grid of bw x bh = (w / 4) x (h / 4) BLOCKS of 4 x 4 samples.  Over a block's 16 samples
//     s1 = sum a        s2 = sum b        ss = sum (a a + b b)        s12 = sum a b                      (at most 4080, 4080, 2 080 800, 1 040 400)
// Every 2 x 2 group of adjacent blocks is a WINDOW of 8 x 8 samples; neighbouring windows overlap by one block, a plane has (bw - 1) (bh - 1) of them.  S1, S2, SS, S12
// are the sums of the four blocks' sums, and with C1 = 416 = floor((0.01 255)^2 64 + 0.5), C2 = 235963 = floor((0.03 255)^2 64 63 + 0.5)
//     var = 64 SS - S1 S1 - S2 S2          cov = 64 S12 - S1 S2
//     N = (2 S1 S2 + C1) (2 cov + C2)      D = (S1 S1 + S2 S2 + C1) (var + C2)
//     q = floor(2^30 N / D)                the floor towards minus infinity: N may be negative
// in exact integers.  The plane's result is the sum of q over its windows, a signed 64-bit value; its mean SSIM is sum / (2^30 windows).
// Bounds: S1, S2 <= 16320, so 2 S1 S2 + C1 and S1 S1 + S2 S2 + C1 are at most 532 685 216 < 2^29 and the first is not above the second (2 x y <= x x + y y).  var is
// 64 sum a a - (sum a)^2 plus the same for b: each part is 64 times the window's sum of squared deviations, at least 0 and at most 64^2 (255 / 2)^2 = 66 585 600, so
// 0 <= var <= 133 171 200 < 2^27, and |2 cov| <= var (Cauchy-Schwarz, then 2 sqrt(x y) <= x + y).  Hence 0 < D < 2^57 (C1, C2 > 0), |N| <= D, -2^30 <= q <= 2^30,
// and q = 2^30 exactly when N = D: S1 = S2 and var = 2 cov, that is 64 sum (a - b)^2 = (sum (a - b))^2 = 0 - the window's samples are equal.
// 2^30 |N| does not fit 64 bits, and six 64-bit divisions (long division, six bits a time) cost some 800 instructions per window on the device.  The quotient is
// therefore PROPOSED in binary64 and DECIDED in integers: e = trunc((double)|N| 2^30 / (double)D).  Three roundings of at most 2^-53 each (the two conversions and
// the division; the scaling by 2^30 is exact) put the binary64 quotient within 2^30 2^-51 = 2^-21 of the true one, so e is floor(2^30 |N| / D) or one beside it.  The
// remainder r = 2^30 |N| - e D then lies in (-D, 2 D), inside (-2^57, 2^58), so computing it modulo 2^64 and reading it as a signed value is exact, and ONE correction
// step - r < 0: e - 1, r + D;  r >= D: e + 1, r - D - leaves the exact quotient with its exact remainder in [0, D).  A negative N with a remainder left rounds one
// further down.  Nothing depends on how the binary64 division rounds: any estimate within 1 of the quotient gives the same result, bit for bit, on host and device.
#pragma once
#include <stdint.h>

#define HMR_SSIM_C1 416
#define HMR_SSIM_C2 235963
#define HMR_SSIM_ONE_BITS 30         // q = 2^30 for equal windows

// q of one window from its four sums
__host__ __device__ inline int64_t hmr_ssim_window(uint32_t S1, uint32_t S2, uint32_t SS, uint32_t S12)
{
	const uint32_t p12 = S1 * S2, sq = S1 * S1 + S2 * S2;                 // <= 266 342 400, 532 684 800
	const uint32_t var = 64u * SS - sq;                                  // < 2^27
	const int32_t cov2 = 2 * (int32_t)(64u * S12 - p12);                 // |2 cov| <= var
	const int64_t N = (int64_t)(2u * p12 + HMR_SSIM_C1) * (int64_t)(cov2 + HMR_SSIM_C2);
	const uint64_t D = (uint64_t)(sq + HMR_SSIM_C1) * (uint64_t)(var + HMR_SSIM_C2);
	const uint64_t n = (uint64_t)(N < 0 ? -N : N);
	uint64_t q = (uint64_t)((double)n * 1073741824.0 / (double)D);
	int64_t r = (int64_t)((n << HMR_SSIM_ONE_BITS) - q * D);      // (modulo 2^64)
	if (r < 0) { q--; r += (int64_t)D; }
	else if (r >= (int64_t)D) { q++; r -= (int64_t)D; }
	return N < 0 ? -(int64_t)q - (r ? 1 : 0) : (int64_t)q;
}

// the windows of a w x h plane (w, h multiples of 4, at least 8)
__host__ __device__ inline int64_t hmr_ssim_windows(int w, int h) { return (int64_t)((w >> 2) - 1) * ((h >> 2) - 1); }

// What the SSIM calls refuse of a picture size, as text (NULL: accepted): every plane needs whole blocks and at least one window.
static inline const char *hmr_ssim_refusal(int width, int height)
{
	if (width <= 0 || (width & 7)) return "width: must be a positive multiple of 8";
	if (height <= 0 || (height & 7)) return "height: must be a positive multiple of 8";
	if (width < 16) return "width: below 16 (a chroma plane with fewer than two block columns has no window)";
	if (height < 16) return "height: below 16 (a chroma plane with fewer than two block rows has no window)";
	return nullptr;
}

// One plane over host memory, the definition as it stands: `step` bytes from sample to sample of a row (2: one half of NV12's pairs).
static inline int64_t hmr_ssim_plane_host(const uint8_t *a, int64_t pitch_a, int step_a, const uint8_t *b, int64_t pitch_b, int step_b, int w, int h)
{
	int64_t sum = 0;
	for (int wy = 0; wy + 1 < (h >> 2); wy++)
		for (int wx = 0; wx + 1 < (w >> 2); wx++) {
			uint32_t S1 = 0, S2 = 0, SS = 0, S12 = 0;
			for (int y = 4 * wy; y < 4 * wy + 8; y++)
				for (int x = 4 * wx; x < 4 * wx + 8; x++) {
					const uint32_t va = a[(int64_t)y * pitch_a + (int64_t)x * step_a], vb = b[(int64_t)y * pitch_b + (int64_t)x * step_b];
					S1 += va; S2 += vb; SS += va * va + vb * vb; S12 += va * vb;
				}
			sum += hmr_ssim_window(S1, S2, SS, S12);
		}
	return sum;
}
