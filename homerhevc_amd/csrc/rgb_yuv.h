// RGB -> 8-bit 4:2:0 Y'CbCr, defined in integers (include/homer_gpu.h section 12f).  ONE arithmetic: k_ingest_rgb (picture_io.hip) and hmr_gpu_rgb_convert_host (picture_host.cpp) compile
// these functions, and a caller can reproduce every sample from this comment.
//
// Inputs are 8-bit R, G, B.  A float sample x (binary16 is widened exactly to binary32 first) becomes
//     q = x > 0 ? (x < 1 ? x : 1) : 0        (NaN gives 0)
//     v = (int)rintf(q * 255.0f)             one binary32 product, round half to even: np.rint(np.float32(q) * np.float32(255))
// Luma, per pixel:                  Y = ((Yr R + Yg G + Yb B + 32768) >> 16) + yoff
// Chroma, per 2 x 2 block with SR, SG, SB the sums of its four pixels (0 .. 1020) - the block's average, sited at its centre:
//     U = clamp(((Ur SR + Ug SG + Ub SB + 131072) >> 18) + 128, 0, 255),  V likewise with its own row
// `>>` is the arithmetic shift of a 32-bit signed value (floor); the largest magnitude is 66 846 720.
//
//     matrix, range     Yr, Yg, Yb            Ur, Ug, Ub               Vr, Vg, Vb              yoff
//     BT.601 limited    16829, 33039, 6416    -9714, -19070, 28784     28784, -24103, -4681    16
//     BT.601 full       19595, 38470, 7471    -11058, -21710, 32768    32768, -27439, -5329    0
//     BT.709 limited    11966, 40254, 4064    -6596, -22188, 28784     28784, -26145, -2639    16
//     BT.709 full       13933, 46871, 4732    -7509, -25259, 32768     32768, -29763, -3005    0
// 16 fraction bits; the green coefficient is chosen so that a luma row sums to the rounded range scale (56284 = round(65536 x 219 / 255), or 65536) and a chroma row to 0:
// grey gives U = V = 128 at every level.  Every output is within 0.51 of the real-valued BT formula (half an LSB of rounding plus at most 3 x 1020 x 0.5 / 2^18 of
// coefficient error); luma is inside 16 .. 235 (limited) or 0 .. 255 (full), limited chroma inside 16 .. 240 before the clamp, full-range chroma reaches 256 before it.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/homer_gpu.h"      // (the formats rgb_sample reads)

struct RgbMatrix {
	int32_t y[3], u[3], v[3], yoff;
};

// matrix: HMR_GPU_MATRIX_BT601 (0) / _BT709 (1); full_range: 0 / 1
static inline RgbMatrix hmr_rgb_matrix(int matrix, int full_range)
{
	static const RgbMatrix table[2][2] = {
		{{{16829, 33039, 6416}, {-9714, -19070, 28784}, {28784, -24103, -4681}, 16}, {{19595, 38470, 7471}, {-11058, -21710, 32768}, {32768, -27439, -5329}, 0}},
		{{{11966, 40254, 4064}, {-6596, -22188, 28784}, {28784, -26145, -2639}, 16}, {{13933, 46871, 4732}, {-7509, -25259, 32768}, {32768, -29763, -3005}, 0}},
	};
	return table[matrix & 1][full_range & 1];
}

__host__ __device__ inline int hmr_rgb_quantize(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
	// the same q for every input, NaN included (maxNum / minNum return the operand that is a number), as v_max_f32 / v_min_f32: compares and selects would hold a
	// scalar register pair per sample in flight
	const float q = fminf(fmaxf(x, 0.0f), 1.0f);
#else
	const float q = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;
#endif
	return (int)rintf(q * 255.0f);
}
// a sample of an RGB picture as 8 bits: `plane` is the packed plane or the channel's own; host and device pointers alike (hmr_gpu_rgb_convert_host, a row's tail)
template <class Bytes, class Halves, class Floats>
__host__ __device__ __forceinline__ int rgb_sample(Bytes plane, int64_t pitch, int format, int pixel_bytes, int offset, int x, int y)
{
	const Bytes row = plane + (int64_t)y * pitch;
	switch (format) {
	case HMR_GPU_RGB_PACKED8: return row[x * pixel_bytes + offset];
	case HMR_GPU_RGB_PLANAR8: return row[x];
	case HMR_GPU_RGB_PLANAR_F16: return hmr_rgb_quantize((float)((Halves)row)[x]);
	default: return hmr_rgb_quantize(((Floats)row)[x]);
	}
}
// coefficient x sample (or sum of four): both fit 24 bits, so the device's full-rate 24-bit multiply gives the same product
__host__ __device__ inline int hmr_rgb_mul(int k, int s)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __mul24(k, s);
#else
	return k * s;
#endif
}
__host__ __device__ inline int hmr_rgb_luma(const RgbMatrix &m, int r, int g, int b)
{
	return ((hmr_rgb_mul(m.y[0], r) + hmr_rgb_mul(m.y[1], g) + hmr_rgb_mul(m.y[2], b) + 32768) >> 16) + m.yoff;
}
// k: a chroma row of the matrix; sr, sg, sb: the sums over the 2 x 2 block
__host__ __device__ inline int hmr_rgb_chroma(const int32_t k[3], int sr, int sg, int sb)
{
	const int c = ((hmr_rgb_mul(k[0], sr) + hmr_rgb_mul(k[1], sg) + hmr_rgb_mul(k[2], sb) + 131072) >> 18) + 128;
	return c < 0 ? 0 : c > 255 ? 255 : c;
}
