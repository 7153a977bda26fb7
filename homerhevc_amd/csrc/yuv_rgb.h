// 8-bit 4:2:0 Y'CbCr -> RGB, defined in integers (include/homer_gpu.h section 12i): the mirror image of rgb_yuv.h.  ONE arithmetic: k_egress_rgb (picture_io.hip) and
// hmr_gpu_rgb_from_yuv_host (picture_host.cpp) compile these functions, and a caller can reproduce every sample from this comment.
//
// Inputs are 8-bit Y [H, W] and U, V [H / 2, W / 2]; chroma sample (cx, cy) is sited at the centre of the luma block (2 cx .. 2 cx + 1, 2 cy .. 2 cy + 1) - the siting
// rgb_yuv.h produces.
// Chroma at luma position (x, y): bilinear, scaled by 16, not rounded.  Rows, with cy = y >> 1: an even y takes rows cy - 1 (weight 1) and cy (weight 3), an odd y takes
// rows cy (weight 3) and cy + 1 (weight 1); columns: the same rule with x.  Indices are clamped to the plane, so a sample at an edge gets the full weight.
//     C16 = sum of wy wx C over the four samples, 0 .. 4080; a flat plane gives exactly 16 C
// Per pixel, with L = 16 Ky (Y - yoff), U' = U16 - 2048, V' = V16 - 2048:
//     R = clamp((L + Rv V' + 131072) >> 18, 0, 255)
//     G = clamp((L + Gu U' + Gv V' + 131072) >> 18, 0, 255)
//     B = clamp((L + Bu U' + 131072) >> 18, 0, 255)
// `>>` is the arithmetic shift of a 32-bit signed value (floor); the largest magnitude in front of it is below 1.5e8.
//
//     matrix, range     Ky      Rv      Gu      Gv       Bu      yoff
//     BT.601 limited    19077   26149   -6419   -13320   33050   16
//     BT.601 full       16384   22970   -5638   -11700   29032   0
//     BT.709 limited    19077   29372   -3494   -8731    34610   16
//     BT.709 full       16384   25802   -3069   -7670    30402   0
// Every coefficient is round(real x 2^14) of the inverse BT matrix: 255 / 219 for luma and 255 / 224 x 2 (1 - Kr), ... for chroma in limited range, 1 and 2 (1 - Kr), ...
// in full range.  14 fraction bits on values scaled by 16: 18 bits are shifted out.  Every output is within 0.52 of the real-valued formula applied to the same bilinear
// chroma; flat chroma 128 gives R = G = B, and in full range R = G = B = Y at all 256 levels.
//
// Float outputs of an 8-bit value v: x = (float)v / 255.0f, ONE correctly rounded binary32 division (np.float32(v) / np.float32(255)); binary16 is that value rounded to
// nearest even.  hmr_rgb_quantize (rgb_yuv.h) of either returns v for all 256 values.  No fast-math on this file: the division must stay correctly rounded on the device.
#pragma once
#include <stdint.h>
#include "../../include/homer_gpu.h"      // (the formats rgb_put writes)

struct YuvMatrix {
	int32_t ky, rv, gu, gv, bu, yoff;
};

// matrix: HMR_GPU_MATRIX_BT601 (0) / _BT709 (1); full_range: 0 / 1
static inline YuvMatrix hmr_yuv_matrix(int matrix, int full_range)
{
	static const YuvMatrix table[2][2] = {
		{{19077, 26149, -6419, -13320, 33050, 16}, {16384, 22970, -5638, -11700, 29032, 0}},
		{{19077, 29372, -3494, -8731, 34610, 16}, {16384, 25802, -3069, -7670, 30402, 0}},
	};
	return table[matrix & 1][full_range & 1];
}

// coefficient x value: both fit 24 bits (|Ky (Y - yoff)| <= 19077 x 239, |U'| <= 2048), so the device's full-rate 24-bit multiply gives the same product
__host__ __device__ inline int hmr_yuv_mul(int k, int s)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __mul24(k, s);
#else
	return k * s;
#endif
}
__host__ __device__ inline int hmr_yuv_clamp(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// y: the luma sample; u16, v16: the bilinear chroma, scaled by 16
__host__ __device__ inline void hmr_yuv_rgb(const YuvMatrix &m, int y, int u16, int v16, int &r, int &g, int &b)
{
	const int l = hmr_yuv_mul(m.ky, y - m.yoff) * 16 + 131072, u = u16 - 2048, v = v16 - 2048;
	r = hmr_yuv_clamp((l + hmr_yuv_mul(m.rv, v)) >> 18);
	g = hmr_yuv_clamp((l + hmr_yuv_mul(m.gu, u) + hmr_yuv_mul(m.gv, v)) >> 18);
	b = hmr_yuv_clamp((l + hmr_yuv_mul(m.bu, u)) >> 18);
}

// the bilinear chroma, scaled by 16, of a cw x ch plane (sample (cx, cy) at plane[cy * stride + cx]) at luma position (x, y)
template <class Samples>
__host__ __device__ inline int hmr_yuv_chroma16(Samples plane, int64_t stride, int cw, int ch, int x, int y)
{
	const int xa = (x & 1) ? x >> 1 : (x >> 1) - 1, ya = (y & 1) ? y >> 1 : (y >> 1) - 1;      // the first of the two columns / rows; an odd position weighs it 3, an even one 1
	const int wxa = (x & 1) ? 3 : 1, wya = (y & 1) ? 3 : 1;
	const int x0 = xa < 0 ? 0 : xa, x1 = xa + 1 > cw - 1 ? cw - 1 : xa + 1, y0 = ya < 0 ? 0 : ya, y1 = ya + 1 > ch - 1 ? ch - 1 : ya + 1;
	const int top = wxa * (int)plane[(int64_t)y0 * stride + x0] + (4 - wxa) * (int)plane[(int64_t)y0 * stride + x1];
	const int bottom = wxa * (int)plane[(int64_t)y1 * stride + x0] + (4 - wxa) * (int)plane[(int64_t)y1 * stride + x1];
	return wya * top + (4 - wya) * bottom;
}

// an 8-bit value as a float output sample
__host__ __device__ inline float hmr_rgb_unit(int v) { return (float)v / 255.0f; }

// a sample of an RGB picture written as 8 bits' worth: host and device pointers alike (hmr_gpu_rgb_from_yuv_host, a row's tail)
template <class Bytes, class Halves, class Floats>
__host__ __device__ __forceinline__ void rgb_put(Bytes plane, int64_t pitch, int format, int pixel_bytes, int offset, int x, int y, int v)
{
	const Bytes row = plane + (int64_t)y * pitch;
	switch (format) {
	case HMR_GPU_RGB_PACKED8: row[x * pixel_bytes + offset] = (uint8_t)v; break;
	case HMR_GPU_RGB_PLANAR8: row[x] = (uint8_t)v; break;
	case HMR_GPU_RGB_PLANAR_F16: ((Halves)row)[x] = (_Float16)hmr_rgb_unit(v); break;
	default: ((Floats)row)[x] = hmr_rgb_unit(v); break;
	}
}
// the byte of a 4-byte pixel that holds no channel
__host__ __device__ __forceinline__ int rgb_alpha_offset(const int32_t offset[3]) { return 6 - offset[0] - offset[1] - offset[2]; }
