// Y'CbCr of 8 .. 16 bits in 4:2:0, 4:2:2 or 4:4:4 -> 8-bit 4:2:0 Y'CbCr, defined in integers (include/homer_gpu.h section 12k).  ONE arithmetic: k_ingest_yuv
// (picture_io.hip) and hmr_gpu_yuv_convert_host (picture_host.cpp) compile these functions, and a caller can reproduce every sample from this comment.
//
// A source sample is an unsigned integer in a container of 1 byte (bits == 8) or 2 bytes (bits 9 .. 16, little endian).
//     raw    = the container's value
//     v      = msb_aligned ? raw >> (16 - bits) : min(raw, 2^bits - 1)
//     s      = bits - 8
//     luma:    Y(x, y) = min(255, (v + r(s)) >> s)                          r(t) = t ? 1 << (t - 1) : 0
//     chroma:  n = 2^k taps, S = their sum of v
//              C(cx, cy) = min(255, (S + r(s + k)) >> (s + k))
//       4:2:0  k = 0: the sample (cx, cy)
//       4:2:2  k = 1: column cx of chroma rows 2 cy and 2 cy + 1           (vertical average; horizontal siting untouched)
//       4:4:4  k = 2: the 2 x 2 block (2 cx .., 2 cy ..)                    (the block's average, sited at its centre: what section 12f makes)
// ONE rounding and nothing in between, in unsigned 32-bit arithmetic: 4 x 65535 + 2^9 < 2^32.
//
// What follows from it (tests/test_yuv_ingest_cpu.py holds each of these):
//   - every output is within 0.5 of the real-valued average of v / 2^s; where that average is >= 255.5 the result is 255 (10-bit 1023 -> 255, four 16-bit 65535 -> 255);
//   - 8-bit 4:2:0 is the identity: the slot is bit for bit what hmr_gpu_enc_load_sources_device gives for the same planes;
//   - an 8-bit picture widened to any depth (v << s, in either alignment) comes back unchanged, for every chroma format when the widened chroma is constant over its taps;
//   - 10-bit limited range stays limited range: 64 -> 16, 940 -> 235, 960 -> 240.
// There is NO range conversion, no tone mapping, no dithering and no change of the transfer function: the numbers are rounded to 8 bits and that is all.  The stream
// carries no colour description (section 12f): whoever decodes it has to be told by other means what the source was.
//
// Where a sample lies (sb = the container's bytes; `index` counts samples along a row of a plane, row y of a plane starts at plane + y * pitch):
//     PLANAR       luma (x, y): plane[0], index x            chroma c (i, j): plane[c], index i
//     SEMIPLANAR   luma (x, y): plane[0], index x            chroma c (i, j): plane[1], index 2 i + offset[c]
//     PACKED422    luma (x, y): plane[0], index 2 x + offset[0]      chroma c (i, j): plane[0], index 4 i + offset[c]
// (i, j) are a sample's column and row in the SOURCE's chroma grid: Wc x Hc with Wc = W / 2 (4:2:0, 4:2:2) or W (4:4:4), Hc = H / 2 (4:2:0) or H.
#pragma once
#include <stdint.h>

enum { HMR_YUV_PLANAR = 0, HMR_YUV_SEMIPLANAR = 1, HMR_YUV_PACKED422 = 2 };      // hmr_gpu_yuv_picture.format (include/homer_gpu.h restates them)

// a descriptor's form as the arithmetic uses it; a job of k_ingest_yuv carries one, so a launch mixes forms
struct YuvForm {
	int32_t format;          // HMR_YUV_*
	int32_t k;               // log2 of the chroma taps: 0, 1, 2 for 4:2:0, 4:2:2, 4:4:4
	int32_t sb;              // bytes of a container: 1 or 2
	int32_t rs;              // msb_aligned ? 16 - bits : 0
	uint32_t maxv;           // 2^bits - 1
	int32_t s;               // bits - 8
	int32_t offset[3];       // the descriptor's
	int32_t reserved;
};
static_assert(sizeof(YuvForm) % 8 == 0, "a job that holds one keeps its pointers aligned");

static inline YuvForm hmr_yuv_form(int format, int chroma, int bits, int msb_aligned, const int32_t offset[3])
{
	YuvForm f;
	f.format = format; f.k = chroma; f.sb = bits > 8 ? 2 : 1;
	f.rs = msb_aligned ? 16 - bits : 0;
	f.maxv = (1u << bits) - 1u;
	f.s = bits - 8;
	f.offset[0] = offset[0]; f.offset[1] = offset[1]; f.offset[2] = offset[2];
	f.reserved = 0;
	return f;
}

// v of a container's value
__host__ __device__ inline uint32_t hmr_yuv_value(const YuvForm &f, uint32_t raw)
{
	const uint32_t v = raw >> f.rs;
	return v < f.maxv ? v : f.maxv;
}
// min(255, (S + r(t)) >> t): S a sum of 2^k values v, t = s + k
__host__ __device__ inline uint32_t hmr_yuv_round(uint32_t sum, int t)
{
	const uint32_t q = (sum + (t ? 1u << (t - 1) : 0u)) >> t;
	return q < 255u ? q : 255u;
}

// the container at `index` of row y of a plane, read byte by byte (little endian; any address): host and device pointers alike
template <class Bytes>
__host__ __device__ inline uint32_t hmr_yuv_raw(Bytes plane, int64_t pitch, int sb, int64_t index, int y)
{
	const Bytes p = plane + (int64_t)y * pitch + index * sb;
	return sb == 1 ? (uint32_t)p[0] : (uint32_t)p[0] | (uint32_t)p[1] << 8;
}
// Y(x, y); planes / pitches: the descriptor's
template <class Bytes, class Planes>
__host__ __device__ inline uint32_t hmr_yuv_luma(const Planes &plane, const int64_t pitch[3], const YuvForm &f, int x, int y)
{
	const int64_t index = f.format == HMR_YUV_PACKED422 ? 2 * (int64_t)x + f.offset[0] : x;
	return hmr_yuv_round(hmr_yuv_value(f, hmr_yuv_raw((Bytes)plane[0], pitch[0], f.sb, index, y)), f.s);
}
// C(cx, cy) of component c = 1 (U) or 2 (V)
template <class Bytes, class Planes>
__host__ __device__ inline uint32_t hmr_yuv_chroma(const Planes &plane, const int64_t pitch[3], const YuvForm &f, int c, int cx, int cy)
{
	const int rows = f.k >= 1 ? 2 : 1, cols = f.k == 2 ? 2 : 1;
	const int p = f.format == HMR_YUV_PLANAR ? c : f.format == HMR_YUV_SEMIPLANAR ? 1 : 0;
	uint32_t sum = 0;
	for (int r = 0; r < rows; r++)
		for (int t = 0; t < cols; t++) {
			const int64_t i = (int64_t)cx * cols + t;
			const int64_t index = f.format == HMR_YUV_PLANAR ? i : f.format == HMR_YUV_SEMIPLANAR ? 2 * i + f.offset[c] : 4 * i + f.offset[c];
			sum += hmr_yuv_value(f, hmr_yuv_raw((Bytes)plane[p], pitch[p], f.sb, index, cy * rows + r));
		}
	return hmr_yuv_round(sum, f.s + f.k);
}
