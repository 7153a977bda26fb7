// Picture conversion on the device (include/homer_gpu.h sections 12d .. 12m): pictures in device memory - any base address, any pitch - to and from the int16 planes of
// the frame encoder (sample (x, y) at y * stride + x), and quality and scene-cut sums between such planes.  ONE launch for a batch of pictures; k_ingest and k_egress have no
// arithmetic to speak of and are bound by HBM.  The file holds the twelve kernels, behind each the PictureKernel<Job> that names it and its grid size for
// hmr_picture_launch, the launch itself and the three scale job builders (they need scale_tile); everything else on the host is picture_host.cpp.
//
// k_ingest: 8-bit pictures into int16 planes - the source planes of a picture slot, or a reference picture: sample (x, y) at y * stride + x, nothing outside
// width x height touched.  1.5 W H bytes read, 3 W H written per picture.
// k_egress: the frame encoder's final pictures (int16 planes with margins) into 8-bit pictures, and / or the exact sums of squared differences of each plane against the
// int16 source planes of a picture slot.  Per picture 3 W H bytes read (final picture), 3 W H read (slot, when sums are asked for), 1.5 W H written (when a picture is
// asked for).
//
// k_ingest_rgb (section 12f): RGB pictures - packed 8-bit with 3 or 4 bytes per pixel and any channel order, planar 8-bit, planar binary16, planar binary32 - into the same
// int16 planes, converted to 4:2:0 Y'CbCr by the integer arithmetic of rgb_yuv.h in the same pass.  3, 4, 3, 6 or 12 W H bytes read, 4 W H written per picture
//.  blockIdx.y = picture, blockIdx.x = a chunk of CHUNK_ROWS luma rows = CHUNK_ROWS / 2 chroma rows; a lane takes a span of 16
// pixels of TWO adjacent rows, so the 2 x 2 sums of the chroma samples never leave the lane: 16-byte loads at whatever address the pitch gives (per row: three for
// 3-byte pixels, four for 4-byte pixels, one per plane for planar 8-bit, two / four per plane for binary16 / binary32), channels picked by v_alignbyte_b32 / v_bfe_u32 with
// the job's byte offsets, four 16-byte stores of int16 luma and one each of eight U and eight V samples.  A row's tail of fewer than 16 pixels goes sample by sample, a lane per 2 x 2 block.
//
// k_downscale (section 12g): 8-bit pictures of a larger size into the same int16 planes, area-averaged by the integer arithmetic of scale_area.h in the same pass; its
// mapping (tiles through LDS) is described at the kernel.
//
// k_rgb_ladder (section 12j): RGB pictures of a larger size into the same int16 planes, converted as k_ingest_rgb converts and area-averaged as k_downscale averages
// in the same pass; described at the kernel.
//
// k_yuv_ladder (section 12l): Y'CbCr pictures of 8 .. 16 bits of a larger size, in any of k_ingest_yuv's forms, into the same int16 planes, rounded as k_ingest_yuv
// rounds and area-averaged as k_downscale averages in the same pass; described at the kernel.
//
// Mapping (struct Chunk): blockIdx.y = picture (a record of the job table), blockIdx.x = a chunk of CHUNK_ROWS rows of it - first the luma rows, then the chroma rows (a
// chroma row is its U and its V part: as many 8-bit bytes as a luma row) - so that one grid covers the three planes of every picture; pictures smaller than the largest
// of the launch leave their last chunks empty.  A lane takes a span of 16 samples.  Ingest: one 16-byte load, two 16-byte stores of int16; NV12 chroma: one 16-byte load
// of eight U, V pairs, one 16-byte store to each plane.  Egress: two 16-byte loads of the final picture (four with the slot's samples), the low bytes packed by
// v_perm_b32 into ONE 16-byte store; NV12 chroma: a 16-byte load of eight U and one of eight V samples, interleaved into one 16-byte store.  The int16 side is always
// 16-byte aligned (strides and margins are multiples of 8 elements, the planes come from hipMalloc, a lane starts at a multiple of 8 elements).  The 8-bit side is
// whatever the caller made: its 16-byte load or store is issued at whatever address the row gives it (load16 / store16 below); a row's tail of fewer than 16 samples
// goes sample by sample.  No lane reads or writes a byte of an 8-bit plane outside [plane + y * pitch, plane + y * pitch + row bytes).
//
// Sums: a lane adds the squares of its differences into 32-bit accumulators (one for luma or U, one for V), the wavefront's lanes are summed by the DPP butterfly of
// common.h, the workgroup's four wavefronts through LDS in 64 bits, and one lane adds the workgroup's sum to the picture's 64-bit sum of that plane with one vector atomic
// (global_atomic_add_x2).  Integer sums: exact whatever the order.  A chunk holds at most CHUNK_ROWS x EGRESS_MAX_WIDTH samples of one plane, each difference at most 255:
// 8 x 8192 x 255^2 = 4 261 478 400 < 2^32, so neither a lane's nor a wavefront's accumulator wraps; a picture's sum does not fit 32 bits (255^2 x 3840 x 2160 = 5.4e11).
#include <math.h>
#include <string.h>
#include "picture_io.h"

namespace {
// A job type's kernel and the grid's x size one of its jobs needs: specialised right behind each kernel, read by hmr_picture_launch.
template <class Job> struct PictureKernel;

constexpr int CHUNK_ROWS = 8;
static_assert((uint64_t)CHUNK_ROWS * EGRESS_MAX_WIDTH * 255 * 255 < (1ull << 32), "a workgroup's partial sum of one plane fits 32 bits");

// The job tables hold plain pointers; the kernels address them as global memory (global_load / global_store instead of the flat forms).
#define GLOBAL_AS __attribute__((address_space(1)))
typedef GLOBAL_AS const uint8_t *bytes_in;
typedef GLOBAL_AS uint8_t *bytes_out;
typedef GLOBAL_AS const int16_t *samples_in;
typedef GLOBAL_AS int16_t *samples_out;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_unaligned __attribute__((aligned(1)));

// Exactly the 16 bytes at s / d, whatever the alignment: ONE global_load_dwordx4 / global_store_dwordx4 (the memory pipeline takes vector accesses at any byte address;
// one that straddles a cache line costs a second line access, no more bytes).  Spelling the unaligned case as dword or byte accesses gives the same instruction: the
// backend merges them.
__device__ __forceinline__ u32x4 load16(bytes_in s) { return *(GLOBAL_AS const u32x4_unaligned *)s; }
__device__ __forceinline__ void store16(bytes_out d, u32x4 v) { *(GLOBAL_AS u32x4_unaligned *)d = v; }

// What workgroup b of a W x H picture does.  Its class: luma(), chroma, or nothing (empty()); its rows of that class: [rows().y0, rows().y0 + rows().n); the spans of one row:
// luma_spans() of 16 samples; chroma as pairs (NV12): pair_spans() of 8 U, V pairs; chroma as planes (I420): plane_spans() of 16 samples of the row's U part, then as
// many of its V part.  (Accessors, not fields: each is evaluated where a kernel has already branched on the class, so nothing is computed for another class.)
struct Rows {
	int y0, n;
};
struct Chunk {
	int b, W, H;
	__host__ __device__ __forceinline__ int luma_chunks() const { return (H + CHUNK_ROWS - 1) / CHUNK_ROWS; }
	__host__ __device__ __forceinline__ int chroma_chunks() const { return ((H >> 1) + CHUNK_ROWS - 1) / CHUNK_ROWS; }
	__host__ __device__ __forceinline__ int chunks() const { return luma_chunks() + chroma_chunks(); }      // (the grid's x size for this picture)
	__host__ __device__ __forceinline__ bool luma() const { return b < luma_chunks(); }
	__host__ __device__ __forceinline__ bool empty() const { return b >= chunks(); }
	__host__ __device__ __forceinline__ Rows rows() const
	{
		const int y0 = (luma() ? b : b - luma_chunks()) * CHUNK_ROWS, left = (luma() ? H : H >> 1) - y0;
		return Rows{y0, left < CHUNK_ROWS ? left : CHUNK_ROWS};
	}
	__host__ __device__ __forceinline__ int luma_spans() const { return (W + 15) >> 4; }
	__host__ __device__ __forceinline__ int pair_spans() const { return ((W >> 1) + 7) >> 3; }
	__host__ __device__ __forceinline__ int plane_spans() const { return ((W >> 1) + 15) >> 4; }
};

// ---- ingest ----
__device__ __forceinline__ uint32_t even_bytes(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c020c00u); }      // bytes 0 and 2 of w as two 16-bit values
__device__ __forceinline__ uint32_t odd_bytes(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c030c01u); }       // bytes 1 and 3
__device__ __forceinline__ uint32_t low_bytes(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c010c00u); }       // bytes 0 and 1
__device__ __forceinline__ uint32_t high_bytes(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c030c02u); }      // bytes 2 and 3

// n <= 16 samples of a plane row, widened; d is 16-byte aligned
__device__ __forceinline__ void widen_span(bytes_in s, samples_out d, int n)
{
	if (n == 16) {
		const u32x4 v = load16(s);
		GLOBAL_AS u32x4 *o = (GLOBAL_AS u32x4 *)d;
		o[0] = u32x4{low_bytes(v.x), high_bytes(v.x), low_bytes(v.y), high_bytes(v.y)};
		o[1] = u32x4{low_bytes(v.z), high_bytes(v.z), low_bytes(v.w), high_bytes(v.w)};
		return;
	}
	for (int i = 0; i < n; i++) d[i] = s[i];      // (a row's tail)
}
// n <= 8 pairs of an NV12 chroma row into the U and the V plane; du / dv are 16-byte aligned
__device__ __forceinline__ void split_span(bytes_in s, samples_out du, samples_out dv, int n)
{
	if (n == 8) {
		const u32x4 v = load16(s);
		*(GLOBAL_AS u32x4 *)du = u32x4{even_bytes(v.x), even_bytes(v.y), even_bytes(v.z), even_bytes(v.w)};
		*(GLOBAL_AS u32x4 *)dv = u32x4{odd_bytes(v.x), odd_bytes(v.y), odd_bytes(v.z), odd_bytes(v.w)};
		return;
	}
	for (int i = 0; i < n; i++) { du[i] = s[2 * i]; dv[i] = s[2 * i + 1]; }
}

__global__ __launch_bounds__(HMR_BLOCK) void k_ingest(const IngestJob *jobs)
{
	const IngestJob j = jobs[blockIdx.y];
	const int W = j.width, cw = W >> 1, t = (int)threadIdx.x;
	const Chunk k{(int)blockIdx.x, W, j.height};
	if (k.luma()) {
		const Rows rw = k.rows();
		const int y0 = rw.y0, rows = rw.n, per_row = k.luma_spans();
		const bytes_in src = (bytes_in)j.src[0];
		const samples_out dst = (samples_out)j.dst[0];
		const int64_t pitch = j.pitch[0];
		const int stride = j.stride_y;
		for (int i = t; i < rows * per_row; i += HMR_BLOCK) {
			const int r = i / per_row, x = (i - r * per_row) << 4, y = y0 + r;
			widen_span(src + (int64_t)y * pitch + x, dst + (size_t)y * stride + x, W - x < 16 ? W - x : 16);
		}
		return;
	}
	if (k.empty()) return;
	const Rows rw = k.rows();
	const int y0 = rw.y0, rows = rw.n;
	const int stride = j.stride_c;
	if (j.format == HMR_GPU_PIC_NV12) {
		const int per_row = k.pair_spans();
		const bytes_in src = (bytes_in)j.src[1];
		const samples_out du = (samples_out)j.dst[1], dv = (samples_out)j.dst[2];
		const int64_t pitch = j.pitch[1];
		for (int i = t; i < rows * per_row; i += HMR_BLOCK) {
			const int r = i / per_row, x = (i - r * per_row) << 3, y = y0 + r;
			const size_t o = (size_t)y * stride + x;
			split_span(src + (int64_t)y * pitch + 2 * x, du + o, dv + o, cw - x < 8 ? cw - x : 8);
		}
		return;
	}
	const int per_plane = k.plane_spans(), per_row = 2 * per_plane;      // (a row's U part, then its V part)
	const bytes_in su = (bytes_in)j.src[1], sv = (bytes_in)j.src[2];
	const samples_out du = (samples_out)j.dst[1], dv = (samples_out)j.dst[2];
	const int64_t pu = j.pitch[1], pv = j.pitch[2];
	for (int i = t; i < rows * per_row; i += HMR_BLOCK) {
		const int r = i / per_row, g = i - r * per_row, y = y0 + r;
		const bool is_v = g >= per_plane;
		const int x = (is_v ? g - per_plane : g) << 4;
		widen_span((is_v ? sv : su) + (int64_t)y * (is_v ? pv : pu) + x, (is_v ? dv : du) + (size_t)y * stride + x, cw - x < 16 ? cw - x : 16);
	}
}
template <> struct PictureKernel<IngestJob> { static constexpr auto kernel = k_ingest; static int chunks(const IngestJob &j) { return Chunk{0, j.width, j.height}.chunks(); } };

// ---- RGB ingest ----
// The forms a span is read in (a launch mixes them: one per picture).  PX pixels of a row are held as raw dwords: packed - the row's bytes as they lie; planar - PX
// samples of R, then of G, then of B.
enum { RGB_PACKED3, RGB_PACKED4, RGB_PLANAR8, RGB_F16, RGB_F32 };
template <int V> struct RgbForm {
	static constexpr int PX = V == RGB_F32 ? 8 : 16;      // pixels read at a time (binary32: half a span, 96 bytes a row)
	static constexpr int PLANE = V == RGB_PLANAR8 ? PX / 4 : V == RGB_F16 ? PX / 2 : PX;      // dwords per channel (planar)
	static constexpr int WORDS = V == RGB_PACKED3 ? 3 * PX / 4 : V == RGB_PACKED4 ? PX : 3 * PLANE;
	static constexpr int FMT = V == RGB_PLANAR8 ? HMR_GPU_RGB_PLANAR8 : V == RGB_F16 ? HMR_GPU_RGB_PLANAR_F16 : V == RGB_F32 ? HMR_GPU_RGB_PLANAR_F32 : HMR_GPU_RGB_PACKED8;      // (for rgb_sample)
};
// a compile-time tag: what rgb_dispatch / yuv_dispatch hand a generic callable
template <int N> struct Int { static constexpr int value = N; };
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
// which of the forms RGB_PACKED3 .. RGB_F32 a descriptor's format and pixel bytes are
__host__ __device__ __forceinline__ int rgb_form(int format, int pixel_bytes)
{
	return format == HMR_GPU_RGB_PACKED8 ? (pixel_bytes == 3 ? RGB_PACKED3 : RGB_PACKED4) : format == HMR_GPU_RGB_PLANAR8 ? RGB_PLANAR8 : format == HMR_GPU_RGB_PLANAR_F16 ? RGB_F16 : RGB_F32;
}

template <int V, class Job>
__device__ __forceinline__ void rgb_load_row(const Job &j, int x, int y, uint32_t *raw)
{
	typedef RgbForm<V> F;
	if (V == RGB_PACKED3 || V == RGB_PACKED4) {
		const bytes_in s = (bytes_in)j.src[0] + (int64_t)y * j.pitch[0] + (int64_t)x * (V == RGB_PACKED3 ? 3 : 4);
#pragma unroll
		for (int k = 0; k < F::WORDS / 4; k++) {
			const u32x4 v = load16(s + 16 * k);
			raw[4 * k] = v.x; raw[4 * k + 1] = v.y; raw[4 * k + 2] = v.z; raw[4 * k + 3] = v.w;
		}
		return;
	}
	constexpr int elem = V == RGB_PLANAR8 ? 1 : V == RGB_F16 ? 2 : 4;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const bytes_in s = (bytes_in)j.src[c] + (int64_t)y * j.pitch[c] + (int64_t)x * elem;
#pragma unroll
		for (int k = 0; k < F::PLANE / 4; k++) {
			const u32x4 v = load16(s + 16 * k);
			uint32_t *o = raw + c * F::PLANE + 4 * k;
			o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
		}
	}
}

// R, G, B of pixel i of a row's raw dwords; sh[c] = 8 * offset[c] (packed)
template <int V>
__device__ __forceinline__ void rgb_pixel(const uint32_t *raw, int i, const int sh[3], int &r, int &g, int &b)
{
	typedef RgbForm<V> F;
	if (V == RGB_PACKED3 || V == RGB_PACKED4) {
		uint32_t w;
		if (V == RGB_PACKED4) w = raw[i];
		else {
			const int d = (3 * i) >> 2, s = (3 * i) & 3;      // the pixel's three bytes start at byte s of dword d
			w = s ? __builtin_amdgcn_alignbyte(d + 1 < F::WORDS ? raw[d + 1] : 0u, raw[d], (uint32_t)s) : raw[d];
		}
		r = (int)((w >> sh[0]) & 255u); g = (int)((w >> sh[1]) & 255u); b = (int)((w >> sh[2]) & 255u);
		return;
	}
	const uint32_t *pr = raw, *pg = raw + F::PLANE, *pb = raw + 2 * F::PLANE;
	if (V == RGB_PLANAR8) {
		const int d = i >> 2, s = 8 * (i & 3);
		r = (int)((pr[d] >> s) & 255u); g = (int)((pg[d] >> s) & 255u); b = (int)((pb[d] >> s) & 255u);
	} else if (V == RGB_F16) {
		const int d = i >> 1;
		const f16x2 hr = __builtin_bit_cast(f16x2, pr[d]), hg = __builtin_bit_cast(f16x2, pg[d]), hb = __builtin_bit_cast(f16x2, pb[d]);
		r = hmr_rgb_quantize((float)((i & 1) ? hr.y : hr.x)); g = hmr_rgb_quantize((float)((i & 1) ? hg.y : hg.x)); b = hmr_rgb_quantize((float)((i & 1) ? hb.y : hb.x));
	} else {
		r = hmr_rgb_quantize(__builtin_bit_cast(float, pr[i])); g = hmr_rgb_quantize(__builtin_bit_cast(float, pg[i])); b = hmr_rgb_quantize(__builtin_bit_cast(float, pb[i]));
	}
}

// the sample-by-sample R, G, B of pixel (px, py) of a job's picture of format FMT: rgb_yuv.h's rgb_sample - the one the host twin runs - on global pointers (the rows' tails)
template <int FMT, class Job>
__device__ __forceinline__ void rgb_sample3(const Job &j, int px, int py, int c3[3])
{
	constexpr bool packed = FMT == HMR_GPU_RGB_PACKED8;
#pragma unroll
	for (int c = 0; c < 3; c++)
		c3[c] = rgb_sample<bytes_in, GLOBAL_AS const _Float16 *, GLOBAL_AS const float *>((bytes_in)j.src[packed ? 0 : c], j.pitch[packed ? 0 : c], FMT, j.pixel_bytes, j.offset[c], px, py);
}

// the 2 x 2 block of pixels i, i + 1 of two adjacent rows a, b: its four pixels (a's two, then b's) and their R, G, B sums - what one chroma sample is made of
template <int V>
__device__ __forceinline__ void rgb_quad(const uint32_t *a, const uint32_t *b, int i, const int sh[3], int px[4][3], int s[3])
{
#pragma unroll
	for (int k = 0; k < 4; k++) rgb_pixel<V>(k < 2 ? a : b, i + (k & 1), sh, px[k][0], px[k][1], px[k][2]);
#pragma unroll
	for (int c = 0; c < 3; c++) s[c] = px[0][c] + px[1][c] + px[2][c] + px[3][c];
}

// 16 pixels at (x, y) of rows y and y + 1 in pieces of F::PX pixels (binary32: two halves, the other forms one load a row): half(h, a, b, i0) for h = 0, 1 - the
// eight pixels of half h are pixels i0 .. i0 + 7 of the raw rows a and b
template <int V, class Job, class Half>
__device__ __forceinline__ void rgb_two_rows(const Job &j, int x, int y, Half half)
{
	typedef RgbForm<V> F;
	if (F::PX == 8) {
#pragma unroll
		for (int h = 0; h < 2; h++) {
			uint32_t a[F::WORDS], b[F::WORDS];
			rgb_load_row<V>(j, x + 8 * h, y, a);
			rgb_load_row<V>(j, x + 8 * h, y + 1, b);
			half(h, a, b, 0);
		}
	} else {
		uint32_t a[F::WORDS], b[F::WORDS];
		rgb_load_row<V>(j, x, y, a);
		rgb_load_row<V>(j, x, y + 1, b);
#pragma unroll
		for (int h = 0; h < 2; h++) half(h, a, b, 8 * h);
	}
}

// pixels i0 .. i0 + 7 of two adjacent rows a, b: eight luma samples of each row and four U and four V samples, as int16 pairs
template <int V>
__device__ __forceinline__ void rgb_convert8(const uint32_t *a, const uint32_t *b, int i0, const RgbMatrix &m, const int sh[3], u32x4 &ya, u32x4 &yb, uint32_t *u, uint32_t *v)
{
	uint32_t la[4], lb[4], cu[4], cv[4];
#pragma unroll
	for (int p = 0; p < 4; p++) {
		int px[4][3], s[3];
		rgb_quad<V>(a, b, i0 + 2 * p, sh, px, s);
		la[p] = (uint32_t)hmr_rgb_luma(m, px[0][0], px[0][1], px[0][2]) | (uint32_t)hmr_rgb_luma(m, px[1][0], px[1][1], px[1][2]) << 16;
		lb[p] = (uint32_t)hmr_rgb_luma(m, px[2][0], px[2][1], px[2][2]) | (uint32_t)hmr_rgb_luma(m, px[3][0], px[3][1], px[3][2]) << 16;
		cu[p] = (uint32_t)hmr_rgb_chroma(m.u, s[0], s[1], s[2]);
		cv[p] = (uint32_t)hmr_rgb_chroma(m.v, s[0], s[1], s[2]);
	}
	ya = u32x4{la[0], la[1], la[2], la[3]};
	yb = u32x4{lb[0], lb[1], lb[2], lb[3]};
	u[0] = cu[0] | cu[1] << 16; u[1] = cu[2] | cu[3] << 16;
	v[0] = cv[0] | cv[1] << 16; v[1] = cv[2] | cv[3] << 16;
}

// 16 pixels at (x, y) of rows y and y + 1 (x a multiple of 16, y even): 32 luma samples, 8 U and 8 V samples
template <int V>
__device__ __forceinline__ void rgb_span(const RgbIngestJob &j, int x, int y, const int sh[3])
{
	u32x4 ya[2], yb[2];
	uint32_t u[4], v[4];
	rgb_two_rows<V>(j, x, y, [&](int h, const uint32_t *a, const uint32_t *b, int i0) { rgb_convert8<V>(a, b, i0, j.m, sh, ya[h], yb[h], u + 2 * h, v + 2 * h); });
	GLOBAL_AS u32x4 *oa = (GLOBAL_AS u32x4 *)((samples_out)j.dst[0] + (size_t)y * j.stride_y + x), *ob = (GLOBAL_AS u32x4 *)((samples_out)j.dst[0] + (size_t)(y + 1) * j.stride_y + x);
	oa[0] = ya[0]; oa[1] = ya[1];
	ob[0] = yb[0]; ob[1] = yb[1];
	const size_t oc = (size_t)(y >> 1) * j.stride_c + (x >> 1);
	*(GLOBAL_AS u32x4 *)((samples_out)j.dst[1] + oc) = u32x4{u[0], u[1], u[2], u[3]};
	*(GLOBAL_AS u32x4 *)((samples_out)j.dst[2] + oc) = u32x4{v[0], v[1], v[2], v[3]};
}

// the 2 x 2 block at (bx, y) of a picture of format FMT, sample by sample (a row's tail)
template <int FMT>
__device__ __forceinline__ void rgb_block(const RgbIngestJob &j, int bx, int y)
{
	const samples_out dy = (samples_out)j.dst[0];
	int s[3] = {0, 0, 0};
#pragma unroll
	for (int k = 0; k < 4; k++) {
		const int px = bx + (k & 1), py = y + (k >> 1);
		int c3[3];
		rgb_sample3<FMT>(j, px, py, c3);
#pragma unroll
		for (int c = 0; c < 3; c++) s[c] += c3[c];
		dy[(size_t)py * j.stride_y + px] = (int16_t)hmr_rgb_luma(j.m, c3[0], c3[1], c3[2]);
	}
	const size_t oc = (size_t)(y >> 1) * j.stride_c + (bx >> 1);
	((samples_out)j.dst[1])[oc] = (int16_t)hmr_rgb_chroma(j.m.u, s[0], s[1], s[2]);
	((samples_out)j.dst[2])[oc] = (int16_t)hmr_rgb_chroma(j.m.v, s[0], s[1], s[2]);
}

// The chunk walk of k_ingest_rgb and k_ingest_yuv: block b of a picture takes the CHUNK_ROWS luma rows from b * CHUNK_ROWS on, two at a time - span(x, y) for every whole
// span of 16 pixels of rows y and y + 1, then block(bx, y) for the 2 x 2 blocks of the row's tail of fewer than 16 pixels, a lane per block.
__host__ __device__ __forceinline__ int pair_chunks(int height) { return (height + CHUNK_ROWS - 1) / CHUNK_ROWS; }
template <class Job, class Span, class Block>
__device__ __forceinline__ void pair_chunk(const Job &j, int y0, Span span, Block block)
{
	const int left = j.height - y0, pairs = (left < CHUNK_ROWS ? left : CHUNK_ROWS) >> 1, per_row = j.width >> 4;      // (whole spans)
	for (int i = (int)threadIdx.x; i < pairs * per_row; i += HMR_BLOCK) {
		const int r = i / per_row, x = (i - r * per_row) << 4, y = y0 + 2 * r;
		span(x, y);
	}
	const int tail = (j.width & 15) >> 1;
	for (int i = (int)threadIdx.x; i < pairs * tail; i += HMR_BLOCK) {
		const int r = i / tail;
		block((j.width & ~15) + 2 * (i - r * tail), y0 + 2 * r);
	}
}

// The forms of the RGB family, once: with(Int<V>) for the form V of a job's picture (k_ingest_rgb, k_rgb_ladder; a launch mixes forms, one per picture)
template <class Job, class With>
__device__ __forceinline__ void rgb_dispatch(const Job &j, With with)
{
	switch (rgb_form(j.format, j.pixel_bytes)) {
	case RGB_PACKED3: with(Int<RGB_PACKED3>{}); break;
	case RGB_PACKED4: with(Int<RGB_PACKED4>{}); break;
	case RGB_PLANAR8: with(Int<RGB_PLANAR8>{}); break;
	case RGB_F16: with(Int<RGB_F16>{}); break;
	default: with(Int<RGB_F32>{}); break;
	}
}

__global__ __launch_bounds__(HMR_BLOCK) void k_ingest_rgb(const RgbIngestJob *jobs)
{
	const RgbIngestJob j = jobs[blockIdx.y];
	const int y0 = (int)blockIdx.x * CHUNK_ROWS;
	if (y0 >= j.height) return;
	const int sh[3] = {8 * j.offset[0], 8 * j.offset[1], 8 * j.offset[2]};
	rgb_dispatch(j, [&](auto form) {
		constexpr int V = decltype(form)::value;
		pair_chunk(j, y0, [&](int x, int y) { rgb_span<V>(j, x, y, sh); }, [&](int bx, int y) { rgb_block<RgbForm<V>::FMT>(j, bx, y); });
	});
}
template <> struct PictureKernel<RgbIngestJob> { static constexpr auto kernel = k_ingest_rgb; static int chunks(const RgbIngestJob &j) { return pair_chunks(j.height); } };

// ---- deep / 4:2:2 / 4:4:4 ingest (section 12k) ----
// k_ingest_yuv: Y'CbCr pictures of 8 .. 16 bits - 4:2:0, 4:2:2 or 4:4:4; planar, semi-planar in either order, or packed 4:2:2 in any of its four orders - into the int16
// planes of a slot, rounded to 8-bit 4:2:0 by the integer arithmetic of yuv_depth.h in the same pass.  sb (W H + 2 Wc Hc) bytes read, 3 W H written per picture
//.  The mapping is k_ingest_rgb's: blockIdx.y = picture, blockIdx.x = a chunk of CHUNK_ROWS luma rows; a lane takes a span of 16
// pixels of TWO adjacent luma rows and every chroma sample that lies over them, so the 1, 2 or 4 taps of a chroma output never leave the lane and a packed picture's
// bytes are read once for luma and chroma.  Per lane: the luma rows' bytes by 16-byte loads at whatever address the pitch gives (one a row for 8-bit planes, two for
// 16-bit planes or 8-bit packed, four for 16-bit packed); the chroma rows' (one row for 4:2:0, two otherwise; 8 columns, 16 for 4:4:4; ONE 8-byte load where a row's
// part is 8 bytes: 8-bit planar 4:2:0 / 4:2:2); four 16-byte stores of int16 luma and one each of eight U and eight V samples.  The kernel is specialised on the layout,
// the container's width and the tap count (14 instantiations, picked per job: a launch mixes forms); the shifts, the clamp and the offsets inside a pair or a group are
// the job's and uniform over a workgroup.  Samples are picked from the loaded dwords at indices fixed at compile time (v_bfe_u32 / v_perm_b32; a 16-bit group of four by a
// 64-bit shift, v_lshrrev_b64).  A row's tail of fewer than 16 pixels goes sample by sample, a lane per 2 x 2 block, through yuv_depth.h's own sample functions - the
// ones the host twin runs.  No LDS, no atomics.  No lane reads a byte outside [plane + y * pitch, plane + y * pitch + row bytes): whole spans lie inside the width.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_unaligned __attribute__((aligned(1)));
__device__ __forceinline__ u32x2 load8(bytes_in s) { return *(GLOBAL_AS const u32x2_unaligned *)s; }

// BYTES (8, or a multiple of 16) bytes at s as dwords
template <int BYTES>
__device__ __forceinline__ void yuv_load(bytes_in s, uint32_t *w)
{
	if (BYTES == 8) {
		const u32x2 v = load8(s);
		w[0] = v.x; w[1] = v.y;
		return;
	}
#pragma unroll
	for (int k = 0; k < BYTES / 16; k++) {
		const u32x4 v = load16(s + 16 * k);
		w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
	}
}

// The container `shift` bits into group g (a compile-time index) of a row's dwords; a group is G containers of SB bytes: a sample of a plane (G = 1), a pair of a
// semi-planar chroma plane or of a packed row's luma (G = 2), two pixels of a packed row (G = 4).
template <int SB, int G>
__device__ __forceinline__ uint32_t yuv_pick(const uint32_t *w, int g, int shift)
{
	constexpr int GROUP_BITS = 8 * SB * G;
	constexpr uint32_t mask = SB == 1 ? 255u : 65535u;
	if (GROUP_BITS == 64) return (uint32_t)((((uint64_t)w[2 * g + 1] << 32) | w[2 * g]) >> shift) & mask;
	if (GROUP_BITS == 32) return (w[g] >> shift) & mask;
	if (GROUP_BITS == 16) return (w[g >> 1] >> (16 * (g & 1) + shift)) & mask;
	return (w[g >> 2] >> (8 * (g & 3))) & mask;
}

enum { YUV_PLANAR = HMR_YUV_PLANAR, YUV_SEMI = HMR_YUV_SEMIPLANAR, YUV_PACKED = HMR_YUV_PACKED422 };
// what a lane reads of a row: L the layout, SB the container's bytes, K log2 of the chroma taps
template <int L, int SB, int K> struct YuvSpan {
	static constexpr int LUMA_BYTES = (L == YUV_PACKED ? 32 : 16) * SB;             // 16 pixels of a luma (or packed) row
	static constexpr int COLS = K == 2 ? 16 : 8;                                     // chroma columns under 16 pixels
	static constexpr int ROWS = K == 0 ? 1 : 2;                                      // chroma rows under two luma rows
	static constexpr int CHROMA_BYTES = COLS * SB * (L == YUV_SEMI ? 2 : 1);         // of one row of one chroma plane (planar) or of the pairs' plane
	static constexpr int TAPS = K == 2 ? 2 : 1;                                      // per row
};

// The chroma tap sums of eight columns of the converted 4:2:0 chroma planes, added into su (U) and sv (V); the caller rounds a sum with f.s + K.  (8 bits: s = 0,
// maxv = 255, rs = 0 - hmr_yuv_value is the identity and is left out.)  Two forms, both for k_ingest_yuv's spans and k_yuv_ladder's chroma tiles:
// a packed row that is already in registers - group c of its 8 groups (16 pixels) holds chroma column c; the two rows under a chroma row make K = 1
template <int SB>
__device__ __forceinline__ void yuv_taps_packed(const YuvForm &f, const uint32_t *g, uint32_t *su, uint32_t *sv)
{
	const int bits1 = 8 * SB * f.offset[1], bits2 = 8 * SB * f.offset[2];
#pragma unroll
	for (int c = 0; c < 8; c++) {
		const uint32_t u = yuv_pick<SB, 4>(g, c, bits1), v = yuv_pick<SB, 4>(g, c, bits2);
		su[c] += SB == 1 ? u : hmr_yuv_value(f, u);
		sv[c] += SB == 1 ? v : hmr_yuv_value(f, v);
	}
}
// the planar and semi-planar layouts: loads the F::ROWS x 8 F::TAPS containers of U and of V under columns cx .. cx + 7 of converted chroma row cy (Job: YuvIngestJob, YuvScaleJob)
template <int L, int SB, int K, class Job>
__device__ __forceinline__ void yuv_taps_planes(const Job &j, int cx, int cy, uint32_t *su, uint32_t *sv)
{
	typedef YuvSpan<L, SB, K> F;
	const YuvForm &f = j.f;
	const int bits1 = 8 * SB * f.offset[1], bits2 = 8 * SB * f.offset[2];
	const int row0 = K == 0 ? cy : 2 * cy, col0 = K == 2 ? 2 * cx : cx;
#pragma unroll
	for (int r = 0; r < F::ROWS; r++) {
		uint32_t cu[F::CHROMA_BYTES / 4], cv[F::CHROMA_BYTES / 4];
		yuv_load<F::CHROMA_BYTES>((bytes_in)j.src[1] + (int64_t)(row0 + r) * j.pitch[1] + (int64_t)col0 * SB * (L == YUV_SEMI ? 2 : 1), cu);
		if (L == YUV_PLANAR) yuv_load<F::CHROMA_BYTES>((bytes_in)j.src[2] + (int64_t)(row0 + r) * j.pitch[2] + (int64_t)col0 * SB, cv);
#pragma unroll
		for (int c = 0; c < 8; c++)
#pragma unroll
			for (int t = 0; t < F::TAPS; t++) {
				const int i = c * F::TAPS + t;
				const uint32_t u = L == YUV_SEMI ? yuv_pick<SB, 2>(cu, i, bits1) : yuv_pick<SB, 1>(cu, i, 0);
				const uint32_t v = L == YUV_SEMI ? yuv_pick<SB, 2>(cu, i, bits2) : yuv_pick<SB, 1>(cv, i, 0);
				su[c] += SB == 1 ? u : hmr_yuv_value(f, u);
				sv[c] += SB == 1 ? v : hmr_yuv_value(f, v);
			}
	}
}

// 16 pixels at (x, y) of rows y and y + 1 (x a multiple of 16, y even): 32 luma samples, 8 U and 8 V samples
template <int L, int SB, int K>
__device__ __forceinline__ void yuv_span(const YuvIngestJob &j, int x, int y)
{
	typedef YuvSpan<L, SB, K> F;
	const YuvForm &f = j.f;
	const int bits0 = 8 * SB * f.offset[0];
	uint32_t la[2][F::LUMA_BYTES / 4];
#pragma unroll
	for (int r = 0; r < 2; r++) yuv_load<F::LUMA_BYTES>((bytes_in)j.src[0] + (int64_t)(y + r) * j.pitch[0] + (int64_t)x * (L == YUV_PACKED ? 2 : 1) * SB, la[r]);
#pragma unroll
	for (int r = 0; r < 2; r++) {
		uint32_t o[8];
#pragma unroll
		for (int q = 0; q < 8; q++) {
			if (SB == 1 && L != YUV_PACKED) {      // 8 bits: the sample itself
				o[q] = (q & 1) ? high_bytes(la[r][q >> 1]) : low_bytes(la[r][q >> 1]);
				continue;
			}
			const uint32_t a = L == YUV_PACKED ? yuv_pick<SB, 2>(la[r], 2 * q, bits0) : yuv_pick<SB, 1>(la[r], 2 * q, 0);
			const uint32_t b = L == YUV_PACKED ? yuv_pick<SB, 2>(la[r], 2 * q + 1, bits0) : yuv_pick<SB, 1>(la[r], 2 * q + 1, 0);
			o[q] = SB == 1 ? a | b << 16 : hmr_yuv_round(hmr_yuv_value(f, a), f.s) | hmr_yuv_round(hmr_yuv_value(f, b), f.s) << 16;
		}
		GLOBAL_AS u32x4 *d = (GLOBAL_AS u32x4 *)((samples_out)j.dst[0] + (size_t)(y + r) * j.stride_y + x);
		d[0] = u32x4{o[0], o[1], o[2], o[3]};
		d[1] = u32x4{o[4], o[5], o[6], o[7]};
	}
	uint32_t su[8] = {}, sv[8] = {};
	if (L == YUV_PACKED) {      // the rows are here already
#pragma unroll
		for (int r = 0; r < 2; r++) yuv_taps_packed<SB>(f, la[r], su, sv);
	} else yuv_taps_planes<L, SB, K>(j, x >> 1, y >> 1, su, sv);
	const int t = f.s + K;
	uint32_t ou[4], ov[4];
#pragma unroll
	for (int q = 0; q < 4; q++) {
		ou[q] = hmr_yuv_round(su[2 * q], t) | hmr_yuv_round(su[2 * q + 1], t) << 16;
		ov[q] = hmr_yuv_round(sv[2 * q], t) | hmr_yuv_round(sv[2 * q + 1], t) << 16;
	}
	const size_t oc = (size_t)(y >> 1) * j.stride_c + (x >> 1);
	*(GLOBAL_AS u32x4 *)((samples_out)j.dst[1] + oc) = u32x4{ou[0], ou[1], ou[2], ou[3]};
	*(GLOBAL_AS u32x4 *)((samples_out)j.dst[2] + oc) = u32x4{ov[0], ov[1], ov[2], ov[3]};
}

// the 2 x 2 block at (bx, y), sample by sample (a row's tail): yuv_depth.h's functions on global pointers
__device__ __forceinline__ void yuv_block(const YuvIngestJob &j, int bx, int y)
{
	const samples_out dy = (samples_out)j.dst[0];
#pragma unroll
	for (int k = 0; k < 4; k++) {
		const int px = bx + (k & 1), py = y + (k >> 1);
		dy[(size_t)py * j.stride_y + px] = (int16_t)hmr_yuv_luma<bytes_in>(j.src, j.pitch, j.f, px, py);
	}
	const size_t oc = (size_t)(y >> 1) * j.stride_c + (bx >> 1);
	((samples_out)j.dst[1])[oc] = (int16_t)hmr_yuv_chroma<bytes_in>(j.src, j.pitch, j.f, 1, bx >> 1, y >> 1);
	((samples_out)j.dst[2])[oc] = (int16_t)hmr_yuv_chroma<bytes_in>(j.src, j.pitch, j.f, 2, bx >> 1, y >> 1);
}

// The forms of the Y'CbCr family, once (k_ingest_yuv, k_yuv_ladder; a launch mixes forms, one per picture): yuv_dispatch gives with(Int<L>, Int<SB>) for the layout and
// the container of a form, yuv_dispatch_taps then with(Int<K>) for its tap count - apart, because a ladder's luma tiles do not depend on K, and a packed picture is K = 1 only.
template <class With>
__device__ __forceinline__ void yuv_dispatch(const YuvForm &f, With with)
{
	const bool wide = f.sb == 2;
	switch (f.format) {
	case HMR_YUV_PLANAR:
		if (wide) with(Int<YUV_PLANAR>{}, Int<2>{});
		else with(Int<YUV_PLANAR>{}, Int<1>{});
		break;
	case HMR_YUV_SEMIPLANAR:
		if (wide) with(Int<YUV_SEMI>{}, Int<2>{});
		else with(Int<YUV_SEMI>{}, Int<1>{});
		break;
	default:
		if (wide) with(Int<YUV_PACKED>{}, Int<2>{});
		else with(Int<YUV_PACKED>{}, Int<1>{});
		break;
	}
}
template <int L, class With>
__device__ __forceinline__ void yuv_dispatch_taps(const YuvForm &f, With with)
{
	if (L == YUV_PACKED || f.k == 1) with(Int<1>{});
	else if (f.k == 0) with(Int<0>{});
	else with(Int<2>{});
}

__global__ __launch_bounds__(HMR_BLOCK) void k_ingest_yuv(const YuvIngestJob *jobs)
{
	const YuvIngestJob j = jobs[blockIdx.y];
	const int y0 = (int)blockIdx.x * CHUNK_ROWS;
	if (y0 >= j.height) return;
	yuv_dispatch(j.f, [&](auto layout, auto container) {
		constexpr int L = decltype(layout)::value, SB = decltype(container)::value;
		yuv_dispatch_taps<L>(j.f, [&](auto taps) {
			pair_chunk(j, y0, [&](int x, int y) { yuv_span<L, SB, decltype(taps)::value>(j, x, y); }, [&](int bx, int y) { yuv_block(j, bx, y); });
		});
	});
}
template <> struct PictureKernel<YuvIngestJob> { static constexpr auto kernel = k_ingest_yuv; static int chunks(const YuvIngestJob &j) { return pair_chunks(j.height); } };

// ---- downscaling ingest (section 12g) ----
// k_downscale: 8-bit pictures of one size, area-averaged (scale_area.h) into the int16 planes of a smaller - or equal - size.  1.5 Ws Hs bytes read, 3 Wd Hd written per
// picture.  blockIdx.y = picture; blockIdx.x = a tile of tile_rows output rows x SCALE_TILE_W output columns of one plane class - the
// luma tiles first, then the chroma tiles (a chroma tile holds SCALE_TILE_W / 2 columns of U and as many of V, so that NV12's pairs are read once); smaller pictures
// leave their last blocks empty.  Vertical pass first (scale_columns16 with the row policy ScaleBytes): a lane takes a span of 16 bytes of the source columns the tile covers and ONE output row, walks that row's source
// rows (at most nine) with 16-byte loads at whatever address the pitch gives and keeps the sixteen weighted column sums in 32-bit registers; they go to LDS, a span in
// SCALE_SPAN_WORDS words (16 and 4 of padding: the eight lanes of a 16-byte LDS store hit eight different quads of banks).  NV12's pairs stay interleaved in LDS - the
// vertical pass works on bytes - and the horizontal pass picks every second column.  Horizontal pass: a lane per output sample, consecutive lanes consecutive columns,
// the taps read from LDS, ONE division (a multiplication by the job's reciprocal, exact: hmr_scale_div), the int16 result to a second LDS tile; from there a lane per
// eight samples writes whole 16-byte stores (the int16 side is 16-byte aligned: tiles start at multiples of 128 / 64 columns), a row's tail sample by sample.
// A source row that two output rows of a tile share is loaded by two lanes of the same workgroup; the row or column two TILES share is read by both.  No lane reads a
// byte outside [plane + y * pitch, plane + y * pitch + row bytes) or writes outside dst_w x dst_h.
// tile_rows: the LDS holds SCALE_LDS_WORDS column sums; a tile row needs (spans of the tile) x SCALE_SPAN_WORDS of them, at most SCALE_MAX_SPANS spans at ratio 8
// (128 x 8 + 1 luma columns: 65 spans; 2 x (64 x 8 + 1) chroma columns: 66), so 8 rows always fit and a picture scaled by less gets taller tiles, up to 32 rows:
// more loads in flight per workgroup.  42 240 + 8 192 bytes of LDS: three workgroups a CU.
constexpr int SCALE_TILE_W = 128, SCALE_SPAN_WORDS = 20, SCALE_MIN_ROWS = 8, SCALE_MAX_ROWS = 32, SCALE_MAX_SPANS = 66;
constexpr int SCALE_LDS_WORDS = SCALE_MIN_ROWS * SCALE_MAX_SPANS * SCALE_SPAN_WORDS;
static_assert((SCALE_TILE_W * HMR_SCALE_MAX_RATIO + 1 + 15) / 16 <= SCALE_MAX_SPANS && 2 * ((SCALE_TILE_W / 2 * HMR_SCALE_MAX_RATIO + 1 + 15) / 16) <= SCALE_MAX_SPANS, "a tile row at the largest ratio");
static_assert(SCALE_LDS_WORDS * 4 + SCALE_MAX_ROWS * SCALE_TILE_W * 2 <= 80 * 1024, "two workgroups a CU at least");

// The tile of block b of a picture: its class and plane size, its outputs [x0, x0 + nx) x [y0, y0 + ny), the source columns [c0, c1) they touch, and how those are
// read: `streams` runs of `spans` 16-byte spans per source row, starting at byte `b0` of a row of `row_bytes` bytes.
struct ScaleTile {
	bool luma, empty, pairs;      // pairs: NV12 chroma
	int x0, nx, y0, ny, c0, streams, spans, b0, row_bytes;
	__host__ __device__ __forceinline__ int total() const { return streams * spans; }
};
__host__ __device__ __forceinline__ int scale_tiles_x(int w, bool luma) { return luma ? (w + SCALE_TILE_W - 1) / SCALE_TILE_W : ((w >> 1) + SCALE_TILE_W / 2 - 1) / (SCALE_TILE_W / 2); }
__host__ __device__ __forceinline__ int scale_tiles_y(int h, int rows, bool luma) { return ((luma ? h : h >> 1) + rows - 1) / rows; }
template <class Job>
__host__ __device__ __forceinline__ int scale_tiles(const Job &j)
{
	return scale_tiles_x(j.dst_w, true) * scale_tiles_y(j.dst_h, j.tile_rows, true) + scale_tiles_x(j.dst_w, false) * scale_tiles_y(j.dst_h, j.tile_rows, false);
}
// (Job: ScaleJob, or RgbScaleJob / YuvScaleJob - whose source is never read in pairs, and whose chroma tile's columns are columns of the converted chroma planes)
template <class Job>
__host__ __device__ __forceinline__ ScaleTile scale_tile(const Job &j, int b, bool nv12)
{
	ScaleTile t;
	const int luma_tiles = scale_tiles_x(j.dst_w, true) * scale_tiles_y(j.dst_h, j.tile_rows, true);
	t.luma = b < luma_tiles;
	if (!t.luma) b -= luma_tiles;
	const int across = scale_tiles_x(j.dst_w, t.luma), down = scale_tiles_y(j.dst_h, j.tile_rows, t.luma);
	t.empty = b >= across * down;
	const int ty = b / across, tx = b - ty * across, per = t.luma ? SCALE_TILE_W : SCALE_TILE_W / 2;
	const int pw = t.luma ? j.dst_w : j.dst_w >> 1, ph = t.luma ? j.dst_h : j.dst_h >> 1, sw = t.luma ? j.src_w : j.src_w >> 1;
	t.x0 = tx * per; t.nx = pw - t.x0 < per ? pw - t.x0 : per;
	t.y0 = ty * j.tile_rows; t.ny = ph - t.y0 < j.tile_rows ? ph - t.y0 : j.tile_rows;
	t.pairs = !t.luma && nv12;
	t.c0 = t.empty ? 0 : (int)hmr_scale_first(j.ax, (uint32_t)t.x0);
	const int c1 = t.empty ? 0 : (int)hmr_scale_end(j.ax, (uint32_t)(t.x0 + t.nx - 1));
	t.streams = t.luma || t.pairs ? 1 : 2;
	t.b0 = t.pairs ? 2 * t.c0 : t.c0;
	t.row_bytes = t.pairs ? 2 * sw : sw;
	t.spans = ((t.pairs ? 2 : 1) * (c1 - t.c0) + 15) >> 4;
	return t;
}

// the word of LDS (inside a tile row) that holds the column sum of byte `b` of a stream's window
__device__ __forceinline__ int scale_word(int b) { return (b >> 4) * SCALE_SPAN_WORDS + (b & 15); }

// The horizontal pass and the store pass of a tile whose column sums lie in `sums` (every lane of the workgroup comes here, behind the barrier that follows the
// vertical pass): k_downscale, k_rgb_ladder and k_yuv_ladder share them.
__device__ __forceinline__ void scale_finish(const ScaleTile &k, const ScaleAxis &ax, uint32_t den, uint32_t mden, const uint32_t *sums, u32x4 *outs4, int row_words, int16_t *dst_y, int16_t *dst_u,
					     int16_t *dst_v, int stride_y, int stride_c)
{
	int16_t *outs = (int16_t *)outs4;
	const int t = (int)threadIdx.x;
	// horizontal: an output sample per lane; a chroma tile row: SCALE_TILE_W / 2 of U, then as many of V
	const int half_w = SCALE_TILE_W / 2;
	for (int i = t; i < k.ny * SCALE_TILE_W; i += HMR_BLOCK) {
		const int r = i / SCALE_TILE_W, q = i - r * SCALE_TILE_W;
		const int second = k.luma ? 0 : q / half_w, xx = k.luma ? q : q - second * half_w;
		if (xx >= k.nx) continue;
		const uint32_t x = (uint32_t)(k.x0 + xx), hi = (x + 1) * ax.s;
		const uint32_t *line = sums + r * row_words + (second && !k.pairs ? k.spans * SCALE_SPAN_WORDS : 0);
		uint32_t sum = den >> 1;
		for (uint32_t c = hmr_scale_first(ax, x); c * ax.d < hi; c++) {
			const int rel = (int)c - k.c0;
			sum += hmr_scale_weight(ax, x, c) * line[scale_word(k.pairs ? 2 * rel + second : rel)];
		}
		outs[i] = (int16_t)hmr_scale_div(sum, den, mden);
	}
	__syncthreads();

	// eight samples per lane to the planes
	const int stride = k.luma ? stride_y : stride_c;
	for (int i = t; i < k.ny * (SCALE_TILE_W / 8); i += HMR_BLOCK) {
		const int r = i / (SCALE_TILE_W / 8), q = i - r * (SCALE_TILE_W / 8);
		const int second = k.luma ? 0 : q / (half_w / 8), xx = (k.luma ? q : q - second * (half_w / 8)) << 3;
		if (xx >= k.nx) continue;
		const samples_out d = (samples_out)(k.luma ? dst_y : second ? dst_v : dst_u) + (size_t)(k.y0 + r) * stride + k.x0 + xx;
		if (k.nx - xx >= 8) *(GLOBAL_AS u32x4 *)d = outs4[i];
		else
			for (int m = 0; m < k.nx - xx; m++) d[m] = outs[8 * i + m];      // (a row's tail)
	}
}

// The vertical pass of a tile (k_downscale, k_rgb_ladder, k_yuv_ladder): every lane of the workgroup comes here, in front of the barrier.  What a source row gives is
// the kernel's ROW POLICY P: built once a tile from the job, in front of the lane loop, its one function add(j, k, p or cx, sy, w, sums) adds w times the 8-bit samples
// of source row sy under the lane's columns to the lane's sums - by 16-byte loads where the columns lie inside the row, sample by sample, every sample checked against
// the width, where they reach past its end.  (The policy multiplies and adds itself: handed back to be weighted here, the samples make a different program.  What a
// policy copies from a job that is read where it lies - the Y'CbCr form - it copies in its constructor: read in add, the compiler has to read it again in the row's tail,
// no longer knows the container width the dispatch tested, and k_yuv_ladder grows by 14 KB.)
// scale_columns16: a lane takes ONE output row and span p of the tile's `streams` x `spans` spans of 16 source columns, walks the row's source rows (at most nine) and
// keeps the sixteen weighted column sums in 32-bit registers; they go to LDS, a span in SCALE_SPAN_WORDS words.  k_downscale's tiles and the ladders' luma tiles.
template <class P, class Job>
__device__ __forceinline__ void scale_columns16(const Job &j, const ScaleTile &k, u32x4 *sums4, int row_words)
{
	const ScaleAxis ay = j.ay;
	const P row(j);
	const int total = k.total();
	for (int i = (int)threadIdx.x; i < total * k.ny; i += HMR_BLOCK) {
		const int r = i / total, p = i - r * total;
		const uint32_t y = (uint32_t)(k.y0 + r), hi = (y + 1) * ay.s;
		uint32_t acc[16] = {};
		for (uint32_t sy = hmr_scale_first(ay, y); sy * ay.d < hi; sy++) row.add(j, k, p, sy, hmr_scale_weight(ay, y, sy), acc);
		u32x4 *o = &sums4[(r * row_words + p * SCALE_SPAN_WORDS) >> 2];
#pragma unroll
		for (int m = 0; m < 4; m++) o[m] = u32x4{acc[4 * m], acc[4 * m + 1], acc[4 * m + 2], acc[4 * m + 3]};
	}
}
// scale_columns8x2, the ladders' chroma tiles: a lane takes ONE chroma output row and a span of EIGHT columns of the converted 4:2:0 chroma planes (k.row_bytes wide) and accumulates U and V apart; its
// sixteen sums are half a span of the U stream and half a span of the V stream (two 16-byte LDS stores each: eight lanes of such a store hit six different quads of
// banks, two of them twice).  Sixteen chroma columns a lane would hold 32 sums beside the source rows under them: eight keeps every form free of spills.
template <class P, class Job>
__device__ __forceinline__ void scale_columns8x2(const Job &j, const ScaleTile &k, u32x4 *sums4, int row_words)
{
	const ScaleAxis ay = j.ay;
	const P row(j);
	const int halves = 2 * k.spans;
	for (int i = (int)threadIdx.x; i < halves * k.ny; i += HMR_BLOCK) {
		const int r = i / halves, q = i - r * halves, cx = k.c0 + (q << 3);
		if (cx >= k.row_bytes) continue;      // (the second half of the last span may lie beyond the plane: no tap reads its sums)
		const uint32_t y = (uint32_t)(k.y0 + r), hi = (y + 1) * ay.s;
		uint32_t au[8] = {}, av[8] = {};
		for (uint32_t sy = hmr_scale_first(ay, y); sy * ay.d < hi; sy++) row.add(j, k, cx, sy, hmr_scale_weight(ay, y, sy), au, av);
		u32x4 *o = &sums4[(r * row_words + scale_word(q << 3)) >> 2];
		o[0] = u32x4{au[0], au[1], au[2], au[3]}; o[1] = u32x4{au[4], au[5], au[6], au[7]};
		o += (k.spans * SCALE_SPAN_WORDS) >> 2;      // (the V stream lies behind the U stream)
		o[0] = u32x4{av[0], av[1], av[2], av[3]}; o[1] = u32x4{av[4], av[5], av[6], av[7]};
	}
}

// k_downscale's source row (scale_columns16): the sixteen bytes of span p of the tile's window themselves; I420 chroma: the V plane's spans behind the U plane's
struct ScaleBytes {
	__device__ __forceinline__ ScaleBytes(const ScaleJob &) {}
	__device__ __forceinline__ void add(const ScaleJob &j, const ScaleTile &k, int p, uint32_t sy, uint32_t w, uint32_t *acc) const
	{
		const bool second = p >= k.spans;
		const int b = k.b0 + ((second ? p - k.spans : p) << 4);
		const bytes_in row = (bytes_in)(k.luma ? j.src[0] : second ? j.src[2] : j.src[1]) + (int64_t)sy * (k.luma ? j.pitch[0] : second ? j.pitch[2] : j.pitch[1]) + b;
		if (b + 16 <= k.row_bytes) {
			const u32x4 v4 = load16(row);
			const uint32_t d[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
			for (int m = 0; m < 16; m++) acc[m] += w * ((d[m >> 2] >> (8 * (m & 3))) & 255u);
		} else {
#pragma unroll
			for (int m = 0; m < 16; m++) acc[m] += b + m < k.row_bytes ? w * row[m] : 0u;      // (the row's last bytes: sample by sample)
		}
	}
};

__global__ __launch_bounds__(HMR_BLOCK) void k_downscale(const ScaleJob *jobs)
{
	__shared__ u32x4 sums4[SCALE_LDS_WORDS / 4];
	__shared__ u32x4 outs4[SCALE_MAX_ROWS * SCALE_TILE_W / 8];
	// (read where it lies, as the ladders': of a copy, ScaleBytes' choice of a plane by the lane's stream goes through private memory)
	const ScaleJob &j = jobs[blockIdx.y];
	const ScaleTile k = scale_tile(j, (int)blockIdx.x, j.format == HMR_GPU_PIC_NV12);
	if (k.empty) return;
	const int row_words = k.total() * SCALE_SPAN_WORDS;
	scale_columns16<ScaleBytes>(j, k, sums4, row_words);
	__syncthreads();
	scale_finish(k, j.ax, j.den, j.mden, (const uint32_t *)sums4, outs4, row_words, j.dst[0], j.dst[1], j.dst[2], j.stride_y, j.stride_c);
}
template <> struct PictureKernel<ScaleJob> { static constexpr auto kernel = k_downscale; static int chunks(const ScaleJob &j) { return scale_tiles(j); } };

// ---- downscaling RGB ingest (section 12j) ----
// k_rgb_ladder: RGB pictures of one size, in any of k_ingest_rgb's forms, into the int16 planes of a smaller - or equal - size: every slot sample is section 12g's
// area average of the 8-bit 4:2:0 picture section 12f makes of the source, and that picture never exists in memory.  12f's luma is a function of one pixel and its
// chroma of one 2 x 2 block, so a lane converts what it has loaded in registers with k_ingest_rgb's own pieces (rgb_load_row, rgb_pixel, rgb_two_rows, rgb_quad; the
// rows' tails by rgb_sample3) and accumulates the weighted 8-bit results: the column sums are k_downscale's, bit for bit, and so are the tiles, the vertical pass, the
// LDS layout, the horizontal pass and the stores (scale_tile, scale_columns16 / scale_columns8x2, scale_finish).  What the kernel adds are the two row policies below.
// Per source row a luma lane issues the loads of k_ingest_rgb's form (binary32: two halves of eight pixels) and sixteen multiply-adds; a chroma lane's eight columns are
// sixteen pixels of two pixel rows: the loads of a luma lane twice.
// Luma and chroma tiles each read the RGB source: 2 x (3, 4, 3, 6 or 12) Ws Hs bytes read, 3 Wd Hd written per picture.  No lane
// reads a byte outside [plane + y * pitch, plane + y * pitch + row bytes) or writes outside dst_w x dst_h.  The weighted sums fit 32 bits as section 12g's do: the
// converted samples are 8-bit.  LDS: k_downscale's.
// a luma tile's source row (scale_columns16): the luma of the 16 pixels at (x, sy)
template <int V> struct RgbLadderLuma {
	const int sh[3];
	__device__ __forceinline__ RgbLadderLuma(const RgbScaleJob &j) : sh{8 * j.offset[0], 8 * j.offset[1], 8 * j.offset[2]} {}
	__device__ __forceinline__ void add(const RgbScaleJob &j, const ScaleTile &k, int p, uint32_t sy, uint32_t w, uint32_t *acc) const
	{
		const int x = k.c0 + (p << 4);
		typedef RgbForm<V> F;
		if (x + 16 <= j.src_w) {
#pragma unroll
			for (int h = 0; h < 16 / F::PX; h++) {
				uint32_t raw[F::WORDS];
				rgb_load_row<V>(j, x + F::PX * h, (int)sy, raw);
#pragma unroll
				for (int m = 0; m < F::PX; m++) {
					int cr, cg, cb;
					rgb_pixel<V>(raw, m, sh, cr, cg, cb);
					acc[F::PX * h + m] += w * (uint32_t)hmr_rgb_luma(j.m, cr, cg, cb);
				}
			}
			return;
		}
#pragma unroll
		for (int m = 0; m < 16; m++) {      // (the row's last pixels)
			if (x + m >= j.src_w) continue;
			int c3[3];
			rgb_sample3<F::FMT>(j, x + m, (int)sy, c3);
			acc[m] += w * (uint32_t)hmr_rgb_luma(j.m, c3[0], c3[1], c3[2]);
		}
	}
};
// a chroma tile's source row (scale_columns8x2): U and V of the eight 2 x 2 blocks at chroma (cx, sy) - sixteen pixels of two pixel rows, the loads of a luma lane twice
template <int V> struct RgbLadderChroma {
	const int sh[3];
	__device__ __forceinline__ RgbLadderChroma(const RgbScaleJob &j) : sh{8 * j.offset[0], 8 * j.offset[1], 8 * j.offset[2]} {}
	__device__ __forceinline__ void add(const RgbScaleJob &j, const ScaleTile &k, int cx, uint32_t sy, uint32_t w, uint32_t *au, uint32_t *av) const
	{
		const int py = 2 * (int)sy, cw = k.row_bytes;      // (the source's chroma width)
		if (cx + 8 <= cw) {
			rgb_two_rows<V>(j, 2 * cx, py, [&](int h, const uint32_t *a, const uint32_t *b, int i0) {
#pragma unroll
				for (int p = 0; p < 4; p++) {
					int px[4][3], s[3];
					rgb_quad<V>(a, b, i0 + 2 * p, sh, px, s);
					au[4 * h + p] += w * (uint32_t)hmr_rgb_chroma(j.m.u, s[0], s[1], s[2]);
					av[4 * h + p] += w * (uint32_t)hmr_rgb_chroma(j.m.v, s[0], s[1], s[2]);
				}
			});
			return;
		}
#pragma unroll
		for (int m = 0; m < 8; m++) {      // (the row's last blocks)
			if (cx + m >= cw) continue;
			int s[3] = {0, 0, 0};
#pragma unroll
			for (int c = 0; c < 4; c++) {
				int c3[3];
				rgb_sample3<RgbForm<V>::FMT>(j, 2 * (cx + m) + (c & 1), py + (c >> 1), c3);
				s[0] += c3[0]; s[1] += c3[1]; s[2] += c3[2];
			}
			au[m] += w * (uint32_t)hmr_rgb_chroma(j.m.u, s[0], s[1], s[2]);
			av[m] += w * (uint32_t)hmr_rgb_chroma(j.m.v, s[0], s[1], s[2]);
		}
	}
};

__global__ __launch_bounds__(HMR_BLOCK) void k_rgb_ladder(const RgbScaleJob *jobs)
{
	__shared__ u32x4 sums4[SCALE_LDS_WORDS / 4];
	__shared__ u32x4 outs4[SCALE_MAX_ROWS * SCALE_TILE_W / 8];
	const RgbScaleJob &j = jobs[blockIdx.y];      // (read where it lies: a copy of its 192 bytes in scalar registers leaves too few for the five forms)
	const ScaleTile k = scale_tile(j, (int)blockIdx.x, false);
	if (k.empty) return;
	const int row_words = k.total() * SCALE_SPAN_WORDS;
	rgb_dispatch(j, [&](auto form) {
		constexpr int V = decltype(form)::value;
		if (k.luma) scale_columns16<RgbLadderLuma<V>>(j, k, sums4, row_words);
		else scale_columns8x2<RgbLadderChroma<V>>(j, k, sums4, row_words);
	});
	__syncthreads();
	scale_finish(k, j.ax, j.den, j.mden, (const uint32_t *)sums4, outs4, row_words, j.dst[0], j.dst[1], j.dst[2], j.stride_y, j.stride_c);
}
template <> struct PictureKernel<RgbScaleJob> { static constexpr auto kernel = k_rgb_ladder; static int chunks(const RgbScaleJob &j) { return scale_tiles(j); } };

// ---- downscaling deep / 4:2:2 / 4:4:4 ingest (section 12l) ----
// k_yuv_ladder: Y'CbCr pictures of one size, in any of k_ingest_yuv's forms, into the int16 planes of a smaller - or equal - size: every slot sample is section 12g's
// area average of the 8-bit 4:2:0 picture section 12k makes of the source, and that picture never exists in memory.  12k's luma is a function of one container and its
// chroma of 1, 2 or 4 containers of one plane, so a lane rounds what it has loaded in registers (yuv_load, yuv_pick, hmr_yuv_value, hmr_yuv_round; the chroma taps by
// k_ingest_yuv's own yuv_taps_packed / yuv_taps_planes) and accumulates the weighted 8-bit results: the column sums are k_downscale's, bit for bit, and so are the tiles,
// the vertical pass, the LDS layout, the horizontal pass and the stores (scale_tile with a chroma tile's columns those of the converted 4:2:0 chroma planes,
// scale_columns16 / scale_columns8x2, scale_finish).  What the kernel adds are the two row policies below.
// Per source row a luma lane issues the loads k_ingest_yuv issues for the layout and the container (16 bytes for 8-bit planes, 32 for 16-bit planes or 8-bit packed, 64
// for 16-bit packed) and sixteen multiply-adds; a chroma lane reads, per converted chroma row, one (4:2:0) or two source chroma rows, 8 (4:2:0, 4:2:2) or 16 (4:4:4)
// columns of U and of V.  The rows' tails go through yuv_depth.h's own hmr_yuv_luma / hmr_yuv_chroma - the ones the host twin runs.  The policies are specialised as
// k_ingest_yuv is, through the same yuv_dispatch (14 classes, picked per job: a launch mixes forms; luma does not depend on the taps).
// Planar and semi-planar sources are read once - luma tiles read the luma plane, chroma tiles the chroma planes: sb (Ws Hs + 2 Wc Hc) bytes read, 3 Wd Hd written per
// picture; a packed source's single plane is read by both tile classes: 2 x 2 sb Ws Hs read.  No lane reads a byte outside [plane + y * pitch, plane + y * pitch +
// row bytes) or writes outside dst_w x dst_h.  The weighted sums fit 32 bits as section 12g's do: the converted samples are 8-bit.  No atomics.  LDS: k_downscale's.
// a luma tile's source row (scale_columns16): the 16 rounded samples at (x, sy); as 32-bit values for the multiply-adds, where yuv_span packs int16 pairs for its stores
template <int L, int SB> struct YuvLadderLuma {
	const YuvForm f;
	__device__ __forceinline__ YuvLadderLuma(const YuvScaleJob &j) : f(j.f) {}
	__device__ __forceinline__ void add(const YuvScaleJob &j, const ScaleTile &k, int p, uint32_t sy, uint32_t w, uint32_t *acc) const
	{
		const int x = k.c0 + (p << 4);
		typedef YuvSpan<L, SB, 0> F;
		const int bits0 = 8 * SB * f.offset[0];
		if (x + 16 <= j.src_w) {
			uint32_t la[F::LUMA_BYTES / 4];
			yuv_load<F::LUMA_BYTES>((bytes_in)j.src[0] + (int64_t)sy * j.pitch[0] + (int64_t)x * (L == YUV_PACKED ? 2 : 1) * SB, la);
#pragma unroll
			for (int m = 0; m < 16; m++) {
				const uint32_t raw = L == YUV_PACKED ? yuv_pick<SB, 2>(la, m, bits0) : yuv_pick<SB, 1>(la, m, 0);
				acc[m] += w * (SB == 1 ? raw : hmr_yuv_round(hmr_yuv_value(f, raw), f.s));      // (8 bits: the sample itself)
			}
			return;
		}
#pragma unroll
		for (int m = 0; m < 16; m++)      // (the row's last pixels: yuv_depth.h's own function - the one the host twin runs)
			if (x + m < j.src_w) acc[m] += w * hmr_yuv_luma<bytes_in>(j.src, j.pitch, f, x + m, (int)sy);
	}
};
// a chroma tile's source row (scale_columns8x2): U and V of the eight converted chroma columns at (cx, sy), the tap sums rounded with s + K exactly as yuv_span rounds them
template <int L, int SB, int K> struct YuvLadderChroma {
	const YuvForm f;
	__device__ __forceinline__ YuvLadderChroma(const YuvScaleJob &j) : f(j.f) {}
	__device__ __forceinline__ void add(const YuvScaleJob &j, const ScaleTile &k, int cx, uint32_t sy, uint32_t w, uint32_t *au, uint32_t *av) const
	{
		typedef YuvSpan<L, SB, K> F;
		const int cw = k.row_bytes;      // (the converted chroma width: src_w / 2)
		if (cx + 8 <= cw) {
			uint32_t su[8] = {}, sv[8] = {};
			if (L == YUV_PACKED) {
#pragma unroll
				for (int r = 0; r < 2; r++) {
					uint32_t g[F::LUMA_BYTES / 4];
					yuv_load<F::LUMA_BYTES>((bytes_in)j.src[0] + (int64_t)(2 * (int)sy + r) * j.pitch[0] + (int64_t)cx * 4 * SB, g);
					yuv_taps_packed<SB>(f, g, su, sv);
				}
			} else yuv_taps_planes<L, SB, K>(j, cx, (int)sy, su, sv);
			const int t = f.s + K;
#pragma unroll
			for (int c = 0; c < 8; c++) {
				au[c] += w * hmr_yuv_round(su[c], t);
				av[c] += w * hmr_yuv_round(sv[c], t);
			}
		} else {
#pragma unroll
			for (int m = 0; m < 8; m++) {      // (the row's last columns: yuv_depth.h's own function)
				if (cx + m >= cw) continue;
				au[m] += w * hmr_yuv_chroma<bytes_in>(j.src, j.pitch, f, 1, cx + m, (int)sy);
				av[m] += w * hmr_yuv_chroma<bytes_in>(j.src, j.pitch, f, 2, cx + m, (int)sy);
			}
		}
	}
};

__global__ __launch_bounds__(HMR_BLOCK) void k_yuv_ladder(const YuvScaleJob *jobs)
{
	__shared__ u32x4 sums4[SCALE_LDS_WORDS / 4];
	__shared__ u32x4 outs4[SCALE_MAX_ROWS * SCALE_TILE_W / 8];
	const YuvScaleJob &j = jobs[blockIdx.y];      // (read where it lies, as k_rgb_ladder's)
	const ScaleTile k = scale_tile(j, (int)blockIdx.x, false);
	if (k.empty) return;
	const int row_words = k.total() * SCALE_SPAN_WORDS;
	yuv_dispatch(j.f, [&](auto layout, auto container) {
		constexpr int L = decltype(layout)::value, SB = decltype(container)::value;
		if (k.luma) scale_columns16<YuvLadderLuma<L, SB>>(j, k, sums4, row_words);
		else yuv_dispatch_taps<L>(j.f, [&](auto taps) { scale_columns8x2<YuvLadderChroma<L, SB, decltype(taps)::value>>(j, k, sums4, row_words); });
	});
	__syncthreads();
	scale_finish(k, j.ax, j.den, j.mden, (const uint32_t *)sums4, outs4, row_words, j.dst[0], j.dst[1], j.dst[2], j.stride_y, j.stride_c);
}
template <> struct PictureKernel<YuvScaleJob> { static constexpr auto kernel = k_yuv_ladder; static int chunks(const YuvScaleJob &j) { return scale_tiles(j); } };

// ---- egress ----
// two dwords of two int16 samples each -> their four low bytes
__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x06040200u); }
// a dword of two U samples, a dword of two V samples -> U0 V0 U1 V1
__device__ __forceinline__ uint32_t weave4(uint32_t u, uint32_t v) { return __builtin_amdgcn_perm(v, u, 0x06020400u); }
__device__ __forceinline__ u32x4 pack16(u32x4 a, u32x4 b) { return u32x4{pack4(a.x, a.y), pack4(a.z, a.w), pack4(b.x, b.y), pack4(b.z, b.w)}; }

// squared differences of two int16 pairs
__device__ __forceinline__ uint32_t sq2(uint32_t a, uint32_t b)
{
	const int d0 = (int)(int16_t)a - (int)(int16_t)b, d1 = ((int)a >> 16) - ((int)b >> 16);
	return (uint32_t)(d0 * d0) + (uint32_t)(d1 * d1);
}
__device__ __forceinline__ uint32_t sq8(u32x4 a, u32x4 b) { return sq2(a.x, b.x) + sq2(a.y, b.y) + sq2(a.z, b.z) + sq2(a.w, b.w); }

// n <= 16 samples of a plane row: r / s 16-byte aligned (s NULL: no sum), d anywhere (NULL: no picture); returns the sum of squared differences
__device__ __forceinline__ uint32_t narrow_span(samples_in r, samples_in s, bytes_out d, int n)
{
	uint32_t acc = 0;
	if (n == 16) {
		const GLOBAL_AS u32x4 *rv = (const GLOBAL_AS u32x4 *)r;
		const u32x4 a = rv[0], b = rv[1];
		if (s) {
			const GLOBAL_AS u32x4 *sv = (const GLOBAL_AS u32x4 *)s;
			acc = sq8(sv[0], a) + sq8(sv[1], b);
		}
		if (d) store16(d, pack16(a, b));
		return acc;
	}
	for (int i = 0; i < n; i++) {      // (a row's tail)
		const int v = r[i];
		if (s) { const int e = s[i] - v; acc += (uint32_t)(e * e); }
		if (d) d[i] = (uint8_t)v;
	}
	return acc;
}
// n <= 8 samples of a U and of a V row into n pairs of an NV12 chroma row; the sums of both planes
__device__ __forceinline__ void weave_span(samples_in ru, samples_in rv, samples_in su, samples_in sv, bytes_out d, int n, uint32_t &acc_u, uint32_t &acc_v)
{
	if (n == 8) {
		const u32x4 u = *(const GLOBAL_AS u32x4 *)ru, v = *(const GLOBAL_AS u32x4 *)rv;
		if (su) {
			acc_u += sq8(*(const GLOBAL_AS u32x4 *)su, u);
			acc_v += sq8(*(const GLOBAL_AS u32x4 *)sv, v);
		}
		if (d) store16(d, u32x4{weave4(u.x, v.x), weave4(u.y, v.y), weave4(u.z, v.z), weave4(u.w, v.w)});
		return;
	}
	for (int i = 0; i < n; i++) {
		const int u = ru[i], v = rv[i];
		if (su) { const int eu = su[i] - u, ev = sv[i] - v; acc_u += (uint32_t)(eu * eu); acc_v += (uint32_t)(ev * ev); }
		if (d) { d[2 * i] = (uint8_t)u; d[2 * i + 1] = (uint8_t)v; }
	}
}

// the workgroup's sum of `acc` to sum[0] and, when `two`, of `acc2` to sum[1]; every lane of the workgroup comes here
__device__ __forceinline__ void add_sums(GLOBAL_AS uint64_t *sum, uint32_t acc, uint32_t acc2, bool two)
{
	__shared__ uint32_t part[2][HMR_WAVES_PER_BLOCK];
	const uint32_t w0 = wave_sum(acc), w1 = two ? wave_sum(acc2) : 0u;
	if (lane_id() == 0) { part[0][wave_in_block()] = w0; part[1][wave_in_block()] = w1; }
	__syncthreads();
	if (threadIdx.x < (two ? 2u : 1u)) {
		uint64_t total = 0;
		for (int k = 0; k < HMR_WAVES_PER_BLOCK; k++) total += part[threadIdx.x][k];
		if (total) __hip_atomic_fetch_add(sum + threadIdx.x, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

__global__ __launch_bounds__(HMR_BLOCK) void k_egress(const EgressJob *jobs)
{
	const EgressJob j = jobs[blockIdx.y];
	const int W = j.width, cw = W >> 1, t = (int)threadIdx.x;
	const Chunk k{(int)blockIdx.x, W, j.height};
	const bool luma = k.luma(), sums = j.src[0] != nullptr, picture = j.dst[0] != nullptr;
	GLOBAL_AS uint64_t *ssd = (GLOBAL_AS uint64_t *)j.ssd;
	if (luma) {
		const Rows rw = k.rows();
		const int y0 = rw.y0, rows = rw.n, per_row = k.luma_spans();
		const samples_in rec = (samples_in)j.rec[0], src = (samples_in)j.src[0];
		const bytes_out dst = (bytes_out)j.dst[0];
		const int64_t pitch = j.pitch[0];
		uint32_t acc = 0;
		for (int i = t; i < rows * per_row; i += HMR_BLOCK) {
			const int r = i / per_row, x = (i - r * per_row) << 4, y = y0 + r;
			acc += narrow_span(rec + (size_t)y * j.stride_y + x, sums ? src + (size_t)y * j.src_stride_y + x : nullptr, picture ? dst + (int64_t)y * pitch + x : nullptr,
					   W - x < 16 ? W - x : 16);
		}
		if (sums) add_sums(ssd, acc, 0, false);
		return;
	}
	if (k.empty()) return;
	const Rows rw = k.rows();
	const int y0 = rw.y0, rows = rw.n;
	const samples_in ru = (samples_in)j.rec[1], rv = (samples_in)j.rec[2], su = (samples_in)j.src[1], sv = (samples_in)j.src[2];
	uint32_t acc_u = 0, acc_v = 0;
	if (j.format == HMR_GPU_PIC_NV12 && picture) {      // (sums alone: plane by plane)
		const int per_row = k.pair_spans();
		const bytes_out dst = (bytes_out)j.dst[1];
		const int64_t pitch = j.pitch[1];
		for (int i = t; i < rows * per_row; i += HMR_BLOCK) {
			const int r = i / per_row, x = (i - r * per_row) << 3, y = y0 + r;
			const size_t o = (size_t)y * j.stride_c + x, so = (size_t)y * j.src_stride_c + x;
			weave_span(ru + o, rv + o, sums ? su + so : nullptr, sums ? sv + so : nullptr, dst + (int64_t)y * pitch + 2 * x, cw - x < 8 ? cw - x : 8, acc_u, acc_v);
		}
	} else {
		const int per_plane = k.plane_spans(), per_row = 2 * per_plane;      // (a row's U part, then its V part)
		const bytes_out du = (bytes_out)j.dst[1], dv = (bytes_out)j.dst[2];
		const int64_t pu = j.pitch[1], pv = j.pitch[2];
		for (int i = t; i < rows * per_row; i += HMR_BLOCK) {
			const int r = i / per_row, g = i - r * per_row, y = y0 + r;
			const bool is_v = g >= per_plane;
			const int x = (is_v ? g - per_plane : g) << 4;
			const uint32_t a = narrow_span((is_v ? rv : ru) + (size_t)y * j.stride_c + x, sums ? (is_v ? sv : su) + (size_t)y * j.src_stride_c + x : nullptr,
						       picture ? (is_v ? dv : du) + (int64_t)y * (is_v ? pv : pu) + x : nullptr, cw - x < 16 ? cw - x : 16);
			if (is_v) acc_v += a; else acc_u += a;
		}
	}
	if (sums) add_sums(ssd + 1, acc_u, acc_v, true);
}
template <> struct PictureKernel<EgressJob> { static constexpr auto kernel = k_egress; static int chunks(const EgressJob &j) { return Chunk{0, j.width, j.height}.chunks(); } };

// ---- RGB egress (section 12i) ----
// k_egress_rgb: int16 planes - a final picture (with margins) or a picture slot (without: every chroma index is clamped here) - into RGB pictures in any of the ingest's
// forms by the integer arithmetic of yuv_rgb.h, and / or the exact sums of squared differences between the 8-bit R, G, B values and a reference RGB picture in any form.
// 3 W H bytes read, the reference's 3, 4, 3, 6 or 12 W H read, 3, 4, 3, 6 or 12 W H written per picture.
// blockIdx.y = picture, blockIdx.x = a chunk of RGB_PAIRS row pairs; pair p is the luma rows 2 p - 1 and 2 p, which both take their chroma from rows p - 1 and p (the
// pairs 0 and H / 2 have one row, and one chroma row twice: the clamp): H / 2 + 1 pairs, at most CHUNK_ROWS luma rows a chunk.  A lane takes a span of 16 pixels of a
// pair: one aligned 16-byte load of eight samples per chroma row and plane plus the two neighbour columns (clamped; they are another lane's span: served from cache),
// weighted vertically two samples to a dword (3 a + b <= 1020: the halves do not carry), then per luma row two 16-byte loads, the sixteen pixels' arithmetic, the
// channels packed four pixels to a dword, and 16-byte stores at whatever address the pitch gives: one per plane (planar 8-bit), two / four per plane (binary16 /
// binary32), three / four (3- / 4-byte pixels, the bytes placed by the job's offsets, the fourth byte 255).  The reference's row is read by the ingest's loaders
// (rgb_load_row, rgb_pixel).  A row's tail of fewer than 16 pixels goes sample by sample, a lane per pixel.  No lane writes a byte outside
// [plane + y * pitch, plane + y * pitch + row bytes).  Sums: a lane's three 32-bit accumulators through add_sums; a chunk holds at most CHUNK_ROWS x EGRESS_MAX_WIDTH
// pixels, each difference at most 255: the bound at the top of the file.
constexpr int RGB_PAIRS = CHUNK_ROWS / 2;
__host__ __device__ __forceinline__ int rgb_egress_chunks(int height) { return ((height >> 1) + 1 + RGB_PAIRS - 1) / RGB_PAIRS; }

__device__ __forceinline__ uint32_t byte_of(const uint32_t *p, int i) { return (p[i >> 2] >> (8 * (i & 3))) & 255u; }

// sixteen pixels of a luma row: ya, yb its int16 samples, two to a dword; cu, cv the vertically weighted chroma of columns x / 2 - 1 .. x / 2 + 8; the channels come
// back as bytes, four pixels to a dword
__device__ __forceinline__ void yuv_row16(const YuvMatrix &m, u32x4 ya, u32x4 yb, const int *cu, const int *cv, uint32_t *pr, uint32_t *pg, uint32_t *pb)
{
	const uint32_t yw[8] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
#pragma unroll
	for (int d = 0; d < 4; d++) {
		uint32_t r4 = 0, g4 = 0, b4 = 0;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const int i = 4 * d + k, c = i >> 1;
			const int y = (int)((yw[i >> 1] >> (16 * (i & 1))) & 255u);
			const int u16 = (i & 1) ? 3 * cu[c + 1] + cu[c + 2] : cu[c] + 3 * cu[c + 1];
			const int v16 = (i & 1) ? 3 * cv[c + 1] + cv[c + 2] : cv[c] + 3 * cv[c + 1];
			int r, g, b;
			hmr_yuv_rgb(m, y, u16, v16, r, g, b);
			// (opaque: AMD clang 22.0.0git of ROCm 7.2.0 otherwise fuses shift, clamp and packing of two pixels into v_ashr_pk_u8_i32 and takes the upper half of its
			// result for zero; on the MI355X the bytes of the two other pixels, or-ed in above it, then came out with stray bits.  Masking r, g, b with 255 does not
			// help: the compiler knows them to be inside 0 .. 255 and drops the mask.  tests/test_gpu_rgb_egress.py's equality tests hold this.)
			asm("" : "+v"(r), "+v"(g), "+v"(b));
			r4 |= (uint32_t)r << (8 * k); g4 |= (uint32_t)g << (8 * k); b4 |= (uint32_t)b << (8 * k);
		}
		// (opaque to the optimiser: it would otherwise see through the packing and keep the 48 values themselves alive until the row's stores, instead of 12 dwords)
		asm volatile("" : "+v"(r4), "+v"(g4), "+v"(b4));
		pr[d] = r4; pg[d] = g4; pb[d] = b4;
	}
}

// Sixteen pixels at (x, y) of the reference picture, read in form V, quantised to 8 bits (rgb_yuv.h) and packed like the converted row: four pixels of a channel to a
// dword.  The packed forms through the ingest's loaders (the three channels lie in the same bytes); the planar forms plane by plane.
template <int V>
__device__ __forceinline__ void rgb_ref_row(const RgbEgressJob &j, int x, int y, uint32_t *qr, uint32_t *qg, uint32_t *qb)
{
	if (V == RGB_PACKED3 || V == RGB_PACKED4) {
		typedef RgbForm<V> F;
		const int sh[3] = {8 * j.src_offset[0], 8 * j.src_offset[1], 8 * j.src_offset[2]};
		uint32_t raw[F::WORDS];
		rgb_load_row<V>(j, x, y, raw);
#pragma unroll
		for (int d = 0; d < 4; d++) {
			uint32_t r4 = 0, g4 = 0, b4 = 0;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				int r, g, b;
				rgb_pixel<V>(raw, 4 * d + k, sh, r, g, b);
				r4 |= (uint32_t)r << (8 * k); g4 |= (uint32_t)g << (8 * k); b4 |= (uint32_t)b << (8 * k);
			}
			qr[d] = r4; qg[d] = g4; qb[d] = b4;
		}
		return;
	}
	constexpr int elem = V == RGB_PLANAR8 ? 1 : V == RGB_F16 ? 2 : 4;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		uint32_t *q = c == 0 ? qr : c == 1 ? qg : qb;
		const bytes_in s = (bytes_in)j.src[c] + (int64_t)y * j.pitch[c] + (int64_t)x * elem;
#pragma unroll
		for (int k = 0; k < elem; k++) {      // sixteen bytes of the plane: 16 / elem samples
			const u32x4 v = load16(s + 16 * k);
			const uint32_t w[4] = {v.x, v.y, v.z, v.w};
			if (V == RGB_PLANAR8) { q[0] = w[0]; q[1] = w[1]; q[2] = w[2]; q[3] = w[3]; }
			else if (V == RGB_F16) {
#pragma unroll
				for (int d = 0; d < 2; d++) {
					const f16x2 h0 = __builtin_bit_cast(f16x2, w[2 * d]), h1 = __builtin_bit_cast(f16x2, w[2 * d + 1]);
					q[2 * k + d] = (uint32_t)hmr_rgb_quantize((float)h0.x) | (uint32_t)hmr_rgb_quantize((float)h0.y) << 8 | (uint32_t)hmr_rgb_quantize((float)h1.x) << 16 |
						       (uint32_t)hmr_rgb_quantize((float)h1.y) << 24;
				}
			} else
				q[k] = (uint32_t)hmr_rgb_quantize(__builtin_bit_cast(float, w[0])) | (uint32_t)hmr_rgb_quantize(__builtin_bit_cast(float, w[1])) << 8 |
				       (uint32_t)hmr_rgb_quantize(__builtin_bit_cast(float, w[2])) << 16 | (uint32_t)hmr_rgb_quantize(__builtin_bit_cast(float, w[3])) << 24;
		}
	}
}
// acc + the squared differences of the sixteen bytes of q and p: sum (q - p)^2 = sum q q + sum p p - 2 sum q p, each a v_dot4_u32_u8 per dword (modulo 2^32: exact,
// the result is not negative)
__device__ __forceinline__ uint32_t sq_bytes(uint32_t acc, const uint32_t *q, const uint32_t *p)
{
	uint32_t cross = 0;
#pragma unroll
	for (int d = 0; d < 4; d++) {
		acc = __builtin_amdgcn_udot4(q[d], q[d], __builtin_amdgcn_udot4(p[d], p[d], acc, false), false);
		cross = __builtin_amdgcn_udot4(q[d], p[d], cross, false);
	}
	return acc - 2u * cross;
}

// Sixteen pixels at (x, y) of the output picture, written in the form `form` (uniform over the workgroup).  The forms that share arithmetic share its code - the two
// packed forms a pixel's dword, the two float forms the division - and branch where they differ, group of four values by group: written as one case per form, the
// compiler hoists the shared arithmetic of ALL sixteen pixels in front of the branch and a lane holds 48 quotients at once.
__device__ __forceinline__ void rgb_store_row(const RgbEgressJob &j, int form, int x, int y, const uint32_t *pr, const uint32_t *pg, const uint32_t *pb)
{
	if (form == RGB_PACKED3 || form == RGB_PACKED4) {
		const bool four = form == RGB_PACKED4;
		const int s0 = 8 * j.offset[0], s1 = 8 * j.offset[1], s2 = 8 * j.offset[2];
		const uint32_t alpha = four ? 255u << (8 * rgb_alpha_offset(j.offset)) : 0u;
		const bytes_out d = (bytes_out)j.dst[0] + (int64_t)y * j.dst_pitch[0] + (int64_t)x * (four ? 4 : 3);
		uint32_t o[12];      // (3-byte pixels: four pixels in three dwords)
#pragma unroll
		for (int k = 0; k < 4; k++) {
			uint32_t w[4];
#pragma unroll
			for (int i = 0; i < 4; i++) w[i] = byte_of(pr, 4 * k + i) << s0 | byte_of(pg, 4 * k + i) << s1 | byte_of(pb, 4 * k + i) << s2 | alpha;
			if (four) store16(d + 16 * k, u32x4{w[0], w[1], w[2], w[3]});
			else {
				o[3 * k] = w[0] | w[1] << 24;
				o[3 * k + 1] = w[1] >> 8 | w[2] << 16;
				o[3 * k + 2] = w[2] >> 16 | w[3] << 8;
			}
		}
		if (!four) {
#pragma unroll
			for (int k = 0; k < 3; k++) store16(d + 16 * k, u32x4{o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]});
		}
		return;
	}
	const bool halves = form == RGB_F16;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const uint32_t *p = c == 0 ? pr : c == 1 ? pg : pb;
		const bytes_out d = (bytes_out)j.dst[c] + (int64_t)y * j.dst_pitch[c] + (int64_t)x * (form == RGB_PLANAR8 ? 1 : halves ? 2 : 4);
		if (form == RGB_PLANAR8) {
			store16(d, u32x4{p[0], p[1], p[2], p[3]});
			continue;
		}
		uint32_t h[4];
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const float f0 = hmr_rgb_unit((int)byte_of(p, 4 * k)), f1 = hmr_rgb_unit((int)byte_of(p, 4 * k + 1)), f2 = hmr_rgb_unit((int)byte_of(p, 4 * k + 2)), f3 = hmr_rgb_unit((int)byte_of(p, 4 * k + 3));
			if (!halves) {
				store16(d + 16 * k, u32x4{__builtin_bit_cast(uint32_t, f0), __builtin_bit_cast(uint32_t, f1), __builtin_bit_cast(uint32_t, f2), __builtin_bit_cast(uint32_t, f3)});
				continue;
			}
			const f16x2 a = {(_Float16)f0, (_Float16)f1}, b = {(_Float16)f2, (_Float16)f3};
			h[2 * (k & 1)] = __builtin_bit_cast(uint32_t, a); h[2 * (k & 1) + 1] = __builtin_bit_cast(uint32_t, b);
			if (k & 1) store16(d + 16 * (k >> 1), u32x4{h[0], h[1], h[2], h[3]});
		}
	}
}

__global__ __launch_bounds__(HMR_BLOCK) void k_egress_rgb(const RgbEgressJob *jobs)
{
	const RgbEgressJob j = jobs[blockIdx.y];
	const int W = j.width, H = j.height, cw = W >> 1, ch = H >> 1, t = (int)threadIdx.x;
	const int p0 = (int)blockIdx.x * RGB_PAIRS;
	if (p0 > ch) return;
	const int pairs = ch + 1 - p0 < RGB_PAIRS ? ch + 1 - p0 : RGB_PAIRS, per_row = W >> 4;      // (whole spans)
	const bool sums = j.src_format >= 0, picture = j.format >= 0;
	const int src_form = rgb_form(j.src_format, j.src_pixel_bytes), dst_form = rgb_form(j.format, j.pixel_bytes);
	const samples_in py = (samples_in)j.yuv[0], pu = (samples_in)j.yuv[1], pv = (samples_in)j.yuv[2];
	uint32_t acc_r = 0, acc_g = 0, acc_b = 0;
	for (int i = t; i < pairs * per_row; i += HMR_BLOCK) {
		const int r = i / per_row, x = (i - r * per_row) << 4, p = p0 + r, cx = x >> 1;
		const int ca = p > 0 ? p - 1 : 0, cb = p < ch ? p : ch - 1, cl = cx > 0 ? cx - 1 : 0, cr = cx + 8 < cw ? cx + 8 : cw - 1;
		const size_t oa = (size_t)ca * j.stride_c, ob = (size_t)cb * j.stride_c;
		const u32x4 ua = *(const GLOBAL_AS u32x4 *)(pu + oa + cx) & 0x00ff00ffu, ub = *(const GLOBAL_AS u32x4 *)(pu + ob + cx) & 0x00ff00ffu;
		const u32x4 va = *(const GLOBAL_AS u32x4 *)(pv + oa + cx) & 0x00ff00ffu, vb = *(const GLOBAL_AS u32x4 *)(pv + ob + cx) & 0x00ff00ffu;
		// the neighbour columns of both rows, left | right << 16: weighted like the spans
		const uint32_t una = (uint32_t)(pu[oa + cl] & 255) | (uint32_t)(pu[oa + cr] & 255) << 16, unb = (uint32_t)(pu[ob + cl] & 255) | (uint32_t)(pu[ob + cr] & 255) << 16;
		const uint32_t vna = (uint32_t)(pv[oa + cl] & 255) | (uint32_t)(pv[oa + cr] & 255) << 16, vnb = (uint32_t)(pv[ob + cl] & 255) | (uint32_t)(pv[ob + cr] & 255) << 16;
#pragma unroll 1
		for (int half = 0; half < 2; half++) {
			const int y = 2 * p - 1 + half;
			if (y < 0 || y >= H) continue;
			const uint32_t wa = half ? 1u : 3u, wb = 4u - wa;      // (row 2 p - 1 is the odd row of chroma row p - 1, row 2 p the even row of chroma row p)
			const u32x4 u2 = ua * wa + ub * wb, v2 = va * wa + vb * wb;
			const uint32_t un = una * wa + unb * wb, vn = vna * wa + vnb * wb;
			const int cu[10] = {(int)(un & 0xffffu), (int)(u2.x & 0xffffu), (int)(u2.x >> 16), (int)(u2.y & 0xffffu), (int)(u2.y >> 16), (int)(u2.z & 0xffffu), (int)(u2.z >> 16),
					    (int)(u2.w & 0xffffu), (int)(u2.w >> 16), (int)(un >> 16)};
			const int cv[10] = {(int)(vn & 0xffffu), (int)(v2.x & 0xffffu), (int)(v2.x >> 16), (int)(v2.y & 0xffffu), (int)(v2.y >> 16), (int)(v2.z & 0xffffu), (int)(v2.z >> 16),
					    (int)(v2.w & 0xffffu), (int)(v2.w >> 16), (int)(vn >> 16)};
			const GLOBAL_AS u32x4 *ly = (const GLOBAL_AS u32x4 *)(py + (size_t)y * j.stride_y + x);
			uint32_t pr[4], pg[4], pb[4];
			yuv_row16(j.m, ly[0], ly[1], cu, cv, pr, pg, pb);
			if (sums) {
				uint32_t qr[4], qg[4], qb[4];
				switch (src_form) {
				case RGB_PACKED3: rgb_ref_row<RGB_PACKED3>(j, x, y, qr, qg, qb); break;
				case RGB_PACKED4: rgb_ref_row<RGB_PACKED4>(j, x, y, qr, qg, qb); break;
				case RGB_PLANAR8: rgb_ref_row<RGB_PLANAR8>(j, x, y, qr, qg, qb); break;
				case RGB_F16: rgb_ref_row<RGB_F16>(j, x, y, qr, qg, qb); break;
				default: rgb_ref_row<RGB_F32>(j, x, y, qr, qg, qb); break;
				}
				acc_r = sq_bytes(acc_r, qr, pr); acc_g = sq_bytes(acc_g, qg, pg); acc_b = sq_bytes(acc_b, qb, pb);
			}
			if (picture) rgb_store_row(j, dst_form, x, y, pr, pg, pb);
		}
	}
	// a row's tail of fewer than 16 pixels: a lane per pixel of the chunk's rows 2 p0 - 1 .. 2 (p0 + pairs - 1)
	const int tail = W & 15, x0 = W & ~15, y0 = p0 ? 2 * p0 - 1 : 0, y1 = 2 * (p0 + pairs - 1) < H ? 2 * (p0 + pairs - 1) : H - 1;
	const bool src_packed = j.src_format == HMR_GPU_RGB_PACKED8, dst_packed = j.format == HMR_GPU_RGB_PACKED8;
	for (int i = t; i < (y1 - y0 + 1) * tail; i += HMR_BLOCK) {
		const int r = i / tail, x = x0 + i - r * tail, y = y0 + r;
		int c3[3];
		hmr_yuv_rgb(j.m, py[(size_t)y * j.stride_y + x] & 255, hmr_yuv_chroma16(pu, j.stride_c, cw, ch, x, y), hmr_yuv_chroma16(pv, j.stride_c, cw, ch, x, y), c3[0], c3[1], c3[2]);
		if (sums) {
			const int dr = c3[0] - rgb_sample<bytes_in, GLOBAL_AS const _Float16 *, GLOBAL_AS const float *>((bytes_in)j.src[0], j.pitch[0], j.src_format, j.src_pixel_bytes, j.src_offset[0], x, y);
			const int dg = c3[1] - rgb_sample<bytes_in, GLOBAL_AS const _Float16 *, GLOBAL_AS const float *>((bytes_in)j.src[src_packed ? 0 : 1], j.pitch[src_packed ? 0 : 1], j.src_format, j.src_pixel_bytes, j.src_offset[1], x, y);
			const int db = c3[2] - rgb_sample<bytes_in, GLOBAL_AS const _Float16 *, GLOBAL_AS const float *>((bytes_in)j.src[src_packed ? 0 : 2], j.pitch[src_packed ? 0 : 2], j.src_format, j.src_pixel_bytes, j.src_offset[2], x, y);
			acc_r += (uint32_t)(dr * dr); acc_g += (uint32_t)(dg * dg); acc_b += (uint32_t)(db * db);
		}
		if (picture) {
			rgb_put<bytes_out, GLOBAL_AS _Float16 *, GLOBAL_AS float *>((bytes_out)j.dst[0], j.dst_pitch[0], j.format, j.pixel_bytes, j.offset[0], x, y, c3[0]);
			rgb_put<bytes_out, GLOBAL_AS _Float16 *, GLOBAL_AS float *>((bytes_out)j.dst[dst_packed ? 0 : 1], j.dst_pitch[dst_packed ? 0 : 1], j.format, j.pixel_bytes, j.offset[1], x, y, c3[1]);
			rgb_put<bytes_out, GLOBAL_AS _Float16 *, GLOBAL_AS float *>((bytes_out)j.dst[dst_packed ? 0 : 2], j.dst_pitch[dst_packed ? 0 : 2], j.format, j.pixel_bytes, j.offset[2], x, y, c3[2]);
			if (dst_packed && j.pixel_bytes == 4) ((bytes_out)j.dst[0])[(int64_t)y * j.dst_pitch[0] + 4 * x + rgb_alpha_offset(j.offset)] = 255;
		}
	}
	if (!sums) return;
	GLOBAL_AS uint64_t *ssd = (GLOBAL_AS uint64_t *)j.ssd;
	add_sums(ssd, acc_r, acc_g, true);
	__syncthreads();      // (add_sums' partial sums are read by two lanes while the other wavefronts go on)
	add_sums(ssd + 2, acc_b, 0, false);
}
template <> struct PictureKernel<RgbEgressJob> { static constexpr auto kernel = k_egress_rgb; static int chunks(const RgbEgressJob &j) { return rgb_egress_chunks(j.height); } };

// ---- SSIM (section 12h) ----
// k_ssim: the exact sums of ssim_window.h's fixed-point SSIM values over every window of every plane, between the int16 planes of a picture slot (a) and the final
// picture's (b).  Both pictures are read, 6 W H bytes per picture; nothing is written but three 64-bit sums.  blockIdx.y = picture;
// blockIdx.x = a tile of SSIM_TW x SSIM_TH windows of one plane, row by row - the luma tiles first, then U's, then V's; smaller pictures leave their last blocks empty.
// A tile of 32 x 8 windows needs 33 x 9 blocks of 4 x 4 samples.
// Stage 1, a lane per (block row, 16-byte span): tiles start at even block columns, so a span of 8 samples is two adjacent blocks and is 16-byte aligned in both
// pictures (strides and margins are multiples of 8 elements); four 16-byte loads of each picture, the sums and products of the sample pairs by v_dot2_i32_i16, three
// words per block to LDS: s1 | s2 << 16, ss, s12.  33 blocks are 17 spans: 153 of the 256 lanes load, all eight loads of a lane are in flight at once, and the 34th
// block of a row is loaded but not used - 34 x 9 / (32 x 8) = 1.20 times the plane's bytes leave the caches, the re-read part from a tile that a neighbouring
// workgroup reads at about the same time.  The last span of a plane with an odd number of block columns reaches 4 samples beyond the row's end: inside the row's
// stride (a multiple of 8 elements), never used.  No load leaves [row, row + stride) of the plane's h rows.
// Stage 2, a lane per window, consecutive lanes consecutive columns: the four blocks' words are read from LDS at a 3-word stride between lanes - 3 is odd, so the 32
// lanes of a window row hit 32 different banks - and the window's q comes from hmr_ssim_window: a few 32-bit products and six 64-bit divisions.
// The lanes' 64-bit values are summed over the wavefront, the workgroup's four wavefronts through LDS, and one lane adds the workgroup's sum to the picture's sum of
// that plane with ONE 64-bit vector atomic (two's complement: the signed sum is exact whatever the order).
// Why 32 x 8: 256 windows are one per lane, so each stage is ONE pass without a loop and the division, the costly part, runs with every lane busy; a 32 x 16 tile
// would re-read 1.13 instead of 1.20 times the plane, but needs two passes per stage with 33 of 256 lanes busy in the second load pass, twice the registers of
// stage 2 or a loop around it, and wastes more of the last tile row (1080p: 269 window rows are 33 tiles of 8 and 5 rows, against 16 of 16 and 13).  3.7 KB of LDS and
// no loop-carried state: eight workgroups a CU, whose loads cover each other's divisions.
constexpr int SSIM_TW = 32, SSIM_TH = 8, SSIM_SPANS = (SSIM_TW + 2) / 2, SSIM_ROW_WORDS = 3 * 2 * SSIM_SPANS;
static_assert(SSIM_TW * SSIM_TH == HMR_BLOCK && SSIM_SPANS * (SSIM_TH + 1) <= HMR_BLOCK && SSIM_TW % 2 == 0, "one pass per stage, tiles start at even block columns");

// The tile of block b of a W x H picture: its plane (3: none), the plane's size in blocks, the tile's first block and its windows [0, nx) x [0, ny).
struct SsimTile {
	int plane, bw, bh, bx0, by0, nx, ny;
};
__host__ __device__ __forceinline__ int ssim_tiles_x(int w) { return ((w >> 2) - 1 + SSIM_TW - 1) / SSIM_TW; }
__host__ __device__ __forceinline__ int ssim_tiles_y(int h) { return ((h >> 2) - 1 + SSIM_TH - 1) / SSIM_TH; }
__host__ __device__ __forceinline__ int ssim_tiles(int W, int H) { return ssim_tiles_x(W) * ssim_tiles_y(H) + 2 * ssim_tiles_x(W >> 1) * ssim_tiles_y(H >> 1); }
__host__ __device__ __forceinline__ SsimTile ssim_tile(int W, int H, int b)
{
	SsimTile t;
	const int luma = ssim_tiles_x(W) * ssim_tiles_y(H), chroma = ssim_tiles_x(W >> 1) * ssim_tiles_y(H >> 1);
	t.plane = b < luma ? 0 : b < luma + chroma ? 1 : b < luma + 2 * chroma ? 2 : 3;
	if (t.plane) b -= luma + (t.plane - 1) * chroma;
	const int w = t.plane ? W >> 1 : W, h = t.plane ? H >> 1 : H, across = ssim_tiles_x(w);
	const int ty = b / across, tx = b - ty * across;
	t.bw = w >> 2; t.bh = h >> 2;
	t.bx0 = tx * SSIM_TW; t.by0 = ty * SSIM_TH;
	t.nx = t.bw - 1 - t.bx0 < SSIM_TW ? t.bw - 1 - t.bx0 : SSIM_TW;
	t.ny = t.bh - 1 - t.by0 < SSIM_TH ? t.bh - 1 - t.by0 : SSIM_TH;
	return t;
}

typedef short i16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t dot2(uint32_t a, uint32_t b, uint32_t c) { return (uint32_t)__builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2, a), __builtin_bit_cast(i16x2, b), (int)c, false); }

// The loader, the only part that knows the planes hold int16: the 8 samples at (x, y) of four rows, two to a dword (x a multiple of 8).
__device__ __forceinline__ void ssim_load(samples_in plane, int stride, int x, int y, u32x4 rows[4])
{
#pragma unroll
	for (int i = 0; i < 4; i++) rows[i] = *(const GLOBAL_AS u32x4 *)(plane + (size_t)(y + i) * stride + x);
}

__global__ __launch_bounds__(HMR_BLOCK) void k_ssim(const SsimJob *jobs)
{
	__shared__ uint32_t blocks[(SSIM_TH + 1) * SSIM_ROW_WORDS];
	__shared__ int64_t part[HMR_WAVES_PER_BLOCK];
	const SsimJob &j = jobs[blockIdx.y];      // (read where it lies: the planes are picked by a run-time index, which a copy in registers would turn into scratch)
	const SsimTile k = ssim_tile(j.width, j.height, (int)blockIdx.x);
	if (k.plane == 3) return;
	const int t = (int)threadIdx.x;

	// stage 1: the sums of two adjacent blocks per lane
	const int r = t / SSIM_SPANS, p = t - r * SSIM_SPANS;
	if (r <= k.ny && 2 * p <= k.nx) {      // (ny + 1 block rows, nx + 1 block columns)
		const int x = 4 * (k.bx0 + 2 * p), y = 4 * (k.by0 + r);
		u32x4 a[4], b[4];
		ssim_load((samples_in)j.a[k.plane], k.plane ? j.stride_a_c : j.stride_a_y, x, y, a);
		ssim_load((samples_in)j.b[k.plane], k.plane ? j.stride_b_c : j.stride_b_y, x, y, b);
		uint32_t *o = blocks + r * SSIM_ROW_WORDS + 6 * p;
#pragma unroll
		for (int h = 0; h < 2; h++) {
			uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
#pragma unroll
			for (int i = 0; i < 4; i++) {
				const uint32_t a0 = h ? a[i].z : a[i].x, a1 = h ? a[i].w : a[i].y, b0 = h ? b[i].z : b[i].x, b1 = h ? b[i].w : b[i].y;
				s1 = dot2(a0, 0x00010001u, dot2(a1, 0x00010001u, s1));
				s2 = dot2(b0, 0x00010001u, dot2(b1, 0x00010001u, s2));
				ss = dot2(a0, a0, dot2(a1, a1, dot2(b0, b0, dot2(b1, b1, ss))));
				s12 = dot2(a0, b0, dot2(a1, b1, s12));
			}
			o[3 * h] = s1 | s2 << 16; o[3 * h + 1] = ss; o[3 * h + 2] = s12;
		}
	}
	__syncthreads();

	// stage 2: a window per lane
	const int wy = t / SSIM_TW, wx = t - wy * SSIM_TW;
	int64_t q = 0;
	if (wx < k.nx && wy < k.ny) {
		const uint32_t *top = blocks + wy * SSIM_ROW_WORDS + 3 * wx, *bottom = top + SSIM_ROW_WORDS;
		const uint32_t s = top[0] + top[3] + bottom[0] + bottom[3];      // (the halves do not carry: S1, S2 <= 16320)
		q = hmr_ssim_window(s & 0xffffu, s >> 16, top[1] + top[4] + bottom[1] + bottom[4], top[2] + top[5] + bottom[2] + bottom[5]);
	}
	const int64_t w = wave_sum(q);
	if (lane_id() == 0) part[wave_in_block()] = w;
	__syncthreads();
	if (t == 0) {
		int64_t total = 0;
		for (int i = 0; i < HMR_WAVES_PER_BLOCK; i++) total += part[i];
		if (total) __hip_atomic_fetch_add((GLOBAL_AS uint64_t *)j.sum + k.plane, (uint64_t)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}
template <> struct PictureKernel<SsimJob> { static constexpr auto kernel = k_ssim; static int chunks(const SsimJob &j) { return ssim_tiles(j.width, j.height); } };

// ---- scene-cut statistics (section 12m) ----
// k_cut: cut_stats.h's values of a picture slot (cur) against the slot of the frame before (prev).  Both pictures are read as int16 planes, nothing is written but eight
// 64-bit values and 2 x 256 histogram bins a picture.  blockIdx.y = picture; blockIdx.x = first the luma tiles of CUT_TW x CUT_TH = 16 x 8 blocks of 8 x 8 samples
// (128 x 64 samples), row by row, then chunks of CHUNK_ROWS chroma rows (U and V); smaller pictures leave their last blocks empty.
// A luma tile.  Stage 1, a lane per 16-byte span of 8 samples (tiles start at multiples of 128 samples: every span is 16-byte aligned): prev's search window - the
// tile and a rim of 8 samples, 144 x 80 samples, 18 x 80 spans, and a row of zeros behind them - and cur's tile, 16 x 64 spans, go to LDS as BYTES (the slots hold 0 .. 255: v_perm_b32 packs the low
// bytes of four dwords into two).  A span outside W x H is not loaded - its bytes are 0 and no valid vector reads them.  A window row is 38 words: 36 of the window
// and two of padding that the last vector group reads and discards.  12 312 + 8 192 bytes.  2.20 times the tile's 2 x 2 x 8192 bytes of cur and prev leave the
// caches (the rim: 144 x 80 / (128 x 64) = 1.41 of prev), the re-read part from tiles that neighbouring workgroups read at about the same time.
// Stage 2, a lane per word of cur's tile (8 words a lane): SAD_Y and LUMA by v_sad_u8 against prev's word and against 0, and the two histograms by eight ds_add_u32
// on 2 x 256 counts in LDS; behind a barrier each lane adds two counts to the picture's bins with vector atomics (global_atomic_add; a zero count is skipped).
// Stage 3, a wavefront per block, the tile's blocks dealt round robin: act(b) with a sample per lane (two wave sums); then the 289 vectors as 9 x 5 = 45 TASKS, one
// per lane - two adjacent vertical offsets, dy = 2 m - 8 and 2 m - 7, and a group of four adjacent horizontal ones, dx = 4 g - 8 .. 4 g - 5.  A task reads nine
// rows of three aligned words of the window (12 bytes: the group starts at a multiple of 4 bytes; rows 1 .. 7 serve both offsets) and runs v_qsad_pk_u16_u8 - the
// unmasked sliding form: four SADs of four bytes at byte offsets 0 .. 3, accumulated in 16 bits each (a block's SAD is at most 16 320) - 2 x 16 times, against cur's
// two words of each row, which every lane holds in registers (16 words, one LDS broadcast read per block).  Per block and wavefront: 32 v_qsad_pk_u16_u8, 27 LDS
// words a lane, and 360 candidate slots for 289 vectors (the fifth group has one vector, dx = 8; the ninth pair one offset, dy = 8, its other reads the window's
// padding row); per picture W H / 64 x 32 quad-SAD wave instructions for 289 x W H candidate-sample differences.  Vectors that leave the picture or the range
// (hmr_cut_valid) are dropped when the lane takes its minimum; the wavefront's minimum comes by six ds_bpermute steps.  INTRA, INTER and NINTRA stay in registers,
// uniform over the wavefront; no private memory, no loop-carried state in memory.  (One offset a task, 85 tasks in two rounds, issues the same 32 quad SADs but
// reads 48 LDS words a lane: measured 4.82 ms against this mapping's 4.39 ms over 256 x 1080p.)
// Sums: the workgroup's four wavefronts through LDS, then ONE 64-bit vector atomic per value (global_atomic_add_x2) - five for a luma tile, two for a chroma chunk.
// A chroma chunk: a lane per span of 8 samples of U or V of both pictures, packed as above, two v_sad_u8; a row's last four samples, where the width is no multiple of 16, come
// by an 8-byte load.  No load touches a sample outside W x H of any plane.
// HIST needs the finished bins of the whole picture: k_cut_finish, a second small kernel in the same call (a workgroup per picture, a lane per histogram value),
// forms it.  Chosen over the last workgroup of the picture doing it: that needs a device-wide count of finished workgroups and release / acquire fences around it in
// every workgroup, to save a launch of a few microseconds behind a kernel of milliseconds.
// Why 16 x 8 blocks: 22.6 KB of LDS lets seven workgroups share a CU, the rim costs 1.41 reads of prev (8 x 4 blocks: 1.88; 16 x 16: 1.27 at 40 KB), and 128 blocks
// are 32 per wavefront, so the staging is a small part of a workgroup's time.  What binds: the issue of the quad SADs, not the bytes - 256 x 1080p take 4.39 ms
// (tools/cut_bench.py), in which the 2.2 x 6 W H bytes pass at 1.6 TB/s, a quarter of what HBM gives, while 32 quad SADs per block are 259 000 per SIMD, 40 cycles
// each at 2.4 GHz; nearly halving the LDS words of the search (48 to 27 a lane and block) gained 9 %.
constexpr int CUT_TW = 16, CUT_TH = 8, CUT_ROWS = 8 * CUT_TH, CUT_CUR_WORDS = 2 * CUT_TW, CUT_WIN_SPANS = CUT_TW + 3, CUT_WIN_WORDS = 2 * CUT_WIN_SPANS;
constexpr int CUT_WIN_ROWS = CUT_ROWS + 2 * HMR_CUT_RANGE + 1, CUT_GROUPS = (2 * HMR_CUT_RANGE + 1 + 3) / 4, CUT_TASKS = (2 * HMR_CUT_RANGE + 1 + 1) / 2 * CUT_GROUPS;
static_assert(HMR_CUT_RANGE == 8 && HMR_CUT_BLOCK == 8 && HMR_WAVE == 64, "a sample per lane, window rims of one span, groups that start at multiples of 4 bytes");
static_assert(2 * (CUT_TW - 1) + (CUT_GROUPS - 1) + 2 < CUT_WIN_WORDS && CUT_TASKS <= HMR_WAVE, "the last group's three words lie inside a window row; a task per lane");
static_assert((CUT_WIN_ROWS * CUT_WIN_WORDS + CUT_ROWS * CUT_CUR_WORDS + 2 * 256 + 5 * HMR_WAVES_PER_BLOCK) * 4 <= 40 * 1024, "four workgroups a CU at least");
static_assert((uint64_t)CUT_TW * CUT_TH * HMR_CUT_MAX_ACT < (1ull << 32) && (uint64_t)CHUNK_ROWS * EGRESS_MAX_WIDTH * 255 < (1ull << 32), "a workgroup's partial sums fit 32 bits");

__host__ __device__ __forceinline__ int cut_tiles_x(int W) { return ((W >> 3) + CUT_TW - 1) / CUT_TW; }
__host__ __device__ __forceinline__ int cut_tiles_y(int H) { return ((H >> 3) + CUT_TH - 1) / CUT_TH; }
__host__ __device__ __forceinline__ int cut_chroma_chunks(int H) { return ((H >> 1) + CHUNK_ROWS - 1) / CHUNK_ROWS; }
__host__ __device__ __forceinline__ int cut_chunks(int W, int H) { return cut_tiles_x(W) * cut_tiles_y(H) + cut_chroma_chunks(H); }

// the 8 samples at p (16-byte aligned) as bytes
__device__ __forceinline__ u32x2 cut_load(samples_in p)
{
	const u32x4 v = *(const GLOBAL_AS u32x4 *)p;
	return u32x2{__builtin_amdgcn_perm(v.y, v.x, 0x06040200u), __builtin_amdgcn_perm(v.w, v.z, 0x06040200u)};
}
// the 4 samples at p (8-byte aligned) as bytes: a chroma row's last half span
__device__ __forceinline__ u32x2 cut_load_half(samples_in p)
{
	const u32x2 v = *(const GLOBAL_AS u32x2 *)p;
	return u32x2{__builtin_amdgcn_perm(v.y, v.x, 0x06040200u), 0u};
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
	for (int m = HMR_WAVE / 2; m >= 1; m >>= 1) {
		const uint32_t o = (uint32_t)__shfl_xor((int)v, m, HMR_WAVE);
		v = o < v ? o : v;
	}
	return v;
}
// the workgroup's sums of `count` values (each lane of a wavefront holds its wavefront's) added to stats[index[k]]: one 64-bit atomic per value
template <int COUNT>
__device__ __forceinline__ void cut_add(uint32_t (*part)[5], const uint32_t (&v)[COUNT], const int (&index)[COUNT], int64_t *stats)
{
	if (lane_id() == 0)
#pragma unroll
		for (int k = 0; k < COUNT; k++) part[wave_in_block()][k] = v[k];
	__syncthreads();
	const int t = (int)threadIdx.x;
	if (t < COUNT) {
		uint64_t total = 0;
		for (int i = 0; i < HMR_WAVES_PER_BLOCK; i++) total += part[i][t];
		int at = index[0];
#pragma unroll
		for (int k = 1; k < COUNT; k++) at = t == k ? index[k] : at;
		if (total) __hip_atomic_fetch_add((GLOBAL_AS uint64_t *)stats + at, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

__global__ __launch_bounds__(HMR_BLOCK) void k_cut(const CutJob *jobs)
{
	__shared__ u32x2 win2[CUT_WIN_ROWS * CUT_WIN_SPANS];
	__shared__ u32x2 cur2[CUT_ROWS * CUT_TW];
	__shared__ uint32_t hist[2 * 256];
	__shared__ uint32_t part[HMR_WAVES_PER_BLOCK][5];
	const CutJob &j = jobs[blockIdx.y];
	const int W = j.width, H = j.height, t = (int)threadIdx.x;
	const int across = cut_tiles_x(W), luma_tiles = across * cut_tiles_y(H);
	if ((int)blockIdx.x >= luma_tiles) {
		// a chunk of chroma rows: SAD_U, SAD_V
		const int y0 = ((int)blockIdx.x - luma_tiles) * CHUNK_ROWS, ch = H >> 1, cw = W >> 1;
		if (y0 >= ch) return;
		const int rows = ch - y0 < CHUNK_ROWS ? ch - y0 : CHUNK_ROWS, spans = (cw + 7) >> 3, stride = j.stride_c;
		uint32_t sad[2] = {0, 0};
		for (int i = t; i < 2 * rows * spans; i += HMR_BLOCK) {
			const int plane = i / (rows * spans), k = i - plane * rows * spans, r = k / spans, x = (k - r * spans) << 3;
			const size_t at = (size_t)(y0 + r) * stride + x;
			const bool half = x + 8 > cw;      // (a row's last four samples)
			const u32x2 a = half ? cut_load_half((samples_in)j.cur[1 + plane] + at) : cut_load((samples_in)j.cur[1 + plane] + at);
			const u32x2 b = half ? cut_load_half((samples_in)j.prev[1 + plane] + at) : cut_load((samples_in)j.prev[1 + plane] + at);
			const uint32_t d = __builtin_amdgcn_sad_u8(a.x, b.x, __builtin_amdgcn_sad_u8(a.y, b.y, 0u));
			sad[0] += plane ? 0u : d;
			sad[1] += plane ? d : 0u;
		}
		const uint32_t sums[2] = {wave_sum(sad[0]), wave_sum(sad[1])};
		const int index[2] = {HMR_CUT_SAD_U, HMR_CUT_SAD_V};
		cut_add(part, sums, index, j.stats);
		return;
	}
	uint32_t *win = (uint32_t *)win2, *cur = (uint32_t *)cur2;
	const int ty = (int)blockIdx.x / across, tx = (int)blockIdx.x - ty * across, x0 = tx * (8 * CUT_TW), y0 = ty * CUT_ROWS, stride = j.stride_y;
	const int nbx = (W - x0) >> 3 < CUT_TW ? (W - x0) >> 3 : CUT_TW, nby = (H - y0) >> 3 < CUT_TH ? (H - y0) >> 3 : CUT_TH;      // the tile's blocks

	// stage 1: prev's window and cur's tile as bytes
	hist[t] = 0; hist[t + 256] = 0;
	for (int i = t; i < CUT_WIN_ROWS * CUT_WIN_SPANS; i += HMR_BLOCK) {
		const int r = i / CUT_WIN_SPANS, p = i - r * CUT_WIN_SPANS, x = x0 - HMR_CUT_RANGE + 8 * p, y = y0 - HMR_CUT_RANGE + r;
		u32x2 v = {0u, 0u};
		if (p < CUT_TW + 2 && r < CUT_WIN_ROWS - 1 && x >= 0 && x < W && y >= 0 && y < H) v = cut_load((samples_in)j.prev[0] + (size_t)y * stride + x);
		win2[i] = v;
	}
	for (int i = t; i < CUT_ROWS * CUT_TW; i += HMR_BLOCK) {
		const int r = i / CUT_TW, p = i - r * CUT_TW, x = x0 + 8 * p, y = y0 + r;
		u32x2 v = {0u, 0u};
		if (x < W && y < H) v = cut_load((samples_in)j.cur[0] + (size_t)y * stride + x);
		cur2[i] = v;
	}
	__syncthreads();

	// stage 2: SAD_Y, LUMA and the histograms of the tile's samples, a word per lane and pass
	uint32_t sad = 0, luma = 0;
	for (int i = t; i < CUT_ROWS * CUT_CUR_WORDS; i += HMR_BLOCK) {
		const int r = i / CUT_CUR_WORDS, q = i - r * CUT_CUR_WORDS;
		if (q >= 2 * nbx || r >= 8 * nby) continue;
		const uint32_t c = cur[i], p = win[(r + HMR_CUT_RANGE) * CUT_WIN_WORDS + 2 + q];
		sad = __builtin_amdgcn_sad_u8(c, p, sad);
		luma = __builtin_amdgcn_sad_u8(c, 0u, luma);
#pragma unroll
		for (int k = 0; k < 4; k++) {
			__hip_atomic_fetch_add(&hist[(c >> (8 * k)) & 255u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			__hip_atomic_fetch_add(&hist[256 + ((p >> (8 * k)) & 255u)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		}
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < 2; k++)
		if (const uint32_t n = hist[t + 256 * k]) __hip_atomic_fetch_add((GLOBAL_AS uint32_t *)j.bins + t + 256 * k, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

	// stage 3: a block per wavefront
	const int l = lane_id();
	const uint8_t *cur8 = (const uint8_t *)cur;
	uint32_t intra = 0, inter = 0, nintra = 0;
	for (int k = wave_in_block(); k < nbx * nby; k += HMR_WAVES_PER_BLOCK) {
		const int by = k / nbx, bx = k - by * nbx;
		const uint32_t x = cur8[(8 * by + (l >> 3)) * (4 * CUT_CUR_WORDS) + 8 * bx + (l & 7)];
		const uint32_t S = wave_sum(x), act = wave_sum(hmr_cut_deviation(x, S));
		uint32_t c[16];
#pragma unroll
		for (int r = 0; r < 8; r++) {
			const u32x2 v = cur2[(8 * by + r) * CUT_TW + bx];
			c[2 * r] = v.x; c[2 * r + 1] = v.y;
		}
		uint32_t best = ~0u;
		if (l < CUT_TASKS) {
			const int m = l / CUT_GROUPS, g = l - m * CUT_GROUPS;      // dy = 2 m - 8 and 2 m - 7, dx = 4 g - 8 + i
			const uint32_t *p = win + (8 * by + 2 * m) * CUT_WIN_WORDS + 2 * bx + g;
			uint32_t w[9][3];
#pragma unroll
			for (int r = 0; r < 9; r++) {
				w[r][0] = p[r * CUT_WIN_WORDS]; w[r][1] = p[r * CUT_WIN_WORDS + 1]; w[r][2] = p[r * CUT_WIN_WORDS + 2];
			}
			uint64_t acc[2] = {0, 0};
#pragma unroll
			for (int r = 0; r < 8; r++)
#pragma unroll
				for (int k = 0; k < 2; k++) {
					acc[k] = __builtin_amdgcn_qsad_pk_u16_u8((uint64_t)w[r + k][1] << 32 | w[r + k][0], c[2 * r], acc[k]);
					acc[k] = __builtin_amdgcn_qsad_pk_u16_u8((uint64_t)w[r + k][2] << 32 | w[r + k][1], c[2 * r + 1], acc[k]);
				}
#pragma unroll
			for (int k = 0; k < 2; k++)
#pragma unroll
				for (int i = 0; i < 4; i++) {
					const uint32_t s = (uint32_t)(acc[k] >> (16 * i)) & 0xffffu;
					if (hmr_cut_valid(x0 + 8 * bx, y0 + 8 * by, 4 * g - HMR_CUT_RANGE + i, 2 * m + k - HMR_CUT_RANGE, W, H)) best = s < best ? s : best;
				}
		}
		const CutBlock b = hmr_cut_block(act, wave_min(best));
		intra += b.intra; inter += b.inter; nintra += b.nintra;
	}
	const uint32_t sums[5] = {wave_sum(sad), intra, inter, nintra, wave_sum(luma)};
	const int index[5] = {HMR_CUT_SAD_Y, HMR_CUT_INTRA, HMR_CUT_INTER, HMR_CUT_NINTRA, HMR_CUT_LUMA};
	cut_add(part, sums, index, j.stats);
}
template <> struct PictureKernel<CutJob> { static constexpr auto kernel = k_cut; static int chunks(const CutJob &j) { return cut_chunks(j.width, j.height); } };

// HIST of picture blockIdx.x from its finished bins, a histogram value per lane: the only writer of that value
__global__ __launch_bounds__(HMR_BLOCK) void k_cut_finish(const CutJob *jobs)
{
	__shared__ uint32_t part[HMR_WAVES_PER_BLOCK];
	const CutJob &j = jobs[blockIdx.x];
	const int t = (int)threadIdx.x;
	const uint32_t hc = ((GLOBAL_AS const uint32_t *)j.bins)[t], hp = ((GLOBAL_AS const uint32_t *)j.bins)[256 + t];
	const uint32_t w = wave_sum(hc < hp ? hp - hc : hc - hp);      // (at most 2 W H < 2^32)
	if (lane_id() == 0) part[wave_in_block()] = w;
	__syncthreads();
	if (t == 0) {
		int64_t total = 0;
		for (int i = 0; i < HMR_WAVES_PER_BLOCK; i++) total += part[i];
		((GLOBAL_AS int64_t *)j.stats)[HMR_CUT_HIST] = total;
	}
}
// what a job type launches behind its kernel: nothing, but for k_cut
template <class Job> void picture_finish(hipStream_t, const Job *, int) {}
void picture_finish(hipStream_t stream, const CutJob *d_jobs, int n) { hipLaunchKernelGGL(k_cut_finish, dim3(n), dim3(HMR_BLOCK), 0, stream, d_jobs); }

// ---- launches ----
// a job table from page-locked host memory to the device by a kernel, `words` 32-bit words per job: a host-to-device copy would queue on the copy engines behind a
// batch's multi-megabyte download (k_encode_batch.inc, k_batch_stage)
__global__ __launch_bounds__(64) void k_picture_jobs(const uint32_t *h_jobs, uint32_t *d_jobs, int words)
{
	for (int k = threadIdx.x; k < words; k += blockDim.x) d_jobs[blockIdx.x * words + k] = h_jobs[blockIdx.x * words + k];
}
}  // namespace

template <class Job>
int hmr_picture_launch(hipStream_t stream, const Job *h_jobs, Job *d_jobs, int n)
{
	static_assert(sizeof(Job) % 4 == 0, "word copies");
	if (!h_jobs || !d_jobs || n < 1 || n > PICTURE_MAX_JOBS) return HMR_GPU_ERR_ARG;
	int chunks = 0;      // of the tallest picture
	for (int i = 0; i < n; i++) chunks = std::max(chunks, PictureKernel<Job>::chunks(h_jobs[i]));
	hipLaunchKernelGGL(k_picture_jobs, dim3(n), dim3(64), 0, stream, (const uint32_t *)h_jobs, (uint32_t *)d_jobs, (int)(sizeof(Job) / 4));
	hipLaunchKernelGGL(PictureKernel<Job>::kernel, dim3(chunks, n), dim3(HMR_BLOCK), 0, stream, (const Job *)d_jobs);
	picture_finish(stream, (const Job *)d_jobs, n);
	HIP_TRY(hipGetLastError());
	return HMR_GPU_OK;
}
#define HMR_PICTURE_LAUNCH(Job) template int hmr_picture_launch<Job>(hipStream_t, const Job *, Job *, int);
HMR_PICTURE_LAUNCH(IngestJob) HMR_PICTURE_LAUNCH(RgbIngestJob) HMR_PICTURE_LAUNCH(YuvIngestJob) HMR_PICTURE_LAUNCH(ScaleJob)
HMR_PICTURE_LAUNCH(RgbScaleJob) HMR_PICTURE_LAUNCH(YuvScaleJob) HMR_PICTURE_LAUNCH(EgressJob) HMR_PICTURE_LAUNCH(RgbEgressJob) HMR_PICTURE_LAUNCH(SsimJob) HMR_PICTURE_LAUNCH(CutJob)

// The output rows of a job's tiles: the widest tile row of the picture, in spans (it does not depend on the tile's rows; at most SCALE_MAX_SPANS at the ratios
// hmr_gpu_scale_check lets through), and the rows the LDS then holds.  The job's sizes and ratios are set.
template <class Job>
static int scale_tile_rows(Job &j, bool nv12)
{
	j.tile_rows = SCALE_MIN_ROWS;
	int widest = 1;
	for (int luma = 0; luma < 2; luma++)
		for (int tx = 0; tx < scale_tiles_x(j.dst_w, luma != 0); tx++)
			widest = std::max(widest, scale_tile(j, (luma ? 0 : scale_tiles_x(j.dst_w, true) * scale_tiles_y(j.dst_h, j.tile_rows, true)) + tx, nv12).total());
	return std::min(SCALE_MAX_ROWS, std::max(SCALE_MIN_ROWS, SCALE_LDS_WORDS / (widest * SCALE_SPAN_WORDS)));
}

ScaleJob hmr_scale_job(const hmr_gpu_picture &pic, int src_w, int src_h, int16_t *const dst[3], int stride_y, int stride_c, int dst_w, int dst_h)
{
	ScaleJob j;
	memset(&j, 0, sizeof j);
	hmr_job_planes(j, pic, dst, stride_y, stride_c);
	j.src_w = src_w; j.src_h = src_h; j.dst_w = dst_w; j.dst_h = dst_h;
	j.format = pic.format;
	j.ax = hmr_scale_axis(src_w, dst_w); j.ay = hmr_scale_axis(src_h, dst_h);
	j.den = j.ax.s * j.ay.s; j.mden = hmr_scale_magic(j.den);
	j.tile_rows = scale_tile_rows(j, pic.format == HMR_GPU_PIC_NV12);
	return j;
}

RgbScaleJob hmr_rgb_scale_job(const hmr_gpu_rgb_picture &pic, int src_w, int src_h, int16_t *const dst[3], int stride_y, int stride_c, int dst_w, int dst_h)
{
	RgbScaleJob j;
	memset(&j, 0, sizeof j);
	hmr_rgb_source(j, pic, dst, stride_y, stride_c);
	j.src_w = src_w; j.src_h = src_h; j.dst_w = dst_w; j.dst_h = dst_h;
	j.ax = hmr_scale_axis(src_w, dst_w); j.ay = hmr_scale_axis(src_h, dst_h);
	j.den = j.ax.s * j.ay.s; j.mden = hmr_scale_magic(j.den);
	j.tile_rows = scale_tile_rows(j, false);
	return j;
}

YuvScaleJob hmr_yuv_scale_job(const hmr_gpu_yuv_picture &pic, int src_w, int src_h, int16_t *const dst[3], int stride_y, int stride_c, int dst_w, int dst_h)
{
	YuvScaleJob j;
	memset(&j, 0, sizeof j);
	hmr_job_planes(j, pic, dst, stride_y, stride_c);
	j.f = hmr_yuv_form(pic.format, pic.chroma, pic.bits, pic.msb_aligned, pic.offset);
	j.src_w = src_w; j.src_h = src_h; j.dst_w = dst_w; j.dst_h = dst_h;
	j.ax = hmr_scale_axis(src_w, dst_w); j.ay = hmr_scale_axis(src_h, dst_h);
	j.den = j.ax.s * j.ay.s; j.mden = hmr_scale_magic(j.den);
	j.tile_rows = scale_tile_rows(j, false);
	return j;
}
