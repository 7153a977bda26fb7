// Device ingest (include/homer_gpu.h section 12d): 8-bit 4:2:0 pictures that already lie in device memory - I420 planes or NV12, any base address, any pitch - into
// the int16 source planes of their encoders' picture slots (what k_widen_plane makes of a host picture: sample (x, y) at y * stride + x, nothing outside width x height
// touched).  ONE launch for a batch of pictures; it has no arithmetic and is bound by HBM: 1.5 W H bytes read, 3 W H written per picture.
//
// Mapping: blockIdx.y = picture (a record of the job table), blockIdx.x = a chunk of INGEST_ROWS rows of it - first the luma rows, then the chroma rows (a chroma row is its
// U and its V part: as many source bytes as a luma row) - so that one grid covers the three planes of every picture; pictures smaller than the largest of the launch leave
// their last chunks empty.  A lane takes 16 source samples: one 16-byte load, two 16-byte stores of int16; NV12 chroma: one 16-byte load of eight U, V pairs, one 16-byte
// store to each plane.  The destination side is always 16-byte aligned (strides are multiples of 8 elements, the planes come from hipMalloc, a lane starts at a multiple
// of 8 elements).  The source side is whatever the producer made: the 16-byte load is issued at whatever address the row gives it (load16 below); a
// row's tail of fewer than 16 samples takes the narrow path, sample by sample.  No lane reads a byte outside [plane + y * pitch, plane + y * pitch + row bytes).
#include "ingest.h"

namespace {
constexpr int INGEST_ROWS = 8;

__device__ __forceinline__ uint32_t even_bytes(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c020c00u); }      // bytes 0 and 2 of w as two 16-bit values
__device__ __forceinline__ uint32_t odd_bytes(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c030c01u); }       // bytes 1 and 3
__device__ __forceinline__ uint32_t low_bytes(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c010c00u); }       // bytes 0 and 1
__device__ __forceinline__ uint32_t high_bytes(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c030c02u); }      // bytes 2 and 3

// The job table holds plain pointers; the kernel addresses them as global memory (global_load / global_store instead of the flat forms).
#define GLOBAL_AS __attribute__((address_space(1)))
typedef GLOBAL_AS const uint8_t *src_ptr;
typedef GLOBAL_AS int16_t *dst_ptr;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_unaligned __attribute__((aligned(1)));

// Exactly the 16 bytes at s, whatever its alignment: ONE global_load_dwordx4 (the memory pipeline takes vector loads at any byte address; one that straddles a
// cache line costs a second line access, no more bytes).  Spelling the unaligned case as dword or byte loads gives the same instruction: the backend merges them.
__device__ __forceinline__ u32x4 load16(src_ptr s)
{
	return *(GLOBAL_AS const u32x4_unaligned *)s;
}

// n <= 16 samples of a plane row, widened; d is 16-byte aligned
__device__ __forceinline__ void widen_span(src_ptr s, dst_ptr d, int n)
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
__device__ __forceinline__ void split_span(src_ptr s, dst_ptr du, dst_ptr dv, int n)
{
	if (n == 8) {
		const u32x4 v = load16(s);
		*(GLOBAL_AS u32x4 *)du = u32x4{even_bytes(v.x), even_bytes(v.y), even_bytes(v.z), even_bytes(v.w)};
		*(GLOBAL_AS u32x4 *)dv = u32x4{odd_bytes(v.x), odd_bytes(v.y), odd_bytes(v.z), odd_bytes(v.w)};
		return;
	}
	for (int i = 0; i < n; i++) { du[i] = s[2 * i]; dv[i] = s[2 * i + 1]; }
}

__global__ __launch_bounds__(256) void k_ingest(const IngestJob *jobs)
{
	const IngestJob j = jobs[blockIdx.y];
	const int W = j.width, H = j.height, cw = W >> 1, ch = H >> 1;
	const int luma_chunks = (H + INGEST_ROWS - 1) / INGEST_ROWS, chroma_chunks = (ch + INGEST_ROWS - 1) / INGEST_ROWS;
	const int b = (int)blockIdx.x, t = (int)threadIdx.x;
	if (b < luma_chunks) {
		const int y0 = b * INGEST_ROWS, rows = H - y0 < INGEST_ROWS ? H - y0 : INGEST_ROWS, per_row = (W + 15) >> 4;
		const src_ptr src = (src_ptr)j.src[0];
		const dst_ptr dst = (dst_ptr)j.dst[0];
		const int64_t pitch = j.pitch[0];
		const int stride = j.stride_y;
		for (int i = t; i < rows * per_row; i += 256) {
			const int r = i / per_row, x = (i - r * per_row) << 4, y = y0 + r;
			widen_span(src + (int64_t)y * pitch + x, dst + (size_t)y * stride + x, W - x < 16 ? W - x : 16);
		}
		return;
	}
	if (b >= luma_chunks + chroma_chunks) return;
	const int y0 = (b - luma_chunks) * INGEST_ROWS, rows = ch - y0 < INGEST_ROWS ? ch - y0 : INGEST_ROWS;
	const int stride = j.stride_c;
	if (j.format == HMR_GPU_PIC_NV12) {
		const int per_row = (cw + 7) >> 3;
		const src_ptr src = (src_ptr)j.src[1];
		const dst_ptr du = (dst_ptr)j.dst[1], dv = (dst_ptr)j.dst[2];
		const int64_t pitch = j.pitch[1];
		for (int i = t; i < rows * per_row; i += 256) {
			const int r = i / per_row, x = (i - r * per_row) << 3, y = y0 + r;
			const size_t o = (size_t)y * stride + x;
			split_span(src + (int64_t)y * pitch + 2 * x, du + o, dv + o, cw - x < 8 ? cw - x : 8);
		}
		return;
	}
	const int per_plane = (cw + 15) >> 4, per_row = 2 * per_plane;      // (a row's U part, then its V part)
	const src_ptr su = (src_ptr)j.src[1], sv = (src_ptr)j.src[2];
	const dst_ptr du = (dst_ptr)j.dst[1], dv = (dst_ptr)j.dst[2];
	const int64_t pu = j.pitch[1], pv = j.pitch[2];
	for (int i = t; i < rows * per_row; i += 256) {
		const int r = i / per_row, g = i - r * per_row, y = y0 + r;
		const bool is_v = g >= per_plane;
		const int x = (is_v ? g - per_plane : g) << 4;
		widen_span((is_v ? sv : su) + (int64_t)y * (is_v ? pv : pu) + x, (is_v ? dv : du) + (size_t)y * stride + x, cw - x < 16 ? cw - x : 16);
	}
}

// the job table from page-locked host memory to the device by a kernel: a host-to-device copy would queue on the copy engines behind a batch's multi-megabyte download
// (k_encode_batch.inc, k_batch_stage)
__global__ __launch_bounds__(64) void k_ingest_jobs(const uint32_t *h_jobs, uint32_t *d_jobs)
{
	constexpr int WORDS = (int)(sizeof(IngestJob) / 4);
	for (int k = threadIdx.x; k < WORDS; k += blockDim.x) d_jobs[blockIdx.x * WORDS + k] = h_jobs[blockIdx.x * WORDS + k];
}
}  // namespace

int hmr_ingest_launch(hipStream_t stream, const IngestJob *h_jobs, IngestJob *d_jobs, int n)
{
	static_assert(sizeof(IngestJob) % 4 == 0, "word copies");
	if (!h_jobs || !d_jobs || n < 1 || n > INGEST_MAX_JOBS) return HMR_GPU_ERR_ARG;
	int chunks = 0;
	for (int i = 0; i < n; i++) {
		const int c = (h_jobs[i].height + INGEST_ROWS - 1) / INGEST_ROWS + (h_jobs[i].height / 2 + INGEST_ROWS - 1) / INGEST_ROWS;
		if (c > chunks) chunks = c;
	}
	hipLaunchKernelGGL(k_ingest_jobs, dim3(n), dim3(64), 0, stream, (const uint32_t *)h_jobs, (uint32_t *)d_jobs);
	hipLaunchKernelGGL(k_ingest, dim3(chunks, n), dim3(256), 0, stream, (const IngestJob *)d_jobs);
	HIP_TRY(hipGetLastError());
	return HMR_GPU_OK;
}

static int refuse(const char *what)
{
	hmr_set_error("hmr_gpu_picture: %s", what);
	return HMR_GPU_ERR_ARG;
}
// a descriptor against a picture size, on the host alone
extern "C" int hmr_gpu_picture_check(const hmr_gpu_picture *pic, int width, int height)
{
	if (!pic) return refuse("the descriptor is NULL");
	if (pic->format != HMR_GPU_PIC_I420 && pic->format != HMR_GPU_PIC_NV12) return refuse("format: neither HMR_GPU_PIC_I420 nor HMR_GPU_PIC_NV12");
	if (pic->reserved != 0) return refuse("reserved: must be 0");
	if (width <= 0 || (width & 1)) return refuse("width: must be positive and even");
	if (height <= 0 || (height & 1)) return refuse("height: must be positive and even");
	const int planes = pic->format == HMR_GPU_PIC_NV12 ? 2 : 3;
	static const char *const missing[3] = {"plane[0]: NULL", "plane[1]: NULL", "plane[2]: NULL"};
	static const char *const negative[3] = {"pitch[0]: negative", "pitch[1]: negative", "pitch[2]: negative"};
	static const char *const narrow[3] = {"pitch[0]: less than a row's bytes (width)", "pitch[1]: less than a row's bytes (I420: width / 2, NV12: width)", "pitch[2]: less than a row's bytes (width / 2)"};
	for (int c = 0; c < planes; c++) {
		if (!pic->plane[c]) return refuse(missing[c]);
		if (pic->pitch[c] < 0) return refuse(negative[c]);
		const int row_bytes = c == 0 || pic->format == HMR_GPU_PIC_NV12 ? width : width / 2;
		if (pic->pitch[c] < row_bytes) return refuse(narrow[c]);
	}
	if (planes == 2 && pic->plane[2]) return refuse("plane[2]: must be NULL for NV12 (plane[1] holds the U, V pairs)");
	return HMR_GPU_OK;
}
