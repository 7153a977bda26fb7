// Device egress (include/homer_gpu.h section 12e), the mirror image of k_ingest.hip: the frame encoder's final pictures - int16 planes with margins, sample (x, y) at
// y * stride + x - into the caller's 8-bit 4:2:0 pictures in device memory (I420 planes or NV12, any base address, any pitch), and / or the exact sums of squared differences
// of each plane against the int16 source planes of a picture slot.  ONE launch for a batch of pictures; bound by HBM: per picture 3 W H bytes read (final picture), 3 W H read
// (slot, when sums are asked for), 1.5 W H written (when a picture is asked for) - hmr_egress_bytes in egress.h.
//
// Mapping: as k_ingest - blockIdx.y = picture (a record of the job table), blockIdx.x = a chunk of EGRESS_ROWS rows of it, first the luma rows, then the chroma rows (a chroma
// row is its U and its V part), pictures smaller than the largest of the launch leave their last chunks empty.  A lane takes 16 samples: two 16-byte loads of the final
// picture (four with the slot's samples), the low bytes packed by v_perm_b32 into ONE 16-byte store issued at whatever address the row gives it; NV12 chroma: a 16-byte load of
// eight U and one of eight V samples, interleaved into one 16-byte store.  The int16 side is always 16-byte aligned (strides and margins are multiples of 8 elements, the
// planes come from hipMalloc, a lane starts at a multiple of 8 elements).  A row's tail of fewer than 16 samples goes sample by sample.  No lane writes a byte outside
// [plane + y * pitch, plane + y * pitch + row bytes).
//
// Sums: a lane adds the squares of its differences into 32-bit accumulators (one for luma or U, one for V), the wavefront's lanes are summed by the DPP butterfly of
// common.h, the workgroup's four wavefronts through LDS in 64 bits, and one lane adds the workgroup's sum to the picture's 64-bit sum of that plane with one vector atomic
// (global_atomic_add_x2).  Integer sums: exact whatever the order.  A chunk holds at most EGRESS_ROWS x EGRESS_MAX_WIDTH samples of one plane, each difference at most 255:
// 8 x 8192 x 255^2 = 4 261 478 400 < 2^32, so neither a lane's nor a wavefront's accumulator wraps; a picture's sum does not fit 32 bits (255^2 x 3840 x 2160 = 5.4e11).
#include <math.h>
#include "egress.h"

namespace {
constexpr int EGRESS_ROWS = 8;
static_assert((uint64_t)EGRESS_ROWS * EGRESS_MAX_WIDTH * 255 * 255 < (1ull << 32), "a workgroup's partial sum of one plane fits 32 bits");

#define GLOBAL_AS __attribute__((address_space(1)))
typedef GLOBAL_AS const int16_t *pic_ptr;
typedef GLOBAL_AS uint8_t *out_ptr;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_unaligned __attribute__((aligned(1)));

// two dwords of two int16 samples each -> their four low bytes
__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x06040200u); }
// a dword of two U samples, a dword of two V samples -> U0 V0 U1 V1
__device__ __forceinline__ uint32_t weave4(uint32_t u, uint32_t v) { return __builtin_amdgcn_perm(v, u, 0x06020400u); }
__device__ __forceinline__ u32x4 pack16(u32x4 a, u32x4 b) { return u32x4{pack4(a.x, a.y), pack4(a.z, a.w), pack4(b.x, b.y), pack4(b.z, b.w)}; }
// exactly the 16 bytes at d, whatever its alignment: ONE global_store_dwordx4 (k_ingest's load16 in the other direction)
__device__ __forceinline__ void store16(out_ptr d, u32x4 v) { *(GLOBAL_AS u32x4_unaligned *)d = v; }

// squared differences of two int16 pairs
__device__ __forceinline__ uint32_t sq2(uint32_t a, uint32_t b)
{
	const int d0 = (int)(int16_t)a - (int)(int16_t)b, d1 = ((int)a >> 16) - ((int)b >> 16);
	return (uint32_t)(d0 * d0) + (uint32_t)(d1 * d1);
}
__device__ __forceinline__ uint32_t sq8(u32x4 a, u32x4 b) { return sq2(a.x, b.x) + sq2(a.y, b.y) + sq2(a.z, b.z) + sq2(a.w, b.w); }

// n <= 16 samples of a plane row: r / s 16-byte aligned (s NULL: no sum), d anywhere (NULL: no picture); returns the sum of squared differences
__device__ __forceinline__ uint32_t narrow_span(pic_ptr r, pic_ptr s, out_ptr d, int n)
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
__device__ __forceinline__ void weave_span(pic_ptr ru, pic_ptr rv, pic_ptr su, pic_ptr sv, out_ptr d, int n, uint32_t &acc_u, uint32_t &acc_v)
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
	const int W = j.width, H = j.height, cw = W >> 1, ch = H >> 1;
	const int luma_chunks = (H + EGRESS_ROWS - 1) / EGRESS_ROWS, chroma_chunks = (ch + EGRESS_ROWS - 1) / EGRESS_ROWS;
	const int b = (int)blockIdx.x, t = (int)threadIdx.x;
	const bool sums = j.src[0] != nullptr, picture = j.dst[0] != nullptr;
	GLOBAL_AS uint64_t *ssd = (GLOBAL_AS uint64_t *)j.ssd;
	if (b < luma_chunks) {
		const int y0 = b * EGRESS_ROWS, rows = H - y0 < EGRESS_ROWS ? H - y0 : EGRESS_ROWS, per_row = (W + 15) >> 4;
		const pic_ptr rec = (pic_ptr)j.rec[0], src = (pic_ptr)j.src[0];
		const out_ptr dst = (out_ptr)j.dst[0];
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
	if (b >= luma_chunks + chroma_chunks) return;
	const int y0 = (b - luma_chunks) * EGRESS_ROWS, rows = ch - y0 < EGRESS_ROWS ? ch - y0 : EGRESS_ROWS;
	const pic_ptr ru = (pic_ptr)j.rec[1], rv = (pic_ptr)j.rec[2], su = (pic_ptr)j.src[1], sv = (pic_ptr)j.src[2];
	uint32_t acc_u = 0, acc_v = 0;
	if (j.format == HMR_GPU_PIC_NV12 && picture) {
		const int per_row = (cw + 7) >> 3;
		const out_ptr dst = (out_ptr)j.dst[1];
		const int64_t pitch = j.pitch[1];
		for (int i = t; i < rows * per_row; i += HMR_BLOCK) {
			const int r = i / per_row, x = (i - r * per_row) << 3, y = y0 + r;
			const size_t o = (size_t)y * j.stride_c + x, so = (size_t)y * j.src_stride_c + x;
			weave_span(ru + o, rv + o, sums ? su + so : nullptr, sums ? sv + so : nullptr, dst + (int64_t)y * pitch + 2 * x, cw - x < 8 ? cw - x : 8, acc_u, acc_v);
		}
	} else {
		const int per_plane = (cw + 15) >> 4, per_row = 2 * per_plane;      // (a row's U part, then its V part)
		const out_ptr du = (out_ptr)j.dst[1], dv = (out_ptr)j.dst[2];
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

// the job table from page-locked host memory to the device by a kernel, as k_ingest_jobs does (a copy would queue on the copy engines behind a batch's download)
__global__ __launch_bounds__(64) void k_egress_jobs(const uint32_t *h_jobs, uint32_t *d_jobs)
{
	constexpr int WORDS = (int)(sizeof(EgressJob) / 4);
	for (int k = threadIdx.x; k < WORDS; k += blockDim.x) d_jobs[blockIdx.x * WORDS + k] = h_jobs[blockIdx.x * WORDS + k];
}
}  // namespace

int hmr_egress_launch(hipStream_t stream, const EgressJob *h_jobs, EgressJob *d_jobs, int n)
{
	static_assert(sizeof(EgressJob) % 4 == 0, "word copies");
	if (!h_jobs || !d_jobs || n < 1 || n > EGRESS_MAX_JOBS) return HMR_GPU_ERR_ARG;
	int chunks = 0;
	for (int i = 0; i < n; i++) {
		const int c = (h_jobs[i].height + EGRESS_ROWS - 1) / EGRESS_ROWS + (h_jobs[i].height / 2 + EGRESS_ROWS - 1) / EGRESS_ROWS;
		if (c > chunks) chunks = c;
	}
	hipLaunchKernelGGL(k_egress_jobs, dim3(n), dim3(64), 0, stream, (const uint32_t *)h_jobs, (uint32_t *)d_jobs);
	hipLaunchKernelGGL(k_egress, dim3(chunks, n), dim3(HMR_BLOCK), 0, stream, (const EgressJob *)d_jobs);
	HIP_TRY(hipGetLastError());
	return HMR_GPU_OK;
}

// homer_psnr's arithmetic (hmr_metics.c:66-104) on sums of squared differences: pure host
extern "C" int hmr_gpu_psnr(const uint64_t ssd[3], int width, int height, double psnr[3])
{
	if (!ssd || !psnr || width <= 0 || height <= 0 || (width & 1) || (height & 1)) {
		hmr_set_error("hmr_gpu_psnr: needs three sums, three results and a positive even width and height (%d x %d)", width, height);
		return HMR_GPU_ERR_ARG;
	}
	for (int c = 0; c < 3; c++) {
		const double samples = c ? (double)(width / 2) * (height / 2) : (double)width * height;
		psnr[c] = ssd[c] ? 10.0 * log10(255.0 * 255.0 * samples / (double)ssd[c]) : 99.99;
	}
	return HMR_GPU_OK;
}
