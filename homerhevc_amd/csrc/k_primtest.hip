// Test harness for the block primitives of the frame encoder (enc/enc_prims.h): the product's CTU walk (k_encode_pool) runs THESE primitives, not the table kernels of
// k_pixel / k_transform / k_intra ... that the drop-in and batched ABI expose - and until now they were only checked through whole streams.  Every entry below has the
// flat signature of the table function it restates (include/homer_gpu.h section 1; low_level_funcs_t, hmr_private.h:1063-1092) under the prefix hmr_gpu_prim_, so that the
// case generator of tests/kernel_cases.py drives them like the oracle's and the table kernels' (tests/test_gpu_prims.py).  One wavefront runs the primitive as the worker
// does (WaveGrp).  hmr_gpu_prim_bytes(1): the sample operands the worker keeps as bytes (source, prediction: src_t / pred_t) are narrowed before the call, i.e. the
// <uint8_t> instantiations run - valid for cases whose samples are 0 .. 255; (0): the 16-bit instantiations (what the one-lane checker build compiles).
// Host pointers in, synchronous; not a performance path.
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "common.h"
#include "enc/enc_inter.h"

using namespace henc;

hmr_gpu_ctx *hmr_default_ctx();

namespace {

enum { PT_SAD = 1, PT_SSD, PT_PREDICT, PT_RECONST, PT_VARIANCE, PT_INTRA_PRED, PT_FILL_REFS, PT_ADI_FILTER, PT_TRANSFORM, PT_ITRANSFORM, PT_QUANT, PT_INV_QUANT };

struct PtArgs {
	int op, bytes;
	int p[12];
	long off[6];      // element offsets of the operands in the arena (int16 elements; byte operands use the same element offsets in the byte arena)
};

int g_bytes = 0;

// arena: 16-bit image of every operand; arena8: the same elements narrowed to bytes (for the operands a primitive takes as bytes)
__global__ __launch_bounds__(64) void k_primtest(PtArgs a, int16_t *arena, uint8_t *arena8, const DevTables *T, uint32_t *ret)
{
	const WaveGrp g{(int)threadIdx.x};
	const int *p = a.p;
	auto A = [&](int k) { return arena + a.off[k]; };
	auto B = [&](int k) { return arena8 + a.off[k]; };
	uint32_t r = 0;
	switch (a.op) {
	case PT_SAD: r = blk_sad(g, A(0), p[0], A(1), p[1], p[2]); break;
	case PT_SSD: r = a.bytes ? blk_ssd(g, B(0), p[0], B(1), p[1], p[2]) : blk_ssd(g, A(0), p[0], A(1), p[1], p[2]); break;
	case PT_PREDICT:
		if (a.bytes) blk_predict(g, B(0), p[0], B(1), p[1], A(2), p[2], p[3]);
		else blk_predict(g, A(0), p[0], A(1), p[1], A(2), p[2], p[3]);
		break;
	case PT_RECONST: {
		const int16_t *res = p[1] ? A(1) : nullptr;      // (residual stride 0: the reference passes a zeroed row)
		if (a.bytes) blk_reconst(g, B(0), p[0], res, p[1], A(2), p[2], p[3]);
		else blk_reconst(g, A(0), p[0], res, p[1], A(2), p[2], p[3]);
		break;
	}
	case PT_VARIANCE: r = a.bytes ? blk_modified_variance(g, B(0), p[1], p[0], p[2]) : blk_modified_variance(g, A(0), p[1], p[0], p[2]); break;
	case PT_INTRA_PRED:      // p: pred stride, n, mode, is_luma
		if (a.bytes) {
			intra_predict(g, B(0), p[0], A(1), p[1], p[2], p[3]);
			g.sync();
			for (int i = g.tid; i < p[1] * p[1]; i += 64) A(0)[(i / p[1]) * p[0] + i % p[1]] = B(0)[(i / p[1]) * p[0] + i % p[1]];
		} else intra_predict(g, A(0), p[0], A(1), p[1], p[2], p[3]);
		break;
	case PT_FILL_REFS: intra_fill_refs(g, A(0), p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], A(1)); break;
	case PT_ADI_FILTER: intra_adi_filter(g, A(0), A(1), p[0], p[1]); break;
	case PT_TRANSFORM:      // block - 0 through the residual-forming first stage (RowDiff), as the worker's TUs call it
		if (a.bytes) tr_forward(g, (const FastTables *)nullptr, T, B(0), p[0], B(3), p[0], A(1), A(2), p[1], p[2]);
		else tr_forward(g, (const FastTables *)nullptr, T, A(0), p[0], A(3), p[0], A(1), A(2), p[1], p[2]);
		break;
	case PT_ITRANSFORM: tr_inverse(g, (const FastTables *)nullptr, T, A(0), p[0], A(1), A(2), p[1], p[2]); break;
	case PT_QUANT: r = (uint32_t)quantize(g, (const FastTables *)nullptr, T, A(0), A(1), A(2), p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]); break;
	case PT_INV_QUANT: dequantize(g, (const FastTables *)nullptr, T, A(0), A(1), p[0], p[1], p[2], p[3], p[4], p[5]); break;
	default: break;
	}
	g.sync();
	if (g.tid == 0) *ret = r;
}

// one operand of a call: a host block of `elems` int16 elements starting at `host` (nullptr: scratch of that size)
struct Operand {
	const int16_t *in;
	int16_t *out;
	size_t elems;
};

uint32_t run(int op, const int *p, int np, Operand *ops, int nops)
{
	hmr_gpu_ctx *c = hmr_default_ctx();
	if (!c) { fprintf(stderr, "hmr_gpu_prim_*: no device\n"); abort(); }
	PtArgs a;
	memset(&a, 0, sizeof a);
	a.op = op;
	a.bytes = g_bytes;
	for (int i = 0; i < np; i++) a.p[i] = p[i];
	size_t total = 0;
	for (int k = 0; k < nops; k++) {
		a.off[k] = (long)total;
		total += (ops[k].elems + 31) & ~(size_t)31;      // (64-byte aligned operands)
	}
	std::vector<int16_t> h(total, 0);
	std::vector<uint8_t> h8(total, 0);
	for (int k = 0; k < nops; k++)
		if (ops[k].in) memcpy(h.data() + a.off[k], ops[k].in, ops[k].elems * 2);
	for (size_t i = 0; i < total; i++) h8[i] = (uint8_t)h[i];
	int16_t *d = nullptr;
	uint8_t *d8 = nullptr;
	uint32_t *dr = nullptr, r = 0;
	if (hipMalloc((void **)&d, total * 2 + 64) != hipSuccess || hipMalloc((void **)&d8, total + 64) != hipSuccess || hipMalloc((void **)&dr, 4) != hipSuccess) abort();
	(void)hipMemcpy(d, h.data(), total * 2, hipMemcpyHostToDevice);
	(void)hipMemcpy(d8, h8.data(), total, hipMemcpyHostToDevice);
	hipLaunchKernelGGL(k_primtest, dim3(1), dim3(64), 0, c->stream, a, d, d8, (const DevTables *)c->tables, dr);
	if (hipStreamSynchronize(c->stream) != hipSuccess) { fprintf(stderr, "hmr_gpu_prim_*: %s\n", hipGetErrorString(hipGetLastError())); abort(); }
	(void)hipMemcpy(h.data(), d, total * 2, hipMemcpyDeviceToHost);
	(void)hipMemcpy(&r, dr, 4, hipMemcpyDeviceToHost);
	for (int k = 0; k < nops; k++)
		if (ops[k].out) memcpy(ops[k].out, h.data() + a.off[k], ops[k].elems * 2);
	(void)hipFree(d); (void)hipFree(d8); (void)hipFree(dr);
	return r;
}

// the motion search's multi-candidate byte SAD as cand_sads (enc_inter.h) calls it: one list of candidates per workgroup, every result
template <int MAXC>
__device__ __forceinline__ void multi_sad_all(const WaveGrp g, const uint8_t *src, const uint8_t *plane, const long long *off, int stride, int n, uint32_t *out)
{
	const uint8_t *cand[MAXC];
#pragma unroll
	for (int k = 0; k < MAXC; k++) cand[k] = off[k] < 0 ? nullptr : plane + off[k];
	uint32_t r[MAXC];
	multi_sad_u8<MAXC>(g, src, n, cand, stride, r);
	if (g.tid == 0) {
#pragma unroll
		for (int k = 0; k < MAXC; k++) out[k] = r[k];
	}
}
__global__ __launch_bounds__(64) void k_primtest_multi_sad(int maxc, const uint8_t *src, const uint8_t *plane, const long long *off, int stride, int n, uint32_t *out)
{
	const WaveGrp g{(int)threadIdx.x};
	off += (size_t)blockIdx.x * maxc;
	out += (size_t)blockIdx.x * maxc;
	if (maxc == 4) multi_sad_all<4>(g, src, plane, off, stride, n, out);
	else if (maxc == 8) multi_sad_all<8>(g, src, plane, off, stride, n, out);
	else multi_sad_all<9>(g, src, plane, off, stride, n, out);
}

// The walk's motion search, one case per workgroup.  motion_estimation takes an Enc whose members are fixed places of a worker's LDS (enc_lds.h): the
// kernel lays out what the search reads - the source block in the worker's source window, the picture size and the planes' pitch, the planes, the two lists - and
// calls it as cu_motion_estimation does, for a block at the window's origin.
constexpr unsigned ME_LDS_BYTES = LDS_OFF_ENC + LDS_ENC_BYTES;
static_assert(sizeof(hmr_gpu_prim_me_case) == 80 && sizeof(hmr_gpu_prim_me_out) == 20, "include/homer_gpu.h section 15 states these layouts");
__global__ __launch_bounds__(64) void k_primtest_motion_search(const hmr_gpu_prim_me_case *cases, const uint8_t *src, const uint8_t *plane0, int size, int stride, int width, int height,
							       hmr_gpu_prim_me_out *out)
{
	const WaveGrp g{(int)threadIdx.x};
	const hmr_gpu_prim_me_case &cs = cases[blockIdx.x];
	lds_zero(ME_LDS_BYTES, g.tid, 64);
	g.sync();
	Work *lw = lds_work();
	Seq *lseq = lds_seq();
	FrameCtx *lframe = lds_frame();
	const uint8_t *blk = src + (size_t)blockIdx.x * size * size;
	for (int i = g.tid; i < size * size; i += 64) lw->curr_y[(i / size) * 64 + i % size] = blk[i];
	if (g.tid == 0) {
		lseq->width = width;
		lseq->height = height;
		lseq->stride_y = stride;
		lframe->sub_y = plane0;
		lw->amvp.num = cs.n_amvp;
		for (int i = 0; i < 2; i++) { lw->amvp.mv[i].x = cs.amvp[i][0]; lw->amvp.mv[i].y = cs.amvp[i][1]; }
		lw->search_cands.num = cs.n_search;
		for (int i = 0; i < 3; i++) { lw->search_cands.mv[i].x = cs.search[i][0]; lw->search_cands.mv[i].y = cs.search[i][1]; }
	}
	g.sync();
	Enc &e = lds_enc();
	HENC_ENC_IN_LDS(e);
	MV mv = {cs.start[0], cs.start[1]}, subpix = {0, 0};
	const uint32_t sad = motion_estimation(g, e, 0, 0, uni(cs.gx), uni(cs.gy), size, lw->amvp, lw->search_cands, cs.corr, uni(cs.action), &mv, &subpix);
	if (g.tid == 0) {
		hmr_gpu_prim_me_out &o = out[blockIdx.x];
		o.mv[0] = mv.x; o.mv[1] = mv.y;
		o.subpix[0] = subpix.x; o.subpix[1] = subpix.y;
		o.sad = sad;
	}
}

size_t span(int stride, int rows, int cols) { return stride ? (size_t)stride * (rows - 1) + cols : (size_t)cols; }

}  // namespace

extern "C" {

void hmr_gpu_prim_bytes(int on) { g_bytes = on ? 1 : 0; }

uint32_t hmr_gpu_prim_sad(int16_t *src, uint32_t src_stride, int16_t *pred, uint32_t pred_stride, int size)
{
	if (g_bytes) {      // the device's search: the source block at the worker's pitch of 64, the candidate in a byte plane - twice among skipped ones, every result looked at
		std::vector<uint8_t> blk(64 * 64, 0), plane(span((int)pred_stride, size, size));
		for (int y = 0; y < size; y++)
			for (int x = 0; x < size; x++) {
				blk[y * 64 + x] = (uint8_t)src[(size_t)y * src_stride + x];
				plane[(size_t)y * pred_stride + x] = (uint8_t)pred[(size_t)y * pred_stride + x];
			}
		const int64_t off[4] = {0, -1, 0, -1};
		uint32_t out[4] = {0, 0, 0, 0};
		// (a failure is reported as a sum no block has, which no comparison with a reference passes, and in hmr_gpu_last_error: the caller's process goes on)
		if (hmr_gpu_prim_multi_sad(4, blk.data(), plane.data(), plane.size(), off, 1, (int)pred_stride, size, out) != HMR_GPU_OK) { fprintf(stderr, "hmr_gpu_prim_sad: %s\n", hmr_gpu_last_error()); return 0xFFFFFFFFu; }
		if (out[1] != 0 || out[3] != 0 || out[2] != out[0]) {
			hmr_set_error("hmr_gpu_prim_sad: candidates {p, -, p, -} gave %u %u %u %u", out[0], out[1], out[2], out[3]);
			fprintf(stderr, "%s\n", hmr_gpu_last_error());
			return 0xFFFFFFFFu;
		}
		return out[0];
	}
	Operand ops[2] = {{src, nullptr, span((int)src_stride, size, size)}, {pred, nullptr, span((int)pred_stride, size, size)}};
	const int p[3] = {(int)src_stride, (int)pred_stride, size};
	return run(PT_SAD, p, 3, ops, 2);
}
uint32_t hmr_gpu_prim_ssd16b(int16_t *src, uint32_t src_stride, int16_t *pred, uint32_t pred_stride, int size)
{
	Operand ops[2] = {{src, nullptr, span((int)src_stride, size, size)}, {pred, nullptr, span((int)pred_stride, size, size)}};
	const int p[3] = {(int)src_stride, (int)pred_stride, size};
	return run(PT_SSD, p, 3, ops, 2);
}
void hmr_gpu_prim_predict(int16_t *orig, int orig_stride, int16_t *pred, int pred_stride, int16_t *residual, int residual_stride, int size)
{
	Operand ops[3] = {{orig, nullptr, span(orig_stride, size, size)}, {pred, nullptr, span(pred_stride, size, size)}, {residual, residual, span(residual_stride, size, size)}};
	const int p[4] = {orig_stride, pred_stride, residual_stride, size};
	run(PT_PREDICT, p, 4, ops, 3);
}
void hmr_gpu_prim_reconst(int16_t *pred, int pred_stride, int16_t *residual, int residual_stride, int16_t *decoded, int decoded_stride, int size)
{
	Operand ops[3] = {{pred, nullptr, span(pred_stride, size, size)}, {residual, nullptr, span(residual_stride, size, size)}, {decoded, decoded, span(decoded_stride, size, size)}};
	const int p[4] = {pred_stride, residual_stride, decoded_stride, size};
	run(PT_RECONST, p, 4, ops, 3);
}
uint32_t hmr_gpu_prim_modified_variance(int16_t *ptr, int size, int stride, int modif)
{
	Operand ops[1] = {{ptr, nullptr, span(stride, size, size)}};
	const int p[3] = {size, stride, modif};
	return run(PT_VARIANCE, p, 3, ops, 1);
}
void hmr_gpu_prim_intra_angular(int16_t *prediction, int pred_stride, int16_t *adi, int adi_size, int cu_size, int cu_mode, int is_luma)
{
	Operand ops[2] = {{prediction, prediction, span(pred_stride, cu_size, cu_size)}, {adi, nullptr, (size_t)adi_size}};
	const int p[4] = {pred_stride, cu_size, cu_mode, is_luma};
	run(PT_INTRA_PRED, p, 4, ops, 2);
}
void hmr_gpu_prim_intra_planar(int16_t *prediction, int pred_stride, int16_t *adi, int adi_size, int cu_size)
{
	hmr_gpu_prim_intra_angular(prediction, pred_stride, adi, adi_size, cu_size, PLANAR_IDX, 1);
}
void hmr_gpu_prim_fill_reference_samples(int16_t *decoded_corner, int stride, int n, int left, int top, int bottom_left, int top_right, int bl_size, int tr_size, int16_t *adi)
{
	Operand ops[2] = {{decoded_corner, nullptr, span(stride, 2 * n + 1, 2 * n + 1)}, {adi, adi, (size_t)(4 * n + 1)}};
	const int p[8] = {stride, n, left, top, bottom_left, top_right, bl_size, tr_size};
	run(PT_FILL_REFS, p, 8, ops, 2);
}
void hmr_gpu_prim_adi_filter(int16_t *adi, int16_t *out, int adi_size, int n, int strong_enabled)
{
	Operand ops[2] = {{adi, nullptr, (size_t)adi_size}, {out, out, (size_t)adi_size}};
	const int p[2] = {n, strong_enabled};
	run(PT_ADI_FILTER, p, 2, ops, 2);
}
void hmr_gpu_prim_transform(int16_t *block, int16_t *coeff, int block_stride, int n, int is_dst)
{
	if (g_bytes) {      // the worker's call: source and prediction windows of bytes (the transforms on the matrix cores) - block = source - prediction, both 0 .. 255
		const size_t el = span(block_stride, n, n);
		std::vector<int16_t> o(el, 0), q(el, 0);
		for (int y = 0; y < n; y++)
			for (int x = 0; x < n; x++) {
				const int b = block[(size_t)y * block_stride + x];
				if (b < -255 || b > 255) { fprintf(stderr, "hmr_gpu_prim_transform: a residual of %d is not the difference of two bytes\n", b); abort(); }
				o[(size_t)y * block_stride + x] = (int16_t)(b > 0 ? b : 0);
				q[(size_t)y * block_stride + x] = (int16_t)(b < 0 ? -b : 0);
			}
		Operand ops[4] = {{o.data(), nullptr, el}, {nullptr, coeff, (size_t)n * n}, {nullptr, nullptr, (size_t)n * n}, {q.data(), nullptr, el}};
		const int p[3] = {block_stride, n, is_dst};
		run(PT_TRANSFORM, p, 3, ops, 4);
		return;
	}
	Operand ops[4] = {{block, nullptr, span(block_stride, n, n)}, {nullptr, coeff, (size_t)n * n}, {nullptr, nullptr, (size_t)n * n}, {nullptr, nullptr, span(block_stride, n, n)}};
	const int p[3] = {block_stride, n, is_dst};
	run(PT_TRANSFORM, p, 3, ops, 4);
}
void hmr_gpu_prim_itransform(int16_t *block, int16_t *coeff, int block_stride, int n, int is_dst)
{
	Operand ops[3] = {{block, block, span(block_stride, n, n)}, {coeff, nullptr, (size_t)n * n}, {nullptr, nullptr, (size_t)n * n}};
	const int p[3] = {block_stride, n, is_dst};
	run(PT_ITRANSFORM, p, 3, ops, 3);
}
void hmr_gpu_prim_quant(int16_t *src, int16_t *dst, int16_t *delta_u, int scan_mode, int depth, int comp, int is_intra, int slice_is_intra, int sign_hiding, int *ac_sum,
			int cu_size, int per, int rem)
{
	Operand ops[3] = {{src, nullptr, (size_t)cu_size * cu_size}, {nullptr, dst, (size_t)cu_size * cu_size}, {nullptr, delta_u, (size_t)cu_size * cu_size}};
	const int p[9] = {scan_mode, depth, comp, is_intra, slice_is_intra, sign_hiding, cu_size, per, rem};
	*ac_sum = (int)run(PT_QUANT, p, 9, ops, 3);
}
void hmr_gpu_prim_inv_quant(int16_t *src, int16_t *dst, int depth, int comp, int is_intra, int cu_size, int per, int rem)
{
	Operand ops[2] = {{src, nullptr, (size_t)cu_size * cu_size}, {nullptr, dst, (size_t)cu_size * cu_size}};
	const int p[6] = {depth, comp, is_intra, cu_size, per, rem};
	run(PT_INV_QUANT, p, 6, ops, 2);
}
int hmr_gpu_prim_multi_sad(int maxc, const uint8_t *src, const uint8_t *plane, size_t plane_bytes, const int64_t *cand_off, int ncalls, int stride, int n, uint32_t *out)
{
	if (!src || !plane || !cand_off || !out || ncalls < 1 || ncalls > 65536 || (maxc != 4 && maxc != 8 && maxc != 9) || (n != 8 && n != 16 && n != 32 && n != 64) || stride < 1) {
		hmr_set_error("hmr_gpu_prim_multi_sad: maxc 4 / 8 / 9, n 8 / 16 / 32 / 64, a stride of at least 1, 1 .. 65536 lists");
		return HMR_GPU_ERR_ARG;
	}
	for (int i = 0; i < ncalls * maxc; i++) {
		const int64_t o = cand_off[i];
		if (o == -1) continue;
		if (o < 0 || (uint64_t)o + (uint64_t)(n - 1) * (uint64_t)stride + (uint64_t)n > (uint64_t)plane_bytes) {
			hmr_set_error("hmr_gpu_prim_multi_sad: candidate %d of list %d does not lie inside the plane", i % maxc, i / maxc);
			return HMR_GPU_ERR_ARG;
		}
	}
	hmr_gpu_ctx *c = hmr_default_ctx();
	if (!c) { hmr_set_error("hmr_gpu_prim_multi_sad: no device"); return HMR_GPU_ERR_NO_DEVICE; }
	HIP_TRY(hipSetDevice(c->device));
	struct Bufs {
		void *p[4] = {nullptr, nullptr, nullptr, nullptr};
		~Bufs() { for (void *q : p) if (q) (void)hipFree(q); }
	} b;
	const size_t nres = (size_t)ncalls * maxc;
	HIP_TRY(hipMalloc(&b.p[0], 64 * 64));
	HIP_TRY(hipMalloc(&b.p[1], plane_bytes));
	HIP_TRY(hipMalloc(&b.p[2], nres * 8));
	HIP_TRY(hipMalloc(&b.p[3], nres * 4));
	HIP_TRY(hipMemsetAsync(b.p[0], 0, 64 * 64, c->stream));
	HIP_TRY(hipMemcpyAsync(b.p[0], src, (size_t)64 * n, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(b.p[1], plane, plane_bytes, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(b.p[2], cand_off, nres * 8, hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(k_primtest_multi_sad, dim3(ncalls), dim3(64), 0, c->stream, maxc, (const uint8_t *)b.p[0], (const uint8_t *)b.p[1], (const long long *)b.p[2], stride, n, (uint32_t *)b.p[3]);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, b.p[3], nres * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return HMR_GPU_OK;
}

int hmr_gpu_prim_motion_search(const hmr_gpu_prim_me_case *cases, int ncases, int size, const uint8_t *src, const uint8_t *planes, size_t plane_bytes, int64_t origin, int stride,
			       int width, int height, hmr_gpu_prim_me_out *out)
{
	if (!cases || !src || !planes || !out || ncases < 1 || ncases > 65536 || (size != 8 && size != 16 && size != 32 && size != 64) || width < size || height < size || width > 8192 ||
	    height > 8192 || stride < width || stride > (1 << 16)) {
		hmr_set_error("hmr_gpu_prim_motion_search: size 8 / 16 / 32 / 64, a picture of size .. 8192 samples each way, a stride of width .. 65536, 1 .. 65536 cases");
		return HMR_GPU_ERR_ARG;
	}
	// every block the search can read: whole-sample positions stay inside the picture (the window), the sub-sample rounds reach one sample further
	if (origin - 16 * (int64_t)stride - 1 < 0 || (uint64_t)origin + ((uint64_t)height * 16 + 15) * (uint64_t)stride + (uint64_t)width + 1 > (uint64_t)plane_bytes) {
		hmr_set_error("hmr_gpu_prim_motion_search: the planes do not hold the picture with one sample around it");
		return HMR_GPU_ERR_ARG;
	}
	auto vec_ok = [](const int32_t *v) { return v[0] >= -32768 && v[0] <= 32767 && v[1] >= -32768 && v[1] <= 32767; };
	for (int i = 0; i < ncases; i++) {
		const hmr_gpu_prim_me_case &k = cases[i];
		bool ok = k.gx >= 0 && k.gx <= width - size && k.gy >= 0 && k.gy <= height - size && k.n_amvp >= 0 && k.n_amvp <= 2 && k.n_search >= 0 && k.n_search <= 3 && k.action >= 1 &&
			  k.action <= 7 && k.corr >= 0. && k.corr <= 1e6 && vec_ok(k.amvp[0]) && vec_ok(k.amvp[1]) && vec_ok(k.search[0]) && vec_ok(k.search[1]) && vec_ok(k.search[2]) &&
			  vec_ok(k.start);
		if (ok && !(k.action & ME_PEL)) {
			const int xlow = (k.gx - SEARCH_RANGE_X) < 0 ? -k.gx : -SEARCH_RANGE_X, xhigh = (k.gx + SEARCH_RANGE_X) > (width - size) ? width - k.gx - size : SEARCH_RANGE_X;
			const int ylow = (k.gy - SEARCH_RANGE_Y) < 0 ? -k.gy : -SEARCH_RANGE_Y, yhigh = (k.gy + SEARCH_RANGE_Y) > (height - size) ? height - k.gy - size : SEARCH_RANGE_Y;
			const int x = k.start[0] >> 2, y = k.start[1] >> 2;
			ok = x >= xlow && x <= xhigh && y >= ylow && y <= yhigh;
		}
		if (!ok) {
			hmr_set_error("hmr_gpu_prim_motion_search: case %d is outside the ranges of include/homer_gpu.h section 15", i);
			return HMR_GPU_ERR_ARG;
		}
	}
	hmr_gpu_ctx *c = hmr_default_ctx();
	if (!c) { hmr_set_error("hmr_gpu_prim_motion_search: no device"); return HMR_GPU_ERR_NO_DEVICE; }
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipFuncSetAttribute((const void *)k_primtest_motion_search, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ME_LDS_BYTES));
	struct Bufs {
		void *p[4] = {nullptr, nullptr, nullptr, nullptr};
		~Bufs() { for (void *q : p) if (q) (void)hipFree(q); }
	} b;
	const size_t case_bytes = sizeof(hmr_gpu_prim_me_case) * (size_t)ncases, src_bytes = (size_t)ncases * size * size, out_bytes = sizeof(hmr_gpu_prim_me_out) * (size_t)ncases;
	HIP_TRY(hipMalloc(&b.p[0], case_bytes));
	HIP_TRY(hipMalloc(&b.p[1], src_bytes));
	HIP_TRY(hipMalloc(&b.p[2], plane_bytes));
	HIP_TRY(hipMalloc(&b.p[3], out_bytes));
	HIP_TRY(hipMemcpyAsync(b.p[0], cases, case_bytes, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(b.p[1], src, src_bytes, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(b.p[2], planes, plane_bytes, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemsetAsync(b.p[3], 0, out_bytes, c->stream));
	hipLaunchKernelGGL(k_primtest_motion_search, dim3(ncases), dim3(64), ME_LDS_BYTES, c->stream, (const hmr_gpu_prim_me_case *)b.p[0], (const uint8_t *)b.p[1],
			   (const uint8_t *)b.p[2] + origin, size, stride, width, height, (hmr_gpu_prim_me_out *)b.p[3]);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, b.p[3], out_bytes, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return HMR_GPU_OK;
}

}  // extern "C"
