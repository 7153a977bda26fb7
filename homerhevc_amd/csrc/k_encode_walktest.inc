// Test aid (include/homer_gpu.h section 16): the device-only forms of the CTU walk, one step at a time on a synthetic worker.
//
// Three bodies of code exist on the device only - the one-lane checker build has none of them, so no device / checker comparison sees them, and whole streams
// reach them only with what an encode happens to produce: the merge tiles of enc/enc_quad.h (quad_chain: the TU chains of all merge slots of an 8 x 8 or
// 16 x 16 CU in one matrix-core tile), and the two-halves instantiation of the inter TU chain (encode_inter_tu<PairGrp>: the helper wavefront's U and V plane
// side by side).  Both take an Enc whose members are fixed places of a worker's LDS and read the partition geometry from henc_geo_table, which is why the
// harness lives in this translation unit.  k_walk_forms lays one worker's LDS out as k_encode_pool does (the same offsets, the dynamic size of a launch
// without RD_FULL pictures), fills what the step reads from the case description, runs the step as the walk calls it and copies the results out.
// Host pointers in, one upload, one launch, one download per call; not a performance path.

hmr_gpu_ctx *hmr_default_ctx();

namespace {

static_assert(sizeof(hmr_gpu_walk_case) == 136 && sizeof(hmr_gpu_walk_out) == 5376, "include/homer_gpu.h section 16 states these layouts");
static_assert(offsetof(Work, curr_c) == offsetof(Work, curr_y) + 64 * 64 * sizeof(src_t) && sizeof(((Work *)nullptr)->curr_c) == 2 * 32 * 32 * sizeof(src_t), "the source windows are one block of Work");
static_assert(offsetof(Work, pred_c) == offsetof(Work, pred_y) + 64 * 64 * sizeof(pred_t) && sizeof(((Work *)nullptr)->pred_c) == 2 * 32 * 32 * sizeof(pred_t), "the prediction windows are one block of Work");
static_assert(sizeof(src_t) == 1 && sizeof(pred_t) == 1, "a case's window images are bytes");
// The groups of the steps: the wavefront and its two halves under types of the harness's own, as WaveGrpLat is one (enc_platform.h).  Every function template of the
// walk is then instantiated again for the harness - the same statements - and the product kernels' call graph stays what it is without this file: with the harness as
// one more caller of their instantiations the compiler's inlining of k_encode_pool changed (8 accumulation registers, half the occupancy).
struct WalkGrp : WaveGrp {};
struct WalkPairGrp : PairGrp {};
constexpr uint32_t WALK_POISON = 0x12341234u;      // every int16 of the worker's windows in HBM before a step
constexpr int WALK_WINDOW_BYTES = 64 * 64 + 2 * 32 * 32, WALK_MAX_GROUPS = 96;

__global__ __launch_bounds__(64) void k_walk_forms(const hmr_gpu_walk_case *cases, int ncases, const uint8_t *arena, const DevTables *tables, WorkSlow *slow, hmr_gpu_walk_out *out, unsigned lds_bytes)
{
	const WalkGrp g{{(int)threadIdx.x}};
	WorkSlow *const my_slow = slow + blockIdx.x;
	uint32_t *const slow_words = (uint32_t *)my_slow;
	constexpr int SLOW_WORDS = (int)(sizeof(WorkSlow) / 4);
	for (int i = g.tid; i < SLOW_WORDS; i += 64) slow_words[i] = WALK_POISON;
	g.sync();
	for (int ci = (int)blockIdx.x; ci < ncases; ci += (int)gridDim.x) {
		const hmr_gpu_walk_case &cs = cases[ci];
		hmr_gpu_walk_out &o = out[ci];
		const int step = uni(cs.step), ni = uni(cs.node), comp = uni(cs.comp);
		const bool on_helper = step == HMR_GPU_WALK_QUAD8_C || step == HMR_GPU_WALK_QUAD16_C || step == HMR_GPU_WALK_TU_PAIR || (step == HMR_GPU_WALK_TU && comp != COMP_Y);
		// a worker's LDS starts from zero (rows_enter); then what the step reads
		lds_zero(lds_bytes, g.tid, 64);
		g.sync();
		Work *lw = lds_work();
		Seq *lseq = lds_seq();
		FrameCtx *lframe = lds_frame();
		wave_copy_words(lw->curr_y, arena + cs.curr, WALK_WINDOW_BYTES, g.tid);
		if (cs.pred >= 0) wave_copy_words(lw->pred_y, arena + cs.pred, WALK_WINDOW_BYTES, g.tid);
		if (g.tid == 0) {
			lw->slow = (HENC_GLOBAL_PTR(WorkSlow))my_slow;
			lseq->stride_y = cs.stride_y;
			lseq->stride_c = cs.stride_c;
			lseq->sign_hiding = cs.sign_hiding;
			lseq->chroma_qp_offset = cs.chroma_qp_offset;
			lseq->perf_mode = 1;
			lframe->slice_type = cs.slice_type;
			lframe->avg_dist = cs.avg_dist;
			lframe->chroma_weight = cs.chroma_weight;
			lframe->sub_y = arena + cs.sub_y;
			lframe->sub_c[0] = arena + cs.sub_c[0];
			lframe->sub_c[1] = arena + cs.sub_c[1];
		}
		// the context of the wavefront that runs the step in the walk: the worker's, or its helper's (helper_serve, HJOB_NEW_CTU)
		Enc &e = on_helper ? lds_helper_enc(0) : lds_enc();
		HENC_ENC_IN_LDS(e);
		int16_t *const hscratch = lds_helper_scratch();
		// (the members the steps read, and no more: everything else is zero, and a step's kernel keeps the register budget it was pinned with)
		e.T = tables;
		e.geo.p = nullptr;
		e.on_helper = on_helper ? 1 : 0;
		e.scratch_a = on_helper ? hscratch : lw->pred_aux;
		e.scratch_b = on_helper ? hscratch + 1024 : lw->delta_u;
		e.adi_c = on_helper ? hscratch + 2048 : lw->adi;
		e.ctu_x = cs.ctu_x;
		e.ctu_y = cs.ctu_y;
		e.node_quad = ni >= NODES_RESIDENT ? node_quadrant(ni) : -1;
		g.sync();
		Node &nd = node_of(e, ni);
		const Geo &q = e.geo[ni];
		if (g.tid == 0) nd.qp = (uint8_t)cs.qp;
		QuadScratch &qs = quad_scratch(e);
		if (g.tid < 4) { qs.mv[g.tid].x = cs.mv[g.tid][0]; qs.mv[g.tid].y = cs.mv[g.tid][1]; }
		g.sync();
		if (step == HMR_GPU_WALK_TU || step == HMR_GPU_WALK_TU_PAIR) {
			// one TU of the node's size at the node's depth (PART_2Nx2N): what encode_inter's transform tree calls for a CU that is one TU
			const int depth = q.depth, wnd = depth + 1;
			if (step == HMR_GPU_WALK_TU) {
				int sum = 0;
				uint32_t raw = 0;
				const uint32_t d = encode_inter_tu(g, e, ni, comp, depth, PART_2Nx2N, &sum, &raw);
				g.sync();
				if (g.tid == 0) { o.dist[0][comp] = d; o.sum[0][comp] = sum; o.raw[0][comp] = raw; o.cbf[0][comp] = nd.inter_cbf[comp]; }
			} else {
				// (helper_serve, HJOB_INTER_TU: both planes side by side, a half of the wavefront each)
				int sum = 0;
				uint32_t raw = 0;
				const WalkPairGrp pg{{g.tid & 31, g.tid >> 5}};
				const uint32_t d = encode_inter_tu(pg, e, ni, COMP_U + pg.half, depth, PART_2Nx2N, &sum, &raw, pg.half * 512);
				g.sync();
				if (pg.tid == 0) { o.dist[0][COMP_U + pg.half] = d; o.sum[0][COMP_U + pg.half] = sum; o.raw[0][COMP_U + pg.half] = raw; o.cbf[0][COMP_U + pg.half] = nd.inter_cbf[COMP_U + pg.half]; }
			}
			// levels and reconstruction from the windows of the TU's depth, which then get their poison back: what is not poison after that was written outside the blocks
			const int c_lo = step == HMR_GPU_WALK_TU ? comp : COMP_U, c_hi = step == HMR_GPU_WALK_TU ? comp : COMP_V;
			for (int c = c_lo; c <= c_hi; c++) {
				const int n = c == COMP_Y ? q.size : q.size_chroma, x = c == COMP_Y ? q.x : q.xc, y = c == COMP_Y ? q.y : q.yc, ds = dec_stride(c);
				const int off = c == COMP_Y ? (q.abs_index << 4) : ((q.abs_index << 4) >> 2), at = c == COMP_V ? n * n : 0;
				int16_t *dec = dec_ptr(*lw, wnd, c) + y * ds + x, *lev = tq_ptr(*lw, wnd, c) + off;
				for (int i = g.tid; i < n * n; i += 64) {
					o.pred[0][at + i] = pred_ptr(*lw, c)[(y + i / n) * ctu_stride(c) + x + i % n];
					o.rec[0][at + i] = dec[(i / n) * ds + i % n];
					o.lv[0][at + i] = lev[i];
					dec[(i / n) * ds + i % n] = (int16_t)0x1234;
					lev[i] = (int16_t)0x1234;
				}
			}
			g.sync();
			uint32_t stray = 0;
			for (int i = g.tid; i < SLOW_WORDS; i += 64)
				if (slow_words[i] != WALK_POISON) { stray++; slow_words[i] = WALK_POISON; }
			stray = g.sum(stray);
			if (g.tid == 0) o.stray = stray;
			g.sync();
			continue;
		}
#if defined(HENC_QUAD)
		int per = 0, nslots = 0;      // elements of a slot's block(s) of the step's component class, slots the CU's tile shapes hold
		const uint8_t *sp = nullptr, *sr = nullptr;
		const int16_t *sl = nullptr;
		if (step == HMR_GPU_WALK_QUAD8_Y) {
			quad_chain<8, false>(g.tid, e, ni, qs, 0, qs.s8.wk_lv, qs.s8.wk_cf, qs.s8.wk_du, qs.acs);      // (quad_prepare<8>)
			per = 64; nslots = 4; sp = qs.s8.pred_y[0]; sr = qs.s8.rec_y[0]; sl = qs.s8.lv_y[0];
		} else if (step == HMR_GPU_WALK_QUAD8_C) {
			quad_chroma_job(g, e, ni, 8);
			per = 32; nslots = 4; sp = qs.s8.pred_c[0][0]; sr = qs.s8.rec_c[0][0]; sl = qs.s8.lv_c[0][0];
		} else if (step == HMR_GPU_WALK_QUAD16_Y) {
			int16_t *x0 = lw->iq_y;      // (quad_prepare<16>: the exchange buffers are the worker's level slot)
			quad_chain<16, false>(g.tid, e, ni, qs, uni(cs.one_slot), x0, x0 + 256, x0 + 512, qs.acs);
			per = 256; nslots = 2; sp = qs.s16.pred_y[0]; sr = qs.s16.rec_y[0]; sl = qs.s16.lv_y[0];
		} else {
			quad_chroma_job(g, e, ni, 16);
			per = 128; nslots = 2; sp = qs.s16.pred_c[0][0]; sr = qs.s16.rec_c[0][0]; sl = qs.s16.lv_c[0][0];
		}
		g.sync();
		for (int i = g.tid; i < nslots * per; i += 64) {
			const int s = i / per, j = i % per;
			o.pred[s][j] = sp[i];
			o.rec[s][j] = sr[i];
			o.lv[s][j] = sl[i];
		}
		if (g.tid < 12) {
			const int s = g.tid / 3, c = g.tid % 3;
			o.dist[s][c] = qs.res[s].dist[c]; o.sum[s][c] = qs.res[s].sum[c]; o.raw[s][c] = qs.res[s].raw[c]; o.cbf[s][c] = qs.res[s].cbf[c];
		}
		g.sync();
#endif
	}
}

// [lo, hi): the bytes of the arena an n x n block at `base` with row pitch `pitch` covers
bool walk_block_inside(int64_t base, int64_t pitch, int n, size_t arena_bytes)
{
	const int64_t lo = base, hi = base + (int64_t)(n - 1) * pitch + n;
	return pitch > 0 && lo >= 0 && hi <= (int64_t)arena_bytes;
}

// every address the step of a case can form lies inside the arena (the phase-plane addressing of section 13: motion_compensate_cu, quad_chain)
const char *walk_case_refused(const hmr_gpu_walk_case &c, const Geo *geo, size_t arena_bytes)
{
	const bool quad8 = c.step == HMR_GPU_WALK_QUAD8_Y || c.step == HMR_GPU_WALK_QUAD8_C, quad16 = c.step == HMR_GPU_WALK_QUAD16_Y || c.step == HMR_GPU_WALK_QUAD16_C;
	const bool tu = c.step == HMR_GPU_WALK_TU || c.step == HMR_GPU_WALK_TU_PAIR;
	if (!quad8 && !quad16 && !tu) return "step";
#if !defined(HENC_QUAD)
	if (!tu) return "step (the library was built without the merge tiles)";
#endif
	if (c.node < 0 || c.node >= NNODES) return "node";
	const Geo &q = geo[c.node];
	if (quad8 && q.size != 8) return "node (an 8 x 8 CU: 21 .. 84)";
	if (quad16 && q.size != 16) return "node (a 16 x 16 CU: 5 .. 20)";
	if (tu && q.size != 8 && q.size != 16) return "node (a TU of an 8 x 8 or 16 x 16 CU)";
	if (c.step == HMR_GPU_WALK_TU && (c.comp < COMP_Y || c.comp > COMP_V)) return "comp";
	if (c.one_slot < 0 || c.one_slot > 1) return "one_slot";
	if (c.qp < 0 || c.qp > 51) return "qp";
	if (c.chroma_qp_offset < -12 || c.chroma_qp_offset > 12) return "chroma_qp_offset";
	if (c.slice_type != SLICE_P && c.slice_type != SLICE_I && c.slice_type != SLICE_B) return "slice_type";
	if (c.sign_hiding != 0 && c.sign_hiding != 1) return "sign_hiding";
	if (!(c.avg_dist >= 0.) || !(c.chroma_weight > 0.)) return "avg_dist / chroma_weight";
	if (c.curr < 0 || c.curr % 4 || (size_t)c.curr + WALK_WINDOW_BYTES > arena_bytes) return "curr";
	if (tu) {
		if (c.pred < 0 || c.pred % 4 || (size_t)c.pred + WALK_WINDOW_BYTES > arena_bytes) return "pred";
		return nullptr;
	}
	if (c.pred >= 0 && (c.pred % 4 || (size_t)c.pred + WALK_WINDOW_BYTES > arena_bytes)) return "pred";
	if (c.stride_y <= 0 || c.stride_c <= 0 || c.stride_y > (1 << 20) || c.stride_c > (1 << 20)) return "stride";
	if (c.ctu_x < -(1 << 20) || c.ctu_x > (1 << 20) || c.ctu_y < -(1 << 20) || c.ctu_y > (1 << 20)) return "ctu_x / ctu_y";
	for (int s = 0; s < 4; s++) {
		const int mx = c.mv[s][0], my = c.mv[s][1];
		if (mx < -(1 << 15) || mx >= (1 << 15) || my < -(1 << 15) || my >= (1 << 15)) return "mv";
		if (c.step == HMR_GPU_WALK_QUAD8_Y || c.step == HMR_GPU_WALK_QUAD16_Y) {
			const int64_t sy = 16 * (int64_t)c.stride_y;
			const int64_t base = c.sub_y + (((my & 3) << 2) | (mx & 3)) * (int64_t)c.stride_y + (int64_t)(c.ctu_y + q.y + (my >> 2)) * sy + c.ctu_x + q.x + (mx >> 2);
			if (!walk_block_inside(base, sy, q.size, arena_bytes)) return "a luma prediction block outside the arena";
		} else {
			const int64_t sc = 64 * (int64_t)c.stride_c;
			const int64_t oc = (((my & 7) << 3) | (mx & 7)) * (int64_t)c.stride_c + (int64_t)((c.ctu_y >> 1) + q.yc + (my >> 3)) * sc + (c.ctu_x >> 1) + q.xc + (mx >> 3);
			for (int p = 0; p < 2; p++)
				if (!walk_block_inside(c.sub_c[p] + oc, sc, q.size_chroma, arena_bytes)) return "a chroma prediction block outside the arena";
		}
	}
	return nullptr;
}

}  // namespace

extern "C" int hmr_gpu_walk_forms(const hmr_gpu_walk_case *cases, int ncases, const uint8_t *arena, size_t arena_bytes, hmr_gpu_walk_out *out)
{
	if (!cases || ncases < 1 || ncases > (1 << 20) || !arena || !arena_bytes || !out) {
		hmr_set_error("hmr_gpu_walk_forms: NULL argument or ncases outside 1 .. 2^20");
		return HMR_GPU_ERR_ARG;
	}
	std::vector<Geo> geo(NNODES);
	make_geo(geo.data());
	for (int i = 0; i < ncases; i++) {
		const char *why = walk_case_refused(cases[i], geo.data(), arena_bytes);
		if (why) {
			hmr_set_error("hmr_gpu_walk_forms: case %d refused: %s", i, why);
			return HMR_GPU_ERR_ARG;
		}
	}
	hmr_gpu_ctx *c = hmr_default_ctx();
	if (!c) {
		hmr_set_error("hmr_gpu_walk_forms: no device");
		return HMR_GPU_ERR_NO_DEVICE;
	}
	HIP_TRY(hipSetDevice(c->device));
	// the partition geometry, as hmr_gpu_enc_create leaves it (the same tree for every encoder)
	HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(henc_geo_table), geo.data(), sizeof(Geo) * NNODES));
	const unsigned lds_bytes = (unsigned)lds_request(false);
	HIP_TRY(hipFuncSetAttribute((const void *)k_walk_forms, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
	const int groups = ncases < WALK_MAX_GROUPS ? ncases : WALK_MAX_GROUPS;
	struct Bufs {
		void *p[4] = {nullptr, nullptr, nullptr, nullptr};
		~Bufs() { for (void *q : p) if (q) (void)hipFree(q); }
	} b;
	const size_t case_bytes = sizeof(hmr_gpu_walk_case) * (size_t)ncases, out_bytes = sizeof(hmr_gpu_walk_out) * (size_t)ncases;
	HIP_TRY(hipMalloc(&b.p[0], case_bytes));
	HIP_TRY(hipMalloc(&b.p[1], arena_bytes + 64));
	HIP_TRY(hipMalloc(&b.p[2], sizeof(WorkSlow) * (size_t)groups));
	HIP_TRY(hipMalloc(&b.p[3], out_bytes));
	HIP_TRY(hipMemcpyAsync(b.p[0], cases, case_bytes, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(b.p[1], arena, arena_bytes, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemsetAsync(b.p[3], 0, out_bytes, c->stream));
	hipLaunchKernelGGL(k_walk_forms, dim3(groups), dim3(64), lds_bytes, c->stream, (const hmr_gpu_walk_case *)b.p[0], ncases, (const uint8_t *)b.p[1], (const DevTables *)c->tables,
			   (WorkSlow *)b.p[2], (hmr_gpu_walk_out *)b.p[3], lds_bytes);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, b.p[3], out_bytes, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return HMR_GPU_OK;
}
