// Test aid (include/homer_gpu.h section 19): the merge evaluation of an 8 x 8 or 16 x 16 CU as the device runs it, and the device-only body of motion_compensate_cu.
//
// For these CUs check_rd_cost_merge (enc/enc_ctu.h) does not run its candidate loop on the device: quad_load_cands -> quad_prepare -> quad_merge_loop -> quad_commit
// (enc/enc_quad.h) evaluate every distinct candidate side by side - luma on the worker, chroma on the helper through HJOB_QUAD_C -, replay the loop on figures in registers
// and write what the loop leaves behind once.  The one-lane checker build has none of it; k_walk_forms (section 16) pins the tiles' arithmetic and nothing of the replay.
// Here a workgroup is what it is in k_encode_pool, as in k_encode_helpertest.inc - a worker wavefront and its helper wavefront, the same LDS places, entered through
// rows_enter and left through release_helpers - and the worker runs, per case, the three statements of check_rd_cost_merge on planted input, or motion_compensate_cu.
//
// What keeps the harness from hanging: it has no wait loop of its own - it waits inside quad_prepare (helper_wait behind its one helper_post) and through helper_wait after
// HJOB_NEW_CTU only; the worker has no way out of its loop over the cases but its end (no return, no continue between rows_enter and release_helpers - whatever could make
// it leave early or address outside the arena is refused on the host before the launch).

namespace {

static_assert(sizeof(hmr_gpu_merge_case) == 152 && sizeof(hmr_gpu_merge_out) == 9520, "include/homer_gpu.h section 19 states these layouts");
static_assert(offsetof(hmr_gpu_merge_case, mv) == 64 && offsetof(hmr_gpu_merge_case, avg_dist) == 96 && offsetof(hmr_gpu_merge_case, sub_y) == 112 && offsetof(hmr_gpu_merge_case, pred) == 144,
	      "hmr_gpu_merge_case: tests/merge_cases.py MERGE_CASE");
static_assert(offsetof(hmr_gpu_merge_out, inter_ssq) == 64 && offsetof(hmr_gpu_merge_out, cand_mv) == 88 && offsetof(hmr_gpu_merge_out, cbf_buffs) == 128 && offsetof(hmr_gpu_merge_out, rec_cbf) == 192 &&
		      offsetof(hmr_gpu_merge_out, lv) == 304 && offsetof(hmr_gpu_merge_out, dec) == 1840 && offsetof(hmr_gpu_merge_out, pred) == 3376,
	      "hmr_gpu_merge_out: tests/merge_cases.py MERGE_OUT");
static_assert(sizeof(CtuPublic) % 4 == 0 && offsetof(CtuPublic, cbf) % 2 == 0 && offsetof(CtuPublic, tr_idx) % 2 == 0 && offsetof(CtuPublic, intra_mode) % 2 == 0 && offsetof(CtuPublic, mv_ref_idx) % 2 == 0,
	      "the record's poison: words, and byte arrays that start at even offsets");
// The groups of the steps: types of the harness's own, as HelpGrp is one (k_encode_walktest.inc says why) - the worker's steps and the plain helper loop with everything
// helper_serve calls are instantiated for this file alone, and the product kernels' and the other harnesses' call graphs stay what they are without it.
struct MergeGrp : WaveGrp {};
constexpr int MERGE_MAX_GROUPS = 96;
constexpr int16_t MERGE_POISON16 = 0x1234;

__device__ __forceinline__ uint8_t merge_poison_byte(int k) { return (k & 1) ? (uint8_t)0x12 : (uint8_t)0x34; }

template <class G>
__device__ __forceinline__ void merge_run_case(const G g, Enc &__restrict__ e, const hmr_gpu_merge_case &cs, hmr_gpu_merge_out &o, const uint8_t *arena, WorkSlow *my_slow, CtuInfo *my_ctu)
{
	HENC_ENC_IN_LDS(e);
	HENC_QPROF_T0();
	Work *lw = lds_work();
	Seq *lseq = lds_seq();
	FrameCtx *lframe = lds_frame();
	const int step = uni(cs.step), ni = uni(cs.node);
	const bool merge = step == HMR_GPU_MERGE_MERGE;
	// the worker's LDS below the mailbox starts from zero, as rows_enter left it (the helper is idle: every job has been waited for); the mailbox and the contexts keep
	// their sequence numbers
	lds_zero(LDS_OFF_BOX, g.tid, 64);
	g.sync();
	wave_copy_words(lw->curr_y, arena + cs.curr, WALK_WINDOW_BYTES, g.tid);
	wave_copy_words(lw->pred_y, arena + cs.pred, WALK_WINDOW_BYTES, g.tid);
	if (g.tid == 0) {
		lw->slow = (HENC_GLOBAL_PTR(WorkSlow))my_slow;
		lseq->width = cs.width;
		lseq->height = cs.height;
		lseq->margin_y = cs.margin;
		lseq->stride_y = cs.stride_y;
		lseq->stride_c = cs.stride_c;
		lseq->perf_mode = cs.perf_mode;
		lseq->sign_hiding = cs.sign_hiding;
		lseq->chroma_qp_offset = cs.chroma_qp_offset;
		lframe->slice_type = SLICE_P;
		lframe->avg_dist = cs.avg_dist;
		lframe->chroma_weight = cs.chroma_weight;
		lframe->sub_y = arena + cs.sub_y;
		lframe->sub_c[0] = arena + cs.sub_c[0];
		lframe->sub_c[1] = arena + cs.sub_c[1];
		// (what get_merge_candidates leaves in the worker: the list; its inter_modes are the caller's local)
		lw->merge_cands.num = CFG_NUM_MERGE_CAND;
		for (int k = 0; k < CFG_NUM_MERGE_CAND; k++) {
			lw->merge_cands.mv[k].x = cs.mv[k][0];
			lw->merge_cands.mv[k].y = cs.mv[k][1];
			lw->merge_cands.ref_idx[k] = cs.ref_idx[k];
		}
	}
	// what ctu_begin gives the context for a CTU (enc_ctu.h): no neighbour CTUs
	e.node_quad = ni >= NODES_RESIDENT ? node_quadrant(ni) : -1;
	e.scratch_a = lw->pred_aux;
	e.scratch_b = lw->delta_u;
	e.adi_c = lw->adi;
	e.ctu_x = cs.ctu_x;
	e.ctu_y = cs.ctu_y;
	e.nb_ctus = 0;
	e.n_spec_reads = e.n_ratio_cmp = 0;
	e.n_stale_pred = 0;
	e.amvp_node = -1;
	e.last_slog = -1;
	e.inter_ssq[0] = e.inter_ssq[1] = e.inter_ssq[2] = 0xEEEEEEEEu;
	e.inter_ssq_valid = -1;
	g.sync();
	Node &nd = node_of(e, ni);
	const Geo &q = e.geo[ni];
	CtuPublic &c = *e.ctu;
	const int n = q.size, nc = q.size_chroma, depth = q.depth, units = q.num_part, abs_index = q.abs_index;
	// the planted values: the node, the per-depth buffers, the record's cbf
	static_assert(sizeof(Node) % 4 == 0, "the node is planted in words");
	if (g.tid < (int)(sizeof(Node) / 4)) ((uint32_t *)&nd)[g.tid] = 0xEEEEEEEEu;
	g.sync();
	if (g.tid == 0) {
		nd.qp = (uint8_t)cs.qp;
		nd.inter_ref_index = (int8_t)cs.old_ref_index;
	}
	if (merge && g.tid < units) {
		const int a = abs_index + g.tid;
		for (int k = 0; k < 2; k++) lw->intra_mode_buffs[k][depth][a] = (uint8_t)(0x40 + 0x20 * k + (g.tid & 15));
		for (int k = 0; k < 3; k++) {
			lw->cbf_buffs[k][depth][a] = 0x77;
			c.cbf[k][a] = (uint8_t)(0xa0 + k);
		}
		lw->tr_idx_buffs[depth][a] = 0x77;
	}
	// the helper takes the CTU: it copies the worker's context (enc_ctu.h ctu_begin)
	g.sync();
	helper_post(g, e, 0, HJOB_NEW_CTU);
	helper_wait(g, e, 0);

	int slots = -1;
	uint32_t best = 0;
	if (merge) {
#if defined(HENC_QUAD)
		// check_rd_cost_merge, enc_ctu.h: the three statements behind get_merge_candidates
		uint8_t inter_modes[5] = {(uint8_t)uni(cs.inter_modes[0]), (uint8_t)uni(cs.inter_modes[1]), 255, 255, 255};
		const QuadCands mc = quad_load_cands(e);
		slots = q.size == 8 ? quad_prepare<8>(g, e, ni, mc HENC_QPROF_PASS) : (q.size == 16 ? quad_prepare<16>(g, e, ni, mc HENC_QPROF_PASS) : -1);
		if (slots >= 0) best = q.size == 8 ? quad_merge_loop<8>(g, e, ni, slots, mc, inter_modes HENC_QPROF_PASS) : quad_merge_loop<16>(g, e, ni, slots, mc, inter_modes HENC_QPROF_PASS);
#endif
	} else {
		const MV mv = {uni(cs.mv[0][0]), uni(cs.mv[0][1])};
		motion_compensate_cu(g, e, ni, mv);
	}
	g.sync();
	// copy out; the CU's blocks of the four windows and its entries of the record get their poison back
	if (merge) {
		if (g.tid == 0) {
			o.slots = slots; o.ret = best;
			o.skipped = nd.skipped; o.inter_mv[0] = nd.inter_mv.x; o.inter_mv[1] = nd.inter_mv.y; o.inter_ref_index = nd.inter_ref_index;
			o.cost = nd.cost; o.distortion = nd.distortion;
			o.merge_flag = nd.merge_flag; o.merge_idx = nd.merge_idx; o.inter_mode = nd.inter_mode; o.sum = nd.sum;
			for (int k = 0; k < 3; k++) { o.inter_cbf[k] = nd.inter_cbf[k]; o.inter_ssq[k] = e.inter_ssq[k]; }
			o.inter_tr_idx = nd.inter_tr_idx;
			o.inter_ssq_valid = e.inter_ssq_valid;
		}
		if (g.tid < units) {
			const int u = g.tid, a = abs_index + u;
			const uint8_t pz = merge_poison_byte(a);
			for (int k = 0; k < 3; k++) { o.cbf_buffs[k][u] = lw->cbf_buffs[k][depth][a]; o.rec_cbf[k][u] = c.cbf[k][a]; c.cbf[k][a] = pz; }
			o.tr_idx_buffs[u] = lw->tr_idx_buffs[depth][a];
			o.rec_tr_idx[u] = c.tr_idx[a]; c.tr_idx[a] = pz;
			for (int k = 0; k < 2; k++) { o.rec_intra_mode[k][u] = c.intra_mode[k][a]; c.intra_mode[k][a] = pz; }
			o.rec_mv_ref_idx[u] = c.mv_ref_idx[a]; c.mv_ref_idx[a] = (int8_t)pz;
		}
		for (int wi = 0; wi < 2; wi++) {
			const int wnd = wi == 0 ? depth + 1 : 0;
			int at = 0;
			for (int comp = 0; comp < 3; comp++) {
				const int m = comp ? nc : n, x = comp ? q.xc : q.x, y = comp ? q.yc : q.y, ds = dec_stride(comp);
				int16_t *lev = tq_ptr(*lw, wnd, comp) + (comp ? (abs_index << 4) >> 2 : abs_index << 4), *dec = dec_ptr(*lw, wnd, comp) + y * ds + x;
				for (int k = g.tid; k < m * m; k += 64) {
					o.lv[wi][at + k] = lev[k]; lev[k] = MERGE_POISON16;
					o.dec[wi][at + k] = dec[(k / m) * ds + k % m]; dec[(k / m) * ds + k % m] = MERGE_POISON16;
				}
				at += m * m;
			}
		}
	}
	// the whole prediction window, and the checksum of what lies outside the CU's three blocks
	uint32_t rest = 0;
	const uint8_t *pw = lw->pred_y;
	for (int k = g.tid; k < WALK_WINDOW_BYTES; k += 64) {
		const uint8_t v = pw[k];
		o.pred[k] = v;
		const int comp = k < 4096 ? 0 : 1, kk = comp ? (k - 4096) & 1023 : k, st = comp ? 32 : 64, x = kk % st, y = kk / st;
		const int bx = comp ? q.xc : q.x, by = comp ? q.yc : q.y, m = comp ? nc : n;
		if (!(x >= bx && x < bx + m && y >= by && y < by + m)) rest += (uint32_t)(k + 1) * v;
	}
	rest = g.sum(rest);
	g.sync();
	// stray: whatever else of the windows and of the record does not hold the poison any more
	uint32_t *const slow_words = (uint32_t *)my_slow, *const rec_words = (uint32_t *)(CtuPublic *)my_ctu;
	uint32_t stray = 0;
	for (int i = g.tid; i < (int)(sizeof(WorkSlow) / 4); i += 64)
		if (slow_words[i] != WALK_POISON) { stray++; slow_words[i] = WALK_POISON; }
	for (int i = g.tid; i < (int)(sizeof(CtuPublic) / 4); i += 64)
		if (rec_words[i] != WALK_POISON) { stray++; rec_words[i] = WALK_POISON; }
	stray = g.sum(stray);
	if (g.tid == 0) { o.stray = stray; o.pred_rest = rest; }
	g.sync();
}

// (the register budget of the pool kernels, as k_walk_helpers has it: k_encode_helpertest.inc says why)
__global__ __launch_bounds__(ENC_THREADS) __attribute__((amdgpu_waves_per_eu(HENC_WAVES_PER_EU))) void k_walk_merge(const hmr_gpu_merge_case *cases, int ncases, const uint8_t *arena, const DevTables *tables, WorkSlow *slow, CtuInfo *ctus,
												       hmr_gpu_merge_out *out, unsigned lds_bytes)
{
	if (!rows_enter<false, MergeGrp>(lds_bytes)) return;      // (the helper wavefront: through its loop until release_helpers)
	const MergeGrp g{(int)(threadIdx.x & 63)};
	WorkSlow *const my_slow = slow + blockIdx.x;
	CtuInfo *const my_ctu = ctus + blockIdx.x;
	uint32_t *const slow_words = (uint32_t *)my_slow, *const rec_words = (uint32_t *)(CtuPublic *)my_ctu;
	for (int i = g.tid; i < (int)(sizeof(WorkSlow) / 4); i += 64) slow_words[i] = WALK_POISON;
	for (int i = g.tid; i < (int)(sizeof(CtuPublic) / 4); i += 64) rec_words[i] = WALK_POISON;
	g.sync();
	// the worker's context, as encode_row builds it, on the workgroup's one CTU record
	Enc &e = lds_enc();
	HENC_ENC_IN_LDS(e);
	enc_prepare(e, tables, my_ctu, nullptr);
	e.ctu = my_ctu;
	e.ctu_g = my_ctu;
	e.coeff = nullptr;
	g.sync();
	for (int ci = (int)blockIdx.x; ci < ncases; ci += (int)gridDim.x) merge_run_case(g, e, cases[ci], out[ci], arena, my_slow, my_ctu);
	int hseq[NHELP];
	for (int h = 0; h < NHELP; h++) hseq[h] = e.hseq[h];
	release_helpers(hseq);
}

// every address the step of a case can form lies inside what it was given, and nothing can make the worker leave its loop early
const char *merge_case_refused(const hmr_gpu_merge_case &c, const Geo *geo, size_t arena_bytes)
{
	if (c.step != HMR_GPU_MERGE_MERGE && c.step != HMR_GPU_MERGE_MC) return "step";
	if (NHELP != 1) return "step (the library was built with a helper per chroma plane)";
	const bool merge = c.step == HMR_GPU_MERGE_MERGE;
#if !defined(HENC_QUAD)
	if (merge) return "step (the library was built without the merge tiles)";
#endif
	if (c.node < 0 || c.node >= NNODES) return "node";
	const Geo &q = geo[c.node];
	if (merge && q.size != 8 && q.size != 16) return "node (MERGE: an 8 x 8 or 16 x 16 CU)";
	if (!merge && q.size < 8) return "node (MC: a CU of 8 to 64)";
	if (c.qp < 0 || c.qp > 51) return "qp";
	if (c.perf_mode < 0 || c.perf_mode > 3) return "perf_mode";
	if (c.chroma_qp_offset < -12 || c.chroma_qp_offset > 12) return "chroma_qp_offset";
	if (c.sign_hiding != 0 && c.sign_hiding != 1) return "sign_hiding";
	if (!(c.avg_dist >= 0.) || !(c.avg_dist <= 1e12) || !(c.chroma_weight > 0.) || !(c.chroma_weight <= 1e3)) return "avg_dist / chroma_weight";
	if (c.ctu_x < 0 || c.ctu_y < 0 || c.ctu_x % 64 || c.ctu_y % 64 || c.ctu_x > 8192 || c.ctu_y > 8192) return "ctu_x / ctu_y";
	if (c.width < 8 || c.height < 8 || c.width > 8192 + 64 || c.height > 8192 + 64 || c.margin < 0 || c.margin > 1024) return "width / height / margin";
	if (c.stride_y <= 0 || c.stride_c <= 0 || c.stride_y > (1 << 20) || c.stride_c > (1 << 20)) return "stride";
	if (c.reserved[0] || c.reserved[1]) return "reserved";
	for (int k = 0; k < 2; k++) {
		if (c.mv[k][0] < -(1 << 15) || c.mv[k][0] >= (1 << 15) || c.mv[k][1] < -(1 << 15) || c.mv[k][1] >= (1 << 15)) return "mv";
		if (c.ref_idx[k] < -1 || c.ref_idx[k] > 15) return "ref_idx";
		if (c.inter_modes[k] < 0 || c.inter_modes[k] > 255) return "inter_modes";
	}
	if (c.old_ref_index < -128 || c.old_ref_index > 127) return "old_ref_index";
	if (!help_piece_inside(c.curr, WALK_WINDOW_BYTES, arena_bytes)) return "curr";
	if (!help_piece_inside(c.pred, WALK_WINDOW_BYTES, arena_bytes)) return "pred";
	// the phase-plane addressing of section 13 (quad_chain, motion_compensate_cu): every candidate's three blocks (MC: mv[0]'s), whether or not quad_prepare takes the CU
	for (int k = 0; k < (merge ? 2 : 1); k++) {
		const int mx = c.mv[k][0], my = c.mv[k][1];
		const int64_t sy = 16 * (int64_t)c.stride_y, sc = 64 * (int64_t)c.stride_c;
		const int64_t base = c.sub_y + (((my & 3) << 2) | (mx & 3)) * (int64_t)c.stride_y + (int64_t)(c.ctu_y + q.y + (my >> 2)) * sy + c.ctu_x + q.x + (mx >> 2);
		if (!walk_block_inside(base, sy, q.size, arena_bytes)) return "a luma prediction block outside the arena";
		const int64_t oc = (((my & 7) << 3) | (mx & 7)) * (int64_t)c.stride_c + (int64_t)((c.ctu_y >> 1) + q.yc + (my >> 3)) * sc + (c.ctu_x >> 1) + q.xc + (mx >> 3);
		for (int p = 0; p < 2; p++)
			if (!walk_block_inside(c.sub_c[p] + oc, sc, q.size_chroma, arena_bytes)) return "a chroma prediction block outside the arena";
	}
	return nullptr;
}

}  // namespace

extern "C" int hmr_gpu_walk_merge_forms(const hmr_gpu_merge_case *cases, int ncases, const uint8_t *arena, size_t arena_bytes, hmr_gpu_merge_out *out)
{
	if (!cases || ncases < 1 || ncases > (1 << 16) || !arena || !arena_bytes || !out) {
		hmr_set_error("hmr_gpu_walk_merge_forms: NULL argument or ncases outside 1 .. 2^16");
		return HMR_GPU_ERR_ARG;
	}
	std::vector<Geo> geo(NNODES);
	make_geo(geo.data());
	for (int i = 0; i < ncases; i++) {
		const char *why = merge_case_refused(cases[i], geo.data(), arena_bytes);
		if (why) {
			hmr_set_error("hmr_gpu_walk_merge_forms: case %d refused: %s", i, why);
			return HMR_GPU_ERR_ARG;
		}
	}
	hmr_gpu_ctx *c = hmr_default_ctx();
	if (!c) {
		hmr_set_error("hmr_gpu_walk_merge_forms: no device");
		return HMR_GPU_ERR_NO_DEVICE;
	}
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(henc_geo_table), geo.data(), sizeof(Geo) * NNODES));
	const unsigned lds_bytes = (unsigned)lds_request(false);
	HIP_TRY(hipFuncSetAttribute((const void *)k_walk_merge, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
	const int groups = ncases < MERGE_MAX_GROUPS ? ncases : MERGE_MAX_GROUPS;
	struct Bufs {
		void *p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
		~Bufs() { for (void *q : p) if (q) (void)hipFree(q); }
	} b;
	const size_t case_bytes = sizeof(hmr_gpu_merge_case) * (size_t)ncases, out_bytes = sizeof(hmr_gpu_merge_out) * (size_t)ncases;
	HIP_TRY(hipMalloc(&b.p[0], case_bytes));
	HIP_TRY(hipMalloc(&b.p[1], arena_bytes + 64));
	HIP_TRY(hipMalloc(&b.p[2], sizeof(WorkSlow) * (size_t)groups));
	HIP_TRY(hipMalloc(&b.p[3], out_bytes));
	HIP_TRY(hipMalloc(&b.p[4], sizeof(CtuInfo) * (size_t)groups));
	HIP_TRY(hipMemcpyAsync(b.p[0], cases, case_bytes, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(b.p[1], arena, arena_bytes, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemsetAsync(b.p[3], 0, out_bytes, c->stream));
	HIP_TRY(hipMemsetAsync(b.p[4], 0, sizeof(CtuInfo) * (size_t)groups, c->stream));
	hipLaunchKernelGGL(k_walk_merge, dim3(groups), dim3(ENC_THREADS), lds_bytes, c->stream, (const hmr_gpu_merge_case *)b.p[0], ncases, (const uint8_t *)b.p[1], (const DevTables *)c->tables,
			   (WorkSlow *)b.p[2], (CtuInfo *)b.p[4], (hmr_gpu_merge_out *)b.p[3], lds_bytes);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, b.p[3], out_bytes, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return HMR_GPU_OK;
}
