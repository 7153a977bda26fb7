// Test aid (include/homer_gpu.h section 18): the worker / helper-wavefront protocol and what runs behind it, one step at a time with real helper wavefronts.
//
// Every `if (HENC_HELPERS(e))` branch of enc/enc_intra.h, enc/enc_ctu.h and enc/enc_common.h, the job bodies of helper_serve (the both-planes SSD has no other copy), the
// helper loops and the background intra search (bg_post / bg_take / bg_quiesce, helper_bg_search) exist on the device only: the one-lane checker build has none of them.
// k_walk_forms (section 16) fakes a helper's context on one wavefront and never touches the mailbox.  Here a workgroup is what it is in k_encode_pool - a worker wavefront
// and its helper wavefront, the same LDS places, entered through rows_enter and left through release_helpers - and the worker runs single steps of the walk on given
// input, posting to and waiting for the real helper.
//
// What keeps the harness from hanging: it has no wait loop of its own - it waits through helper_wait, bg_take and bg_quiesce only; every helper_post is followed by its
// helper_wait before the next post, every background step ends with bg_take or bg_quiesce; the worker has no way out of its loop over the cases but its end (no return,
// no continue between rows_enter and release_helpers - whatever could make it leave early is refused on the host before the launch).

namespace {

static_assert(sizeof(hmr_gpu_helper_case) == 216 && sizeof(hmr_gpu_helper_out) == 12064, "include/homer_gpu.h section 18 states these layouts");
static_assert(sizeof(((Work *)nullptr)->cbf_chroma) == 512 && sizeof(((Work *)nullptr)->adi) == 528 && sizeof(((Work *)nullptr)->srch_sads) == 40 && sizeof(((Work *)nullptr)->srch_modes) == 24,
	      "hmr_gpu_helper_out mirrors these members of Work");
// The groups of the steps: types of the harness's own, as WalkGrp is one (k_encode_walktest.inc says why) - the worker's walk of the plain launch, the worker's walk of
// the launch with the latency kernel's helper loop (G::bg: compiled with the background-search hooks), and the plain helper loop with everything helper_serve calls.
struct HelpGrp : WaveGrp {};
struct HelpGrpLat : WaveGrpLat {};
constexpr int HELP_MAX_GROUPS = 96, HELP_SYNC_SRC = 0, HELP_SYNC_DST = NWND - 1;      // (a SYNC job of a background step copies window 0 to the auxiliary window)
constexpr int16_t HELP_POISON16 = 0x1234;

// the 4 n + 1 places around an n x n block at `blk` (row pitch st) in the order of section 18's nbr: the column left of it, the corner, the row above it
__device__ __forceinline__ int16_t *help_nbr_place(int16_t *blk, int st, int n, int k)
{
	return k < 2 * n ? blk + k * st - 1 : (k == 2 * n ? blk - st - 1 : blk - st + (k - 2 * n - 1));
}

template <class G>
__device__ __forceinline__ void help_run_case(const G g, Enc &__restrict__ e, const hmr_gpu_helper_case &cs, hmr_gpu_helper_out &o, const uint8_t *arena, WorkSlow *my_slow)
{
	HENC_ENC_IN_LDS(e);
	Work *lw = lds_work();
	Seq *lseq = lds_seq();
	FrameCtx *lframe = lds_frame();
	const int step = uni(cs.step), ni = uni(cs.node);
	const bool luma_step = step == HMR_GPU_HELPER_INTRA_SEARCH || step == HMR_GPU_HELPER_INTRA_SEARCH_BG;
	int job[4];
	bool job_sync = false, job_tu = false;
	for (int k = 0; k < 4; k++) {
		job[k] = step == HMR_GPU_HELPER_INTRA_SEARCH_BG ? uni(cs.jobs[k]) : HMR_GPU_HELPER_JOB_NONE;
		job_sync |= job[k] == HMR_GPU_HELPER_JOB_SYNC;
		job_tu |= job[k] == HMR_GPU_HELPER_JOB_INTER_TU;
	}
	// the worker's LDS below the mailbox starts from zero, as rows_enter left it (the helper is idle: every job has been waited for, no background search is outstanding);
	// the mailbox and the contexts keep their sequence numbers
	lds_zero(LDS_OFF_BOX, g.tid, 64);
	g.sync();
	if (cs.curr >= 0) wave_copy_words(lw->curr_y, arena + cs.curr, WALK_WINDOW_BYTES, g.tid);
	if (cs.pred >= 0) wave_copy_words(lw->pred_y, arena + cs.pred, WALK_WINDOW_BYTES, g.tid);
	if (g.tid == 0) {
		lw->slow = (HENC_GLOBAL_PTR(WorkSlow))my_slow;
		lw->thread_seen_intra = cs.seen_intra;
		lseq->width = cs.width;
		lseq->height = cs.height;
		lseq->wctu = (cs.width + 63) >> 6;
		lseq->hctu = (cs.height + 63) >> 6;
		lseq->strong_intra = cs.strong_intra;
		lseq->rd_mode = cs.rd_mode;
		lseq->sign_hiding = cs.sign_hiding;
		lseq->chroma_qp_offset = cs.chroma_qp_offset;
		lseq->perf_mode = 1;
		lframe->slice_type = cs.slice_type;
		lframe->sqrt_lambda = cs.sqrt_lambda;
		lframe->chroma_weight = cs.chroma_weight;
		lframe->avg_dist = cs.avg_dist;
	}
	// what ctu_begin gives the context for a CTU (enc_ctu.h): no neighbour CTUs - a node on the CTU's edge has no neighbour directions
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
	g.sync();
	Node &nd = node_of(e, ni);
	const Geo &q = e.geo[ni];
	const int n = q.size, nc = q.size_chroma, depth = q.depth, coff = (q.abs_index << 4) >> 2;
	if (g.tid == 0) {
		nd.left_nb = (uint8_t)cs.nb[0]; nd.top_nb = (uint8_t)cs.nb[1]; nd.left_bottom_nb = (uint8_t)cs.nb[2]; nd.top_right_nb = (uint8_t)cs.nb[3];
		nd.qp = (uint8_t)cs.qp;
		// the directions of the units left of and above the node, where the worker's mode buffer of the node's depth holds them (intra_neighbour_dirs, read_mode_buff)
		if (luma_step && q.x > 0) lw->intra_mode_buffs[COMP_Y][depth][q.abs_left] = (uint8_t)cs.nb_dir[0];
		if (luma_step && q.y > 0) lw->intra_mode_buffs[COMP_Y][depth][q.abs_top] = (uint8_t)cs.nb_dir[1];
	}
	// the decoded samples around the block, in the window the step reads
	const int16_t *nbr = cs.nbr >= 0 ? (const int16_t *)(arena + cs.nbr) : nullptr;
	int16_t *const blk_y = dec_ptr(*lw, depth + 1, COMP_Y) + q.y * DEC_STRIDE_Y + q.x;
	int16_t *const blk_c[2] = {dec_ptr(*lw, NWND - 1, COMP_U) + q.yc * DEC_STRIDE_C + q.xc, dec_ptr(*lw, NWND - 1, COMP_V) + q.yc * DEC_STRIDE_C + q.xc};
	if (nbr && luma_step)
		for (int k = g.tid; k < 4 * n + 1; k += 64) *help_nbr_place(blk_y, DEC_STRIDE_Y, n, k) = nbr[k];
	if (nbr && !luma_step)
		for (int k = g.tid; k < 2 * (4 * nc + 1); k += 64) {
			const int c = k >= 4 * nc + 1;
			*help_nbr_place(blk_c[c], DEC_STRIDE_C, nc, k - c * (4 * nc + 1)) = nbr[k];
		}
	// the source windows of a SYNC_UV step / a SYNC job: the levels (linear) and the reconstruction (in the window) of both chroma planes
	const bool syncs = step == HMR_GPU_HELPER_SYNC_UV || job_sync;
	const int q_src = step == HMR_GPU_HELPER_SYNC_UV ? uni(cs.wnd[0]) : HELP_SYNC_SRC, q_dst = step == HMR_GPU_HELPER_SYNC_UV ? uni(cs.wnd[1]) : HELP_SYNC_DST;
	const int d_src = step == HMR_GPU_HELPER_SYNC_UV ? uni(cs.wnd[2]) : HELP_SYNC_SRC, d_dst = step == HMR_GPU_HELPER_SYNC_UV ? uni(cs.wnd[3]) : HELP_SYNC_DST;
	if (syncs) {
		const int16_t *sy = (const int16_t *)(arena + cs.sync);
		for (int i = g.tid; i < 2 * nc * nc; i += 64) {
			const int c = i >= nc * nc, j = i - c * nc * nc;
			(tq_ptr(*lw, q_src, COMP_U + c) + coff)[j] = sy[i];
			(dec_ptr(*lw, d_src, COMP_U + c) + q.yc * DEC_STRIDE_C + q.xc)[(j / nc) * DEC_STRIDE_C + j % nc] = sy[2 * nc * nc + i];
		}
	}
	// the helper takes the CTU: it copies the worker's context (enc_ctu.h ctu_begin)
	g.sync();
	helper_post(g, e, 0, HJOB_NEW_CTU);
	helper_wait(g, e, 0);

	// (the launch with the latency kernel's helper loop gets the steps with a background search and no others: each kernel carries the steps it runs)
	if (luma_step) {
		int mode = 0, bits = 0, taken = -1;
		double cost = 0;
		if constexpr (G::bg) {
			const int bg_ni = uni(cs.bg_node), variant = uni(cs.bg_variant);
			bg_post(g, e, bg_ni, e.geo[bg_ni].depth);      // (enc_ctu.h, the P-slice walk after the merge evaluation: bg_post(g, e, curr, curr_depth))
			for (int k = 0; k < 4; k++) {
				// the chroma jobs of the inter evaluation, each waited for before the next (enc_ctu.h skip evaluation, enc_inter.h transform tree, enc_common.h sync_motion_buffers)
				if (job[k] == HMR_GPU_HELPER_JOB_SSD) helper_post(g, e, 0, HJOB_SSD, ni, COMP_UV);
				else if (job[k] == HMR_GPU_HELPER_JOB_INTER_TU) helper_post(g, e, 0, HJOB_INTER_TU, ni, COMP_UV, depth, PART_2Nx2N);
				else if (job[k] == HMR_GPU_HELPER_JOB_SYNC) helper_post(g, e, 0, HJOB_SYNC_CU, ni, COMP_UV, q_src, q_dst, d_src, d_dst);
				if (job[k] != HMR_GPU_HELPER_JOB_NONE) {
					helper_wait(g, e, 0);
					if (g.tid < 6) o.job_r[k][g.tid] = e.box->r[0][g.tid];
				}
			}
			// (enc_intra.h encode_intra_luma: the search the helper ran, or the worker's own)
			if (variant == HMR_GPU_HELPER_BG_QUIESCE) bg_quiesce(g, e);
			else taken = bg_take(g, e, ni, &mode, &bits) ? 1 : 0;
		}
		if (taken == 1) { cost = 0; e.last_slog = -1; }
		else bits = intra_mode_search(g, e, ni, depth, &mode, &cost);
		g.sync();
		if (g.tid == 0) {
			o.mode = mode; o.bits = bits; o.taken = taken; o.last_slog = e.last_slog;
			o.cost_bits = (uint64_t)__double_as_longlong(cost);
		}
		if (g.tid < 5) o.srch_sads[g.tid] = lw->srch_sads[g.tid];
		if (g.tid < 6) o.srch_modes[g.tid] = lw->srch_modes[g.tid];
		for (int i = g.tid; i < 264; i += 64) { o.adi[i] = lw->adi[i]; o.adi_f[i] = lw->adi_f[i]; }
	} else if (G::bg) {
	} else if (step == HMR_GPU_HELPER_CHROMA_SEARCH) {
		// enc_intra.h encode_intra_chroma, the candidate search with a helper wavefront: U there, V here
		uint32_t sad_u[5], sad_v[5];
		int cand[5];
		for (int mi = 0; mi < 5; mi++) cand[mi] = uni(cs.cand[mi]);
		helper_post(g, e, 0, HJOB_CHROMA_SEARCH, ni, COMP_U, cand[0] | (cand[1] << 8) | (cand[2] << 16) | (cand[3] << 24), cand[4]);
		chroma_search_comp(g, e, ni, COMP_V, cand, sad_v);
		helper_wait(g, e, 0);
		for (int mi = 0; mi < 5; mi++) sad_u[mi] = e.box->r[0][mi];
		if (g.tid == 0)
			for (int mi = 0; mi < 5; mi++) { o.sad_u[mi] = sad_u[mi]; o.sad_v[mi] = sad_v[mi]; }
	} else if (step == HMR_GPU_HELPER_CHROMA_TU) {
		// enc_intra.h encode_intra_chroma, one TU of the winner with a helper wavefront: U there in the helper's own scratch, V here
		const int cu_mode = uni(cs.cu_mode);
		const int qp_chroma = chroma_qp_table((int)nd.qp + lseq->chroma_qp_offset);
		const int per = qp_chroma / 6, rem = qp_chroma % 6;
		const int scan_mode = find_scan_mode(1, 0, nc, cu_mode, 0);
		const int shifts = uni(cs.cbf_shift[0]) | (uni(cs.cbf_shift[1]) << 8);
		int sums[2], pc[2];
		helper_post(g, e, 0, HJOB_CHROMA_TU, ni, COMP_U, cu_mode, scan_mode, shifts, per | (rem << 8));
		pc[1] = chroma_tu_comp(g, e, ni, COMP_V, cu_mode, scan_mode, shifts, per, rem, &sums[1]);
		helper_wait(g, e, 0);
		pc[0] = (int)e.box->r[0][0];
		sums[0] = (int)e.box->r[0][1];
		g.sync();
		if (g.tid < 2) { o.tu_dist[g.tid] = pc[g.tid]; o.tu_sum[g.tid] = sums[g.tid]; }
		for (int i = g.tid; i < 512; i += 64) (&o.cbf_chroma[0][0])[i] = (&lw->cbf_chroma[0][0])[i];
		// prediction, levels and reconstruction of both planes; the windows get their poison back
		for (int i = g.tid; i < 2 * nc * nc; i += 64) {
			const int c = i >= nc * nc, j = i - c * nc * nc;
			int16_t *lev = tq_ptr(*lw, NWND - 1, COMP_U + c) + coff + j, *rec = blk_c[c] + (j / nc) * DEC_STRIDE_C + j % nc;
			o.pred[c][j] = pred_ptr(*lw, COMP_U + c)[(q.yc + j / nc) * CTU_STRIDE_C + q.xc + j % nc];
			o.lv[c][j] = *lev;
			o.rec[c][j] = *rec;
			*lev = HELP_POISON16;
			*rec = HELP_POISON16;
		}
	} else if (step == HMR_GPU_HELPER_SSD_UV) {
		// enc_ctu.h, the skip evaluation of a merge candidate: both chroma planes on the helper, luma here
		helper_post(g, e, 0, HJOB_SSD, ni, COMP_UV);
		const uint32_t dist = blk_ssd(g, lw->curr_y + q.y * 64 + q.x, 64, lw->pred_y + q.y * 64 + q.x, 64, n);
		helper_wait(g, e, 0);
		if (g.tid == 0) { o.ssd[0] = e.box->r[0][0]; o.ssd[1] = e.box->r[0][1]; o.ssd[2] = dist; }
	} else {
		// enc_common.h sync_motion_buffers as the walk calls it: HJOB_SYNC_CU for both chroma planes, luma here
		sync_motion_buffers(g, e, ni, q_src, q_dst, d_src, d_dst);
	}
	g.sync();
	// what a SYNC step or job left in the destination windows; source and destination blocks get their poison back
	if (syncs)
		for (int i = g.tid; i < 2 * nc * nc; i += 64) {
			const int c = i >= nc * nc, j = i - c * nc * nc, at = (j / nc) * DEC_STRIDE_C + j % nc;
			int16_t *lev = tq_ptr(*lw, q_dst, COMP_U + c) + coff + j, *rec = dec_ptr(*lw, d_dst, COMP_U + c) + q.yc * DEC_STRIDE_C + q.xc + at;
			o.lv[c][j] = *lev;
			o.rec[c][j] = *rec;
			*lev = HELP_POISON16;
			*rec = HELP_POISON16;
			(tq_ptr(*lw, q_src, COMP_U + c) + coff)[j] = HELP_POISON16;
			(dec_ptr(*lw, d_src, COMP_U + c) + q.yc * DEC_STRIDE_C + q.xc)[at] = HELP_POISON16;
		}
	// the blocks an INTER_TU job wrote (the windows of the TU's depth)
	if (job_tu)
		for (int i = g.tid; i < 2 * nc * nc; i += 64) {
			const int c = i >= nc * nc, j = i - c * nc * nc;
			(tq_ptr(*lw, depth + 1, COMP_U + c) + coff)[j] = HELP_POISON16;
			(dec_ptr(*lw, depth + 1, COMP_U + c) + q.yc * DEC_STRIDE_C + q.xc)[(j / nc) * DEC_STRIDE_C + j % nc] = HELP_POISON16;
		}
	if (nbr && luma_step)
		for (int k = g.tid; k < 4 * n + 1; k += 64) *help_nbr_place(blk_y, DEC_STRIDE_Y, n, k) = HELP_POISON16;
	if (nbr && !luma_step)
		for (int k = g.tid; k < 2 * (4 * nc + 1); k += 64) {
			const int c = k >= 4 * nc + 1;
			*help_nbr_place(blk_c[c], DEC_STRIDE_C, nc, k - c * (4 * nc + 1)) = HELP_POISON16;
		}
	g.sync();
	// stray: whatever else of the windows does not hold the poison any more
	uint32_t *const slow_words = (uint32_t *)my_slow;
	uint32_t stray = 0;
	for (int i = g.tid; i < (int)(sizeof(WorkSlow) / 4); i += 64)
		if (slow_words[i] != WALK_POISON) { stray++; slow_words[i] = WALK_POISON; }
	stray = g.sum(stray);
	if (g.tid == 0) o.stray = stray;
	g.sync();
}

// list: the indices of the cases of this launch (LAT: the steps with a background search, on the latency kernel's helper loop; else the others, on the plain loop)
template <class G, bool LAT>
__device__ __forceinline__ void walk_helpers_body(const hmr_gpu_helper_case *cases, const int *list, int nlist, const uint8_t *arena, const DevTables *tables, WorkSlow *slow, CtuInfo *ctus,
						  hmr_gpu_helper_out *out, unsigned lds_bytes)
{
	if (!rows_enter<LAT, typename std::conditional<LAT, WaveGrp, HelpGrp>::type>(lds_bytes)) return;      // (the helper wavefront: through its loop until release_helpers)
	const G g{(int)(threadIdx.x & 63)};
	WorkSlow *const my_slow = slow + blockIdx.x;
	CtuInfo *const my_ctu = ctus + blockIdx.x;
	uint32_t *const slow_words = (uint32_t *)my_slow;
	for (int i = g.tid; i < (int)(sizeof(WorkSlow) / 4); i += 64) slow_words[i] = WALK_POISON;
	g.sync();
	// the worker's context, as encode_row builds it, on the workgroup's one CTU record
	Enc &e = lds_enc();
	HENC_ENC_IN_LDS(e);
	enc_prepare(e, tables, my_ctu, nullptr);
	e.ctu = my_ctu;
	e.ctu_g = my_ctu;
	e.coeff = nullptr;
	g.sync();
	for (int k = (int)blockIdx.x; k < nlist; k += (int)gridDim.x) {
		const int ci = uni(list[k]);
		help_run_case(g, e, cases[ci], out[ci], arena, my_slow);
	}
	int hseq[NHELP];
	for (int h = 0; h < NHELP; h++) hseq[h] = e.hseq[h];
	release_helpers(hseq);
}

// (the register budget of the pool kernels: the out-of-line functions these launches share with them - helper_loop<true>, helper_serve_out, helper_bg_search - are compiled
// for the loosest budget among their callers'; without the attribute here k_encode_full, k_encode_pool_lat and k_encode_ctus came out with accumulation registers and half
// the occupancy)
__global__ __launch_bounds__(ENC_THREADS) __attribute__((amdgpu_waves_per_eu(HENC_WAVES_PER_EU))) void k_walk_helpers(const hmr_gpu_helper_case *cases, const int *list, int nlist, const uint8_t *arena, const DevTables *tables, WorkSlow *slow,
							      CtuInfo *ctus, hmr_gpu_helper_out *out, unsigned lds_bytes)
{
	walk_helpers_body<HelpGrp, false>(cases, list, nlist, arena, tables, slow, ctus, out, lds_bytes);
}
__global__ __launch_bounds__(ENC_THREADS) __attribute__((amdgpu_waves_per_eu(HENC_WAVES_PER_EU))) void k_walk_helpers_lat(const hmr_gpu_helper_case *cases, const int *list, int nlist, const uint8_t *arena, const DevTables *tables, WorkSlow *slow,
								  CtuInfo *ctus, hmr_gpu_helper_out *out, unsigned lds_bytes)
{
	walk_helpers_body<HelpGrpLat, true>(cases, list, nlist, arena, tables, slow, ctus, out, lds_bytes);
}

// [at, at + bytes) lies inside the arena and starts at a multiple of 4
bool help_piece_inside(int64_t at, size_t bytes, size_t arena_bytes) { return at >= 0 && at % 4 == 0 && (uint64_t)at + bytes <= (uint64_t)arena_bytes; }
bool help_block_in_picture(const hmr_gpu_helper_case &c, const Geo &q) { return c.ctu_x + q.x + q.size <= c.width && c.ctu_y + q.y + q.size <= c.height; }

// every address the step of a case can form lies inside what it was given, and nothing can make the worker leave its loop early
const char *helper_case_refused(const hmr_gpu_helper_case &c, const Geo *geo, size_t arena_bytes)
{
	if (c.step < HMR_GPU_HELPER_INTRA_SEARCH || c.step > HMR_GPU_HELPER_SYNC_UV) return "step";
	if (NHELP != 1) return "step (the library was built with a helper per chroma plane)";
	const bool luma = c.step == HMR_GPU_HELPER_INTRA_SEARCH || c.step == HMR_GPU_HELPER_INTRA_SEARCH_BG, bg = c.step == HMR_GPU_HELPER_INTRA_SEARCH_BG;
	if (c.node < 0 || c.node >= NNODES) return "node";
	const Geo &q = geo[c.node];
	bool any_job = false, tu_job = false, sync_job = false, ssd_job = false;
	for (int k = 0; k < 4; k++) {
		if (c.jobs[k] < HMR_GPU_HELPER_JOB_NONE || c.jobs[k] > HMR_GPU_HELPER_JOB_SYNC || (!bg && c.jobs[k] != HMR_GPU_HELPER_JOB_NONE)) return "jobs";
		any_job |= c.jobs[k] != HMR_GPU_HELPER_JOB_NONE;
		tu_job |= c.jobs[k] == HMR_GPU_HELPER_JOB_INTER_TU;
		sync_job |= c.jobs[k] == HMR_GPU_HELPER_JOB_SYNC;
		ssd_job |= c.jobs[k] == HMR_GPU_HELPER_JOB_SSD;
	}
	if ((!luma || any_job) && q.size < 8) return "node (a chroma step needs a CU of 8 or more)";
	if (tu_job && q.size > 32) return "node (an INTER_TU job: a CU of 8 to 32)";
	if (bg) {
		if (c.bg_variant < HMR_GPU_HELPER_BG_TAKE || c.bg_variant > HMR_GPU_HELPER_BG_QUIESCE) return "bg_variant";
		if (c.bg_node < 0 || c.bg_node >= NNODES) return "bg_node";
		if (c.bg_variant == HMR_GPU_HELPER_BG_TAKE_OTHER ? (c.bg_node == c.node || geo[c.bg_node].depth != q.depth) : c.bg_node != c.node) return "bg_node";
	} else if (c.bg_variant != 0 || c.bg_node != 0) return "bg_variant";
	if (c.ctu_x < 0 || c.ctu_y < 0 || c.ctu_x % 64 || c.ctu_y % 64 || c.ctu_x > 8192 || c.ctu_y > 8192) return "ctu_x / ctu_y";
	if (c.width < 8 || c.height < 8 || c.width % 8 || c.height % 8 || c.width > 8192 + 64 || c.height > 8192 + 64 || !help_block_in_picture(c, q)) return "width / height";
	if (bg && !help_block_in_picture(c, geo[c.bg_node])) return "width / height";
	for (int k = 0; k < 4; k++)
		if (c.nb[k] != 0 && c.nb[k] != 1) return "nb";
	if ((c.strong_intra != 0 && c.strong_intra != 1) || (c.rd_mode != RDM_DIST_ONLY && c.rd_mode != RDM_FAST) || (c.seen_intra != 0 && c.seen_intra != 1)) return "strong_intra / rd_mode / seen_intra";
	if (luma) {
		if (q.x > 0 ? (c.nb_dir[0] < 0 || c.nb_dir[0] > 34) : c.nb_dir[0] != -1) return "nb_dir";
		if (q.y > 0 ? (c.nb_dir[1] < 0 || c.nb_dir[1] > 34) : c.nb_dir[1] != -1) return "nb_dir";
		if (!(c.sqrt_lambda >= 0.) || !(c.sqrt_lambda <= 1e6)) return "sqrt_lambda";
	}
	if (c.qp < 0 || c.qp > 51) return "qp";
	if (c.chroma_qp_offset < -12 || c.chroma_qp_offset > 12) return "chroma_qp_offset";
	if (c.slice_type != SLICE_P && c.slice_type != SLICE_I && c.slice_type != SLICE_B) return "slice_type";
	if (c.sign_hiding != 0 && c.sign_hiding != 1) return "sign_hiding";
	if (!(c.avg_dist >= 0.) || !(c.avg_dist <= 1e12) || !(c.chroma_weight > 0.) || !(c.chroma_weight <= 1e3)) return "avg_dist / chroma_weight";
	if (c.step == HMR_GPU_HELPER_CHROMA_SEARCH)
		for (int k = 0; k < 5; k++)
			if (c.cand[k] < 0 || c.cand[k] > 34) return "cand";
	if (c.step == HMR_GPU_HELPER_CHROMA_TU) {
		if (c.cu_mode < 0 || c.cu_mode > 34) return "cu_mode";
		if (c.cbf_shift[0] < 0 || c.cbf_shift[0] > 4 || c.cbf_shift[1] < 0 || c.cbf_shift[1] > 4) return "cbf_shift";
	}
	if (c.step == HMR_GPU_HELPER_SYNC_UV) {
		for (int k = 0; k < 4; k++)
			if (c.wnd[k] < 0 || c.wnd[k] >= NWND) return "wnd";
		if (c.wnd[0] == c.wnd[1] || c.wnd[2] == c.wnd[3]) return "wnd";
	}
	// the pieces of the arena a step reads
	const bool reads_curr = c.step != HMR_GPU_HELPER_SYNC_UV, reads_pred = c.step == HMR_GPU_HELPER_SSD_UV || tu_job || ssd_job;
	const bool reads_nbr = c.step != HMR_GPU_HELPER_SSD_UV && c.step != HMR_GPU_HELPER_SYNC_UV, reads_sync = c.step == HMR_GPU_HELPER_SYNC_UV || sync_job;
	if (reads_curr ? !help_piece_inside(c.curr, WALK_WINDOW_BYTES, arena_bytes) : c.curr != -1) return "curr";
	if (reads_pred ? !help_piece_inside(c.pred, WALK_WINDOW_BYTES, arena_bytes) : c.pred != -1) return "pred";
	const size_t nbr_bytes = luma ? (size_t)(4 * q.size + 1) * 2 : (size_t)(4 * q.size_chroma + 1) * 4;
	if (reads_nbr ? !help_piece_inside(c.nbr, nbr_bytes, arena_bytes) : c.nbr != -1) return "nbr";
	if (reads_sync ? !help_piece_inside(c.sync, (size_t)q.size_chroma * q.size_chroma * 8, arena_bytes) : c.sync != -1) return "sync";
	return nullptr;
}

}  // namespace

extern "C" int hmr_gpu_walk_helper_forms(const hmr_gpu_helper_case *cases, int ncases, const uint8_t *arena, size_t arena_bytes, hmr_gpu_helper_out *out)
{
	if (!cases || ncases < 1 || ncases > (1 << 16) || !arena || !arena_bytes || !out) {
		hmr_set_error("hmr_gpu_walk_helper_forms: NULL argument or ncases outside 1 .. 2^16");
		return HMR_GPU_ERR_ARG;
	}
	std::vector<Geo> geo(NNODES);
	make_geo(geo.data());
	std::vector<int> list[2];      // the cases of the plain launch, of the launch with the latency kernel's helper loop
	for (int i = 0; i < ncases; i++) {
		const char *why = helper_case_refused(cases[i], geo.data(), arena_bytes);
		if (why) {
			hmr_set_error("hmr_gpu_walk_helper_forms: case %d refused: %s", i, why);
			return HMR_GPU_ERR_ARG;
		}
		list[cases[i].step == HMR_GPU_HELPER_INTRA_SEARCH_BG].push_back(i);
	}
	hmr_gpu_ctx *c = hmr_default_ctx();
	if (!c) {
		hmr_set_error("hmr_gpu_walk_helper_forms: no device");
		return HMR_GPU_ERR_NO_DEVICE;
	}
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(henc_geo_table), geo.data(), sizeof(Geo) * NNODES));
	const unsigned lds_bytes = (unsigned)lds_request(false);
	HIP_TRY(hipFuncSetAttribute((const void *)k_walk_helpers, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
	HIP_TRY(hipFuncSetAttribute((const void *)k_walk_helpers_lat, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
	const int groups = ncases < HELP_MAX_GROUPS ? ncases : HELP_MAX_GROUPS;
	struct Bufs {
		void *p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
		~Bufs() { for (void *q : p) if (q) (void)hipFree(q); }
	} b;
	const size_t case_bytes = sizeof(hmr_gpu_helper_case) * (size_t)ncases, out_bytes = sizeof(hmr_gpu_helper_out) * (size_t)ncases, list_bytes = sizeof(int) * (size_t)ncases;
	std::vector<int> both(list[0]);
	both.insert(both.end(), list[1].begin(), list[1].end());
	HIP_TRY(hipMalloc(&b.p[0], case_bytes));
	HIP_TRY(hipMalloc(&b.p[1], arena_bytes + 64));
	HIP_TRY(hipMalloc(&b.p[2], sizeof(WorkSlow) * (size_t)groups));
	HIP_TRY(hipMalloc(&b.p[3], out_bytes));
	HIP_TRY(hipMalloc(&b.p[4], list_bytes));
	HIP_TRY(hipMalloc(&b.p[5], sizeof(CtuInfo) * (size_t)groups));
	HIP_TRY(hipMemcpyAsync(b.p[0], cases, case_bytes, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(b.p[1], arena, arena_bytes, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(b.p[4], both.data(), list_bytes, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemsetAsync(b.p[3], 0, out_bytes, c->stream));
	HIP_TRY(hipMemsetAsync(b.p[5], 0, sizeof(CtuInfo) * (size_t)groups, c->stream));
	for (int lat = 0; lat < 2; lat++) {
		const int nlist = (int)list[lat].size();
		if (!nlist) continue;
		const int *dev_list = (const int *)b.p[4] + (lat ? list[0].size() : 0);
		hipLaunchKernelGGL(lat ? k_walk_helpers_lat : k_walk_helpers, dim3(nlist < groups ? nlist : groups), dim3(ENC_THREADS), lds_bytes, c->stream, (const hmr_gpu_helper_case *)b.p[0],
				   dev_list, nlist, (const uint8_t *)b.p[1], (const DevTables *)c->tables, (WorkSlow *)b.p[2], (CtuInfo *)b.p[5], (hmr_gpu_helper_out *)b.p[3], lds_bytes);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipMemcpyAsync(out, b.p[3], out_bytes, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return HMR_GPU_OK;
}
