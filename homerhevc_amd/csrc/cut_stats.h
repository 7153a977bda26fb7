// Scene-cut statistics of an 8-bit 4:2:0 picture against its predecessor, defined in integers (include/homer_gpu.h section 12m).  ONE arithmetic: k_cut (picture_io.hip)
// and hmr_gpu_cut_stats_host (picture_host.cpp) compile these functions, and a caller can reproduce every value from this comment.
//
// cur and prev are W x H pictures, W and H multiples of 8: luma is an exact grid of (W / 8) x (H / 8) BLOCKS of 8 x 8 samples.  Eight signed 64-bit values a picture:
//     SAD_Y, SAD_U, SAD_V   the sum of abs(cur - prev) over the plane                                                        (at most 255 W H)
//     HIST                  the sum over v = 0 .. 255 of abs(hc[v] - hp[v]), hc / hp the luma histograms of cur / prev        (0 .. 2 W H)
//     INTRA                 the sum of act(b) over the blocks
//     INTER                 the sum of min(64 msad(b), act(b)) over the blocks
//     NINTRA                the number of blocks with act(b) < 64 msad(b)
//     LUMA                  the sum of cur's luma samples
// act(b): the sum over the block's 64 samples x of abs(64 x - S), S the block's sample sum - 64 times the mean-removed deviation, nothing rounded.  At most
// 522 240: with k samples of 255 and 64 - k of 0, S = 255 k and the sum is 2 x 255 k (64 - k), largest at k = 32; no other block gives more (the sum is convex in
// every sample, so its maximum lies at a corner of [0, 255]^64).
// msad(b): the minimum over the VALID vectors (dx, dy) in [-8, 8]^2 of the sum over the block's samples of abs(cur(bx + i, by + j) - prev(bx + dx + i, by + dy + j));
// valid: the displaced block lies wholly inside the picture (hmr_cut_valid).  (0, 0) is always valid; at most 64 x 255 = 16 320, so 64 msad <= 1 044 480.
// Only the minimum VALUE enters a sum: no tie-break exists.  No sample outside W x H is read.
// Every value is a sum of non-negative integers below 2^31 per block or sample: exact in any order of addition, far inside 64 bits.
#pragma once
#include <stdint.h>

#define HMR_CUT_VALUES 8             // HMR_GPU_CUT_VALUES
#define HMR_CUT_RANGE 8              // HMR_GPU_CUT_RANGE
#define HMR_CUT_BLOCK 8
#define HMR_CUT_MAX_ACT 522240
#define HMR_CUT_MAX_MSAD 16320
enum { HMR_CUT_SAD_Y, HMR_CUT_SAD_U, HMR_CUT_SAD_V, HMR_CUT_HIST, HMR_CUT_INTRA, HMR_CUT_INTER, HMR_CUT_NINTRA, HMR_CUT_LUMA };

// one sample's term of act: abs(64 x - S)
__host__ __device__ inline uint32_t hmr_cut_deviation(uint32_t x, uint32_t S)
{
	const int32_t d = (int32_t)(64u * x) - (int32_t)S;
	return (uint32_t)(d < 0 ? -d : d);
}

// the block at (bx, by) displaced by (dx, dy) lies wholly inside the W x H picture
__host__ __device__ inline bool hmr_cut_valid(int bx, int by, int dx, int dy, int W, int H)
{
	return dx >= -HMR_CUT_RANGE && dx <= HMR_CUT_RANGE && dy >= -HMR_CUT_RANGE && dy <= HMR_CUT_RANGE && bx + dx >= 0 && bx + dx + HMR_CUT_BLOCK <= W && by + dy >= 0 &&
	       by + dy + HMR_CUT_BLOCK <= H;
}

// what a block adds to INTRA, INTER and NINTRA
struct CutBlock {
	uint32_t intra, inter, nintra;
};
__host__ __device__ inline CutBlock hmr_cut_block(uint32_t act, uint32_t msad)
{
	const uint32_t cost = 64u * msad;
	return CutBlock{act, cost < act ? cost : act, act < cost ? 1u : 0u};
}

// What the cut calls refuse of a picture size, as text (NULL: accepted).
static inline const char *hmr_cut_refusal(int width, int height)
{
	if (width <= 0 || height <= 0 || (width & 7) || (height & 7)) return "width and height have to be positive multiples of 8";
	return nullptr;
}

// ---- the host's loops (hmr_gpu_cut_stats_host): a plane's sample (x, y) is p[y * pitch + x * step] ----
static inline int64_t hmr_cut_sad_plane_host(const uint8_t *a, int64_t pitch_a, int step_a, const uint8_t *b, int64_t pitch_b, int step_b, int w, int h)
{
	int64_t sum = 0;
	for (int y = 0; y < h; y++)
		for (int x = 0; x < w; x++) {
			const int d = (int)a[y * pitch_a + (int64_t)x * step_a] - (int)b[y * pitch_b + (int64_t)x * step_b];
			sum += d < 0 ? -d : d;
		}
	return sum;
}

// HIST, INTRA, INTER, NINTRA and LUMA of the luma planes cur and prev (unit step) into stats
static inline void hmr_cut_luma_host(const uint8_t *cur, int64_t pitch_c, const uint8_t *prev, int64_t pitch_p, int W, int H, int64_t *stats)
{
	int64_t hc[256] = {0}, hp[256] = {0}, luma = 0, intra = 0, inter = 0, nintra = 0;
	for (int y = 0; y < H; y++)
		for (int x = 0; x < W; x++) {
			hc[cur[y * pitch_c + x]]++;
			hp[prev[y * pitch_p + x]]++;
			luma += cur[y * pitch_c + x];
		}
	int64_t hist = 0;
	for (int v = 0; v < 256; v++) hist += hc[v] < hp[v] ? hp[v] - hc[v] : hc[v] - hp[v];
	for (int by = 0; by < H; by += HMR_CUT_BLOCK)
		for (int bx = 0; bx < W; bx += HMR_CUT_BLOCK) {
			uint32_t S = 0, act = 0, msad = ~0u;
			for (int j = 0; j < HMR_CUT_BLOCK; j++)
				for (int i = 0; i < HMR_CUT_BLOCK; i++) S += cur[(by + j) * pitch_c + bx + i];
			for (int j = 0; j < HMR_CUT_BLOCK; j++)
				for (int i = 0; i < HMR_CUT_BLOCK; i++) act += hmr_cut_deviation(cur[(by + j) * pitch_c + bx + i], S);
			for (int dy = -HMR_CUT_RANGE; dy <= HMR_CUT_RANGE; dy++)
				for (int dx = -HMR_CUT_RANGE; dx <= HMR_CUT_RANGE; dx++) {
					if (!hmr_cut_valid(bx, by, dx, dy, W, H)) continue;
					uint32_t sad = 0;
					for (int j = 0; j < HMR_CUT_BLOCK; j++)
						for (int i = 0; i < HMR_CUT_BLOCK; i++) {
							const int d = (int)cur[(by + j) * pitch_c + bx + i] - (int)prev[(by + dy + j) * pitch_p + bx + dx + i];
							sad += (uint32_t)(d < 0 ? -d : d);
						}
					if (sad < msad) msad = sad;
				}
			const CutBlock k = hmr_cut_block(act, msad);
			intra += k.intra; inter += k.inter; nintra += k.nintra;
		}
	stats[HMR_CUT_HIST] = hist; stats[HMR_CUT_INTRA] = intra; stats[HMR_CUT_INTER] = inter; stats[HMR_CUT_NINTRA] = nintra; stats[HMR_CUT_LUMA] = luma;
}
