// MultiGroupHead.predict on the device, end to end, with no host round trip:
//   det3d/models/bbox_heads/mg_head_sessd.py:893-943 (predict) and :945-1057 (get_task_detections)
//   det3d/core/bbox/box_torch_ops.py:81-147 (second_box_decode), :527-548 (rotate_nms: topk, keep[:post])
//   det3d/ops/nms/nms_cpu.py:40-51 + det3d/ops/nms/nms_cpu.h:72-168 (rotate_nms_cc, CPU/boost in the reference)
//   det3d/core/bbox/geometry.py:215-277 (frustum test), mg_head_sessd.py:1035-1045 (direction fix, range mask)
// The reference leaves the GPU three times per frame here (boolean-mask indexing, NMS on the CPU,
// frustum test in numba). Pipeline of this file, all on one stream:
//   K1 score_filter   1 thread / BEV location: sigmoid(cls) >= thresh -> 64-bit key (~score | anchor) appended
//                     with a wave-aggregated atomic (order does not matter: the key is a total order)
//   K2 topk_decode    1 workgroup / frame: running top-`pre_max` by bitonic sort in LDS (2048 keys at a time),
//                     then decode ONLY the survivors (box, rectified score, direction label, BEV corners, AABB)
//   K3 rnms_pairs / rnms_clip   suppression bitmask: AABB prefilter (float32, iou_jit eps=0) of every row over the later
//                     candidates, the surviving pairs COMPACTED into one list, then convex polygon clipping in float64 on
//                     dense lanes only; suppress when IoU >= thresh
//   K4 nms_reduce     greedy walk over the mask (staged in LDS), stops at post_max, fused with
//   K5 finalize       frustum (float64 planes), direction fix, centre-range mask, ordered compaction, and the frame's
//                     fixed-size detection record (sessd_predict_fused; the unfused kernels serve pre_max > ~1280)
// DI-NMS (mg_head_sessd.py:999-1018, the reference's other post-processor; sessd_predict_di) replaces K3 - K5 by di_overlap_rows
// (dense overlap rows, stand-up prefilter + float64 clipping) and di_select_finalize (centerness damping, the IoU-weighted
// selection loop, then K5's filters on the averaged boxes and the record): see the comment above those kernels.
// K1 can also run inside the producer of the head tensor (sessd_ssfa_fuse_head_keys, dense_conv.hip): the keys then arrive
// with the head and the frame has one launch and one 35 k-thread pass less.
// Head tensor layout consumed here: planar (B, 22, H*W): ch 0..13 box codes (anchor-major, 7 each),
// 14..15 cls, 16..19 dir (2 per anchor), 20..21 iou; anchor id = pixel*2 + a (mg_head_sessd.py:409-481).
// Multi-task heads (mg_head_sessd.py:893-943: get_task_detections once per task with its own anchors, then concatenation in
// task order with label offsets): (frame b, task t) runs through K1-K5 as the virtual frame v = b * T + t -- the head tensor
// (B, T, 22, H*W), keys, candidates and masks are all indexed by a frame with fixed strides -- into per-task rows of the
// workspace, and one small launch (merge_tasks_kernel) concatenates them per real frame and writes the record. T = 1 has no
// such launch and no such rows: the kernels write the caller's outputs as before.
#include "geom.hpp"
#include "sessd_hip_types.h"

namespace {

constexpr int APL = 2;        // anchors per location
constexpr int HEAD_CH = 22;
constexpr int SORT_N = 2048;  // keys sorted per pass in LDS
constexpr int SORT_NT = 1024;

struct PostCfg {
  int num_pix;         // H*W
  float score_thresh;  // 0.3
  int pre_max, post_max;
  float nms_thresh;
  float range[6];      // post_center_range
  float dir_offset;
  int num_tasks;       // a kernel's frame index is the virtual frame v = b * num_tasks + t (1: v = b)
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(256) void score_filter_kernel(const float* __restrict__ head, PostCfg C,
                                                            unsigned long long* __restrict__ keys, int key_cap,
                                                            int* __restrict__ count) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (pix >= C.num_pix) return;
  const float* hb = head + (size_t)b * HEAD_CH * C.num_pix;
#pragma unroll
  for (int a = 0; a < APL; ++a) {
    const float s = sigmoidf_(hb[(size_t)(14 + a) * C.num_pix + pix]);
    if (s >= C.score_thresh) {
      // IoU rectification (mg_head_sessd.py:971-972): s *= ((iou + 1) * 0.5)^4
      const float r = (hb[(size_t)(20 + a) * C.num_pix + pix] + 1.0f) * 0.5f;
      const float sc = s * (r * r * r * r);
      const unsigned aid = (unsigned)(pix * APL + a);
      const unsigned long long key = ((unsigned long long)(~__float_as_uint(sc)) << 32) | aid;
      const int slot = atomicAdd(&count[b], 1);
      if (slot < key_cap) keys[(size_t)b * key_cap + slot] = key;
    }
  }
}

__device__ __forceinline__ void bitonic_sort_lds(unsigned long long* s, int n) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (n >> 1); t += SORT_NT) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int hi = lo | j;
        const bool up = (lo & k) == 0;
        const unsigned long long a = s[lo], b = s[hi];
        if ((a > b) == up) { s[lo] = b; s[hi] = a; }
      }
      __syncthreads();
    }
  }
}

// Outputs per frame (stride pre_max): cand_box (7), cand_score, cand_dir, corners (8), standup (4), n_top; cand_ioup / cand_axy (2)
// only when cand_ioup != nullptr (DI-NMS)
__global__ __launch_bounds__(SORT_NT) void topk_decode_kernel(const float* __restrict__ head,
                                                               const float* __restrict__ anchors, int anchors_per_frame,
                                                               PostCfg C, const unsigned long long* __restrict__ keys,
                                                               int key_cap, const int* __restrict__ count,
                                                               float* __restrict__ cand_box, float* __restrict__ cand_score,
                                                               int* __restrict__ cand_dir, float* __restrict__ corners,
                                                               float* __restrict__ standup, int* __restrict__ n_top,
                                                               int* __restrict__ rec_cursor, int* __restrict__ rec_base, int batch,
                                                               int* __restrict__ pair_count, float* __restrict__ cand_ioup,
                                                               float* __restrict__ cand_axy) {
  __shared__ unsigned long long s[SORT_N];
  const int b = blockIdx.x;
  if (threadIdx.x == 0) pair_count[b] = 0;  // the suppression-mask launches that follow append this frame's pairs
  // detection records (sessd_predict_fused): this batch takes the ring slots cursor .. cursor + batch - 1; the last kernel of
  // the call reads the base from the workspace
  if (rec_cursor && b == 0 && threadIdx.x == 0) {
    const int c0 = *rec_cursor;
    *rec_base = c0;
    *rec_cursor = c0 + batch;
  }
  const int n = min(count[b], key_cap);
  const unsigned long long* kb = keys + (size_t)b * key_cap;
  int T = 0, pos = 0;
  while (pos < n) {
    const int take = min(n - pos, SORT_N - T);
    int npad = 64;
    while (npad < T + take) npad <<= 1;
    for (int t = threadIdx.x; t < npad - T; t += SORT_NT) s[T + t] = t < take ? kb[pos + t] : ~0ull;
    __syncthreads();
    bitonic_sort_lds(s, npad);
    T = min(T + take, C.pre_max);
    pos += take;
    __syncthreads();
  }
  if (threadIdx.x == 0) n_top[b] = T;
  const float* hb = head + (size_t)b * HEAD_CH * C.num_pix;
  for (int k = threadIdx.x; k < T; k += SORT_NT) {
    const unsigned long long key = s[k];
    const unsigned aid = (unsigned)(key & 0xFFFFFFFFull);
    const float sc = __uint_as_float(~(unsigned)(key >> 32));
    const int pix = aid / APL, a = aid % APL;
    // anchors (T, A, 7) shared by all frames, or one set per (frame, task)
    const float* an = anchors + ((size_t)(anchors_per_frame ? (size_t)b * anchors_per_frame
                                                            : (size_t)(b % C.num_tasks) * (C.num_pix * APL)) + aid) * 7;
    float t[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) t[q] = hb[(size_t)(a * 7 + q) * C.num_pix + pix];
    // second_box_decode (box_torch_ops.py:112-146)
    const float xa = an[0], ya = an[1], za = an[2], wa = an[3], la = an[4], ha = an[5], ra = an[6];
    const float diag = sqrtf(la * la + wa * wa);
    float bx[7];
    bx[0] = t[0] * diag + xa;
    bx[1] = t[1] * diag + ya;
    bx[2] = t[2] * ha + za;
    bx[3] = expf(t[3]) * wa;
    bx[4] = expf(t[4]) * la;
    bx[5] = expf(t[5]) * ha;
    bx[6] = t[6] + ra;
    const size_t o = (size_t)b * C.pre_max + k;
#pragma unroll
    for (int q = 0; q < 7; ++q) cand_box[o * 7 + q] = bx[q];
    cand_score[o] = sc;
    const float d0 = hb[(size_t)(16 + a * 2) * C.num_pix + pix], d1 = hb[(size_t)(17 + a * 2) * C.num_pix + pix];
    cand_dir[o] = d1 > d0 ? 1 : 0;  // torch.max: first maximum on ties
    if (cand_ioup) {  // DI-NMS only: iou_preds as reassigned at mg_head_sessd.py:971, and the candidate's own anchor centre
      cand_ioup[o] = (hb[(size_t)(20 + a) * C.num_pix + pix] + 1.0f) * 0.5f;
      cand_axy[o * 2] = xa;
      cand_axy[o * 2 + 1] = ya;
    }
    // boxes_for_nms = box[:, [0,1,3,4,6]] -> corners (box_np_ops.py:512-532) and stand-up box
    const float det[5] = {bx[0], bx[1], bx[3], bx[4], bx[6]};
    float c8[8];
    sessd_box2d_corners(det, c8);
    float x0 = c8[0], y0 = c8[1], x1 = c8[0], y1 = c8[1];
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      x0 = fminf(x0, c8[2 * q]); x1 = fmaxf(x1, c8[2 * q]);
      y0 = fminf(y0, c8[2 * q + 1]); y1 = fmaxf(y1, c8[2 * q + 1]);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) corners[o * 8 + q] = c8[q];
    standup[o * 4 + 0] = x0; standup[o * 4 + 1] = y0; standup[o * 4 + 2] = x1; standup[o * 4 + 3] = y1;
  }
}

// iou_jit(eps=0) prefilter (box_np_ops.py:1007-1045), float32: stand-up IoU > 0
__device__ __forceinline__ bool rnms_prefilter(const float* si, const float* sj) {
  const float iw = fminf(si[2], sj[2]) - fmaxf(si[0], sj[0]);
  if (!(iw > 0.f)) return false;
  const float ih = fminf(si[3], sj[3]) - fmaxf(si[1], sj[1]);
  if (!(ih > 0.f)) return false;
  const float ua = (si[2] - si[0]) * (si[3] - si[1]) + (sj[2] - sj[0]) * (sj[3] - sj[1]) - iw * ih;
  const float siou = iw * ih / ua;
  return !(siou <= 0.f);
}

// polygon IoU >= thresh (nms_cpu.h:130-160: area(P & Q) / area(P | Q)), float64 clipping
__device__ __forceinline__ bool rnms_polygon(const float* ci, const float* cj, float thresh) {
  const double inter = sessd_quad_inter_area_green(ci, cj);
  if (inter <= 0) return false;
  double px[4], py[4], qx[4], qy[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { px[q] = ci[2 * q]; py[q] = ci[2 * q + 1]; qx[q] = cj[2 * q]; qy[q] = cj[2 * q + 1]; }
  const double uni = fabs(sessd_poly_area2(px, py, 4)) * 0.5 + fabs(sessd_poly_area2(qx, qy, 4)) * 0.5 - inter;
  const double ov = uni > 0 ? inter / uni : 0.0;
  return ov >= (double)thresh;
}

// The suppression mask in two balanced launches. Round 2 gave every (row, 64-column word) a wave and let the lanes that passed
// the stand-up prefilter run the float64 polygon clipping (~1500 instructions, ~6 us per wave) while the rest of the wave
// idled: nearly every one of the 8000 waves paid a full clipping round for 1-3 useful lanes (21.7 us per frame, max 38). A
// first round-3 form (one wave per row: sweep, compact in LDS, clip the row's survivors on dense lanes) was 10.7 us on typical
// frames but 68 us on frames where a few boxes overlap everything (the synthetic weights decode some boxes to kilometres):
// such a row is 16 clipping rounds on ONE wave. So:
//   rnms_pairs_kernel  one wave per row i: clears the row's mask words, sweeps the later candidates j > i with the prefilter
//                      (16-byte coalesced loads) and appends the surviving (i, j) pairs to ONE list per frame (one atomic per
//                      64 candidates); the list holds every pair up to 1024 candidates (measured: frames where kilometre-sized
//                      boxes overlap everything reach hundreds of thousands of pairs); beyond, pairs that do not fit (more than
//                      64 per row on average) are clipped on the spot;
//   rnms_clip_kernel   the list's pairs dealt out over all lanes of the launch: one clipping round on dense lanes whatever
//                      the distribution over rows; bits set with atomicOr.
constexpr int RN_ROWS = 4;       // waves (rows) per workgroup of the pair kernel
constexpr int RN_MAXN = 4096;    // candidates (rotate_nms_common's limit; pairs are packed i << 16 | j)
constexpr int RN_PAIRS_PER_ROW = 64;
// capacity of a frame's pair list: every pair up to 1024 candidates (2 MB), an average of 64 per row beyond
__host__ __device__ inline int rn_pair_cap(int n) { return n <= 1024 ? (n > 1 ? n * (n - 1) / 2 : 1) : n * RN_PAIRS_PER_ROW; }

__device__ __forceinline__ void rnms_clip_pair(const float* __restrict__ cb, int i, int j, float thresh,
                                               unsigned long long* __restrict__ mrow_base, int words) {
  const float4* c4 = reinterpret_cast<const float4*>(cb + (size_t)i * 8);
  const float4 a4 = c4[0], b4 = c4[1];
  const float4* d4 = reinterpret_cast<const float4*>(cb + (size_t)j * 8);
  const float4 e4 = d4[0], f4 = d4[1];
  const float ci[8] = {a4.x, a4.y, a4.z, a4.w, b4.x, b4.y, b4.z, b4.w};
  const float cj[8] = {e4.x, e4.y, e4.z, e4.w, f4.x, f4.y, f4.z, f4.w};
  if (rnms_polygon(ci, cj, thresh)) atomicOr(mrow_base + (size_t)i * words + (j >> 6), 1ull << (j & 63));
}

__global__ __launch_bounds__(RN_ROWS * 64) void rnms_pairs_kernel(const int* __restrict__ n_top, int pre_max, float thresh,
                                                                   const float* __restrict__ corners,
                                                                   const float* __restrict__ standup,
                                                                   unsigned long long* __restrict__ mask, int words,
                                                                   unsigned* __restrict__ pairs, int pair_cap,
                                                                   int* __restrict__ pair_count) {
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * RN_ROWS + (int)(threadIdx.x >> 6);
  const int n = min(n_top[b], pre_max);
  if (i >= n) return;
  unsigned long long* mb = mask + (size_t)b * pre_max * words;
  for (int w = (i >> 6) + lane; w < words; w += 64) mb[(size_t)i * words + w] = 0ull;  // words left of the diagonal are never read
  __builtin_amdgcn_s_waitcnt(0);  // the clears precede any atomicOr of the overflow path below
  const float* cb = corners + (size_t)b * pre_max * 8;
  const float4* sb = reinterpret_cast<const float4*>(standup + (size_t)b * pre_max * 4);
  const float4 s4 = sb[i];
  const float si[4] = {s4.x, s4.y, s4.z, s4.w};
  unsigned* pl = pairs + (size_t)b * pair_cap;
  // sweep: lane c keeps the ballot of chunk c (<= 64 chunks of 64 candidates); ONE atomic per row reserves the row's run of the
  // list (a first version reserved per chunk: sixteen dependent atomic round trips per wave, 22 us on busy frames)
  const int c0 = (i + 1) >> 6;
  unsigned long long mine = 0ull;
  for (int j0 = c0 << 6; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    bool pass = false;
    if (j > i && j < n) {
      const float4 t4 = sb[j];
      const float sj[4] = {t4.x, t4.y, t4.z, t4.w};
      pass = rnms_prefilter(si, sj);
    }
    const unsigned long long bal = __ballot(pass);
    if (lane == (j0 >> 6) - c0) mine = bal;
  }
  const int cnt = __popcll(mine);
  int incl = cnt;  // inclusive prefix of the chunk counts over the lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  const int total = __shfl(incl, 63, 64);
  if (total == 0) return;
  int base = 0;
  if (lane == 0) base = atomicAdd(&pair_count[b], total);
  base = __builtin_amdgcn_readfirstlane(base);
  const int excl = incl - cnt;
  const int nchunk = ((n - 1) >> 6) - c0 + 1;
  for (int c = 0; c < nchunk; ++c) {
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)mine, c), hi = __builtin_amdgcn_readlane((int)(unsigned)(mine >> 32), c);
    const unsigned long long bal = ((unsigned long long)hi << 32) | lo;
    if (bal == 0) continue;
    const int cbase = base + __builtin_amdgcn_readlane(excl, c);
    if ((bal >> lane) & 1ull) {
      const int j = ((c0 + c) << 6) + lane;
      const int idx = cbase + __popcll(bal & ((1ull << lane) - 1ull));
      if (idx < pair_cap) pl[idx] = ((unsigned)i << 16) | (unsigned)j;
      else rnms_clip_pair(cb, i, j, thresh, mb, words);  // list full: this pair is clipped here
    }
  }
}

__global__ __launch_bounds__(256) void rnms_clip_kernel(int pre_max, float thresh, const float* __restrict__ corners,
                                                         unsigned long long* __restrict__ mask, int words,
                                                         const unsigned* __restrict__ pairs, int pair_cap,
                                                         const int* __restrict__ pair_count) {
  const int b = blockIdx.y;
  const int np = min(pair_count[b], pair_cap);
  const float* cb = corners + (size_t)b * pre_max * 8;
  unsigned long long* mb = mask + (size_t)b * pre_max * words;
  const unsigned* pl = pairs + (size_t)b * pair_cap;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < np; p += gridDim.x * 256) {
    const unsigned pr = pl[p];
    rnms_clip_pair(cb, (int)(pr >> 16), (int)(pr & 0xFFFFu), thresh, mb, words);
  }
}

// both launches; pair_count[b] must be zero (sessd_predict_fused: cleared by topk_decode_kernel; rotate_nms_common: by its set kernel)
int launch_rnms_mask(const int* n_top, int batch, int pre_max, float thresh, const float* corners, const float* standup,
                     unsigned long long* mask, int words, unsigned* pairs, int* pair_count, hipStream_t stream) {
  if (pre_max > RN_MAXN) return SESSD_EINVAL;  // pairs are packed i << 16 | j
  const int pair_cap = rn_pair_cap(pre_max);
  SESSD_LAUNCH(rnms_pairs_kernel, dim3(sessd_divup(pre_max, RN_ROWS), batch), dim3(RN_ROWS * 64), 0, stream, n_top, pre_max,
               thresh, corners, standup, mask, words, pairs, pair_cap, pair_count);
  SESSD_CHECK_LAUNCH();
  const int g = sessd_divup(pair_cap, 256) < 512 ? sessd_divup(pair_cap, 256) : 512;
  SESSD_LAUNCH(rnms_clip_kernel, dim3(g, batch), dim3(256), 0, stream, pre_max, thresh, corners, mask, words, pairs, pair_cap,
               pair_count);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

// Post-NMS filters of one frame by ONE wave (mg_head_sessd.py:1024-1055): frustum (B,1,6,4,3) float64 surfaces (or null),
// direction fix, centre-range mask, ordered compaction. keep = the frame's kept candidate rows (global or LDS), nk of them.
// rec != nullptr: the finalized rows also go to rec[row * 9 + {box 7, score, label}] (LDS staging of the detection record).
// Returns the number of detections written (wave-uniform).
__device__ __forceinline__ int finalize_wave(const PostCfg& C, int b, int lane, const int* keep, int nk,
                                             const float* __restrict__ cand_box, const float* __restrict__ cand_score,
                                             const int* __restrict__ cand_dir, const double* __restrict__ frustum,
                                             float* __restrict__ out_box, float* __restrict__ out_score,
                                             int* __restrict__ out_label, float* rec) {
  double nx[6], ny[6], nz[6], nd[6];
  if (frustum) {
    const double* f = frustum + (size_t)(b / C.num_tasks) * 72;  // per real frame
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double* s = f + k * 12;
      const double ax = s[0] - s[3], ay = s[1] - s[4], az = s[2] - s[5];
      const double bx = s[3] - s[6], by = s[4] - s[7], bz = s[5] - s[8];
      nx[k] = ay * bz - az * by;
      ny[k] = az * bx - ax * bz;
      nz[k] = ax * by - ay * bx;
      nd[k] = -s[0] * nx[k] - s[1] * ny[k] - s[2] * nz[k];
    }
  }
  int written = 0;
  for (int base = 0; base < nk; base += 64) {
    const int k = base + lane;
    bool ok = k < nk;
    float bx[7] = {0, 0, 0, 0, 0, 0, 0};
    float sc = 0.f;
    if (ok) {
      const size_t o = (size_t)b * C.pre_max + keep[k];
#pragma unroll
      for (int q = 0; q < 7; ++q) bx[q] = cand_box[o * 7 + q];
      sc = cand_score[o];
      if (frustum) {
#pragma unroll
        for (int p = 0; p < 6; ++p) {
          const double sign = (double)bx[0] * nx[p] + (double)bx[1] * ny[p] + (double)bx[2] * nz[p] + nd[p];
          if (sign >= 0) ok = false;
        }
      }
      const bool opp = ((bx[6] - C.dir_offset) > 0.f) != (cand_dir[o] == 1);
      if (opp) bx[6] += 3.14159265358979323846f;
      ok = ok && bx[0] >= C.range[0] && bx[1] >= C.range[1] && bx[2] >= C.range[2] && bx[0] <= C.range[3] &&
           bx[1] <= C.range[4] && bx[2] <= C.range[5];
    }
    const unsigned long long bal = __ballot(ok);
    if (ok) {
      const int dst = written + __popcll(bal & ((1ull << lane) - 1ull));
      const size_t o = (size_t)b * C.post_max + dst;
#pragma unroll
      for (int q = 0; q < 7; ++q) out_box[o * 7 + q] = bx[q];
      out_score[o] = sc;
      out_label[o] = 0;
      if (rec) {
#pragma unroll
        for (int q = 0; q < 7; ++q) rec[dst * 9 + q] = bx[q];
        rec[dst * 9 + 7] = sc;
        rec[dst * 9 + 8] = 0.f;
      }
    }
    written += __popcll(bal);
  }
  return written;
}

__global__ __launch_bounds__(64) void finalize_kernel(PostCfg C, const int* __restrict__ keep, const int* __restrict__ n_keep,
                                                       const float* __restrict__ cand_box, const float* __restrict__ cand_score,
                                                       const int* __restrict__ cand_dir, const double* __restrict__ frustum,
                                                       float* __restrict__ out_box, float* __restrict__ out_score,
                                                       int* __restrict__ out_label, int* __restrict__ out_count) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nk = min(n_keep[b], C.post_max);
  const int written = finalize_wave(C, b, lane, keep + (size_t)b * C.post_max, nk, cand_box, cand_score, cand_dir, frustum, out_box,
                                    out_score, out_label, nullptr);
  if (lane == 0) out_count[b] = written;
}

// The greedy walk of the rotated NMS over a suppression mask in LDS by ONE wave (nms_cpu.h:86-168: candidates in score order,
// a candidate is kept unless a kept one suppresses it; stops at post_max). lane w owns word w of the running "removed" set.
// Round 2 tested every candidate of a block in turn (~20 scalar-ish instructions x 1000 candidates = 10 us of the 22 us this
// kernel took); here the next kept candidate of a block is the lowest clear bit of (~removed & valid) -- s_ff1 -- so the loop
// runs once per KEPT candidate (<= post_max in total). Kept rows go to `keep_out` (LDS or global); returns their number.
__device__ __forceinline__ int nms_walk_lds(const unsigned long long* sm, int n, int words, int post_max, int lane, int* keep_out) {
  auto rdlane64 = [](unsigned long long v, int l) -> unsigned long long {
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
  };
  const int cb = sessd_divup(n, 64);
  unsigned long long removed = 0;
  int nk = 0;
  for (int blk = 0; blk < cb && nk < post_max; ++blk) {
    const int row = blk * 64 + lane;
    const unsigned long long diag = row < n ? sm[(size_t)row * words + blk] : 0ull;
    unsigned long long rem = rdlane64(removed, blk);
    const int lim = min(64, n - blk * 64);
    const unsigned long long valid = lim >= 64 ? ~0ull : ((1ull << lim) - 1ull);
    unsigned long long kept = 0;
    unsigned long long avail = ~rem & valid;
    while (avail && nk < post_max) {
      const int bb = __builtin_amdgcn_readfirstlane(__builtin_ctzll(avail));
      kept |= 1ull << bb;
      ++nk;
      rem |= rdlane64(diag, bb) | (1ull << bb);
      avail = ~rem & valid;
    }
    {  // kept rows of this block -> output list, ascending
      const int base = nk - __popcll(kept);
      unsigned long long k2 = kept;
      for (int t = 0; k2; ++t, k2 &= k2 - 1)
        if (lane == 0) keep_out[base + t] = blk * 64 + __builtin_ctzll(k2);
    }
    if (nk >= post_max) break;
    if (lane > blk && lane < cb) {
      unsigned long long acc = 0;
      for (unsigned long long k2 = kept; k2; k2 &= k2 - 1)
        acc |= sm[(size_t)(blk * 64 + __builtin_ctzll(k2)) * words + lane];
      removed |= acc;
    }
  }
  return nk;
}

__device__ __forceinline__ void stage_mask_lds(unsigned long long* sm, const unsigned long long* mb, int n, int words) {
  // blind 16-byte copy of the n x words matrix (words left of the diagonal were never written by the mask kernel and are
  // never read by the walk); 8 independent loads per thread in flight
  const int total2 = (n * words + 1) >> 1;
  const uint4* src = reinterpret_cast<const uint4*>(mb);
  uint4* dst = reinterpret_cast<uint4*>(sm);
#pragma unroll 8
  for (int idx = threadIdx.x; idx < total2; idx += 1024) dst[idx] = src[idx];
}

// The greedy reduction with the WHOLE suppression mask staged in LDS (pre_max*ceil(pre_max/64)*8 B = 128 KB for pre_max 1000;
// 160 KB LDS per CU: 1024 threads copy it in one coalesced sweep, then one wave walks it at LDS latency instead of one
// dependent global load per kept row),
// FUSED with the post-NMS filters and the frame's detection record: after the walk the kept rows sit in LDS,
// wave 0 runs finalize_wave on them (<= post_max boxes), the finalized rows are staged in LDS and all threads write the
// fixed-size record (post_max x 9 floats + count; rows beyond the count zero) -- three launches of round 2 (nms_reduce 22 us,
// finalize 4.9 us, pack_detections 4.2 us) as one. Dynamic LDS: mask | keep[post_max] | rec[post_max * 9].
// records == nullptr: no record. rec_base = the slot counter value of this batch's first frame (written by topk_decode).
__global__ __launch_bounds__(1024) void nms_reduce_finalize_kernel(PostCfg C, const int* __restrict__ n_top,
                                                                   const unsigned long long* __restrict__ mask, int words,
                                                                   const float* __restrict__ cand_box,
                                                                   const float* __restrict__ cand_score,
                                                                   const int* __restrict__ cand_dir,
                                                                   const double* __restrict__ frustum, float* __restrict__ out_box,
                                                                   float* __restrict__ out_score, int* __restrict__ out_label,
                                                                   int* __restrict__ out_count, float* __restrict__ records,
                                                                   int* __restrict__ rec_count, int capacity,
                                                                   const int* __restrict__ rec_base) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sm[];
  __shared__ int s_written;
  const int b = blockIdx.x;
  const int n = min(n_top[b], C.pre_max);
  const size_t mask_words = (size_t)C.pre_max * words;
  int* s_keep = reinterpret_cast<int*>(sm + mask_words);
  float* s_rec = reinterpret_cast<float*>(s_keep + C.post_max);
  stage_mask_lds(sm, mask + (size_t)b * mask_words, n, words);
  __syncthreads();
  if (threadIdx.x < 64) {
    const int nk = nms_walk_lds(sm, n, words, C.post_max, threadIdx.x, s_keep);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // lane 0's list is read by the other lanes of this wave
    const int written = finalize_wave(C, b, threadIdx.x, s_keep, nk, cand_box, cand_score, cand_dir, frustum, out_box, out_score,
                                      out_label, records ? s_rec : nullptr);
    if (threadIdx.x == 0) {
      out_count[b] = written;
      s_written = written;
    }
  }
  if (!records) return;
  __syncthreads();
  const int written = s_written;
  const int slot = (rec_base[0] + b) % capacity;
  float* dst = records + (size_t)slot * C.post_max * 9;
  for (int e = threadIdx.x; e < C.post_max * 9; e += 1024) dst[e] = e < written * 9 ? s_rec[e] : 0.f;
  if (threadIdx.x == 0) rec_count[slot] = written;
}

// ---- detection records for the end-of-job gather (tools/dist_test.py:150-186 gathers pickled per-rank dicts; here every frame
// leaves one fixed-size record on the device: (post_max, 9) float32 [box 7 | score | label] + a count), appended by the frame's
// own launch sequence so that a captured graph needs no host-side bookkeeping: slot = (*cursor + b) % capacity, cursor += batch.
__global__ __launch_bounds__(256) void pack_detections_kernel(const float* __restrict__ box, const float* __restrict__ score,
                                                               const int* __restrict__ label, const int* __restrict__ count,
                                                               int batch, int post_max, float* __restrict__ records,
                                                               int* __restrict__ rec_count, int capacity, int* __restrict__ cursor,
                                                               const int* __restrict__ base_in) {
  // base_in: the batch's first slot was already taken (and the cursor advanced) by topk_decode_kernel
  const int c0 = base_in ? *base_in : *cursor;
  const int total = batch * post_max * 9;
  for (int e = threadIdx.x; e < total; e += 256) {
    const int b = e / (post_max * 9), r = (e - b * post_max * 9) / 9, q = e % 9;
    const int n = count[b];
    float v = 0.f;
    if (r < n) v = q < 7 ? box[((size_t)b * post_max + r) * 7 + q] : (q == 7 ? score[(size_t)b * post_max + r] : (float)label[(size_t)b * post_max + r]);
    records[((size_t)((c0 + b) % capacity) * post_max + r) * 9 + q] = v;
  }
  if (threadIdx.x < batch) rec_count[(c0 + threadIdx.x) % capacity] = count[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0 && !base_in) *cursor = c0 + batch;
}

// Multi-task merge (mg_head_sessd.py:932-937): the detections of frame b are the kept rows of task 0, then task 1, ... each in
// NMS order, label = task index (one class per task). task_* = the per-(frame, task) rows K5 left in the workspace, stride
// post_max; outputs (B, T * post_max, ...), rows past out_count[b] are not written. records != nullptr: the frame's record
// (T * post_max, 9) with zero rows past the count, ring slot (rec_base + b) % capacity (the cursor was advanced by K2).
__global__ __launch_bounds__(256) void merge_tasks_kernel(int num_tasks, int post_max, const float* __restrict__ task_box,
                                                           const float* __restrict__ task_score,
                                                           const int* __restrict__ task_count, float* __restrict__ out_box,
                                                           float* __restrict__ out_score, int* __restrict__ out_label,
                                                           int* __restrict__ out_count, int* __restrict__ out_task_count,
                                                           float* __restrict__ records, int* __restrict__ rec_count, int capacity,
                                                           const int* __restrict__ rec_base) {
  const int b = blockIdx.x;
  int start[5];  // num_tasks <= 4
  start[0] = 0;
  for (int t = 0; t < num_tasks; ++t) start[t + 1] = start[t] + min(task_count[b * num_tasks + t], post_max);
  const int total = start[num_tasks], rows = num_tasks * post_max;
  float* rec = records ? records + (size_t)((rec_base[0] + b) % capacity) * rows * 9 : nullptr;
  for (int r = threadIdx.x; r < rows; r += 256) {
    if (r >= total) {
      if (rec)
        for (int q = 0; q < 9; ++q) rec[(size_t)r * 9 + q] = 0.f;
      continue;
    }
    int t = 0;
    while (r >= start[t + 1]) ++t;
    const size_t src = (size_t)(b * num_tasks + t) * post_max + (r - start[t]), dst = (size_t)b * rows + r;
    const float sc = task_score[src];
    for (int q = 0; q < 7; ++q) {
      const float v = task_box[src * 7 + q];
      out_box[dst * 7 + q] = v;
      if (rec) rec[(size_t)r * 9 + q] = v;
    }
    out_score[dst] = sc;
    out_label[dst] = t;
    if (rec) {
      rec[(size_t)r * 9 + 7] = sc;
      rec[(size_t)r * 9 + 8] = (float)t;
    }
  }
  if (threadIdx.x == 0) {
    out_count[b] = total;
    if (rec) rec_count[(rec_base[0] + b) % capacity] = total;
  }
  if (out_task_count && threadIdx.x < num_tasks) out_task_count[b * num_tasks + threadIdx.x] = start[threadIdx.x + 1] - start[threadIdx.x];
}

// single task: out_task_count (B, 1) is out_count (a kernel, not a copy node: see fill.hip)
__global__ __launch_bounds__(256) void copy_counts_kernel(const int* __restrict__ src, int* __restrict__ dst, int n) {
  for (int i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
}

// ---- DI-NMS (box_torch_ops.rotate_weighted_nms, mg_head_sessd.py:999-1018) as the post-processor of the fused call: the
// candidates of virtual frame v come from K2 as before (plus iou_pred and the anchor centre), then
//   di_overlap_rows_kernel     one wave per candidate row i < n_top[v]: stand-up prefilter of the WHOLE row (the core reads
//                              overlap(A, j) for every j, kept or suppressed, before or after A), zeros stored where it fails,
//                              the survivors compacted in LDS and clipped in float64 on dense lanes (rounded to float like
//                              di_overlap_kernel of di_nms.hip). Every entry (i, j), i, j < n_top[v], of the frame's dense
//                              (pre_max, pre_max) matrix is written each call: no clear launch.
//   di_select_finalize_kernel  one 1024-thread workgroup per virtual frame, thread j = candidate j: centerness softmax
//                              (box_torch_ops.py:582-586), normalisation, the sequential loop of nms_cpu.h:173-384 exactly as
//                              di_select_kernel (di_nms.hip) runs it with centerness_c = 0 -- same picks, same box-order cnt
//                              sum, same fixed reduction tree -- then finalize_wave on the AVERAGED boxes and the frame's record.
// Deviations from the reference, both stated in include/sessd_hip.h: the anchors are the task's own (the reference reads task
// 0's x, y for every task: the same grid in the KITTI configs), and the loop stops once post_max boxes are kept (the reference
// wrapper ignores post_max_size; later passes cannot change earlier kept boxes, so this is its keep list cut at post_max).
// A pair's stand-up IoU > 0 test of the suppression rule is implied: overlap > 0 is only ever stored where the prefilter passed.
struct DiCfg {
  float cnt_thresh, suppressed_thresh, centerness_pow;
  int n_interval;
  float interval[8], sigma_sq[8];
};

constexpr int DI_ROWS = 4;     // waves (rows) per workgroup of the overlap kernel
constexpr int DI_MAXN = 1024;  // candidates: one thread each in the selection workgroup

__global__ __launch_bounds__(DI_ROWS * 64) void di_overlap_rows_kernel(const int* __restrict__ n_top, int pre_max,
                                                                        const float* __restrict__ corners,
                                                                        const float* __restrict__ standup,
                                                                        float* __restrict__ overlap) {
  __shared__ unsigned short s_list[DI_ROWS][DI_MAXN];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * DI_ROWS + wv;
  const int n = min(n_top[b], pre_max);
  if (i >= n) return;  // no workgroup barrier below
  const float* cb = corners + (size_t)b * pre_max * 8;
  const float4* sb = reinterpret_cast<const float4*>(standup + (size_t)b * pre_max * 4);
  const float4 s4 = sb[i];
  const float si[4] = {s4.x, s4.y, s4.z, s4.w};
  float* row = overlap + ((size_t)b * pre_max + i) * pre_max;
  int total = 0;
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    bool pass = false;
    if (j < n) {
      const float4 t4 = sb[j];
      const float sj[4] = {t4.x, t4.y, t4.z, t4.w};
      pass = rnms_prefilter(si, sj);
      if (!pass) row[j] = 0.f;
    }
    const unsigned long long bal = __ballot(pass);
    if (pass) s_list[wv][total + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)j;
    total += __popcll(bal);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the list is read by other lanes of this wave
  const float4* c4 = reinterpret_cast<const float4*>(cb + (size_t)i * 8);
  const float4 a4 = c4[0], b4 = c4[1];
  const float ci[8] = {a4.x, a4.y, a4.z, a4.w, b4.x, b4.y, b4.z, b4.w};
  double px[4], py[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { px[q] = ci[2 * q]; py[q] = ci[2 * q + 1]; }
  const double area_i = fabs(sessd_poly_area2(px, py, 4)) * 0.5;
  for (int p = lane; p < total; p += 64) {
    const int j = s_list[wv][p];
    const float4* d4 = reinterpret_cast<const float4*>(cb + (size_t)j * 8);
    const float4 e4 = d4[0], f4 = d4[1];
    const float cj[8] = {e4.x, e4.y, e4.z, e4.w, f4.x, f4.y, f4.z, f4.w};
    float v = 0.f;
    const double inter = sessd_quad_inter_area_green(ci, cj);
    if (inter > 0) {
      double qx[4], qy[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { qx[q] = cj[2 * q]; qy[q] = cj[2 * q + 1]; }
      const float ia = (float)inter;
      const float ua = (float)(area_i + fabs(sessd_poly_area2(qx, qy, 4)) * 0.5 - inter);
      v = ua > 0.f ? ia / ua : 0.f;
    }
    row[j] = v;
  }
}

__device__ __forceinline__ float di_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Dynamic LDS: keep[kcap] (the identity list finalize_wave walks) | rec[kcap * 9], kcap = min(post_max, pre_max).
// di_box / di_score / di_dir: the kept boxes of the frame, stride pre_max like the candidates (finalize_wave's indexing).
__global__ __launch_bounds__(DI_MAXN) void di_select_finalize_kernel(
    PostCfg C, DiCfg D, const int* __restrict__ n_top, const float* __restrict__ overlap, const float* __restrict__ cand_box,
    const float* __restrict__ cand_score, const int* __restrict__ cand_dir, const float* __restrict__ cand_ioup,
    const float* __restrict__ cand_axy, float* di_box, float* di_score, int* di_dir, const double* __restrict__ frustum,
    float* __restrict__ out_box, float* __restrict__ out_score, int* __restrict__ out_label, int* __restrict__ out_count,
    int* __restrict__ di_truncated, int* __restrict__ di_sticky, int* __restrict__ di_keep, int* __restrict__ di_keep_count,
    float* __restrict__ records, int* __restrict__ rec_count, int capacity, const int* __restrict__ rec_base) {
  extern __shared__ __attribute__((aligned(16))) int s_dyn[];
  __shared__ float s_red[16][10];
  __shared__ unsigned long long s_key[16];
  __shared__ float s_bc[12];
  __shared__ float s_terms[DI_MAXN];  // the pass's non-zero cnt terms in box order
  __shared__ int s_nz[16];
  __shared__ int s_written;
  const int v = blockIdx.x;
  const int j = threadIdx.x, lane = j & 63, wv = j >> 6;
  const int n = min(n_top[v], C.pre_max);
  const bool live = j < n;
  const size_t vb = (size_t)v * C.pre_max;
  const int kcap = min(C.post_max, C.pre_max);
  int* s_keep = s_dyn;
  float* s_rec = reinterpret_cast<float*>(s_dyn + kcap);
  float my_box[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) my_box[k] = live ? cand_box[(vb + j) * 7 + k] : 0.f;
  const float my_ioup = live ? cand_ioup[vb + j] : 0.f;
  // ---- centerness damping (box_torch_ops.py:582-586): score *= (1 - softmax(|xy - anchor xy|))^pow, float32, max subtracted
  float my_score = live ? cand_score[vb + j] : 0.f;
  {
    float d = -3.0e38f;
    if (live) {
      const float dx = fabsf(my_box[0] - cand_axy[(vb + j) * 2]), dy = fabsf(my_box[1] - cand_axy[(vb + j) * 2 + 1]);
      d = __fsqrt_rn(dx * dx + dy * dy);
    }
    float m = d;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) s_red[wv][0] = m;
    __syncthreads();
    float dmax = s_red[0][0];
    for (int w = 1; w < 16; ++w) dmax = fmaxf(dmax, s_red[w][0]);
    __syncthreads();
    const float e = live ? expf(d - dmax) : 0.f;
    const float t = di_wave_sum(e);
    if (lane == 0) s_red[wv][0] = t;
    __syncthreads();
    float sum = 0.f;
    for (int w = 0; w < 16; ++w) sum += s_red[w][0];
    __syncthreads();
    if (live) {
      const float damp = 1.0f - e / sum;
      my_score *= D.centerness_pow == 2.0f ? damp * damp : powf(damp, D.centerness_pow);
    }
  }
  // ---- normalised scores (nms_cpu.h:233-262)
  float srw = my_score;
  {
    float m = live ? srw : -10000.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) s_red[wv][0] = m;
    __syncthreads();
    float mx = -10000.f;
    for (int w = 0; w < 16; ++w) mx = fmaxf(mx, s_red[w][0]);
    __syncthreads();
    if (j == 0) s_bc[11] = mx;
    srw /= mx;
  }
  bool suppressed = !live;
  int nkeep = 0;
  int truncated = 0;
  __syncthreads();
  const float score_max4norm = s_bc[11];
  for (;;) {
    const bool cand = !suppressed && my_score > -1.f;
    if (nkeep >= C.post_max) {  // uniform: the outputs hold post_max rows per task
      truncated = __syncthreads_or(cand ? 1 : 0);
      break;
    }
    // ---- the unsuppressed box with the largest (damped) score, lowest index on ties
    unsigned long long key = 0ull;
    if (cand) {
      unsigned u = __float_as_uint(my_score);
      u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
      key = ((unsigned long long)u << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)j);
    }
    if (__ballot(cand)) {  // wave-uniform: a wave without candidates keeps key 0 (the maximum of zeros)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64);
        key = other > key ? other : key;
      }
    }
    if (lane == 0) s_key[wv] = key;
    __syncthreads();
    unsigned long long best = 0ull;
    for (int w = 0; w < 16; ++w) best = s_key[w] > best ? s_key[w] : best;
    if (best == 0ull) break;  // everything suppressed (uniform)
    const int idx = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));  // < n: only live threads make keys
    if (j == idx) suppressed = true;
    const float bx = cand_box[(vb + idx) * 7], by = cand_box[(vb + idx) * 7 + 1];
    const float dist2origin = (float)sqrt((double)bx * bx + (double)by * by);
    // ---- this box's contribution (one class per task: every candidate of the frame carries A's label)
    float cnt = 0.f, wsum = 0.f, avg[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sbox = -1.f;
    bool newly = false, weighs = false;
    if (live) {
      const float ov = overlap[(vb + idx) * C.pre_max + j];
      if (ov > 0.f) {
        cnt = ov * my_ioup;
        if (ov > D.suppressed_thresh) {
          weighs = true;
          sbox = srw;
          float w = 0.f;
          for (int k = 0; k + 1 < D.n_interval; ++k)
            if (dist2origin >= D.interval[k] && dist2origin < D.interval[k + 1]) {
              const double dd = 1.0 - (double)ov;
              w = (float)exp(-(dd * dd) / (double)D.sigma_sq[k]);
            }
          wsum = w * my_ioup;
#pragma unroll
          for (int k = 0; k < 7; ++k) avg[k] = w * my_ioup * my_box[k];
        }
        if (!suppressed && ov >= D.suppressed_thresh) {
          suppressed = true;
          newly = true;
        }
      }
    }
    // ---- cnt in the reference's order (box 0, 1, 2, ... in float32), the other sums in the fixed tree: see di_select_kernel
    const float cnt_term = cnt;
    const unsigned long long nzb = __ballot(cnt_term != 0.f);
    if (__ballot(weighs)) {  // wave-uniform: in a wave without a weighing box every lane already holds the tree's result (0 / -1)
      wsum = di_wave_sum(wsum);
#pragma unroll
      for (int k = 0; k < 7; ++k) avg[k] = di_wave_sum(avg[k]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sbox = fmaxf(sbox, __shfl_xor(sbox, o, 64));
    }
    __syncthreads();  // s_key / s_red of the previous pass are no longer read
    if (lane == 0) {
      s_red[wv][1] = wsum; s_red[wv][9] = sbox;
#pragma unroll
      for (int k = 0; k < 7; ++k) s_red[wv][2 + k] = avg[k];
      s_nz[wv] = __popcll(nzb);
    }
    __syncthreads();
    if (cnt_term != 0.f) {
      int off = 0;
      for (int w = 0; w < wv; ++w) off += s_nz[w];
      s_terms[off + __popcll(nzb & ((1ull << lane) - 1ull))] = cnt_term;
    }
    if (j >= 1 && j < 10) {
      float r = s_red[0][j];
      for (int w = 1; w < 16; ++w) r = (j == 9) ? fmaxf(r, s_red[w][j]) : r + s_red[w][j];
      s_bc[j] = r;
    }
    __syncthreads();
    if (j == 0) {
      int total = 0;
      for (int w = 0; w < 16; ++w) total += s_nz[w];
      float c = 0.f;
      for (int t = 0; t < total; ++t) c += s_terms[t];
      s_bc[0] = c;
    }
    __syncthreads();
    const bool kept = s_bc[0] > D.cnt_thresh;
    if (kept) {  // nkeep < post_max and nkeep < n <= pre_max: inside the frame's rows
      if (j == 0) {
        di_score[vb + nkeep] = s_bc[9] * score_max4norm;
        di_dir[vb + nkeep] = cand_dir[vb + idx];
        if (di_keep) di_keep[(size_t)v * C.post_max + nkeep] = idx;
      }
      if (j < 7) di_box[(vb + nkeep) * 7 + j] = s_bc[2 + j] / s_bc[1];
      ++nkeep;
    } else if (newly) {
      suppressed = false;  // the boxes this pass suppressed come back; A itself stays marked
    }
    __syncthreads();
  }
  // ---- after the core (mg_head_sessd.py:1024-1045): frustum, direction fix, range mask on the averaged boxes, then the record
  for (int k = j; k < nkeep; k += DI_MAXN) s_keep[k] = k;
  __syncthreads();  // the kept rows (global) and the list (LDS) are visible to wave 0
  if (j < 64) {
    const int written = finalize_wave(C, v, j, s_keep, nkeep, di_box, di_score, di_dir, frustum, out_box, out_score, out_label,
                                      records ? s_rec : nullptr);
    if (j == 0) {
      out_count[v] = written;
      s_written = written;
      if (di_truncated) di_truncated[v] = truncated;
      if (di_sticky && truncated) atomicOr(di_sticky, 1);
      if (di_keep_count) di_keep_count[v] = nkeep;
    }
  }
  if (!records) return;
  __syncthreads();
  const int written = s_written;
  const int slot = (rec_base[0] + v) % capacity;
  float* dst = records + (size_t)slot * C.post_max * 9;
  for (int e = j; e < C.post_max * 9; e += DI_MAXN) dst[e] = e < written * 9 ? s_rec[e] : 0.f;
  if (j == 0) rec_count[slot] = written;
}

struct PostWs {
  unsigned long long* keys;
  int* count;
  float* cand_box;
  float* cand_score;
  int* cand_dir;
  float* corners;
  float* standup;
  int* n_top;
  unsigned long long* mask;
  int* keep;
  int* n_keep;
  int* rec_base;
  unsigned* pairs;
  int* pair_count;
  // num_tasks > 1 only: K5's per-(frame, task) rows, merged by merge_tasks_kernel
  float* task_box;
  float* task_score;
  int* task_label;
  int* task_count;
  // DI-NMS only (instead of mask / keep / pairs): K2's extra candidate values, the dense overlap matrices, the kept boxes
  float* cand_ioup;
  float* cand_axy;
  float* overlap;
  float* di_box;
  float* di_score;
  int* di_dir;
};

// batch = virtual frames (B * num_tasks); the single-task layout is unchanged
size_t post_ws_layout(int batch, int num_tasks, int num_anchors, int pre_max, int post_max, PostWs* w, char* base, bool di = false) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off = sessd_align(off + bytes, 256);
    return o;
  };
  const int words = sessd_divup(pre_max, 64);
  size_t o_keys = take((size_t)batch * num_anchors * 8);
  size_t o_count = take((size_t)batch * 4);
  size_t o_box = take((size_t)batch * pre_max * 7 * 4);
  size_t o_score = take((size_t)batch * pre_max * 4);
  size_t o_dir = take((size_t)batch * pre_max * 4);
  size_t o_cor = take((size_t)batch * pre_max * 8 * 4);
  size_t o_su = take((size_t)batch * pre_max * 4 * 4);
  size_t o_nt = take((size_t)batch * 4);
  size_t o_mask = take(di ? 0 : (size_t)batch * pre_max * words * 8);
  size_t o_keep = take(di ? 0 : (size_t)batch * post_max * 4);
  size_t o_nk = take((size_t)batch * 4);
  size_t o_rb = take(4);
  size_t o_pairs = take(di ? 0 : (size_t)batch * rn_pair_cap(pre_max) * 4);
  size_t o_pc = take((size_t)batch * 4);
  size_t o_tb = 0, o_ts = 0, o_tl = 0, o_tc = 0;
  if (num_tasks > 1) {
    o_tb = take((size_t)batch * post_max * 7 * 4);
    o_ts = take((size_t)batch * post_max * 4);
    o_tl = take((size_t)batch * post_max * 4);
    o_tc = take((size_t)batch * 4);
  }
  size_t o_ip = 0, o_ax = 0, o_ov = 0, o_db = 0, o_ds = 0, o_dd = 0;
  if (di) {
    o_ip = take((size_t)batch * pre_max * 4);
    o_ax = take((size_t)batch * pre_max * 2 * 4);
    o_ov = take((size_t)batch * pre_max * pre_max * 4);
    o_db = take((size_t)batch * pre_max * 7 * 4);
    o_ds = take((size_t)batch * pre_max * 4);
    o_dd = take((size_t)batch * pre_max * 4);
  }
  if (w) {
    w->keys = (unsigned long long*)(base + o_keys);
    w->count = (int*)(base + o_count);
    w->cand_box = (float*)(base + o_box);
    w->cand_score = (float*)(base + o_score);
    w->cand_dir = (int*)(base + o_dir);
    w->corners = (float*)(base + o_cor);
    w->standup = (float*)(base + o_su);
    w->n_top = (int*)(base + o_nt);
    w->mask = (unsigned long long*)(base + o_mask);
    w->keep = (int*)(base + o_keep);
    w->n_keep = (int*)(base + o_nk);
    w->rec_base = (int*)(base + o_rb);
    w->pairs = (unsigned*)(base + o_pairs);
    w->pair_count = (int*)(base + o_pc);
    w->task_box = (float*)(base + o_tb);
    w->task_score = (float*)(base + o_ts);
    w->task_label = (int*)(base + o_tl);
    w->task_count = (int*)(base + o_tc);
    w->cand_ioup = (float*)(base + o_ip);
    w->cand_axy = (float*)(base + o_ax);
    w->overlap = (float*)(base + o_ov);
    w->di_box = (float*)(base + o_db);
    w->di_score = (float*)(base + o_ds);
    w->di_dir = (int*)(base + o_dd);
  }
  return off;
}

// batched variant of the greedy reduction (one wave per frame)
__global__ __launch_bounds__(64) void nms_reduce_batch_kernel(const int* __restrict__ n_top, int pre_max,
                                                               const unsigned long long* __restrict__ mask, int words,
                                                               int post_max, int* __restrict__ keep, int* __restrict__ n_keep) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = min(n_top[b], pre_max);
  const unsigned long long* mb = mask + (size_t)b * pre_max * words;
  int* kb = keep + (size_t)b * post_max;
  const int cb = sessd_divup(n, 64);
  unsigned long long removed = 0;  // lane w owns word w (pre_max <= 4096)
  int nk = 0;
  for (int blk = 0; blk < cb && nk < post_max; ++blk) {
    const int row = blk * 64 + lane;
    unsigned long long diag = row < n ? mb[(size_t)row * words + blk] : 0ull;
    unsigned long long rem = __shfl(removed, blk, 64);
    unsigned long long kept = 0;
    const int lim = min(64, n - blk * 64);
    for (int bb = 0; bb < lim; ++bb) {
      const unsigned long long d = __shfl(diag, bb, 64);
      if (!((rem >> bb) & 1ull) && nk < post_max) {
        kept |= 1ull << bb;
        if (lane == 0) kb[nk] = blk * 64 + bb;
        ++nk;
        rem |= d;
      }
    }
    if (nk >= post_max) break;
    for (int bb = 0; bb < lim; ++bb) {
      if (!((kept >> bb) & 1ull)) continue;
      if (lane > blk && lane < cb) removed |= mb[(size_t)(blk * 64 + bb) * words + lane];
    }
  }
  if (lane == 0) n_keep[b] = nk;
}

}  // namespace

extern "C" {

// 0 for batch < 1, num_tasks outside 1..4 and, with di, pre_max_size outside 1..1024
size_t sessd_predict_workspace_bytes(int batch, int num_tasks, int num_anchors, int pre_max_size, int post_max_size, int di) {
  if (batch < 1 || num_tasks < 1 || num_tasks > 4) return 0;
  if (di && (pre_max_size < 1 || pre_max_size > DI_MAXN)) return 0;
  return post_ws_layout(batch * num_tasks, num_tasks, num_anchors, pre_max_size, post_max_size, nullptr, nullptr, di != 0);
}

size_t sessd_predict_args_bytes(void) { return sizeof(sessd_predict_args_t); }

// The post-processor of a batch; the arguments are documented field by field at sessd_predict_args_t (sessd_hip_types.h).
// T = 1: 3 launches per call with external keys and pre_max_size such that the suppression mask fits the LDS (<= ~1280): top-k
// + decode, suppression mask, greedy walk + filters + record. T > 1: the same launches over B*T virtual frames + the merge.
// di != nullptr: DI-NMS (box_torch_ops.rotate_weighted_nms, enable_centerness=True, centerness_c=False) instead of the suppression
// mask and the greedy walk, everything else is shared: see the kernels above and include/sessd_hip.h. 3 launches per call with
// external keys (top-k + decode, overlap rows, selection + filters + record), one fewer than the greedy path; T > 1 adds the merge.
int sessd_predict(const sessd_predict_args_t* args, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!args) return SESSD_EINVAL;
  const sessd_predict_args_t& a = *args;
  const float *head = a.head, *anchors = a.anchors, *post_center_range6 = a.post_center_range;
  const double* frustum = a.frustum;
  const int batch = a.batch, num_tasks = a.num_tasks, num_pixels = a.num_pixels, anchors_per_frame = a.anchors_per_frame;
  const int pre_max_size = a.pre_max_size, post_max_size = a.post_max_size, capacity_frames = a.capacity_frames;
  const float score_thresh = a.score_thresh, nms_iou_thresh = a.nms_iou_thresh, direction_offset = a.direction_offset;
  float *out_box = a.out_box, *out_score = a.out_score, *records = a.records;
  int *out_label = a.out_label, *out_count = a.out_count, *out_task_count = a.out_task_count;
  int *record_counts = a.record_counts, *cursor = a.cursor;
  const unsigned long long* ext_keys = (const unsigned long long*)a.ext_keys;
  const int* ext_key_count = a.ext_key_count;
  int *di_truncated = a.di_truncated, *di_truncated_sticky = a.di_truncated_sticky, *di_keep = a.di_keep;
  int* di_keep_count = a.di_keep_count;
  if (a.di && (a.di->n_interval < 0 || a.di->n_interval > 8)) return SESSD_EINVAL;
  DiCfg D;
  const DiCfg* di = a.di ? &D : nullptr;
  if (a.di) {
    D.cnt_thresh = a.di->cnt_thresh;
    D.suppressed_thresh = a.di->suppressed_thresh;
    D.centerness_pow = a.di->centerness_pow;
    D.n_interval = a.di->n_interval;
    for (int k = 0; k < 8; ++k) {
      D.interval[k] = k < D.n_interval ? a.di->interval[k] : 0.f;
      D.sigma_sq[k] = k + 1 < D.n_interval ? a.di->sigma_sq[k] : 1.f;
    }
  }
  if (batch < 1 || num_pixels < 1 || pre_max_size < 1 || pre_max_size > 4096 || post_max_size < 1) return SESSD_EINVAL;
  if (di && pre_max_size > DI_MAXN) return SESSD_EINVAL;  // one thread per candidate in the selection workgroup
  if ((di_keep == nullptr) != (di_keep_count == nullptr)) return SESSD_EINVAL;
  if (num_tasks < 1 || num_tasks > 4) return SESSD_EINVAL;
  if (pre_max_size > SORT_N - 64) return SESSD_EINVAL;  // running top-k keeps pre_max + a fresh chunk in 2048 slots
  if ((ext_keys == nullptr) != (ext_key_count == nullptr)) return SESSD_EINVAL;
  if (records && (!record_counts || !cursor || capacity_frames < batch || batch > 256)) return SESSD_EINVAL;
  const int A = num_pixels * APL;
  if (anchors_per_frame && anchors_per_frame != A) return SESSD_EINVAL;
  const bool multi = num_tasks > 1;
  const int vbatch = batch * num_tasks;  // virtual frames
  PostWs w;
  if (post_ws_layout(vbatch, num_tasks, A, pre_max_size, post_max_size, &w, (char*)workspace, di != nullptr) > workspace_bytes)
    return SESSD_EWORKSPACE;
  PostCfg C;
  C.num_pix = num_pixels;
  C.score_thresh = score_thresh;
  C.pre_max = pre_max_size;
  C.post_max = post_max_size;
  C.nms_thresh = nms_iou_thresh;
  for (int i = 0; i < 6; ++i) C.range[i] = post_center_range6[i];
  C.dir_offset = direction_offset;
  C.num_tasks = num_tasks;
  const unsigned long long* keys = ext_keys;
  const int* key_count = ext_key_count;
  if (!ext_keys) {
    SESSD_FILL(w.count, 0, vbatch, stream);
    SESSD_LAUNCH(score_filter_kernel, dim3(sessd_divup(num_pixels, 256), vbatch), dim3(256), 0, stream, head, C,
                       w.keys, A, w.count);
    SESSD_CHECK_LAUNCH();
    keys = w.keys;
    key_count = w.count;
  }
  SESSD_LAUNCH(topk_decode_kernel, dim3(vbatch), dim3(SORT_NT), 0, stream, head, anchors, anchors_per_frame, C,
                     keys, A, key_count, w.cand_box, w.cand_score, w.cand_dir, w.corners, w.standup, w.n_top,
                     records ? cursor : (int*)nullptr, w.rec_base, batch, w.pair_count, di ? w.cand_ioup : (float*)nullptr,
                     di ? w.cand_axy : (float*)nullptr);
  SESSD_CHECK_LAUNCH();
  const int words = sessd_divup(pre_max_size, 64);
  if (!di) {
    const int rc = launch_rnms_mask(w.n_top, vbatch, pre_max_size, nms_iou_thresh, w.corners, w.standup, w.mask, words, w.pairs,
                                    w.pair_count, stream);
    if (rc != SESSD_OK) return rc;
  }
  // multi-task: K4/K5 leave per-(frame, task) rows in the workspace; the merge writes the caller's outputs and the record
  float* k_box = multi ? w.task_box : out_box;
  float* k_score = multi ? w.task_score : out_score;
  int* k_label = multi ? w.task_label : out_label;
  int* k_count = multi ? w.task_count : out_count;
  float* k_records = multi ? nullptr : records;
  const size_t lds = (size_t)pre_max_size * words * 8 + (size_t)post_max_size * 4 + (size_t)post_max_size * 9 * 4;
  if (di) {
    SESSD_LAUNCH(di_overlap_rows_kernel, dim3(sessd_divup(pre_max_size, DI_ROWS), vbatch), dim3(DI_ROWS * 64), 0, stream, w.n_top,
                 pre_max_size, w.corners, w.standup, w.overlap);
    SESSD_CHECK_LAUNCH();
    const int kcap = post_max_size < pre_max_size ? post_max_size : pre_max_size;
    SESSD_LAUNCH(di_select_finalize_kernel, dim3(vbatch), dim3(DI_MAXN), (size_t)kcap * 10 * 4, stream, C, *di, w.n_top, w.overlap,
                 w.cand_box, w.cand_score, w.cand_dir, w.cand_ioup, w.cand_axy, w.di_box, w.di_score, w.di_dir, frustum, k_box,
                 k_score, k_label, k_count, di_truncated, di_truncated_sticky, di_keep, di_keep_count, k_records, record_counts,
                 capacity_frames, w.rec_base);
    SESSD_CHECK_LAUNCH();
  } else if (lds <= 160 * 1024 - 1024) {
    static bool attr_set = false;
    if (!attr_set) {
      SESSD_TRY(hipFuncSetAttribute((const void*)nms_reduce_finalize_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    160 * 1024 - 1024));
      attr_set = true;
    }
    SESSD_LAUNCH(nms_reduce_finalize_kernel, dim3(vbatch), dim3(1024), lds, stream, C, w.n_top, w.mask, words, w.cand_box,
                       w.cand_score, w.cand_dir, frustum, k_box, k_score, k_label, k_count, k_records, record_counts,
                       capacity_frames, w.rec_base);
    SESSD_CHECK_LAUNCH();
  } else {
    SESSD_LAUNCH(nms_reduce_batch_kernel, dim3(vbatch), dim3(64), 0, stream, w.n_top, pre_max_size, w.mask, words,
                       post_max_size, w.keep, w.n_keep);
    SESSD_CHECK_LAUNCH();
    SESSD_LAUNCH(finalize_kernel, dim3(vbatch), dim3(64), 0, stream, C, w.keep, w.n_keep, w.cand_box, w.cand_score,
                       w.cand_dir, frustum, k_box, k_score, k_label, k_count);
    SESSD_CHECK_LAUNCH();
    if (k_records) {
      SESSD_LAUNCH(pack_detections_kernel, dim3(1), dim3(256), 0, stream, out_box, out_score, out_label, out_count, batch,
                   post_max_size, records, record_counts, capacity_frames, (int*)nullptr, w.rec_base);
      SESSD_CHECK_LAUNCH();
    }
  }
  if (multi) {
    SESSD_LAUNCH(merge_tasks_kernel, dim3(batch), dim3(256), 0, stream, num_tasks, post_max_size, w.task_box, w.task_score,
                 w.task_count, out_box, out_score, out_label, out_count, out_task_count, records, record_counts, capacity_frames,
                 w.rec_base);
    SESSD_CHECK_LAUNCH();
  } else if (out_task_count) {  // (B, 1): the frame's count
    SESSD_LAUNCH(copy_counts_kernel, dim3(1), dim3(256), 0, stream, out_count, out_task_count, batch);
    SESSD_CHECK_LAUNCH();
  }
  return SESSD_OK;
}

// Stand-alone rotated NMS with the predict-path semantics (box_torch_ops.rotate_nms after its topk):
// dets (N,5) [x,y,w,l,r] sorted by descending score. keep (device int32[post_max]), num_keep (device int).
size_t sessd_rotate_nms_workspace_bytes(int num_boxes) {
  const int words = sessd_divup(num_boxes > 0 ? num_boxes : 1, 64);
  return sessd_align((size_t)num_boxes * 12 * 4, 256) + sessd_align((size_t)num_boxes * words * 8, 256) + 512 +
         sessd_align((size_t)rn_pair_cap(num_boxes > 0 ? num_boxes : 1) * 4, 256);
}

}  // extern "C"

namespace {
__global__ __launch_bounds__(256) void rnms_prep_kernel(const float* __restrict__ dets, int n, float* __restrict__ corners,
                                                         float* __restrict__ standup) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float c8[8];
  sessd_box2d_corners(dets + (size_t)i * 5, c8);
  float x0 = c8[0], y0 = c8[1], x1 = c8[0], y1 = c8[1];
#pragma unroll
  for (int q = 1; q < 4; ++q) {
    x0 = fminf(x0, c8[2 * q]); x1 = fmaxf(x1, c8[2 * q]);
    y0 = fminf(y0, c8[2 * q + 1]); y1 = fmaxf(y1, c8[2 * q + 1]);
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) corners[(size_t)i * 8 + q] = c8[q];
  standup[(size_t)i * 4 + 0] = x0; standup[(size_t)i * 4 + 1] = y0; standup[(size_t)i * 4 + 2] = x1; standup[(size_t)i * 4 + 3] = y1;
}
__global__ void set_int_kernel(int* p, int v) { p[0] = v; p[1] = 0; }  // n_top, pair_count
// corners given by the caller (det3d.ops.nms.nms.rotate_non_max_suppression_cpu, nms_cpu.h:72-168): copy + AABB
__global__ __launch_bounds__(256) void rnms_prep_corners_kernel(const float* __restrict__ in_corners, int n,
                                                                 float* __restrict__ corners, float* __restrict__ standup) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float c8[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) c8[q] = in_corners[(size_t)i * 8 + q];
  float x0 = c8[0], y0 = c8[1], x1 = c8[0], y1 = c8[1];
#pragma unroll
  for (int q = 1; q < 4; ++q) {
    x0 = fminf(x0, c8[2 * q]); x1 = fmaxf(x1, c8[2 * q]);
    y0 = fminf(y0, c8[2 * q + 1]); y1 = fmaxf(y1, c8[2 * q + 1]);
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) corners[(size_t)i * 8 + q] = c8[q];
  standup[(size_t)i * 4 + 0] = x0; standup[(size_t)i * 4 + 1] = y0; standup[(size_t)i * 4 + 2] = x1; standup[(size_t)i * 4 + 3] = y1;
}
}  // namespace

static int rotate_nms_common(const float* dets, const float* in_corners, int num_boxes, float iou_thresh, int post_max_size,
                             int* keep, int* num_keep, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (num_boxes < 0 || num_boxes > 4096 || post_max_size < 1) return SESSD_EINVAL;
  if (workspace_bytes < sessd_rotate_nms_workspace_bytes(num_boxes)) return SESSD_EWORKSPACE;
  if (num_boxes == 0) {
    SESSD_FILL(num_keep, 0, 1, stream);
    return SESSD_OK;
  }
  char* base = (char*)workspace;
  float* corners = (float*)base;
  float* standup = corners + (size_t)num_boxes * 8;
  size_t off = sessd_align((size_t)num_boxes * 12 * 4, 256);
  const int words = sessd_divup(num_boxes, 64);
  unsigned long long* mask = (unsigned long long*)(base + off);
  off += sessd_align((size_t)num_boxes * words * 8, 256);
  int* n_top = (int*)(base + off);
  unsigned* pairs = (unsigned*)(base + off + 512);
  SESSD_LAUNCH(set_int_kernel, dim3(1), dim3(1), 0, stream, n_top, num_boxes);
  if (in_corners)
    SESSD_LAUNCH(rnms_prep_corners_kernel, dim3(sessd_divup(num_boxes, 256)), dim3(256), 0, stream, in_corners,
                       num_boxes, corners, standup);
  else
    SESSD_LAUNCH(rnms_prep_kernel, dim3(sessd_divup(num_boxes, 256)), dim3(256), 0, stream, dets, num_boxes, corners,
                       standup);
  SESSD_CHECK_LAUNCH();
  {
    const int rc = launch_rnms_mask(n_top, 1, num_boxes, iou_thresh, corners, standup, mask, words, pairs, n_top + 1, stream);
    if (rc != SESSD_OK) return rc;
  }
  SESSD_LAUNCH(nms_reduce_batch_kernel, dim3(1), dim3(64), 0, stream, n_top, num_boxes, mask, words, post_max_size,
                     keep, num_keep);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

// The same greedy rotated NMS on caller-supplied corner quads (N,4,2), already in descending-score order: the device
// form of det3d.ops.nms.nms.rotate_non_max_suppression_cpu (nms_cpu.h:72-168; the stand-up IoU prefilter is recomputed
// from the corners' bounding boxes = what nms_cpu.py:45-49 passes in).
extern "C" int sessd_rotate_nms_corners_sorted(const float* corners, int num_boxes, float iou_thresh, int post_max_size,
                                               int* keep, int* num_keep, void* workspace, size_t workspace_bytes,
                                               hipStream_t stream) {
  if (!corners && num_boxes > 0) return SESSD_EINVAL;
  return rotate_nms_common(nullptr, corners, num_boxes, iou_thresh, post_max_size, keep, num_keep, workspace, workspace_bytes,
                           stream);
}

extern "C" int sessd_rotate_nms_sorted(const float* dets, int num_boxes, float iou_thresh, int post_max_size, int* keep,
                                       int* num_keep, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return rotate_nms_common(dets, nullptr, num_boxes, iou_thresh, post_max_size, keep, num_keep, workspace, workspace_bytes,
                           stream);
}

// ---- spconv.utils.rbbox_iou / rbbox_intersection (spconv v1 box_iou: boost polygons on the host), as imported by
// det3d/core/bbox/box_np_ops.py:9 and used by riou_cc / rinter_cc :20-50: pairwise IoU / intersection area of convex quads
// given as corners, skipped (0) where the caller's stand-up IoU is <= standup_thresh. Same float64 clipper as the rotated NMS.
namespace {
__global__ __launch_bounds__(256) void quads_pairwise_kernel(int mode, const float* __restrict__ ca, int n,
                                                              const float* __restrict__ cb, int k,
                                                              const float* __restrict__ standup_iou, float standup_thresh,
                                                              float* __restrict__ out) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (size_t)n * k) return;
  const int i = (int)(id / k), j = (int)(id - (size_t)i * k);
  float v = 0.f;
  if (standup_iou[id] > standup_thresh) {
    const float* pi = ca + (size_t)i * 8;
    const float* pj = cb + (size_t)j * 8;
    const double inter = sessd_quad_inter_area_green(pi, pj);
    if (inter > 0) {
      if (mode == 0) {
        double px[4], py[4], qx[4], qy[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { px[q] = pi[2 * q]; py[q] = pi[2 * q + 1]; qx[q] = pj[2 * q]; qy[q] = pj[2 * q + 1]; }
        const double uni = fabs(sessd_poly_area2(px, py, 4)) * 0.5 + fabs(sessd_poly_area2(qx, qy, 4)) * 0.5 - inter;
        v = uni > 0 ? (float)(inter / uni) : 0.f;
      } else {
        v = (float)inter;
      }
    }
  }
  out[id] = v;
}
}  // namespace

// mode 0: IoU, 1: intersection area. corners (n,4,2) / (k,4,2) float32, standup_iou and out (n,k) row-major.
extern "C" int sessd_quads_pairwise(int mode, const float* corners_a, int n, const float* corners_b, int k,
                                    const float* standup_iou, float standup_thresh, float* out, hipStream_t stream) {
  if (n < 0 || k < 0 || mode < 0 || mode > 1) return SESSD_EINVAL;
  if (n == 0 || k == 0) return SESSD_OK;
  const size_t total = (size_t)n * k;
  SESSD_LAUNCH(quads_pairwise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, mode, corners_a, n,
               corners_b, k, standup_iou, standup_thresh, out);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

extern "C" int sessd_pack_detections(const float* out_box, const float* out_score, const int* out_label, const int* out_count,
                                     int batch, int post_max_size, float* records, int* record_counts, int capacity_frames,
                                     int* cursor, hipStream_t stream) {
  if (batch <= 0 || batch > 256 || post_max_size <= 0 || capacity_frames < batch) return SESSD_EINVAL;
  SESSD_LAUNCH(pack_detections_kernel, dim3(1), dim3(256), 0, stream, out_box, out_score, out_label, out_count, batch,
               post_max_size, records, record_counts, capacity_frames, cursor, (const int*)nullptr);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}
