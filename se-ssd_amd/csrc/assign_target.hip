// Anchor target assignment of the SE-SSD training pipeline on gfx950 ("AssignTarget, nearest-IoU anchor
// matching over 70400 anchors"). Replaces the per-sample numpy / numba code that runs in the reference's DataLoader workers:
//   det3d/datasets/pipelines/preprocess.py:236-358 (AssignTarget) -> det3d/core/anchor/target_assigner.py:68-136 (assign_v2)
//   -> det3d/core/anchor/target_ops_v3.py:11-137 (create_target_np) with det3d/core/bbox/region_similarity.py:85-98
//   (NearestIouSimilarity: rbbox2d_to_near_bbox + iou_jit(eps=0), box_np_ops.py:354-366,1008-1046) and
//   box_np_ops.second_box_encode (:52-110).
// Two launches over the anchors (one thread per anchor, the <= 128 ground-truth boxes of the sample in LDS):
//   1. IoU of the anchor's nearest axis-aligned box with every ground-truth box in the same float32 operation order as
//      iou_jit; per-anchor max / first argmax; per-ground-truth max by wave reduction + atomicMax on the float bits
//      (IoU >= 0, so the unsigned order is the float order; a max is order independent)
//   2. labels: forced positives (anchors that attain a ground truth's maximum, recomputed bit-identically), positives at
//      IoU >= matched, background below unmatched (forced positives win), ignore (-1) in between; regression targets
//      (second_box_encode) and weights of the foreground anchors.
// HBM-bound and tiny: 70400 x 28 B read twice, 70400 x 40 B written.
// sessd_assign_targets_batch (second half of the file) runs the same two passes for every frame and every task of a batch at
// once, with the ground-truth counts read on the device.
#include "common.hpp"
#include "sessd_hip_types.h"

namespace {

constexpr int MAX_GT = 128;
constexpr float PI_F = 3.14159274101257324f;      // np.float32(np.pi)
constexpr float PI_4_F = 0.785398185253143311f;   // np.float32(np.pi / 4)

struct NearBox {
  float x1, y1, x2, y2;
};

// box_np_ops.rbbox2d_to_near_bbox on [x, y, w, l, r]
__device__ __forceinline__ NearBox near_box(float x, float y, float w, float l, float r) {
  const float folded = fabsf(r - floorf(__fdiv_rn(r, PI_F) + 0.5f) * PI_F);
  const bool swap = folded > PI_4_F;
  const float ww = swap ? l : w, ll = swap ? w : l;
  NearBox b;
  b.x1 = x - ww / 2.f; b.y1 = y - ll / 2.f; b.x2 = x + ww / 2.f; b.y2 = y + ll / 2.f;
  return b;
}

// iou_jit(eps = 0): boxes = anchors, query = ground truth
__device__ __forceinline__ float near_iou(const NearBox& a, const NearBox& g, float area_g) {
  const float iw = fminf(a.x2, g.x2) - fmaxf(a.x1, g.x1);
  if (!(iw > 0.f)) return 0.f;
  const float ih = fminf(a.y2, g.y2) - fmaxf(a.y1, g.y1);
  if (!(ih > 0.f)) return 0.f;
  const float inter = iw * ih;
  const float ua = (a.x2 - a.x1) * (a.y2 - a.y1) + area_g - inter;
  return __fdiv_rn(inter, ua);
}

__device__ __forceinline__ void load_gt(const float* __restrict__ gt, int m, NearBox* sg, float* sarea) {
  for (int k = threadIdx.x; k < m; k += blockDim.x) {
    const float* g = gt + (size_t)k * 7;
    const NearBox b = near_box(g[0], g[1], g[3], g[4], g[6]);
    sg[k] = b;
    sarea[k] = (b.x2 - b.x1) * (b.y2 - b.y1);
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void assign_iou_kernel(const float* __restrict__ anchors, int n, const float* __restrict__ gt,
                                                          int m, float* __restrict__ a_max, int* __restrict__ a_arg,
                                                          unsigned* __restrict__ gmax_bits) {
  __shared__ NearBox sg[MAX_GT];
  __shared__ float sarea[MAX_GT];
  load_gt(gt, m, sg, sarea);
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  NearBox a = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float* p = anchors + (size_t)i * 7;
    a = near_box(p[0], p[1], p[3], p[4], p[6]);
  }
  float best = -1.f;
  int arg = 0;
  for (int k = 0; k < m; ++k) {
    const float v = live ? near_iou(a, sg[k], sarea[k]) : 0.f;
    if (v > best) { best = v; arg = k; }  // strict: first maximum, like numpy argmax
    float w = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w = fmaxf(w, __shfl_xor(w, o, 64));
    if ((threadIdx.x & 63) == 0 && w > 0.f) atomicMax(&gmax_bits[k], __float_as_uint(w));
  }
  if (live) { a_max[i] = best; a_arg[i] = arg; }
}

__global__ __launch_bounds__(256) void assign_label_kernel(const float* __restrict__ anchors, int n, const float* __restrict__ gt,
                                                            const int* __restrict__ gt_classes, int m, float matched,
                                                            float unmatched, const float* __restrict__ a_max,
                                                            const int* __restrict__ a_arg, const unsigned* __restrict__ gmax_bits,
                                                            int* __restrict__ labels, float* __restrict__ targets,
                                                            float* __restrict__ weights, int* __restrict__ gt_id) {
  __shared__ NearBox sg[MAX_GT];
  __shared__ float sarea[MAX_GT];
  load_gt(gt, m, sg, sarea);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* p = anchors + (size_t)i * 7;
  float* t = targets + (size_t)i * 7;
  if (m == 0) {  // target_ops_v3.py:90-91,99-100: everything is background
    labels[i] = 0; weights[i] = 0.f; gt_id[i] = -1;
#pragma unroll
    for (int q = 0; q < 7; ++q) t[q] = 0.f;
    return;
  }
  const NearBox a = near_box(p[0], p[1], p[3], p[4], p[6]);
  bool force = false;
  for (int k = 0; k < m; ++k) {
    const unsigned gb = gmax_bits[k];
    if (gb == 0u) continue;  // a ground truth that overlaps no anchor forces nothing (:65-67)
    force = force || (near_iou(a, sg[k], sarea[k]) == __uint_as_float(gb));
  }
  const float best = a_max[i];
  const int arg = a_arg[i];
  const int cls = gt_classes ? gt_classes[arg] : 1;
  int label = -1, gid = -1;
  if (force || best >= matched) { label = cls; gid = arg; }
  const bool fg = label > 0;
  if (best < unmatched) label = 0;
  if (force) label = cls;
  labels[i] = label;
  weights[i] = label > 0 ? 1.f : 0.f;
  gt_id[i] = fg ? gid : -1;
  if (fg) {  // box_np_ops.second_box_encode (:66-110), plain residual yaw
    const float* g = gt + (size_t)arg * 7;
    const float diag = sqrtf(p[4] * p[4] + p[3] * p[3]);
    t[0] = __fdiv_rn(g[0] - p[0], diag);
    t[1] = __fdiv_rn(g[1] - p[1], diag);
    t[2] = __fdiv_rn(g[2] - p[2], p[5]);
    t[3] = logf(__fdiv_rn(g[3], p[3]));
    t[4] = logf(__fdiv_rn(g[4], p[4]));
    t[5] = logf(__fdiv_rn(g[5], p[5]));
    t[6] = g[6] - p[6];
  } else {
#pragma unroll
    for (int q = 0; q < 7; ++q) t[q] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ all frames, all tasks
// sessd_assign_targets_batch: the same assignment for every (frame, task) of a batch in one clear and two launches on the grid
// (256-anchor block, b * T + t). Per block:
//   - the frame's ground truth is staged into LDS through the count (gt_count[b], read on the device) and the task's class
//     filter, compacted in row order (ballot prefix over the two waves that hold the <= 128 rows): rows at or beyond the count
//     are never loaded, a row of another class never enters a decision, and the compacted index is the reference's gt id;
//   - the block's anchor rows, and in the label pass the target rows it writes, go through a 256 x 7 float LDS slab: global
//     traffic is lane-contiguous, the per-thread rows are read and written at a stride of 7 words (odd: conflict free).
// The arithmetic is the functions above, in the order of the two kernels above.
constexpr int NT = 256;
constexpr int MAXT = 4;

struct BatchTasks {
  sessd_assign_task_t t[MAXT];
};

struct BatchWork {
  unsigned* gmax;  // [B * T][MAX_GT] per-ground-truth maximum, float bits
  float* a_max;    // [B * T][A]
  int* a_arg;      // [B * T][A]
};

// The live rows of frame b that belong to the task, compacted in row order into sg / sarea (and the rows themselves into
// sgt, when given). Returns their number, the same in every thread. `scnt` holds two ints.
__device__ __forceinline__ int stage_gt(const sessd_assign_batch_cfg_t& P, const sessd_assign_task_t& K, int b,
                                        const float* __restrict__ gt_boxes, const int* __restrict__ gt_classes,
                                        const int* __restrict__ gt_count, NearBox* sg, float* sarea, float* sgt, int* scnt) {
  const int G = P.gt_capacity, tid = threadIdx.x;
  const int live_rows = gt_count ? min(max(gt_count[b], 0), G) : G;
  bool keep = false;
  if (tid < live_rows) keep = !gt_classes || K.class_id <= 0 || gt_classes[(size_t)b * G + tid] == K.class_id;
  const unsigned long long mask = __ballot(keep);
  if (tid < 2 * 64 && (tid & 63) == 0) scnt[tid >> 6] = __popcll(mask);
  __syncthreads();
  if (keep) {
    const int k = (tid >= 64 ? scnt[0] : 0) + __popcll(mask & ((1ull << (tid & 63)) - 1ull));
    const float* g = gt_boxes + ((size_t)b * G + tid) * 7;
    float v[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) v[q] = g[q];
    const NearBox nb = near_box(v[0], v[1], v[3], v[4], v[6]);
    sg[k] = nb;
    sarea[k] = (nb.x2 - nb.x1) * (nb.y2 - nb.y1);
    if (sgt) {
#pragma unroll
      for (int q = 0; q < 7; ++q) sgt[k * 7 + q] = v[q];
    }
  }
  const int m = scnt[0] + scnt[1];
  __syncthreads();
  return m;
}

// the block's n anchor rows, lane-contiguous, into the slab
__device__ __forceinline__ void stage_anchors(const float* __restrict__ rows, int n, float* slab) {
  for (int j = threadIdx.x; j < n * 7; j += NT) slab[j] = rows[j];
  __syncthreads();
}

__global__ __launch_bounds__(NT) void assign_batch_iou_kernel(BatchTasks TK, sessd_assign_batch_cfg_t P, BatchWork W,
                                                              const float* __restrict__ gt_boxes,
                                                              const int* __restrict__ gt_classes,
                                                              const int* __restrict__ gt_count) {
  __shared__ NearBox sg[MAX_GT];
  __shared__ float sarea[MAX_GT];
  __shared__ int scnt[2];
  __shared__ float slab[NT * 7];
  const int bt = blockIdx.y, b = bt / P.num_tasks, t = bt - b * P.num_tasks, A = P.num_anchors, tid = threadIdx.x;
  const sessd_assign_task_t& K = TK.t[t];
  const int m = stage_gt(P, K, b, gt_boxes, gt_classes, gt_count, sg, sarea, nullptr, scnt);
  if (m == 0) return;  // the label pass reads neither maxima nor arguments of an empty (frame, task)
  const int a0 = blockIdx.x * NT, n = min(NT, A - a0);
  stage_anchors(K.anchors + ((size_t)(P.anchors_per_frame ? b : 0) * A + a0) * 7, n, slab);
  const bool live = tid < n;
  NearBox a = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float* p = slab + tid * 7;
    a = near_box(p[0], p[1], p[3], p[4], p[6]);
  }
  unsigned* gmax = W.gmax + (size_t)bt * MAX_GT;
  float best = -1.f;
  int arg = 0;
  for (int k = 0; k < m; ++k) {
    const float v = live ? near_iou(a, sg[k], sarea[k]) : 0.f;
    if (v > best) { best = v; arg = k; }  // strict: first maximum, like numpy argmax
    float w = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w = fmaxf(w, __shfl_xor(w, o, 64));
    if ((tid & 63) == 0 && w > 0.f) atomicMax(&gmax[k], __float_as_uint(w));
  }
  if (live) {
    const size_t i = (size_t)bt * A + a0 + tid;
    W.a_max[i] = best;
    W.a_arg[i] = arg;
  }
}

__global__ __launch_bounds__(NT) void assign_batch_label_kernel(BatchTasks TK, sessd_assign_batch_cfg_t P, BatchWork W,
                                                                const float* __restrict__ gt_boxes,
                                                                const int* __restrict__ gt_classes,
                                                                const int* __restrict__ gt_count) {
  __shared__ NearBox sg[MAX_GT];
  __shared__ float sarea[MAX_GT];
  __shared__ float sgt[MAX_GT * 7];
  __shared__ unsigned sgmax[MAX_GT];
  __shared__ int scnt[2];
  __shared__ float slab[NT * 7];  // anchor rows in, target rows out
  const int bt = blockIdx.y, b = bt / P.num_tasks, t = bt - b * P.num_tasks, A = P.num_anchors, tid = threadIdx.x;
  const sessd_assign_task_t& K = TK.t[t];
  const int m = stage_gt(P, K, b, gt_boxes, gt_classes, gt_count, sg, sarea, sgt, scnt);
  const int a0 = blockIdx.x * NT, n = min(NT, A - a0);
  const bool live = tid < n;
  const size_t i = (size_t)b * A + a0 + (live ? tid : 0);  // in the task's (B, A) outputs
  int label = 0, gid = -1;
  if (m > 0) {
    if (tid < m) sgmax[tid] = W.gmax[(size_t)bt * MAX_GT + tid];
    stage_anchors(K.anchors + ((size_t)(P.anchors_per_frame ? b : 0) * A + a0) * 7, n, slab);  // its barrier covers sgmax
  }
  if (live && m > 0) {
    float* row = slab + tid * 7;  // this thread's anchor, then this thread's targets: no other thread touches the row
    float p[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) p[q] = row[q];
    const NearBox a = near_box(p[0], p[1], p[3], p[4], p[6]);
    bool force = false;
    for (int k = 0; k < m; ++k) {
      const unsigned gb = sgmax[k];
      if (gb == 0u) continue;  // a ground truth that overlaps no anchor forces nothing (:65-67)
      force = force || (near_iou(a, sg[k], sarea[k]) == __uint_as_float(gb));
    }
    const size_t w = (size_t)bt * A + a0 + tid;
    const float best = W.a_max[w];
    const int arg = W.a_arg[w];
    label = -1;
    if (force || best >= K.matched) { label = 1; gid = arg; }
    const bool fg = label > 0;
    if (best < K.unmatched) label = 0;
    if (force) label = 1;
    if (!fg) gid = -1;
    if (fg) {  // box_np_ops.second_box_encode (:66-110), plain residual yaw
      const float* g = sgt + arg * 7;
      const float diag = sqrtf(p[4] * p[4] + p[3] * p[3]);
      row[0] = __fdiv_rn(g[0] - p[0], diag);
      row[1] = __fdiv_rn(g[1] - p[1], diag);
      row[2] = __fdiv_rn(g[2] - p[2], p[5]);
      row[3] = logf(__fdiv_rn(g[3], p[3]));
      row[4] = logf(__fdiv_rn(g[4], p[4]));
      row[5] = logf(__fdiv_rn(g[5], p[5]));
      row[6] = g[6] - p[6];
    } else {
#pragma unroll
      for (int q = 0; q < 7; ++q) row[q] = 0.f;
    }
  }
  if (live) {
    if (P.labels_i64) ((long long*)K.labels)[i] = label; else ((int*)K.labels)[i] = label;
    if (K.reg_weights) K.reg_weights[i] = label > 0 ? 1.f : 0.f;
    if (K.gt_id) K.gt_id[i] = gid;
  }
  // ---- the block's target rows, lane-contiguous (an empty (frame, task) is all background with zero targets: :90-91,99-100)
  float* out = K.reg_targets + ((size_t)b * A + a0) * 7;
  if (m > 0) {
    __syncthreads();
    for (int j = tid; j < n * 7; j += NT) out[j] = slab[j];
  } else {
    for (int j = tid; j < n * 7; j += NT) out[j] = 0.f;
  }
}

bool batch_cfg_ok(const sessd_assign_batch_cfg_t* c) {
  return c && c->batch >= 1 && c->num_anchors >= 1 && c->num_tasks >= 1 && c->num_tasks <= MAXT && c->gt_capacity >= 1 &&
         c->gt_capacity <= MAX_GT && (long long)c->batch * c->num_tasks <= 65535 &&
         (long long)c->batch * c->num_tasks * c->num_anchors * 7 < (1ll << 31);
}

BatchWork batch_layout(const sessd_assign_batch_cfg_t* c, void* base, size_t* total) {
  const size_t bt = (size_t)c->batch * c->num_tasks, A = c->num_anchors;
  char* p = (char*)base;
  BatchWork W;
  W.gmax = (unsigned*)p; p += sessd_align(bt * MAX_GT * 4, 256);
  W.a_max = (float*)p;   p += sessd_align(bt * A * 4, 256);
  W.a_arg = (int*)p;     p += sessd_align(bt * A * 4, 256);
  *total = (size_t)(p - (char*)base);
  return W;
}

}  // namespace

extern "C" {

size_t sessd_assign_targets_batch_workspace_bytes(const sessd_assign_batch_cfg_t* cfg) {
  if (!batch_cfg_ok(cfg)) return 0;
  size_t total;
  batch_layout(cfg, nullptr, &total);
  return total;
}

int sessd_assign_targets_batch(const sessd_assign_batch_cfg_t* cfg, const sessd_assign_task_t* tasks, const float* gt_boxes,
                               const int32_t* gt_classes, const int32_t* gt_count, void* workspace, size_t workspace_bytes,
                               hipStream_t stream) {
  if (!batch_cfg_ok(cfg) || !tasks || !gt_boxes || !workspace) return SESSD_EINVAL;
  BatchTasks TK = {};
  for (int t = 0; t < cfg->num_tasks; ++t) {
    const sessd_assign_task_t& k = tasks[t];
    if (!k.anchors || !k.labels || !k.reg_targets) return SESSD_EINVAL;
    TK.t[t] = k;
  }
  if (((size_t)workspace & 255) != 0) return SESSD_EINVAL;
  size_t need;
  const BatchWork W = batch_layout(cfg, workspace, &need);
  if (workspace_bytes < need) return SESSD_EWORKSPACE;
  const sessd_assign_batch_cfg_t P = *cfg;
  const int bt = P.batch * P.num_tasks;
  SESSD_FILL(W.gmax, 0u, (size_t)bt * MAX_GT, stream);
  const dim3 grid(sessd_divup(P.num_anchors, NT), bt);
  SESSD_LAUNCH(assign_batch_iou_kernel, grid, dim3(NT), 0, stream, TK, P, W, gt_boxes, gt_classes, gt_count);
  SESSD_CHECK_LAUNCH();
  SESSD_LAUNCH(assign_batch_label_kernel, grid, dim3(NT), 0, stream, TK, P, W, gt_boxes, gt_classes, gt_count);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

size_t sessd_assign_targets_workspace_bytes(int num_anchors) {
  return sessd_align((size_t)MAX_GT * 4, 256) + 2 * sessd_align((size_t)num_anchors * 4, 256);
}

// anchors (n,7), gt_boxes (m,7) [x,y,z,w,l,h,r] float32, gt_classes (m,) int32 or NULL (all 1), m <= 128. Outputs (device):
// labels (n,) int32 in {-1 ignore, 0 background, class}, bbox_targets (n,7), bbox_outside_weights (n,), gt_id (n,) = index of
// the assigned ground truth for the foreground anchors, -1 elsewhere (the reference's positive_gt_id is gt_id[gt_id >= 0]).
int sessd_assign_targets(const float* anchors, int num_anchors, const float* gt_boxes, const int* gt_classes, int num_gt,
                         float matched_threshold, float unmatched_threshold, int* labels, float* bbox_targets,
                         float* bbox_outside_weights, int* gt_id, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (num_anchors <= 0 || num_gt < 0 || num_gt > MAX_GT) return SESSD_EINVAL;
  if (workspace_bytes < sessd_assign_targets_workspace_bytes(num_anchors)) return SESSD_EWORKSPACE;
  char* base = (char*)workspace;
  unsigned* gmax = (unsigned*)base;
  float* a_max = (float*)(base + sessd_align((size_t)MAX_GT * 4, 256));
  int* a_arg = (int*)((char*)a_max + sessd_align((size_t)num_anchors * 4, 256));
  SESSD_FILL(gmax, 0u, MAX_GT, stream);
  const int blocks = sessd_divup(num_anchors, 256);
  if (num_gt > 0) {
    SESSD_LAUNCH(assign_iou_kernel, dim3(blocks), dim3(256), 0, stream, anchors, num_anchors, gt_boxes, num_gt, a_max, a_arg, gmax);
    SESSD_CHECK_LAUNCH();
  }
  SESSD_LAUNCH(assign_label_kernel, dim3(blocks), dim3(256), 0, stream, anchors, num_anchors, gt_boxes, gt_classes, num_gt,
               matched_threshold, unmatched_threshold, a_max, a_arg, gmax, labels, bbox_targets, bbox_outside_weights, gt_id);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

}  // extern "C"
